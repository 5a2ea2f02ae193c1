#!/usr/bin/env python
"""Fixtures of the beam search (tests/beam_ref.py, tests/test_beam_host.py, tests/test_gpu_beam.py).

    python tests/golden/generate_beam.py            # rewrites tests/golden/beam_state.npz (needs the reference)
    python tests/golden/generate_beam.py --seeds    # rewrites tests/golden/beam_seeds.json (the restatement alone)

beam_state.npz: the reference has the state helpers of a beam and no search.  RNNDecoderState.repeat_beam_size_times (decoders/state.py:65-69)
and beam_update (:16-31) run here on an LSTM tuple and on a single GRU tensor, B = 3, W = 4, H = 8, one non-trivial permutation per source row;
inputs and results are recorded.  Keys: lstm_h, lstm_c, gru_h [1, B, H] (inputs); rep_lstm_h, rep_lstm_c, rep_gru_h [1, B W, H] (repeated);
pre_* [1, B W, H] (the repeated state plus noise: the beams of a row differ, as behind a decoder step); positions [B, W]; upd_lstm_h,
upd_lstm_c, upd_gru_h [1, B W, H] (pre_* after beam_update(b, positions[b], W) for every b).

beam_seeds.json: per fixture case and width the seed of the generator-bias noise (beam_ref.noisy_bias) -- the first seed at which, in float64,
every adjacent gap among the top W + 1 candidates of every source row and step is >= 1e-3, EOS is selected, the last step has a finished and
a live beam, a back-pointer differs from the identity, and the free-running float32 restatement makes the same choices (for W = 4 also: the
W = 1 search keeps its gaps and its float32 agreement) -- with the smallest gap found.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
B, W, H = 3, 4, 8


def gen_state():
    sys.path.insert(0, HERE)
    import generate as G  # noqa: F401  (installs the shims, puts the reference on sys.path)
    from neuroir.decoders.state import RNNDecoderState
    g = torch.Generator().manual_seed(1013)
    lstm = (torch.randn(1, B, H, generator=g), torch.randn(1, B, H, generator=g))
    gru = torch.randn(1, B, H, generator=g)
    positions = torch.tensor([[2, 0, 0, 3], [1, 1, 3, 0], [3, 2, 1, 1]])
    out = dict(lstm_h=lstm[0], lstm_c=lstm[1], gru_h=gru, positions=positions)
    for name, st in (("lstm", lstm), ("gru", gru)):
        s = RNNDecoderState(H, tuple(t.clone() for t in st) if isinstance(st, tuple) else st.clone())
        s.repeat_beam_size_times(W)
        names = ["%s_%s" % (name, n) for n in (("h", "c") if name == "lstm" else ("h",))]
        for n, e in zip(names, s._all):
            out["rep_" + n] = e.clone()
        # the W copies of a row are equal behind the repeat: a step's worth of difference, so that the shuffle shows
        s.update_state(tuple(e + torch.randn(e.shape, generator=g) for e in s._all), None)
        for n, e in zip(names, s._all):
            out["pre_" + n] = e.clone()
        for b in range(B):
            s.beam_update(b, positions[b], W)
        for n, e in zip(names, s._all):
            out["upd_" + n] = e.clone()
    # probed: the layout is k B + b
    assert torch.equal(out["rep_gru_h"][0, 2 * B + 1], gru[0, 1])
    np.savez(os.path.join(HERE, "beam_state.npz"), **{k: v.numpy() for k, v in out.items()})
    print("wrote beam_state.npz", {k: tuple(v.shape) for k, v in out.items()})


def gen_seeds(limit=400):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import beam_ref as R
    src, lens, max_len = R.inputs()
    found = {}
    for kind, tag in R.CASES:
        found["%s_%s" % (kind, tag)] = {}
        for Wd in R.widths(kind, tag):
            if Wd == 1:
                continue
            for seed in range(1, limit):
                net, c, cell, lut = R.case(kind, tag, Wd, seed=seed)
                sd = net.state_dict()
                ok, gap = True, None
                for w in ((Wd, 1) if Wd == 4 else (Wd,)):
                    ref = R.decode(sd, c, cell, src, lens, max_len, w, lut)
                    free = R.decode(sd, c, cell, src, lens, max_len, w, lut, torch.float32)
                    cond = R.conditions(ref, free, w)
                    need = ("gap", "f32") if w == 1 else ("gap", "eos", "mixed", "moved", "f32")
                    ok = ok and all(cond[k] for k in need)
                    gap = cond["min_gap"] if gap is None else gap
                    if not ok:
                        break
                if ok:
                    found["%s_%s" % (kind, tag)][str(Wd)] = [seed, gap]
                    print("%s %s W=%d: seed %d, smallest gap %.3g" % (kind, tag, Wd, seed, gap), flush=True)
                    break
            else:
                raise SystemExit("no seed below %d for %s %s W=%d" % (limit, kind, tag, Wd))
    with open(os.path.join(HERE, "beam_seeds.json"), "w") as f:
        json.dump(found, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    gen_seeds() if "--seeds" in sys.argv else gen_state()
