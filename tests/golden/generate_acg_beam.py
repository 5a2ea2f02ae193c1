#!/usr/bin/env python
"""Fixtures of ACG's beam search (tests/acg_beam_ref.py, tests/test_acg_beam_host.py, tests/test_gpu_acg_beam.py).

    python tests/golden/generate_acg_beam.py        # rewrites tests/golden/acg_beam_seeds.json (CPU only, the restatement alone)

acg_beam_seeds.json: per fixture case and width the seed of the network (det_state_dict of the acg.npz case's shapes) and of the generator-bias
noise (beam_ref.noisy_bias) -- the first seed at which, in float64, every adjacent gap among the top W + 1 candidates of every source row and
step is >= 1e-3, EOS is selected, the last step has a finished and a live beam, a back-pointer differs from the identity, a beam k > 0 at a step
>= 1 selects an un-collapsed slot and a target word with nonzero copy mass, and the free-running float32 restatement makes the same choices (for
W = 4 also: the W = 1 search keeps its gaps and its float32 agreement) -- with the smallest gap found.  The network's seed has to vary: copy mass
does not see the generator bias, and with one case's own weights a gap between two slot masses stays below the bar for every bias seed.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def gen_seeds(limit=800):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import acg_beam_ref as R
    d = R.batch()
    VT = len(d["tgt_dict"])
    found = {}
    for kind, tag in R.CASES:
        found["%s_%s" % (kind, tag)] = {}
        for Wd in R.widths(kind, tag):
            if Wd == 1:
                continue
            for seed in range(1, limit):
                net, c, cell = R.case(kind, tag, Wd, seed=seed)
                sd = net.state_dict()
                ok, gap = True, None
                for w in ((Wd, 1) if Wd == 4 else (Wd,)):
                    args = (sd, c, cell, d["src"], d["lens"], R.max_len(w), w, d["idx"], d["e2t"], d["e2s"])
                    ref = R.decode(*args)
                    if float(ref["gaps"].min()) < R.MIN_GAP:
                        ok = False
                        break
                    cond = R.conditions(ref, R.decode(*args, dtype=torch.float32), w, VT, d["e2t"])
                    need = ("gap", "f32") if w == 1 else ("gap", "eos", "mixed", "moved", "slot", "fed", "f32")
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
    with open(os.path.join(HERE, "acg_beam_seeds.json"), "w") as f:
        json.dump(found, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    gen_seeds()
