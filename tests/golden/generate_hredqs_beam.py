#!/usr/bin/env python
"""Fixtures of the HredQS beam search (tests/hredqs_beam_ref.py, tests/test_hredqs_beam_host.py, tests/test_gpu_hredqs_beam.py).

    python tests/golden/generate_hredqs_beam.py    # rewrites tests/golden/hredqs_beam_seeds.json

CPU only; imports this repository alone.  The fixtures are the four cases of tests/golden/hredqs.npz with seeded detinit noise on the generator
bias (beam_ref.noisy_bias): nothing new is recorded from the reference.

hredqs_beam_seeds.json: per case and width [seed, smallest gap, max_len] -- the first seed at which, in float64, every adjacent gap among the
top W + 1 candidates of every source row and step is >= 1e-3, EOS is selected, the last step has a finished and a live beam, a back-pointer
differs from the identity, and the free-running float32 restatement makes the same choices (beam_ref.conditions unchanged; for W = 4 also: the
W = 1 search keeps its gaps and its float32 agreement).  A (case, W) without a seed below the limit at the goldens' max_len is searched again at
max_len 4 (hredqs_beam_ref.SHORT_MAX_LEN); one without a seed there either is recorded as null and leaves the fixtures.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def find(R, BR, cs, tag, Wd, max_len, limit):
    for seed in range(1, limit):
        sd = R.perturbed(tag, Wd, seed=seed)
        ok, gap = True, None
        for w in ((Wd, 1) if Wd == 4 else (Wd,)):
            ref = R.decode(cs, sd, w, max_len=max_len)
            free = R.decode(cs, sd, w, torch.float32, max_len=max_len)
            cond = BR.conditions(ref, free, w)
            ok = ok and R.conditions_ok(cond, w)
            gap = cond["min_gap"] if gap is None else gap
            if not ok:
                break
        if ok:
            return [seed, gap, max_len]
    return None


def gen_seeds(limit=400):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import beam_ref as BR
    import hredqs_beam_ref as R
    found = {}
    for tag in R.CASES:
        cs = R.load_case(tag)
        found[tag] = {}
        for Wd in R.widths(tag):
            if Wd == 1:
                continue
            hit = find(R, BR, cs, tag, Wd, cs["max_len"], limit) or find(R, BR, cs, tag, Wd, R.SHORT_MAX_LEN, limit)
            found[tag][str(Wd)] = hit
            print("%s W=%d: %s" % (tag, Wd, "seed %d, smallest gap %.3g, max_len %d" % tuple(hit) if hit else "no seed below %d" % limit), flush=True)
    with open(os.path.join(HERE, "hredqs_beam_seeds.json"), "w") as f:
        json.dump(found, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    gen_seeds()
