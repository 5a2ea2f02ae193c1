#!/usr/bin/env python
"""Fixtures of the session models' beam search (tests/session_beam_ref.py, tests/test_session_beam_host.py, tests/test_gpu_session_beam.py).

    python tests/golden/generate_session_beam.py    # rewrites tests/golden/session_beam_seeds.json

CPU only; imports this repository alone.  The golden weights of cars_decode / m_match_tensor / mnsrf give flat token distributions, so every
case gets seeded detinit noise (session_beam_ref.perturbed): generator.bias as beam_ref.noisy_bias for M_MATCH_TENSOR / MNSRF; for CARS, whose
token_prob_predictor2 has no bias, CARS_NOISE noise on its weight and a lift of its EOS row along the float64 mean of p1 over the greedy
fixture's rows and steps.

session_beam_seeds.json: per case and width the first seed at which, in float64, every adjacent gap among the top W + 1 candidates of every
source row and step is >= 1e-3, EOS is selected, the last step has a finished and a live beam, a back-pointer differs from the identity, and
the free-running float32 restatement makes the same choices (for W = 4 also: the W = 1 search keeps its gaps and its float32 agreement, and on
CARS the criterion separates the planted session faults wrong_source_row / sess_dropped at the margin's cap) -- with the smallest gap found.
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))


def gen_seeds(limit=400):
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import session_beam_ref as R
    found = {}
    for kind, tag in R.CASES:
        cs = R.load_case(kind, tag)
        found[R.name(kind, tag)] = {}
        for Wd in R.widths(kind, tag):
            if Wd == 1:
                continue
            for seed in range(1, limit):
                sd = R.perturbed(kind, tag, Wd, seed=seed)
                ok, gap = True, None
                for w in ((Wd, 1) if Wd == 4 else (Wd,)):
                    ref = R.decode(cs, sd, w)
                    free = R.decode(cs, sd, w, torch.float32)
                    cond = R.conditions(cs, sd, ref, free, w)
                    ok = ok and R.conditions_ok(cond, w)
                    gap = cond["min_gap"] if gap is None else gap
                    if not ok:
                        break
                if ok:
                    found[R.name(kind, tag)][str(Wd)] = [seed, gap]
                    print("%s %s W=%d: seed %d, smallest gap %.3g" % (kind, tag, Wd, seed, gap), flush=True)
                    break
            else:
                raise SystemExit("no seed below %d for %s %s W=%d" % (limit, kind, tag, Wd))
    with open(os.path.join(HERE, "session_beam_seeds.json"), "w") as f:
        json.dump(found, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    gen_seeds()
