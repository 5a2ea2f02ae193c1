"""Corpus retrieval: ms per search of `nir_retrieve_topk` (csrc/retrieve.hip) over an index of M unit rows of D = 128 components,
for B queries and the k best, three ways that alternate in one process:

    fused    the entry's fused form (score tiles on the fp32 matrix pipe, selection on chip, the chunks' lists merged; no [B, M] buffer)
    plain    the entry's own plain form (the same score tiles written to a [M, B] matrix in the workspace, the same selection reading it back)
    torch    what a user of the library without the entry writes: torch.matmul of pre-normalised operands into [B, M] + torch.topk

One JSON line: per (M, B, k) the median over --rounds alternating rounds of the median of --iters calls (device events, after --warmup), the rounds
themselves, the achieved index-stream rate M D 4 / t against the 6.3 TB/s copy rate, the achieved 2 B M D / t against the 157 TFLOP/s of the fp32
matrix pipe, which of the two floors is the larger one for the shape, and whether fused, plain and torch return the same documents.  Seeded
representations.  Kernel times come from a run of their own:

    rocprofv3 --kernel-trace --stats -d prof_out -- python tools/retrieve_bench.py --M 1000000 --B 64 --k 100 --iters 5 --rounds 1 --ways fused plain

    python tools/retrieve_bench.py [--M 1000000 10000000] [--B 1 16 64] [--k 10 100] [--D 128] [--iters 20] [--warmup 3] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from dssm_bench import timed  # noqa: E402

HBM_BYTES_PER_S, MATRIX_FLOPS = 6.3e12, 157e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, nargs="+", default=[10 ** 6, 10 ** 7])
    ap.add_argument("--B", type=int, nargs="+", default=[1, 16, 64])
    ap.add_argument("--k", type=int, nargs="+", default=[10, 100])
    ap.add_argument("--D", type=int, default=128)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3, help="alternating repeats of the timings; the spread of their medians is reported")
    ap.add_argument("--ways", nargs="+", default=["fused", "plain", "torch"], choices=["fused", "plain", "torch"])
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from context_attentive_ir_amd import retrieval as X
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(1013)
    results = []
    with torch.no_grad():
        for M in a.M:
            index = X.DocumentIndex(a.D, dev, capacity=M)
            plainrows = torch.empty(M, a.D, device=dev) if "torch" in a.ways else None
            for lo in range(0, M, 1 << 20):                          # seeded raw representations, added in pieces
                reps = torch.randn(min(1 << 20, M - lo), a.D, device=dev, generator=gen)
                index.add(reps)
                if plainrows is not None:
                    plainrows[lo:lo + reps.shape[0]] = reps / reps.norm(dim=1, keepdim=True).clamp_min(1e-8)
            for B in a.B:
                q = torch.randn(B, a.D, device=dev, generator=gen)
                qn = q / q.norm(dim=1, keepdim=True).clamp_min(1e-8)
                for k in a.k:
                    fns = {"fused": lambda: index.search(q, k, form="fused"), "plain": lambda: index.search(q, k, form="plain"),
                           "torch": lambda: torch.topk(torch.matmul(qn, plainrows.t()), k, dim=1)}
                    rounds = {w: [] for w in a.ways}
                    for _ in range(max(1, a.rounds)):                # the ways alternate, so that drift of the machine meets all of them
                        for w in a.ways:
                            rounds[w].append(timed(fns[w], a.iters, a.warmup))
                    med = {w: float(np.median(v)) for w, v in rounds.items()}
                    ids = {w: fns[w]()[1].long() for w in a.ways}
                    same = {w: float((ids[w] == ids[a.ways[0]]).float().mean()) for w in a.ways[1:]}
                    floor_mem, floor_mm = M * a.D * 4 / HBM_BYTES_PER_S * 1e3, 2.0 * B * M * a.D / MATRIX_FLOPS * 1e3
                    row = dict(M=M, B=B, k=k, D=a.D, floor_stream_ms=round(floor_mem, 4), floor_matrix_ms=round(floor_mm, 4),
                               bound="stream" if floor_mem >= floor_mm else "matrix", same_ids_as_first=same)
                    for w in a.ways:
                        t = med[w] * 1e-3
                        row[w + "_ms"] = round(med[w], 4)
                        row[w + "_ms_rounds"] = [round(x, 4) for x in rounds[w]]
                        row[w + "_stream_share"] = round(M * a.D * 4 / t / HBM_BYTES_PER_S, 4)
                        row[w + "_matrix_share"] = round(2.0 * B * M * a.D / t / MATRIX_FLOPS, 4)
                    results.append(row)
                    print(json.dumps(row), file=sys.stderr, flush=True)
            del index, plainrows
            torch.cuda.empty_cache()
    out = dict(model="retrieve", D=a.D, iters=a.iters, warmup=a.warmup, rounds=a.rounds, results=results)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
