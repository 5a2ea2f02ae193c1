"""Session models: `Multitask.predict_beam` (csrc/beam.hip: nir_beam_cars_decode / nir_beam_plain_decode) at the benchmark's C3 shape -- 16
sessions of 7 queries (Bd = 96 decode rows), q_len 4, 10 candidates of 64 tokens, a source vocabulary of 100 000 and the default target
vocabulary and max_query_len, detinit weights, synthetic ids.

Per width of --beam_sizes and per model of --models it times, graph replay, CUDA events, median of --iters after --warmup, in --rounds
alternating rounds: predict_beam with the fused generator + top-k kernel forced on (fuse_topk_max_rows lifted); the same with the plain
generator (fp32 GEMM into [R, VT] logits + one workgroup per row); and the greedy predict() of the same batch next to them.  Prints one JSON line per (model, width); --json appends them
to a file.

    python tools/session_beam_bench.py [--models CARS,MNSRF] [--beam_sizes 4,8] [--iters 20] [--warmup 5] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from dssm_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="CARS,MNSRF")
    ap.add_argument("--beam_sizes", default="4,8")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--session", type=int, default=7)
    ap.add_argument("--cands", type=int, default=10)
    ap.add_argument("--qlen", type=int, default=4)
    ap.add_argument("--dlen", type=int, default=64)
    ap.add_argument("--vocab", type=int, default=100000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating repeats of the timings; the spread of their medians is reported")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from context_attentive_ir_amd import synth
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import Multitask
    ex = {k: v.cuda() for k, v in synth.session_batch(a.batch, a.session, a.cands, a.qlen, a.dlen, a.vocab, 1013).items()}
    lines = []
    for kind in a.models.split(","):
        w = Multitask(default_args(kind, src_vocab_size=a.vocab))
        fill_module_(w.network, 1013)
        w.cuda()
        w.id_check_interval = 0
        w.predict_graph_min_calls = 2          # the timed calls replay the captured graph
        net = w.network.eval()
        net.fuse_topk_max_rows = 1 << 30       # both generator forms at every width: the default picks between them by the beam rows
        greedy = lambda: w.predict(ex)["predictions"]                            # noqa: E731
        for W in (int(x) for x in a.beam_sizes.split(",")):
            beam = lambda: w.predict_beam(ex, W)["prediction_ids"]               # noqa: E731
            r = dict(fused=[], plain=[], greedy=[])
            toks = {}
            with torch.no_grad():
                for _ in range(max(1, a.rounds)):        # the forms alternate, so that drift of the machine meets all of them
                    net.fuse_generator_topk = True
                    r["fused"].append(timed(beam, a.iters, a.warmup))
                    toks["fused"] = beam().clone()
                    net.fuse_generator_topk = False
                    r["plain"].append(timed(beam, a.iters, a.warmup))
                    toks["plain"] = beam().clone()
                    net.fuse_generator_topk = True
                    r["greedy"].append(timed(greedy, a.iters, a.warmup))
            med = {k: float(np.median(v)) for k, v in r.items()}
            out = dict(model=kind.lower() + "_beam", beam_size=W, batch=a.batch, session=a.session, decode_rows=a.batch * (a.session - 1), qlen=a.qlen,
                       vocab=a.vocab, tgt_vocab=int(w.args.tgt_vocab_size), max_len=int(w.args.max_query_len),
                       ms_per_predict_beam=round(med["fused"], 4), plain_topk_ms=round(med["plain"], 4),
                       greedy_predict_ms=round(med["greedy"], 4), rounds={k: [round(x, 4) for x in v] for k, v in r.items()},
                       fused_topk_wins_outside_spread=bool(max(r["fused"]) < min(r["plain"])),
                       plain_topk_wins_outside_spread=bool(max(r["plain"]) < min(r["fused"])),
                       tokens_equal_fused_plain=float((toks["fused"] == toks["plain"]).float().mean()))
            print(json.dumps(out), flush=True)
            lines.append(out)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()
