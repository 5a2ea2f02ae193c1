"""Seq2seq.score_candidates (csrc/score.hip): the fused generator log-likelihood against the entry's plain form and against what the library
offered before it, the eval-mode composition of the training loss.

Shape: scripts/recommender.sh of the reference, as tools/seq2seq_bench.py -- batch 64, source width 20, emsize 300, nhid 512, nlayers 1, general
attention, a source vocabulary of 100 000, tgt_vocab_size 30 000, candidates of TL = 20 tokens -- with N = 20 candidates per source (the ranking
protocol of the HRED / MNSRF papers: 24 320 decoder rows) and N = 1 (dev-set perplexity: 1 216 rows).

Three ways to turn the decoder rows into token log-probabilities, timed on the SAME rows, and the whole call with each:
    fused    nir_score_gen_target with the generator fragments: the logits never leave the chip
    plain    nir_score_gen_target without them: fp32 GEMM into a bounded logits buffer, row chunk by row chunk, one workgroup per row behind it
    parent   autograd.linear -> nir_softmax_nll_ent_fwd over [rows, VT] logits (--parent_chunk R: in chunks of R rows)
Seeded data, --warmup calls, then the median of --iters device-timed calls (events), in --rounds alternating rounds; the medians of the
rounds and their spread are reported, and whether the faster of fused / plain wins by more than both spreads.  The fused kernel's MFMA
rate comes from the operations it issues: three 16x16x32 products per block, 3 * 2 * rows * 16 ceil(VT / 16) * K.

    python tools/score_bench.py [--N 20,1] [--iters 10] [--warmup 3] [--rounds 3] [--json out.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--ql", type=int, default=20)
    ap.add_argument("--qmean", type=float, default=8)
    ap.add_argument("--V", type=int, default=100000)
    ap.add_argument("--VT", type=int, default=30000)
    ap.add_argument("--emsize", type=int, default=300)
    ap.add_argument("--nhid", type=int, default=512)
    ap.add_argument("--TL", type=int, default=20)
    ap.add_argument("--N", default="20,1")
    ap.add_argument("--parent_chunk", type=int, default=0, help="rows per chunk of the parent composition (0: all rows at once)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from context_attentive_ir_amd import autograd as A
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.constants import BOS, EOS, PAD
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.multitask import suggest
    from context_attentive_ir_amd.wrappers import Recommender
    rng = np.random.default_rng(1)
    r = Recommender(default_args("SEQ2SEQ", emsize=a.emsize, nhid=a.nhid, nlayers=1, max_query_len=a.TL, src_vocab_size=a.V, tgt_vocab_size=a.VT))
    fill_module_(r.network, 1013)
    r.cuda()
    net = r.network.eval()
    lens = np.clip(rng.poisson(a.qmean, size=a.B), 1, a.ql).astype(np.int64)
    lens[0] = a.ql
    src = rng.integers(4, a.V, size=(a.B, a.ql), dtype=np.int64)
    src[np.arange(a.ql)[None] >= lens[:, None]] = 0
    srcd, lensd = torch.from_numpy(src).cuda(), torch.from_numpy(lens).cuda()
    lut = torch.from_numpy(rng.integers(4, a.V, size=a.VT, dtype=np.int64)).cuda()
    results = []
    for N in [int(v) for v in a.N.split(",")]:
        clen = np.clip(rng.poisson(a.qmean, size=(a.B, N)), 1, a.TL - 2)
        cand = rng.integers(4, a.VT, size=(a.B, N, a.TL), dtype=np.int64)
        pos = np.arange(a.TL)[None, None]
        cand[pos == clen[..., None] + 1] = EOS
        cand[pos > clen[..., None] + 1] = PAD
        cand[..., 0] = BOS
        candd = torch.from_numpy(cand).cuda()
        rows = a.B * N * (a.TL - 1)

        def front():
            return net._candidate_rows(srcd, lensd, candd, None, None, None, lut)

        def whole():
            return net.score_candidates(srcd, lensd, candd, tgt2src=lut)

        def parent_gen(dec_out, w):
            x, t = dec_out.reshape(rows, -1), candd[..., 1:].reshape(-1)
            ch = a.parent_chunk if a.parent_chunk > 0 else rows
            nll = [A._SuggestLossRows.apply(A.linear(x[r0:r0 + ch], w.keep["gen_w"], w.keep["gen_b"]), t[r0:r0 + ch], PAD)[0] for r0 in range(0, rows, ch)]
            lp = -torch.cat(nll).view(a.B * N, a.TL - 1)
            sc, ln = torch.empty(a.B * N, device="cuda"), torch.empty(a.B * N, dtype=torch.int64, device="cuda")
            from context_attentive_ir_amd import lib
            lib.check(lib.load().nir_score_sequences(lib.ptr(lp), lib.ptr(t), a.B * N, a.TL - 1, PAD, EOS, lib.ptr(sc), lib.ptr(ln), lib.stream()),
                      "nir_score_sequences")
            return sc

        t = {k: [] for k in ("front", "fused_gen", "plain_gen", "parent_gen", "fused", "plain", "parent")}
        with torch.no_grad():
            for _ in range(max(1, a.rounds)):                    # the paths alternate, so that drift of the machine meets all of them
                net.fuse_generator_argmax = True
                dec_out, cd, w = front()
                assert w.keep.get("gen_frag") is not None
                gen = lambda: suggest.score_rows(net, dec_out, cd, w.keep["gen_w"], w.keep["gen_b"], w.keep.get("gen_frag"))      # noqa: E731
                t["front"].append(timed(front, a.iters, a.warmup))
                t["fused_gen"].append(timed(gen, a.iters, a.warmup))
                t["fused"].append(timed(whole, a.iters, a.warmup))
                s_fused = whole()["scores"].clone()
                t["parent_gen"].append(timed(lambda: parent_gen(dec_out, w), a.iters, a.warmup))
                t["parent"].append(timed(lambda: parent_gen(*front()[::2]), a.iters, a.warmup))
                s_parent = parent_gen(dec_out, w).view(a.B, N).clone()
                net.fuse_generator_argmax = False
                dec_out, cd, w = front()
                assert w.keep.get("gen_frag") is None
                t["plain_gen"].append(timed(gen, a.iters, a.warmup))
                t["plain"].append(timed(whole, a.iters, a.warmup))
                s_plain = whole()["scores"].clone()
            net.fuse_generator_argmax = True
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: float(max(v) - min(v)) for k, v in t.items()}
        ops = 3 * 2 * rows * 16 * ((a.VT + 15) // 16) * a.nhid
        best, other = ("fused", "plain") if med["fused_gen"] <= med["plain_gen"] else ("plain", "fused")
        out = dict(model="seq2seq_score", B=a.B, QL=a.ql, N=N, TL=a.TL, rows=rows, emsize=a.emsize, nhid=a.nhid, V=a.V, VT=a.VT,
                   ms={k: round(v, 4) for k, v in med.items()}, spread_ms={k: round(v, 4) for k, v in spread.items()},
                   ms_rounds={k: [round(x, 4) for x in v] for k, v in t.items()},
                   fused_mfma_tflops=round(ops / (med["fused_gen"] * 1e-3) / 1e12, 1), faster_generator=best,
                   faster_wins_outside_spread=bool(max(t[best + "_gen"]) < min(t[other + "_gen"])),
                   logits_bytes_not_written=rows * a.VT * 4,
                   max_score_diff_fused_plain=float((s_fused - s_plain).abs().max()), max_score_diff_fused_parent=float((s_fused - s_parent).abs().max()))
        print(json.dumps(out))
        results.append(out)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
