"""ACG: ms per greedy decode of `CopyRecommender.predict` (csrc/acg.hip) with the fused generator statistics and with the plain form (fp32
GEMM + row statistics), next to `Recommender.predict` of Seq2seq at the same shapes -- the yardstick for what the copy step adds.

Shape: ACG's table (nhid 512, tgt_vocab_size 10 000, general attention, reuse_copy_attn), emsize 300, a source vocabulary of 100 000, source
width 20 and max_len 20 as in tools/seq2seq_bench.py.  Every row's dynamic dictionary is built from its own source words (CV = QL + 2, as
the reference's loader guarantees); words of the first tgt_vocab_size source ids are target words too, so part of every dictionary collapses.

Prints one JSON line: ms per batch (median of --iters, CUDA events, after --warmup; the calls replay the captured predict graph) per round of
--rounds alternating rounds and the medians over the rounds, whether the fused and plain tokens agree, and the share of copied words.

--rnn_type GRU builds ACGGRU / Seq2seqGRU (csrc/gru_step.hip) instead.

--beam_size W times `CopyRecommender.predict_nbest(ex, W)` (csrc/beam.hip) instead: the fused generator top-k against
the plain form (fp32 GEMM + row top-k) and against the greedy `predict` of the same model, in the same alternating rounds.

    python tools/acg_bench.py [--rnn_type LSTM|GRU] [--beam_size W] [--B 64] [--iters 20] [--warmup 5] [--rounds 3] [--json out.json]
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
    ap.add_argument("--VT", type=int, default=10000)
    ap.add_argument("--emsize", type=int, default=300)
    ap.add_argument("--nhid", type=int, default=512)
    ap.add_argument("--max_len", type=int, default=20)
    ap.add_argument("--rnn_type", default="LSTM", choices=["LSTM", "GRU"])
    ap.add_argument("--beam_size", type=int, default=0, help="> 0: time predict_nbest at this width (fused / plain top-k, greedy next to them)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating repeats of the timings; the spread of their medians is reported")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import CopyRecommender, Recommender
    rng = np.random.default_rng(1)
    src_dict = [int(x) for x in rng.integers(4, a.V, size=a.V)]             # src_dict[tgt_dict[i]]: tgt_dict = identity
    kw = dict(emsize=a.emsize, nhid=a.nhid, nlayers=1, max_query_len=a.max_len, tgt_vocab_size=a.VT, rnn_type=a.rnn_type)
    acg = CopyRecommender(default_args("ACG", **kw), src_dict, list(range(a.VT)))
    s2s = Recommender(default_args("SEQ2SEQ", **kw), src_dict, list(range(a.VT)))
    for r in (acg, s2s):
        fill_module_(r.network, 1013)
        r.cuda()
        r.predict_graph_min_calls = 2      # the timed calls replay the captured graph
        r.network.eval()
    lens = np.clip(rng.poisson(a.qmean, size=a.B), 1, a.ql).astype(np.int64)
    lens[0] = a.ql
    # half of the source words are target words too (ids below VT): their slots collapse
    src = np.where(rng.random((a.B, a.ql)) < 0.5, rng.integers(4, a.VT, size=(a.B, a.ql)), rng.integers(a.VT, a.V, size=(a.B, a.ql))).astype(np.int64)
    src[np.arange(a.ql)[None] >= lens[:, None]] = 0
    CV = a.ql + 2
    idx = np.zeros((a.B, a.ql), np.int64)
    e2t, e2s = np.full((a.B, CV), -1, np.int64), np.ones((a.B, CV), np.int64)
    for b in range(a.B):                                                     # the row's dictionary: PAD, UNK, then its words in order of appearance
        slot = {}
        for j in range(int(lens[b])):
            w = int(src[b, j])
            c = slot.setdefault(w, 2 + len(slot))
            idx[b, j] = c
            e2s[b, c] = w
            e2t[b, c] = w if w < a.VT else -1
    ex = dict(source_words=torch.from_numpy(src).unsqueeze(1).cuda(), source_lens=torch.from_numpy(lens).unsqueeze(1).cuda())
    exc = dict(ex, copy_src_map_idx=torch.from_numpy(idx).cuda(), copy_ext2tgt=torch.from_numpy(e2t).cuda(), copy_ext2src=torch.from_numpy(e2s).cuda())

    def copy():
        return acg.predict(exc)["prediction_ids"]

    def plain_s2s():
        return s2s.predict(ex)["prediction_ids"]

    if a.beam_size > 0:
        return beam(a, acg, exc, copy, CV)
    with torch.no_grad():
        fused_r, plain_r, s2s_r = [], [], []
        for _ in range(max(1, a.rounds)):                    # the paths alternate, so that drift of the machine meets all of them
            acg.network.fuse_generator_argmax = True         # (part of the graph cache's key: the next call captures the other path)
            fused_r.append(timed(copy, a.iters, a.warmup))
            p_fused = copy().clone()
            acg.network.fuse_generator_argmax = False
            plain_r.append(timed(copy, a.iters, a.warmup))
            p_plain = copy().clone()
            s2s_r.append(timed(plain_s2s, a.iters, a.warmup))
    fused, plain, base = (float(np.median(v)) for v in (fused_r, plain_r, s2s_r))
    out = dict(model="acg", rnn_type=a.rnn_type, B=a.B, QL=a.ql, CV=CV, emsize=a.emsize, nhid=a.nhid, V=a.V, VT=a.VT, max_len=a.max_len,
               ms_per_batch=round(fused, 4), plain_ms_per_batch=round(plain, 4), seq2seq_ms_per_batch=round(base, 4),
               ms_rounds=[round(v, 4) for v in fused_r], plain_ms_rounds=[round(v, 4) for v in plain_r], seq2seq_ms_rounds=[round(v, 4) for v in s2s_r],
               copy_step_ms=round(fused - base, 4), tokens_equal_fused_plain=float((p_fused == p_plain).float().mean()),
               copied_share=float((p_fused >= a.VT).float().mean()))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


def beam(a, acg, exc, greedy, CV):
    W = a.beam_size

    def nbest():
        return acg.predict_nbest(exc, W)["prediction_ids"]

    with torch.no_grad():
        fused_r, plain_r, greedy_r = [], [], []
        for _ in range(max(1, a.rounds)):                    # the paths alternate, so that drift of the machine meets all of them
            acg.network.fuse_generator_topk = True           # (part of the graph cache's key: the next call captures the other path)
            fused_r.append(timed(nbest, a.iters, a.warmup))
            p_fused = nbest().clone()
            acg.network.fuse_generator_topk = False
            plain_r.append(timed(nbest, a.iters, a.warmup))
            p_plain = nbest().clone()
            acg.network.fuse_generator_topk = True
            greedy_r.append(timed(greedy, a.iters, a.warmup))
    fused, plain, base = (float(np.median(v)) for v in (fused_r, plain_r, greedy_r))
    out = dict(model="acg_beam", rnn_type=a.rnn_type, beam_size=W, B=a.B, QL=a.ql, CV=CV, emsize=a.emsize, nhid=a.nhid, V=a.V, VT=a.VT, max_len=a.max_len,
               ms_per_batch=round(fused, 4), plain_ms_per_batch=round(plain, 4), greedy_ms_per_batch=round(base, 4),
               ms_rounds=[round(v, 4) for v in fused_r], plain_ms_rounds=[round(v, 4) for v in plain_r], greedy_ms_rounds=[round(v, 4) for v in greedy_r],
               tokens_equal_fused_plain=float((p_fused == p_plain).float().mean()), copied_share=float((p_fused >= a.VT).float().mean()))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
