"""ACG: ms per sampling decode of `CopyRecommender.sample_extended` (csrc/sample.hip) at tools/acg_bench.py's shape -- nhid
512, tgt_vocab_size 10 000, general attention, reuse_copy_attn, emsize 300, a source vocabulary of 100 000, source width 20, CV = 22, max_len 20,
B 64 -- for N samples per row and top_k in {0, 4}:

    fused    the entry's fused generator form (sample_gen_kernel<.., PAD> + acg_sample_row_kernel; top_k > 0: the fused top-k lists + select)
    plain    the entry's plain form (fp32 GEMM into workspace logits + one workgroup per row)
    beam     `decode_beam` at W = min(N, 8) on the same batch (eager, like the others)
    greedy   the greedy decode of the same R = B N rows (the batch repeated N times, eager)
    user     what a user wrote before the entry existed (LSTM decoder, top_k 0 only): a host loop of max_len steps over the library's operators --
             cell, attention, `A.linear` into [rows, VT] logits with the PAD override, a softmax, the dense [rows, CV] copy distribution as a
             product with the one-hot map, the reference's per-row host collapse (seq2seq.py:162-171: index_add_ and a fill per row), torch
             Gumbel noise on log P / tau, argmax, the token fed back through the two tables.  Timed with --user_iters calls after one warm-up.

One JSON line: per (N, top_k) the median over --rounds alternating rounds of the median of --iters calls (CUDA events, after --warmup), the rounds
themselves, whether the fused and plain tokens agree, the share of copied words among the draws, and the sampler's cost over greedy per step.

    python tools/acg_sample_bench.py [--rnn_type LSTM|GRU] [--num_samples 4 8 12] [--B 64] [--iters 10] [--warmup 3] [--rounds 3] [--json out.json]
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
    ap.add_argument("--num_samples", type=int, nargs="+", default=[4, 8, 12])
    ap.add_argument("--top_k", type=int, nargs="+", default=[0, 4])
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--user_iters", type=int, default=3, help="timed calls of the `user` loop per round (0: leave it out)")
    ap.add_argument("--rounds", type=int, default=3, help="alternating repeats of the timings; the spread of their medians is reported")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from context_attentive_ir_amd import autograd as A
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.constants import BOS
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import CopyRecommender
    rng = np.random.default_rng(1)
    src_dict = [int(x) for x in rng.integers(4, a.V, size=a.V)]             # src_dict[tgt_dict[i]]: tgt_dict = identity
    kw = dict(emsize=a.emsize, nhid=a.nhid, nlayers=1, max_query_len=a.max_len, tgt_vocab_size=a.VT, rnn_type=a.rnn_type)
    acg = CopyRecommender(default_args("ACG", **kw), src_dict, list(range(a.VT)))
    fill_module_(acg.network, 1013)
    acg.cuda()
    acg.args.predict_graphs = False                                          # every path eager: a draw is never captured
    net = acg.network.eval()
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
    t = {k: torch.from_numpy(v).cuda() for k, v in dict(src=src, lens=lens, idx=idx, e2t=e2t, e2s=e2s).items()}

    def ex_of(rep):
        r = {k: v.repeat((rep,) + (1,) * (v.dim() - 1)) for k, v in t.items()}
        return dict(source_words=r["src"].unsqueeze(1), source_lens=r["lens"].unsqueeze(1), copy_src_map_idx=r["idx"], copy_ext2tgt=r["e2t"],
                    copy_ext2src=r["e2s"])
    ex1 = ex_of(1)
    table = net.embedder.word_embeddings.table
    rnn, att, cg = net.decoder.decoder.rnn, net.decoder.decoder.attn, net.copy_generator.linear_copy
    lut = torch.tensor(src_dict[:a.VT], dtype=torch.int64, device="cuda")   # tgt2src: tgt_dict is the identity
    blank = [[c for c in range(2, CV) if e2t[b, c] >= 0] for b in range(a.B)]
    blank_t = [torch.tensor([a.VT + c for c in bl], dtype=torch.int64, device="cuda") for bl in blank]           # built once per batch, as the
    fill_t = [torch.tensor([int(e2t[b, c]) for c in blank[b]], dtype=torch.int64, device="cuda") for b in range(a.B)]   # reference's collate does

    def user(N, tau=0.7):
        R = a.B * N
        state, bank = net._encode_state(t["src"], t["lens"])
        h, c = (s.repeat(N, 1).contiguous() for s in state)
        mem, ln = bank.repeat(N, 1, 1), t["lens"].repeat(N)
        mask = torch.arange(a.ql, device="cuda").unsqueeze(0) < ln.unsqueeze(1)
        onehot = torch.nn.functional.one_hot(t["idx"].repeat(N, 1), CV).float() * mask.unsqueeze(2)      # the reference's dense src_map [R, QL, CV]
        e2s_r = t["e2s"].repeat(N, 1)
        tok = torch.full((R,), BOS, dtype=torch.int64, device="cuda")
        out = []
        for _ in range(a.max_len):
            h, c = torch._VF.lstm_cell(A.embed(tok, table), (h, c), rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)
            hq = h.unsqueeze(1)
            align = net._align(hq, mem)
            ctx = A.softmax_pool(align, mask, mem, mask_div=1).view(R, 1, -1)
            o = A.linear(torch.cat((ctx, hq), 2), att.linear_out.weight, None, act="tanh").view(R, -1)
            attn = torch.softmax(align.view(R, -1).masked_fill(~mask, float("-inf")), 1)                   # reuse_copy_attn
            logits = A.linear(o, net.generator.weight, net.generator.bias)
            logits[:, 0] = -1e-20
            z = torch.sigmoid((o * cg.weight.view(1, -1)).sum(1, keepdim=True) + cg.bias)
            P = torch.cat(((1 - z) * torch.softmax(logits, 1), z * torch.bmm(attn.unsqueeze(1), onehot).squeeze(1)), 1)   # [R, VT + CV]
            for r in range(R):                                                                             # the reference's host collapse
                b = r % a.B
                if blank[b]:
                    P[r].index_add_(0, fill_t[b], P[r].index_select(0, blank_t[b]))
                    P[r].index_fill_(0, blank_t[b], 0.0)
            g = -torch.log(-torch.log(torch.rand_like(P).clamp_(1e-7, 1 - 1e-7)))
            v = (torch.log(P) / tau + g).argmax(1)
            out.append(v)
            tok = torch.where(v < a.VT, lut[v.clamp(max=a.VT - 1)], e2s_r.gather(1, (v - a.VT).clamp(min=0).unsqueeze(1)).squeeze(1))
        return torch.stack(out, 1)
    with_user = a.user_iters > 0 and a.rnn_type == "LSTM" and net.attn_type != "mlp" and net.reuse_copy_attn
    results = []
    with torch.no_grad():
        for N in a.num_samples:
            exN = ex_of(N)
            for K in a.top_k:
                draw = lambda: acg.sample_extended(ex1, N, temperature=0.7, top_k=K, seed=11)["prediction_ids"]      # noqa: E731
                beam = lambda: acg._predict_nbest_body(ex1, min(N, 8))["prediction_ids"]                              # noqa: E731
                greedy = lambda: acg._predict_body(exN)["prediction_ids"]                                             # noqa: E731
                rounds = {k: [] for k in ("fused", "plain", "beam", "greedy") + (("user",) if with_user and K == 0 else ())}
                for _ in range(max(1, a.rounds)):                # the paths alternate, so that drift of the machine meets all of them
                    net.fuse_generator_argmax = net.fuse_generator_topk = True
                    net.fuse_sample_max_rows = 1 << 30           # the cap is what this tool measures: off
                    rounds["fused"].append(timed(draw, a.iters, a.warmup))
                    p_fused = draw().clone()
                    net.fuse_generator_argmax = net.fuse_generator_topk = False
                    rounds["plain"].append(timed(draw, a.iters, a.warmup))
                    p_plain = draw().clone()
                    net.fuse_generator_argmax = net.fuse_generator_topk = True
                    rounds["beam"].append(timed(beam, a.iters, a.warmup))
                    rounds["greedy"].append(timed(greedy, a.iters, a.warmup))
                    if "user" in rounds:
                        rounds["user"].append(timed(lambda: user(N), a.user_iters, 1))
                med = {k: float(np.median(v)) for k, v in rounds.items()}
                results.append(dict(N=N, top_k=K, rows=a.B * N, beam_width=min(N, 8), **{k + "_ms": round(v, 4) for k, v in med.items()},
                                    **{k + "_ms_rounds": [round(x, 4) for x in v] for k, v in rounds.items()},
                                    sampler_over_greedy_ms_per_step=round((med["fused"] - med["greedy"]) / a.max_len, 5),
                                    tokens_equal_fused_plain=float((p_fused == p_plain).float().mean()),
                                    copied_share=float((p_fused >= a.VT).float().mean())))
    out = dict(model="acg_sample", rnn_type=a.rnn_type, B=a.B, QL=a.ql, CV=CV, emsize=a.emsize, nhid=a.nhid, V=a.V, VT=a.VT, max_len=a.max_len,
               temperature=0.7, iters=a.iters, warmup=a.warmup, results=results)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
