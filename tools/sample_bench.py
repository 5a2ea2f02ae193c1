"""Seq2seq.decode_sample (csrc/sample.hip): the fused generator + Gumbel arg-max against the entry's plain form, against what the library offered
before it, and against the two decodes it stands next to.

Shape: scripts/recommender.sh of the reference, as tools/seq2seq_bench.py -- batch 64, source width 20, emsize 300, nhid 512, nlayers 1, general
attention, a source vocabulary of 100 000, tgt_vocab_size 30 000, max_len 20 -- at N = 4, 8 and 12 samples per source row (256, 512 and 768 decode rows).

    fused        decode_sample, the logits never leave the chip (sample_gen_kernel + sample_finish_kernel per step)
    plain        decode_sample with fuse_generator_argmax = False: fp32 GEMM into [rows, VT] logits + sample_row_kernel per step
    topk_fused   decode_sample(top_k = 4): nir_beam_gen_topk's fused form + sample_topk_select_kernel
    topk_plain   the same with fuse_generator_topk = False
    parent       what a user wrote before: per step an LSTM cell, the attention and linear_out on the library's operators, autograd.linear into
                 [rows, VT] logits, torch Gumbel noise, argmax, the token fed back through the lookup table -- a host loop of max_len steps
    beam         decode_beam at W = min(N, 8)
    greedy       decode of the same R rows (the source rows repeated N times): the sampling decode without its noise
Seeded data, --warmup calls, then the median of --iters device-timed calls (events), in --rounds alternating rounds; the medians of the rounds
and their spread are reported, and whether the faster of fused / plain wins by more than both spreads.

    python tools/sample_bench.py [--N 4,8,12] [--iters 10] [--warmup 3] [--rounds 3] [--json out.json]
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
    ap.add_argument("--max_len", type=int, default=20)
    ap.add_argument("--N", default="4,8,12")
    ap.add_argument("--top_k", type=int, default=4)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from context_attentive_ir_amd import autograd as A
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.constants import BOS
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import Recommender
    rng = np.random.default_rng(1)
    r = Recommender(default_args("SEQ2SEQ", emsize=a.emsize, nhid=a.nhid, nlayers=1, max_query_len=a.max_len, src_vocab_size=a.V, tgt_vocab_size=a.VT))
    fill_module_(r.network, 1013)
    r.cuda()
    net = r.network.eval()
    net.fuse_sample_max_rows = 1 << 30                       # `fused` is the fused form at every row count: the default's row cap is what is being measured
    lens = np.clip(rng.poisson(a.qmean, size=a.B), 1, a.ql).astype(np.int64)
    lens[0] = a.ql
    src = rng.integers(4, a.V, size=(a.B, a.ql), dtype=np.int64)
    src[np.arange(a.ql)[None] >= lens[:, None]] = 0
    srcd, lensd = torch.from_numpy(src).cuda(), torch.from_numpy(lens).cuda()
    lut = torch.from_numpy(rng.integers(4, a.V, size=a.VT, dtype=np.int64)).cuda()
    table = net.embedder.word_embeddings.table
    rnn, att = net.decoder.decoder.rnn, net.decoder.decoder.attn
    results = []
    for N in [int(v) for v in a.N.split(",")]:
        R = a.B * N
        W = min(N, 8)
        rep_src, rep_len = srcd.repeat(N, 1), lensd.repeat(N)

        def sample(top_k=0):
            return net.decode_sample(srcd, lensd, a.max_len, N, temperature=1.0, top_k=top_k, seed=7, tgt2src=lut)

        def parent():
            state, bank = net._encode_state(srcd, lensd)
            h, c = (s.repeat(N, 1).contiguous() for s in state)
            mem, ln = bank.repeat(N, 1, 1), lensd.repeat(N)
            mask = torch.arange(a.ql, device="cuda").unsqueeze(0) < ln.unsqueeze(1)
            tok = torch.full((R,), BOS, dtype=torch.int64, device="cuda")
            out = []
            for _ in range(a.max_len):
                h, c = torch._VF.lstm_cell(A.embed(tok, table), (h, c), rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)
                hq = h.unsqueeze(1)
                ctx = A.softmax_pool(net._align(hq, mem), mask, mem, mask_div=1).view(R, 1, -1)
                o = A.linear(torch.cat((ctx, hq), 2), att.linear_out.weight, None, act="tanh").view(R, -1)
                logits = A.linear(o, net.generator.weight, net.generator.bias)
                g = -torch.log(-torch.log(torch.rand_like(logits).clamp_(1e-7, 1 - 1e-7)))
                v = (logits + g).argmax(1)
                out.append(v)
                tok = lut[v]
            return torch.stack(out, 1)

        def beam():
            return net.decode_beam(srcd, lensd, a.max_len, W, tgt2src=lut)

        def greedy():
            return net.decode(rep_src, rep_len, a.max_len, None, None, tgt2src=lut)

        t = {k: [] for k in ("fused", "plain", "topk_fused", "topk_plain", "parent", "beam", "greedy")}
        with torch.no_grad():
            for _ in range(max(1, a.rounds)):                    # the paths alternate, so that drift of the machine meets all of them
                net.fuse_generator_argmax = net.fuse_generator_topk = True
                assert net._decoder_weights().struct.gen_frag
                t["fused"].append(timed(sample, a.iters, a.warmup))
                s_fused = sample()
                t["topk_fused"].append(timed(lambda: sample(a.top_k), a.iters, a.warmup))
                t["beam"].append(timed(beam, a.iters, a.warmup))
                t["greedy"].append(timed(greedy, a.iters, a.warmup))
                t["parent"].append(timed(parent, a.iters, a.warmup))
                net.fuse_generator_topk = False
                t["topk_plain"].append(timed(lambda: sample(a.top_k), a.iters, a.warmup))
                net.fuse_generator_argmax = False
                assert not net._decoder_weights().struct.gen_frag
                t["plain"].append(timed(sample, a.iters, a.warmup))
                s_plain = sample()
            net.fuse_generator_argmax = net.fuse_generator_topk = True
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: float(max(v) - min(v)) for k, v in t.items()}
        best, other = ("fused", "plain") if med["fused"] <= med["plain"] else ("plain", "fused")
        kbest, kother = ("topk_fused", "topk_plain") if med["topk_fused"] <= med["topk_plain"] else ("topk_plain", "topk_fused")
        out = dict(model="seq2seq_sample", B=a.B, QL=a.ql, N=N, rows=R, max_len=a.max_len, emsize=a.emsize, nhid=a.nhid, V=a.V, VT=a.VT, top_k=a.top_k,
                   beam_width=W, ms={k: round(v, 4) for k, v in med.items()}, spread_ms={k: round(v, 4) for k, v in spread.items()},
                   ms_rounds={k: [round(x, 4) for x in v] for k, v in t.items()},
                   faster_form=best, faster_wins_outside_spread=bool(max(t[best]) < min(t[other])),
                   faster_topk_form=kbest, faster_topk_wins_outside_spread=bool(max(t[kbest]) < min(t[kother])),
                   noise_ms_per_step=round((med["fused"] - med["greedy"]) / a.max_len, 4),
                   logits_bytes_not_written_per_step=R * a.VT * 4,
                   tokens_equal_fused_plain=float((s_fused["predictions"] == s_plain["predictions"]).float().mean()),
                   max_score_diff_fused_plain=float((s_fused["scores"] - s_plain["scores"]).abs().max()))
        print(json.dumps(out))
        results.append(out)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
