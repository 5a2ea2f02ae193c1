"""ACG.score_extended (csrc/score.hip: the PAD-substituting generator form + acg_score_finish_kernel): the fused form against
the entry's plain form and against what the library offered before it, the eval-mode composition of forward()'s operators.

Shape: tools/score_bench.py's -- batch 64, source width 20, emsize 300, nhid 512, nlayers 1, general attention,
reuse_copy_attn, a source vocabulary of 100 000, tgt_vocab_size 30 000, candidates of TL = 20 tokens -- with a dynamic dictionary of CV = 22
slots per row, at N = 20 candidates per source (24 320 decoder rows) and N = 1 (1 216 rows).  A third of the candidate tokens are copies: slot
ids, collapsed or not.

Timed on the SAME rows, and the whole call with each:
    fused    nir_acg_score_gen_target with the generator fragments: neither logits nor a copy distribution leave the chip
    plain    the same entry without them: fp32 GEMM into a bounded logits buffer, one workgroup per row, the same finish kernel
    parent   forward()'s operators in eval mode: autograd.linear into [rows, VT] logits, the [rows, QL] hit mask and its sum, A.copy_loss rows;
             its whole call runs behind the glue front, as forward() composes it (the generator part is timed on the same rows as the others)
             (N = 20 writes 2.9 GB of logits: --parent_max_rows skips it where that does not fit)
and the front twice: ONE nir_tf_attend over all rows (front) against _align + masked softmax + softmax_pool (front_glue).
Seeded data, --warmup calls, then the median of --iters device-timed calls (events), in --rounds alternating rounds; the medians of the rounds
and their spread are reported, and whether the faster of fused / plain wins by more than the spread of the rounds.

    python tools/acg_score_bench.py [--N 20,1] [--iters 10] [--warmup 3] [--rounds 3] [--json out.json]
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
    ap.add_argument("--cv", type=int, default=22)
    ap.add_argument("--qmean", type=float, default=8)
    ap.add_argument("--V", type=int, default=100000)
    ap.add_argument("--VT", type=int, default=30000)
    ap.add_argument("--emsize", type=int, default=300)
    ap.add_argument("--nhid", type=int, default=512)
    ap.add_argument("--TL", type=int, default=20)
    ap.add_argument("--N", default="20,1")
    ap.add_argument("--parent_max_rows", type=int, default=1 << 15, help="the parent composition runs up to this many rows (its logits are rows x VT x 4 bytes)")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from context_attentive_ir_amd import autograd as A
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.constants import BOS, EOS, PAD
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import CopyRecommender
    rng = np.random.default_rng(1)
    r = CopyRecommender(default_args("ACG", emsize=a.emsize, nhid=a.nhid, nlayers=1, max_query_len=a.TL, src_vocab_size=a.V, tgt_vocab_size=a.VT,
                                     attn_type="general", reuse_copy_attn=True))
    fill_module_(r.network, 1013)
    r.cuda()
    net = r.network.eval()
    B, QL, CV, VT = a.B, a.ql, a.cv, a.VT
    lens = np.clip(rng.poisson(a.qmean, size=B), 1, QL).astype(np.int64)
    lens[0] = QL
    src = rng.integers(4, a.V, size=(B, QL), dtype=np.int64)
    src[np.arange(QL)[None] >= lens[:, None]] = 0
    idx = np.zeros((B, QL), np.int64)
    e2t = np.full((B, CV), -1, np.int64)
    e2s = np.ones((B, CV), np.int64)
    for b in range(B):                                                  # a dictionary of the row's words behind the four specials, a word in three repeated
        slots = 4 + rng.integers(0, max(1, (2 * int(lens[b]) + 2) // 3), size=int(lens[b]))
        idx[b, :lens[b]] = np.minimum(slots, CV - 1)
        e2s[b] = rng.integers(4, a.V, size=CV)
        hit = rng.random(CV) < 0.5                                      # half of the slots collapse onto a target word
        e2t[b, hit] = rng.integers(4, VT, size=int(hit.sum()))
        e2t[b, :2] = -1
    dev = lambda x: torch.from_numpy(x).cuda()                          # noqa: E731
    srcd, lensd, idxd, e2td, e2sd = dev(src), dev(lens), dev(idx), dev(e2t), dev(e2s)
    lut = dev(rng.integers(4, a.V, size=VT, dtype=np.int64))
    results = []
    for N in [int(v) for v in a.N.split(",")]:
        clen = np.clip(rng.poisson(a.qmean, size=(B, N)), 1, a.TL - 2)
        cand = rng.integers(4, VT, size=(B, N, a.TL), dtype=np.int64)
        copied = rng.random(cand.shape) < 1.0 / 3
        cand[copied] = (VT + rng.integers(2, CV, size=cand.shape))[copied]
        pos = np.arange(a.TL)[None, None]
        cand[pos == clen[..., None] + 1] = EOS
        cand[pos > clen[..., None] + 1] = PAD
        cand[..., 0] = BOS
        candd = dev(cand)
        T = a.TL - 1
        rows = B * N * T

        def front():
            return net._extended_front(srcd, lensd, candd, None, None, None, lut, None, None, None, None, idxd, e2td, e2sd)

        def whole():
            return net.score_extended(srcd, lensd, candd, tgt2src=lut, src_map_idx=idxd, ext2tgt=e2td, ext2src=e2sd)

        def parent_gen(dec_out, a_copy):
            """forward()'s tail on the teacher-forced rows: logits, switch, the hit mask and its mass, the criterion's rows"""
            target = candd[..., 1:].reshape(B, N * T)
            al = torch.where(target >= VT, target - VT, torch.zeros_like(target))
            tseq = torch.where(target >= VT, torch.ones_like(target), target)
            hit = (idxd.unsqueeze(1) == al.unsqueeze(2)).to(a_copy.dtype)
            mass = (a_copy.view(B, N * T, QL) * hit).sum(2)
            cg = net.copy_generator.linear_copy
            switch = (dec_out * cg.weight.view(1, -1)).sum(1) + cg.bias
            logits = A.linear(dec_out, net.generator.weight, net.generator.bias)
            return A.copy_loss(logits, switch, mass.reshape(-1), tseq.reshape(-1), al.reshape(-1), False)

        with_parent = rows <= a.parent_max_rows
        t = {k: [] for k in ("front", "front_glue", "fused_gen", "plain_gen", "parent_gen", "fused", "plain", "parent")}
        with torch.no_grad():
            for _ in range(max(1, a.rounds)):                    # the paths alternate, so that drift of the machine meets all of them
                net.fuse_generator_argmax = net.fuse_teacher_front = True
                c = front()
                assert c[-1].keep.get("gen_frag") is not None
                gen = lambda: net._score_extended_rows(*c)                       # noqa: E731
                t["front"].append(timed(front, a.iters, a.warmup))
                t["fused_gen"].append(timed(gen, a.iters, a.warmup))
                t["fused"].append(timed(whole, a.iters, a.warmup))
                s_fused = whole()["scores"].clone()
                if with_parent:
                    t["parent_gen"].append(timed(lambda: parent_gen(c[0], c[1]), a.iters, a.warmup))
                net.fuse_teacher_front = False
                t["front_glue"].append(timed(front, a.iters, a.warmup))
                if with_parent:                                  # what the library offered before: the glue front AND forward()'s tail
                    t["parent"].append(timed(lambda: parent_gen(*front()[:2]), a.iters, a.warmup))
                s_glue = whole()["scores"].clone()
                net.fuse_teacher_front, net.fuse_generator_argmax = True, False
                c = front()
                assert c[-1].keep.get("gen_frag") is None
                t["plain_gen"].append(timed(gen, a.iters, a.warmup))
                t["plain"].append(timed(whole, a.iters, a.warmup))
                s_plain = whole()["scores"].clone()
            net.fuse_generator_argmax = True
        t = {k: v for k, v in t.items() if v}
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: float(max(v) - min(v)) for k, v in t.items()}
        best, other = ("fused", "plain") if med["fused_gen"] <= med["plain_gen"] else ("plain", "fused")
        fin = torch.isfinite(s_fused) & torch.isfinite(s_plain) & torch.isfinite(s_glue)
        out = dict(model="acg_score", B=B, QL=QL, CV=CV, N=N, TL=a.TL, rows=rows, emsize=a.emsize, nhid=a.nhid, V=a.V, VT=VT,
                   ms={k: round(v, 4) for k, v in med.items()}, spread_ms={k: round(v, 4) for k, v in spread.items()},
                   ms_rounds={k: [round(x, 4) for x in v] for k, v in t.items()}, faster_generator=best,
                   faster_wins_outside_spread=bool(max(t[best + "_gen"]) < min(t[other + "_gen"])),
                   attend_front_faster_outside_spread=bool(max(t["front"]) < min(t["front_glue"])),
                   logits_bytes_not_written=rows * VT * 4, parent_timed=with_parent, finite_scores=int(fin.sum()), sequences=B * N,
                   max_score_diff_fused_plain=float((s_fused - s_plain)[fin].abs().max()), max_score_diff_attend_glue=float((s_fused - s_glue)[fin].abs().max()))
        print(json.dumps(out))
        results.append(out)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
