"""CARS.score_candidates (csrc/tf_attend.hip): the grouped teacher-forced attention in its fused form against its plain form and against
what the library offered before it, the attention of the train-mode forward (`_forward_train`: linear_in over the decoder rows, the
[Bd, N (TL-1), QL, HD] broadcast product, autograd.softmax_pool).

Shape: the reference's CARS script -- 32 sessions of 6 queries (160 decode rows), query width 10, candidates of TL = 10 tokens -- with HD / P /
VT from config.py's defaults (512 / 256 / 30 000) and N = 20 candidates per decode row (the ranking protocol of the papers: 28 800 decoder
rows) and N = 1 (dev-set perplexity: 1 440 rows).  The decoder's inputs (states, encoded queries, session pools) are seeded data of the sizes
the encoder produces: the bench times the scorer, not the encoder in front of it.

Three ways from the decoder states to cat = [ctx ; h], timed on the SAME rows -- the attention kernel alone ("attend"), with the products that
feed it ("attention": the two bank GEMMs for the entry's forms; the bank GEMM, linear_in over all rows and the broadcast product for the
parent's) -- and the whole call with each:
    fused    nir_tf_attend, the banks staged once per 64-row block as fp16 term planes
    plain    nir_tf_attend under exact_f32: one wave per row, fp32
    parent   _forward_train's composition
Seeded data, --warmup calls, then the median of --iters device-timed calls (events), in --rounds alternating rounds; the medians of the
rounds and their spread are reported, and whether the faster of fused / plain wins by more than both spreads.

    python tools/session_score_bench.py [--N 20,1] [--iters 10] [--warmup 3] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

os.environ.setdefault("NIR_DEBUG_TUNABLES", "1")          # the plain form of a fusable shape is reached through the debug tunable exact_f32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from dssm_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=32)
    ap.add_argument("--S", type=int, default=6)
    ap.add_argument("--ql", type=int, default=10)
    ap.add_argument("--qmean", type=float, default=4)
    ap.add_argument("--V", type=int, default=50000)
    ap.add_argument("--TL", type=int, default=10)
    ap.add_argument("--N", default="20,1")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    ap.add_argument("--lib", default="", help="variant library suffix: the geometry alternatives of DESIGN.md section 27 are NIR_VARIANT builds "
                    "(NIR_VARIANT=tfw8 NIR_VARIANT_FLAGS=-DNIR_TF_WAVES=8 python -m context_attentive_ir_amd.build; --lib tfw8)")
    a = ap.parse_args()
    if a.lib:
        from context_attentive_ir_amd import lib as _lib
        _lib.LIB_PATH = os.path.join(ROOT, "context_attentive_ir_amd", "libneuroir_hip_%s.so" % a.lib)
    from context_attentive_ir_amd import autograd as A
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.constants import BOS, EOS, PAD
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.multitask import CARS
    rng = np.random.default_rng(1)
    args = default_args("CARS", src_vocab_size=a.V)
    net = fill_module_(CARS(args), 1013).cuda().eval()
    B, S, SD = a.B, a.S, a.S - 1
    Bd, rows_src = B * SD, B * S
    HD, DQ, HS, VT = args.nhid_decoder, args.nhid_query, args.nhid_session_query, args.tgt_vocab_size
    f = lambda *shape: torch.from_numpy(rng.uniform(-1, 1, size=shape).astype(np.float32)).cuda()      # noqa: E731
    states = (f(1, Bd, HD), f(1, Bd, HD))
    enc = f(rows_src, a.ql, DQ)
    lens = np.clip(rng.poisson(a.qmean, size=rows_src), 1, a.ql).astype(np.int64)
    lens[0] = a.ql
    lensd = torch.from_numpy(lens).cuda()
    attns = (f(B, S, HS), f(B, S, HS))
    lut = torch.from_numpy(rng.integers(4, a.V, size=VT, dtype=np.int64)).cuda()
    att = net.decoder.decoder.attn
    results = []
    for N in [int(v) for v in a.N.split(",")]:
        clen = np.clip(rng.poisson(a.qmean, size=(B, SD, N)), 1, a.TL - 2)
        cand = rng.integers(4, VT, size=(B, SD, N, a.TL), dtype=np.int64)
        pos = np.arange(a.TL)[None, None, None]
        cand[pos == clen[..., None] + 1] = EOS
        cand[pos > clen[..., None] + 1] = PAD
        cand[..., 0] = BOS
        candd = torch.from_numpy(cand).cuda()
        G = N * (a.TL - 1)
        rows = Bd * G
        kw = dict(states=states, candidate_seq=candd, src_dict=None, tgt_dict=None, batch_size=B, session_len=SD, encoded_source=enc, source_len=lensd,
                  session_attns=attns, tgt2src=lut)

        def front():
            return net._score_front(candidate_rep=None, **kw)

        def whole():
            return net.score_candidates(**kw)

        def parent_attention(c):
            """cars.py's train-mode composition on the scorer's rows: [Bd, G, .] in the place of [Bd, TL, .]"""
            h_all = c["h_all"].view(Bd, G, HD)
            mem = A.linear(c["enc"].index_select(0, c["rowmap"]), net.dec_attn.weight)                          # [Bd, QL, HD]
            align = (A.linear(h_all, att.linear_in.weight).unsqueeze(2) * mem.unsqueeze(1)).sum(3)            # [Bd, G, QL] through [Bd, G, QL, HD]
            mask = torch.arange(a.ql, device="cuda").unsqueeze(0) < c["lens"].index_select(0, c["rowmap"]).unsqueeze(1)
            ctx = A.softmax_pool(align, mask, mem, mask_div=G).view(Bd, G, -1)
            return torch.cat((ctx, h_all), 2).view(rows, 2 * HD)

        def parent_whole():
            c = front()
            return net._score_tail(c, parent_attention(c))

        keys = ("front", "fused_attend", "plain_attend", "fused_attention", "plain_attention", "parent_attention", "fused", "plain", "parent")
        t = {k: [] for k in keys}
        with torch.no_grad():
            c = front()
            banks = net._score_banks(c)
            for _ in range(max(1, a.rounds)):                    # the paths alternate, so that drift of the machine meets all of them
                t["front"].append(timed(front, a.iters, a.warmup))
                net.fuse_teacher_attention = True
                t["fused_attend"].append(timed(lambda: net._score_attend(c, banks), a.iters, a.warmup))
                t["fused_attention"].append(timed(lambda: net._score_attend(c), a.iters, a.warmup))
                t["fused"].append(timed(whole, a.iters, a.warmup))
                s_fused = whole()["scores"].clone()
                t["parent_attention"].append(timed(lambda: parent_attention(c), a.iters, a.warmup))
                t["parent"].append(timed(parent_whole, a.iters, a.warmup))
                s_parent = parent_whole()["scores"].clone()
                net.fuse_teacher_attention = False
                t["plain_attend"].append(timed(lambda: net._score_attend(c, banks), a.iters, a.warmup))
                t["plain_attention"].append(timed(lambda: net._score_attend(c), a.iters, a.warmup))
                t["plain"].append(timed(whole, a.iters, a.warmup))
                s_plain = whole()["scores"].clone()
            net.fuse_teacher_attention = True
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: float(max(v) - min(v)) for k, v in t.items()}
        best, other = ("fused", "plain") if med["fused_attend"] <= med["plain_attend"] else ("plain", "fused")
        from context_attentive_ir_amd import lib
        # the form the entry takes by default: fused where the shape has one and a group holds at least TF_MIN_G = 128 rows (csrc/tf_attend.hip);
        # below that BOTH timed paths run the plain kernel
        default_form = "fused" if lib.load().nir_tf_attend_fusable(a.ql, HD, 0) and G >= 128 else "plain"
        out = dict(model="cars_session_score", lib=a.lib or "default", B=B, S=S, QL=a.ql, N=N, TL=a.TL, rows=rows, rows_per_bank=G, HD=HD, DQ=DQ, P=args.nhid_document, V=a.V, VT=VT,
                   ms={k: round(v, 4) for k, v in med.items()}, spread_ms={k: round(v, 4) for k, v in spread.items()},
                   ms_rounds={k: [round(x, 4) for x in v] for k, v in t.items()}, default_form=default_form, faster_attend=best,
                   faster_wins_outside_spread=bool(max(t[best + "_attend"]) < min(t[other + "_attend"])),
                   default_is_the_faster=bool(default_form == "plain" or best == "fused"), fused_beats_parent_attention=bool(max(t["fused_attention"]) < min(t["parent_attention"])),
                   broadcast_product_bytes_not_written=rows * a.ql * HD * 4,
                   max_score_diff_fused_plain=float((s_fused - s_plain).abs().max()), max_score_diff_fused_parent=float((s_fused - s_parent).abs().max()))
        print(json.dumps(out))
        results.append(out)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(results, fh, indent=1)


if __name__ == "__main__":
    main()
