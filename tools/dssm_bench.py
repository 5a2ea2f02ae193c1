"""DSSM / CDSSM: `Ranker.predict` (csrc/dssm.hip) against a plain torch-op composition of the same maths on the same GPU.

Shape: scripts/ranker.sh of the reference -- B 64 queries, N 10 candidates, emsize 300, nhid 300, nout 128, V 30000 char-3-gram ids.
Length model (no MSMARCO data here): a word becomes about 5 n-grams, so document lengths are Poisson(--dmean, default 300) n-grams and
query lengths Poisson(--qmean, 30), each batch padded to its longest row, which is set to --dl (1000) / --ql (100).  The torch
composition embeds every padded position and, for CDSSM, materialises the reference's [B*N, L-2, 3E] interleave and runs Conv1d over it.

Prints per model: ms per batch (median of --iters, CUDA events, after --warmup), query-candidate pairs per second, useful TF/s of the
fused path (multiply-adds over the windows that hold a non-PAD id, x2), the speed-up, and the largest |difference| of the two paths' softmax.

    python tools/dssm_bench.py [--model dssm|cdssm|both] [--iters 20] [--warmup 5] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(rng, B, N, QL, DL, V, qmean, dmean):
    ql = np.clip(rng.poisson(qmean, size=B), 1, QL)
    dl = np.clip(rng.poisson(dmean, size=(B, N)), 1, DL)
    ql[0], dl[0, 0] = QL, DL
    q = rng.integers(4, V, size=(B, QL))
    d = rng.integers(4, V, size=(B, N, DL))
    q[np.arange(QL)[None] >= ql[:, None]] = 0
    d[np.arange(DL)[None, None] >= dl[..., None]] = 0
    t = lambda x: torch.from_numpy(x).cuda()          # noqa: E731
    return {"que_rep": t(q), "que_len": t(ql), "doc_rep": t(d), "doc_len": t(dl)}, ql, dl


def torch_scores(kind, net, q, d):
    """the reference's maths as stock torch ops (fp32), written for this tool"""
    B, N, DL = d.shape
    table = net.word_embeddings.table
    eq, ed = F.embedding(q, table), F.embedding(d.reshape(B * N, DL), table)
    if kind == "dssm":
        rq, rd = net.query_mlp(eq.max(1)[0]), net.doc_mlp(ed.max(1)[0])
    else:
        def tower(x, conv, sem):
            L = x.shape[1]
            inter = torch.cat([x[:, i:L - 2 + i] for i in range(3)], -1)
            return torch.tanh(sem(torch.tanh(conv(inter.transpose(1, 2)).transpose(1, 2)))).max(1)[0]
        rq, rd = tower(eq, net.query_conv, net.query_sem), tower(ed, net.doc_conv, net.doc_sem)
    rd = rd.view(B, N, -1)
    return torch.softmax(F.cosine_similarity(rq.unsqueeze(1).expand_as(rd), rd, dim=2), -1)


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def run(kind, a):
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import Ranker
    r = Ranker(default_args(kind, src_vocab_size=a.V))
    fill_module_(r.network, 1013)
    r.cuda()
    r.network.eval()
    ex, ql, dl = batch(np.random.default_rng(1), a.B, a.N, a.ql, a.dl, a.V, a.qmean, a.dmean)
    q, d = ex["que_rep"], ex["doc_rep"]
    E, NH, NO = a.emsize, 300, 128
    if kind == "dssm":
        useful = 2.0 * (a.B + a.B * a.N) * (E * NH + NH * NO)
    else:
        wq = np.minimum(ql, a.ql - 4).sum()
        wd = np.minimum(dl, a.dl - 4).sum()
        useful = 2.0 * float(wq + wd) * (5 * E * NH + NH * NO)
    with torch.no_grad():
        ours = timed(lambda: r.predict(ex), a.iters, a.warmup)
        ref = timed(lambda: torch_scores(kind, r.network, q, d), a.iters, a.warmup)
        diff = float((r.predict(ex) - torch_scores(kind, r.network, q, d)).abs().max())
    pairs = a.B * a.N
    return dict(model=kind, B=a.B, N=a.N, QL=a.ql, DL=a.dl, mean_q_ngrams=float(ql.mean()), mean_d_ngrams=float(dl.mean()),
                ms_per_batch=round(ours, 4), torch_ms_per_batch=round(ref, 4), pairs_per_s=round(pairs / ours * 1e3, 1),
                torch_pairs_per_s=round(pairs / ref * 1e3, 1), useful_tflops=round(useful / ours * 1e-9, 3), speedup=round(ref / ours, 2),
                max_abs_softmax_diff=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="both", choices=("dssm", "cdssm", "both"))
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--ql", type=int, default=100)
    ap.add_argument("--dl", type=int, default=1000)
    ap.add_argument("--qmean", type=float, default=30)
    ap.add_argument("--dmean", type=float, default=300)
    ap.add_argument("--V", type=int, default=30000)
    ap.add_argument("--emsize", type=int, default=300)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    out = [run(k, a) for k in (("dssm", "cdssm") if a.model == "both" else (a.model,))]
    for o in out:
        print(json.dumps(o))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
