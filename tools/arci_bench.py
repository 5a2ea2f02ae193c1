"""ARC-I: `Ranker.predict` (csrc/arci.hip) against a plain torch-op composition of the same maths on the same GPU and weights.

Shape: scripts/ranker.sh of the reference -- B 64 queries, N 10 candidates, max_query_len 10, max_doc_len 200, emsize 300, the default
arch (filters_1d [256, 128], kernel_size_1d [3, 3], maxpool_size_1d [2, 2]).  ARC-I convolves the padded width whatever the lengths are,
so the length model only decides which ids are PAD.  The torch composition is the reference's forward: embedding, Conv1d -> ReLU ->
MaxPool1d per layer, flatten, concatenate, and the UNFOLDED mlp (a [B*N, 6656] x [6656, 3328] GEMM per batch).

Prints: ms per batch (median of --iters, CUDA events, after --warmup), pairs per second, useful TF/s of the HIP path (the conv multiply-adds
over every pooled-in position x 2, the head not counted), the speed-up and the largest |difference| of the two paths' softmax.

    python tools/arci_bench.py [--iters 20] [--warmup 5] [--eager] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from dssm_bench import batch, timed  # noqa: E402


def torch_scores(net, q, d):
    """the reference's maths (arci.py:60-105) as stock torch ops (fp32), written for this tool"""
    B, N, DL = d.shape
    table = net.word_embeddings.table

    def tower(x, layers):
        x = x.transpose(1, 2)
        for layer in layers:
            x = layer(x)
        return x.flatten(1)
    fq = tower(F.embedding(q, table), net.query_conv1d_layers)
    fd = tower(F.embedding(d.reshape(B * N, DL), table), net.doc_conv1d_layers)
    com = torch.cat((fq.unsqueeze(1).expand(B, N, fq.shape[1]).reshape(B * N, -1), fd), 1)
    return torch.softmax(net.mlp(com).view(B, N), -1)


def conv_flops(net, rows_q, rows_d, QL, DL):
    tot, cin = 0.0, net.word_embeddings.table.shape[1]
    for f, k, p in zip(net.filters_1d, net.kernel_size_1d, net.maxpool_size_1d):
        QL, DL = QL // p, DL // p
        tot += 2.0 * (rows_q * QL + rows_d * DL) * p * k * cin * f
        cin = f
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--ql", type=int, default=10)
    ap.add_argument("--dl", type=int, default=200)
    ap.add_argument("--qmean", type=float, default=6)
    ap.add_argument("--dmean", type=float, default=120)
    ap.add_argument("--V", type=int, default=30000)
    ap.add_argument("--emsize", type=int, default=300)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--eager", action="store_true", help="time network() + softmax without the wrapper's graph replay as well")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import Ranker
    r = Ranker(default_args("ARCI", src_vocab_size=a.V, emsize=a.emsize, max_query_len=a.ql, max_doc_len=a.dl))
    fill_module_(r.network, 1013)
    r.cuda()
    net = r.network.eval()
    ex, _, _ = batch(np.random.default_rng(1), a.B, a.N, a.ql, a.dl, a.V, a.qmean, a.dmean)
    q, d = ex["que_rep"], ex["doc_rep"]
    with torch.no_grad():
        ours = timed(lambda: r.predict(ex), a.iters, a.warmup)
        ref = timed(lambda: torch_scores(net, q, d), a.iters, a.warmup)
        diff = float((r.predict(ex) - torch_scores(net, q, d)).abs().max())
        eager = timed(lambda: torch.softmax(net(q, None, d, None), -1), a.iters, a.warmup) if a.eager else None
    useful = conv_flops(net, a.B, a.B * a.N, a.ql, a.dl)
    pairs = a.B * a.N
    out = dict(model="arci", B=a.B, N=a.N, QL=a.ql, DL=a.dl, emsize=a.emsize, ms_per_batch=round(ours, 4), torch_ms_per_batch=round(ref, 4),
               pairs_per_s=round(pairs / ours * 1e3, 1), torch_pairs_per_s=round(pairs / ref * 1e3, 1), conv_gflop=round(useful * 1e-9, 2),
               useful_tflops=round(useful / ours * 1e-9, 3), speedup=round(ref / ours, 2), max_abs_softmax_diff=diff)
    if eager is not None:
        out["eager_ms_per_batch"] = round(eager, 4)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
