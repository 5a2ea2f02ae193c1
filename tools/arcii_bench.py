"""ARC-II: `Ranker.predict` (csrc/arcii.hip) against a plain torch-op composition of the same maths on the same GPU and weights.

Shape: scripts/ranker.sh of the reference -- B 64 queries, N 10 candidates, max_query_len 10, max_doc_len 100, emsize 300, the default
arch (filters_1d 128, kernel_size_1d 3, filters_2d [256, 128], 3 x 3 kernels, 2 x 2 pools).  ARC-II convolves the padded widths whatever
the lengths are, so the length model only decides which ids are PAD.  The torch composition is the reference's forward, what ARC-II
users run today: embedding, the two Conv1d, the full [B N, 128, DL, QL] broadcast grid, MaxPool2d, Conv2d -> ReLU -> MaxPool2d per
layer, flatten and the UNFOLDED mlp.

Prints: ms per batch (median of --iters, CUDA events, after --warmup) and the spread (min / max) of both paths, pairs per second, useful
TF/s of the HIP path (the conv multiply-adds over every pooled-in position x 2, the head not counted), the speed-up and the largest
|difference| of the two paths' softmax.  --rounds R repeats the two timings R times, alternating, and reports the medians' spread.

    python tools/arcii_bench.py [--iters 20] [--warmup 5] [--rounds 3] [--eager] [--json out.json]
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
    """the reference's maths (arcii.py:58-111) as stock torch ops (fp32), written for this tool"""
    B, N, DL = d.shape
    table = net.word_embeddings.table
    eq = net.conv_query(F.embedding(q, table).transpose(1, 2))
    eq = eq.unsqueeze(1).expand(B, N, eq.shape[1], eq.shape[2]).reshape(B * N, eq.shape[1], eq.shape[2])
    ed = net.conv_doc(F.embedding(d.reshape(B * N, DL), table).transpose(1, 2))
    x = net.maxpool1(ed.unsqueeze(3) + eq.unsqueeze(2))
    for layer in net.conv2d_layers:
        x = layer(x)
    return torch.softmax(net.mlp(x.flatten(1)).view(B, N), -1)


def conv_flops(net, B, N, QL, DL):
    """multiply-adds x 2 of the positions the pools keep: the 1-D stage of both towers, then every 2-D layer"""
    E, F1, k1 = net.word_embeddings.table.shape[1], net.filters_1d, net.kernel_size_1d
    hq, hd = QL // 2, DL // 2
    tot = 2.0 * (B * hq + B * N * hd) * 2 * k1 * E * F1
    cin = F1
    for f, (kh, kw), (ph, pw) in zip(net.filters_2d, net.kernel_size_2d, net.maxpool_size_2d):
        hd, hq = hd // ph, hq // pw
        tot += 2.0 * B * N * hd * hq * ph * pw * kh * kw * cin * f
        cin = f
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--N", type=int, default=10)
    ap.add_argument("--ql", type=int, default=10)
    ap.add_argument("--dl", type=int, default=100)
    ap.add_argument("--qmean", type=float, default=6)
    ap.add_argument("--dmean", type=float, default=60)
    ap.add_argument("--V", type=int, default=30000)
    ap.add_argument("--emsize", type=int, default=300)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating repeats of the two timings; the spread of their medians is reported")
    ap.add_argument("--eager", action="store_true", help="time network() + softmax without the wrapper's graph replay as well")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import Ranker
    r = Ranker(default_args("ARCII", src_vocab_size=a.V, emsize=a.emsize, max_query_len=a.ql, max_doc_len=a.dl))
    fill_module_(r.network, 1013)
    r.cuda()
    net = r.network.eval()
    ex, _, _ = batch(np.random.default_rng(1), a.B, a.N, a.ql, a.dl, a.V, a.qmean, a.dmean)
    q, d = ex["que_rep"], ex["doc_rep"]
    with torch.no_grad():
        ours_r, ref_r = [], []
        for _ in range(max(1, a.rounds)):                    # the two paths alternate, so that drift of the machine meets both
            ours_r.append(timed(lambda: r.predict(ex), a.iters, a.warmup))
            ref_r.append(timed(lambda: torch_scores(net, q, d), a.iters, a.warmup))
        ours, ref = float(np.median(ours_r)), float(np.median(ref_r))
        diff = float((r.predict(ex) - torch_scores(net, q, d)).abs().max())
        eager = timed(lambda: torch.softmax(net(q, None, d, None), -1), a.iters, a.warmup) if a.eager else None
    useful = conv_flops(net, a.B, a.N, a.ql, a.dl)
    pairs = a.B * a.N
    out = dict(model="arcii", B=a.B, N=a.N, QL=a.ql, DL=a.dl, emsize=a.emsize, ms_per_batch=round(ours, 4), torch_ms_per_batch=round(ref, 4),
               ms_rounds=[round(v, 4) for v in ours_r], torch_ms_rounds=[round(v, 4) for v in ref_r],
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
