"""The acceptance criterion of the ARC-II kernels (csrc/arcii.hip): a restatement of neuroir/rankers/arcii.py:58-111 in the reference's op order
(embedding, the two Conv1d without activation, the FULL broadcast grid Ed[m, f, i] + Eq[m // N, f, j], max_pool2d(2 x 2), Conv2d -> ReLU ->
MaxPool2d per layer, flatten(1), the UNFOLDED mlp), evaluated in float64 as the reference and in float32 on the CPU as the yardstick of
what fp32 arithmetic costs, plus the bound a result has to meet.

Bound (the form of tests/arci_ref.py and tests/gemm_ref.py): with s = max |ref64|, e = max |got - ref64| / s and e_chain the same figure
for the float32 chain,

    e <= MARGIN * max(e_chain, 2^-23) + n_split_layers * FMT["fp16x2"]

n_split_layers: the layers that ran on the two-term fp16 path, 1 + len(filters_2d) when all do.
MARGIN: the largest (e - fmt) / max(e_chain, 2^-23) the GPU tests (test_gpu_arcii.py, test_gpu_arcii_envelope.py) print on the MI355X,
doubled, rounded up to a power of two, never above gemm_ref.MARGIN_CAP.  Measured: 1.000 over the 215 envelope
runs (reached on the fp32 path; the split path stays below it) and negative on every network case (e below the format term alone), so
MARGIN = 2.

`fault` plants one of four mistakes a kernel could make, to show on the CPU that the bound rejects them (tests/test_arcii_host.py):
    "grid_pad"    outside the grid a tap of the first Conv2d reads the one-sided sum Pd[i] + 0 (the terms padded, not the grid)
    "hw_swap"     the head indexed with i and j transposed
    "fp16_layer"  both operands of the first Conv2d rounded to ONE fp16 term (the split without its residual)
    "pool_shift"  the first Conv2d's pool windows start one document position late
"""
import json

import numpy as np
import torch
import torch.nn.functional as F

import gemm_ref
from conftest import T, load_golden

EMB = "word_embeddings.make_embedding.emb_luts.0.weight"
MARGIN = 2.0
EPS = gemm_ref.EPS
FAULTS = ("grid_pad", "hw_swap", "fp16_layer", "pool_shift")


def _fp16_one_term(x):
    return torch.from_numpy(gemm_ref.split_terms(x.detach().float().numpy(), "fp16x2")[0].astype(np.float64)).to(x.dtype)


def conv2d_pool(x, w, b, pool, act="relu"):
    """one 2-D layer (arcii.py:38-43) on the position-major x [M, H, W, C] -> [M, H // ph, W // pw, F]"""
    y = F.conv2d(x.permute(0, 3, 1, 2), w, b, padding=(w.shape[2] // 2, w.shape[3] // 2))
    if act == "relu":
        y = torch.relu(y)
    return F.max_pool2d(y, tuple(pool)).permute(0, 2, 3, 1)


def outer_sum(pd, pq, N):
    """pd [M, H, C], pq [M // N, W, C] -> the grid [M, H, W, C]"""
    return pd.unsqueeze(2) + pq.repeat_interleave(N, 0).unsqueeze(1)


def towers(sd, q, d):
    """(Eq expanded over the candidates [B N, F1, QL], Ed [B N, F1, DL]) (arcii.py:73-94)"""
    B, N, DL = d.shape
    table = sd[EMB]
    k1 = sd["conv_query.weight"].shape[2]
    eq = F.conv1d(F.embedding(q, table).transpose(1, 2), sd["conv_query.weight"], sd["conv_query.bias"], padding=k1 // 2)
    ed = F.conv1d(F.embedding(d.reshape(B * N, DL), table).transpose(1, 2), sd["conv_doc.weight"], sd["conv_doc.bias"], padding=k1 // 2)
    eq = eq.unsqueeze(1).expand(B, N, eq.shape[1], eq.shape[2]).reshape(B * N, eq.shape[1], eq.shape[2])
    return eq, ed


def scores(sd, q, d, pools, dtype=torch.float64, fault=None, device="cpu"):
    """[B, N] scores; sd: a state dict with the reference's keys; pools: maxpool_size_2d"""
    return forward({k: v.detach().to(device, dtype) for k, v in sd.items()}, q.to(device), d.to(device), pools, fault)


def forward(sd, q, d, pools, fault=None):
    """the forward on the tensors of sd as they are (they may require grad)"""
    B, N, _ = d.shape
    eq, ed = towers(sd, q, d)
    x = F.max_pool2d(ed.unsqueeze(3) + eq.unsqueeze(2), (2, 2))                    # [B N, F1, DL / 2, QL / 2] (arcii.py:96-104)
    for i, p in enumerate(pools):
        w, b = sd["conv2d_layers.%d.0.weight" % i], sd["conv2d_layers.%d.0.bias" % i]
        kh, kw = w.shape[2], w.shape[3]
        if i == 0 and fault == "fp16_layer":
            x, w = _fp16_one_term(x), _fp16_one_term(w)
        if i == 0 and fault == "grid_pad":
            pd = F.pad(F.max_pool1d(ed, 2), (kh // 2, kh // 2))
            pq = F.pad(F.max_pool1d(eq, 2), (kw // 2, kw // 2))
            y = F.conv2d(pd.unsqueeze(3) + pq.unsqueeze(2), w, b)
        else:
            y = F.conv2d(x, w, b, padding=(kh // 2, kw // 2))
        y = torch.relu(y)
        if i == 0 and fault == "pool_shift":
            y = y.roll(-1, 2)
        x = F.max_pool2d(y, tuple(p))
    f = (x.transpose(2, 3) if fault == "hw_swap" else x).flatten(1)
    h = f @ sd["mlp.0.weight"].t() + sd["mlp.0.bias"]
    return (h @ sd["mlp.1.weight"].t() + sd["mlp.1.bias"]).view(B, N)


def figures(got, ref, chain, n_split):
    """dict(e, e_chain, s, extra, ratio): ratio = (e - fmt) / max(e_chain, 2^-23), the figure MARGIN is chosen from"""
    got = got.detach().cpu().double() if torch.is_tensor(got) else torch.as_tensor(np.asarray(got)).double()
    ref, chain = ref.detach().cpu().double(), chain.detach().cpu().double()
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "non-finite output"
    s = float(ref.abs().max())
    assert s > 0
    e = float((got - ref).abs().max()) / s
    e_chain = float((chain - ref).abs().max()) / s
    extra = n_split * gemm_ref.FMT["fp16x2"]
    return dict(e=e, e_chain=e_chain, s=s, extra=extra, ratio=(e - extra) / max(e_chain, EPS))


def accept(got, ref, chain, n_split, margin=None):
    """(ok, figures): the criterion of the module docstring"""
    margin = MARGIN if margin is None else margin
    assert margin <= gemm_ref.MARGIN_CAP
    r = figures(got, ref, chain, n_split)
    r["bound"] = margin * max(r["e_chain"], EPS) + r["extra"]
    return r["e"] <= r["bound"], r


def accept_scores(got, sd, q, d, pools, n_split=None, margin=None):
    ref = scores(sd, q, d, pools)
    chain = scores(sd, q, d, pools, torch.float32)
    return accept(got, ref, chain, 1 + len(pools) if n_split is None else n_split, margin)


# ------------------------------------------------------------------ the fixture cases (tests/golden/generate_arcii.py)
# (fixture file, key suffix, max_query_len, max_doc_len of construction, key of the arch JSON or None for the defaults)
CASES = [("arcii", "", 9, 23, None), ("arcii", "_w8_22", 9, 23, None), ("arcii", "_w11_23", 9, 23, None), ("arcii", "_padrow", 9, 23, None),
         ("arcii", "_product", 16, 32, "arch_product"), ("arcii", "_long", 10, 100, "arch_long"), ("arcii_arch", "_asym", 7, 13, "arch_asym"),
         ("arcii_arch", "_wide", 8, 12, "arch_wide")]


def case_args(name, tag, mq, md, arch, V=200, **kw):
    from context_attentive_ir_amd.config import default_args
    g = load_golden(name)
    return default_args("ARCII", src_vocab_size=V, max_query_len=mq, max_doc_len=md, **dict(json.loads(str(g[arch])) if arch else {}, **kw))


def case(name, tag, mq, md, arch):
    """(network on the CPU with the fixture's weights, ids q, ids d, recorded scores, recorded softmax)"""
    from context_attentive_ir_amd.detinit import det_state_dict
    from context_attentive_ir_amd.rankers import ARCII
    g = load_golden(name)
    net = ARCII(case_args(name, tag, mq, md, arch))
    sd = det_state_dict({k: v.shape for k, v in net.state_dict().items()})
    if tag == "_padrow":
        sd[EMB][0] = float(g["pad_row_scale"]) * sd[EMB][1]
    net.load_state_dict(sd)
    ids = "" if tag == "_padrow" else tag
    return net, T(g["que_rep" + ids]), T(g["doc_rep" + ids]), g["scores" + tag], g["softmax" + tag]
