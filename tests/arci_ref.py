"""The acceptance criterion of the ARC-I kernels (csrc/arci.hip): a restatement of neuroir/rankers/arci.py:60-105 in the reference's op order
(embedding, Conv1d -> ReLU -> MaxPool1d per layer, channel-major flatten, query features first, the UNFOLDED mlp), evaluated in float64 as
the reference and in float32 on the CPU as the yardstick of what fp32 arithmetic costs, plus the bound a result has to meet.

Bound (the form of tests/gemm_ref.py): with s = max |ref64|, e = max |got - ref64| / s and e_chain the same figure for the float32 chain,

    e <= MARGIN * max(e_chain, 2^-23) + n_split_layers * FMT["fp16x2"]

n_split_layers: the layers that ran on the two-term fp16 path (each operand known to 2^-22, the dropped product another 2^-22 -- gemm_ref.FMT).
MARGIN: the rule is the largest (e - fmt) / max(e_chain, 2^-23) measured on the MI355X over the envelope and network cases, doubled, rounded
up to a power of two, never above gemm_ref.MARGIN_CAP.  NOT MEASURED YET: until it is, the constant sits at the cap,
the largest value the rule can give -- every GPU test prints its ratio, so the first run yields the figure.

`fault` plants one of three mistakes a kernel could make, to show on the CPU that the bound rejects them (tests/test_arci_host.py):
    "fp16_layer1"  both operands of the first layer rounded to ONE fp16 term (the split without its residual)
    "pad_row"      the table's PAD row where the first conv pads zeros
    "pool_shift"   the first layer's pool windows start one position late
"""
import json

import numpy as np
import torch
import torch.nn.functional as F

import gemm_ref
from conftest import T, load_golden

EMB = "word_embeddings.make_embedding.emb_luts.0.weight"
MARGIN = gemm_ref.MARGIN_CAP
EPS = gemm_ref.EPS


def _fp16_one_term(x):
    return torch.from_numpy(gemm_ref.split_terms(x.detach().float().numpy(), "fp16x2")[0].astype(np.float64)).to(x.dtype)


def conv_pool(x, w, b, p, act="relu", fault=None, pad_row=None):
    """one layer (arci.py:31-36): x [M, L, C] position-major -> [M, L // p, F]"""
    k = w.shape[2]
    h = x.transpose(1, 2)
    if fault == "fp16_layer1":
        h, w = _fp16_one_term(h), _fp16_one_term(w)
    if fault == "pad_row" and k > 1:
        edge = pad_row.to(h.dtype).reshape(1, -1, 1).expand(h.shape[0], -1, k // 2)
        y = F.conv1d(torch.cat([edge, h, edge], 2), w, b)
    else:
        y = F.conv1d(h, w, b, padding=k // 2)
    if act == "relu":
        y = torch.relu(y)
    if fault == "pool_shift":
        y = y.roll(-1, 2)
    return F.max_pool1d(y, p).transpose(1, 2)


def tower(x, sd, pre, pools, fault=None, pad_row=None):
    for i, p in enumerate(pools):
        x = conv_pool(x, sd["%s.%d.0.weight" % (pre, i)], sd["%s.%d.0.bias" % (pre, i)], p, fault=fault if i == 0 else None, pad_row=pad_row)
    return x.transpose(1, 2).flatten(1)


def scores(sd, q, d, pools, dtype=torch.float64, fault=None, device="cpu"):
    """[B, N] scores; sd: a state dict with the reference's keys; pools: maxpool_size_1d"""
    sd = {k: v.detach().to(device, dtype) for k, v in sd.items()}
    q, d = q.to(device), d.to(device)
    B, N, DL = d.shape
    table = sd[EMB]
    fq = tower(F.embedding(q, table), sd, "query_conv1d_layers", pools, fault, table[0])
    fd = tower(F.embedding(d.reshape(B * N, DL), table), sd, "doc_conv1d_layers", pools, fault, table[0])
    com = torch.cat((fq.unsqueeze(1).expand(B, N, fq.shape[1]).reshape(B * N, -1), fd), 1)
    h = com @ sd["mlp.0.weight"].t() + sd["mlp.0.bias"]
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
    return accept(got, ref, chain, len(pools) if n_split is None else n_split, margin)


# ------------------------------------------------------------------ the fixture cases (tests/golden/generate_arci.py)
# (fixture file, key suffix, max_query_len, max_doc_len of construction, key of the arch JSON or None for the defaults)
CASES = [("arci", "", 9, 23, None), ("arci", "_w8_20", 9, 23, None), ("arci", "_w9_21", 9, 23, None), ("arci", "_padrow", 9, 23, None),
         ("arci", "_long", 10, 200, "arch_long"), ("arci_arch", "", 5, 9, "arch"), ("arci_arch", "_padrow", 5, 9, "arch")]


def case_args(name, tag, mq, md, arch, V=200, **kw):
    from context_attentive_ir_amd.config import default_args
    g = load_golden(name)
    return default_args("ARCI", src_vocab_size=V, max_query_len=mq, max_doc_len=md, **dict(json.loads(str(g[arch])) if arch else {}, **kw))


def case(name, tag, mq, md, arch):
    """(network on the CPU with the fixture's weights, ids q, ids d, recorded scores, recorded softmax)"""
    from context_attentive_ir_amd.detinit import det_state_dict
    from context_attentive_ir_amd.rankers import ARCI
    g = load_golden(name)
    net = ARCI(case_args(name, tag, mq, md, arch))
    sd = det_state_dict({k: v.shape for k, v in net.state_dict().items()})
    if tag == "_padrow":
        sd[EMB][0] = float(g["pad_row_scale"]) * sd[EMB][1]
    net.load_state_dict(sd)
    ids = "" if tag == "_padrow" else tag
    return net, T(g["que_rep" + ids]), T(g["doc_rep" + ids]), g["scores" + tag], g["softmax" + tag]
