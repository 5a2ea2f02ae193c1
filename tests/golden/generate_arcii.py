#!/usr/bin/env python
"""Golden fixtures of the reference's ARC-II (neuroir/rankers/arcii.py), run on CPU.

Reuses generate.py's compatibility shims, deterministic weights and helpers by import; like there, the fixtures carry ids and
outputs only -- every consumer regenerates the weights from their state-dict keys (context_attentive_ir_amd.detinit).

    python tests/golden/generate_arcii.py          # rewrites tests/golden/arcii.npz and arcii_arch.npz

arcii.npz: the default arch at max_query_len 9 / max_doc_len 23 (scores, a non-zero PAD row, other widths the same model accepts and the
one it refuses), the product rule (a small arch built for 16 / 32 and run at 32 / 16: the final grid is 2 x 4 instead of 4 x 2, the
feature count is the same), a long case (filters_2d [256, 8] at widths 10 / 100: several row tiles, a small head) and three Ranker.update
steps with the embedding table fixed and free.  arcii_arch.npz: an asymmetric arch (kernels 5 x 3 and 1 x 3, pools 3 x 1 and 1 x 2, a
1-D kernel of 5, emsize 37) and a wide one (130 filters, a 3 x 2 pool, a final grid of 2 x 2).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate as G  # noqa: E402  (installs the shims, puts the reference on sys.path)

from generate_arci import PAD_ROW_SCALE, batches, run  # noqa: E402
from neuroir.rankers.arcii import ARCII  # noqa: E402

QL, DL = 9, 23
PRODUCT = dict(emsize=20, filters_1d=12, filters_2d=[10, 6])
PRODUCT_BUILT, PRODUCT_RUN = (16, 32), (32, 16)
LONG = dict(filters_2d=[256, 8])
LONG_WIDTHS = (10, 100)
ASYM = dict(emsize=37, filters_1d=20, kernel_size_1d=5, filters_2d=[24, 12], kernel_size_2d=[[5, 3], [1, 3]], maxpool_size_2d=[[3, 1], [1, 2]])
ASYM_WIDTHS = (7, 13)
WIDE = dict(emsize=33, filters_1d=40, filters_2d=[130], kernel_size_2d=[[3, 3]], maxpool_size_2d=[[3, 2]])
WIDE_WIDTHS = (8, 12)


def model(wq, wd, **kw):
    return G.load_det(ARCII(G.base_args("ARCII", dropout_emb=0.2, fix_embeddings=False, max_query_len=wq, max_doc_len=wd, **kw)))


def record(out, tag, m, rng, B, N, wq, wd):
    q, ql, d, dl = batches(rng, B, N, wq, wd)
    s, p = run(m, q, ql, d, dl)
    out.update({"que_rep" + tag: q, "que_len" + tag: ql, "doc_rep" + tag: d, "doc_len" + tag: dl, "scores" + tag: s, "softmax" + tag: p})
    return q, ql, d, dl


@torch.no_grad()
def gen(out):
    rng = np.random.default_rng(61)
    m = model(QL, DL)
    sd = m.state_dict()
    out.update(sd_keys=np.asarray(list(sd.keys())), sd_shapes=np.asarray(json.dumps([list(v.shape) for v in sd.values()])),
               n_params=np.asarray(sum(p.numel() for p in m.parameters() if p.requires_grad)),
               arch=np.asarray(json.dumps(G.hyparam.get_model_specific_params("ARCII", "arch"))),
               data=np.asarray(json.dumps(G.hyparam.get_model_specific_params("ARCII", "data"))),
               max_query_len=np.asarray(QL), max_doc_len=np.asarray(DL))
    q, ql, d, dl = record(out, "", m, rng, 3, 4, QL, DL)
    # widths other than the ones of construction: accepted when the final grid flattens to the same feature count (arcii.py:108-110)
    for tag, (wq, wd) in (("_w8_22", (8, 22)), ("_w11_23", (11, 23))):
        record(out, tag, m, rng, 3, 4, wq, wd)
    q3, ql3, d3, dl3 = batches(rng, 3, 4, QL, 24)
    try:
        run(m, q3, ql3, d3, dl3)
        raised = ""
    except RuntimeError as e:
        raised = type(e).__name__
    assert raised == "RuntimeError"
    out.update(refused_widths=np.asarray([QL, 24]), refused_error=np.asarray(raised))
    # non-zero PAD row
    emb = m.word_embeddings.word_lut.weight
    emb[0] = PAD_ROW_SCALE * emb[1]
    sp, pp = run(m, q, ql, d, dl)
    out.update(scores_padrow=sp, softmax_padrow=pp, pad_row_scale=np.asarray(PAD_ROW_SCALE))


@torch.no_grad()
def gen_product(out):
    """the product rule: the individual sides of the final grid need not be the ones of construction"""
    rng = np.random.default_rng(67)
    m = model(*PRODUCT_BUILT, **PRODUCT)
    record(out, "_product", m, rng, 2, 3, *PRODUCT_RUN)
    out.update(arch_product=np.asarray(json.dumps(PRODUCT)), built_product=np.asarray(PRODUCT_BUILT), widths_product=np.asarray(PRODUCT_RUN))


@torch.no_grad()
def gen_long(out):
    rng = np.random.default_rng(71)
    m = model(*LONG_WIDTHS, **LONG)
    record(out, "_long", m, rng, 2, 2, *LONG_WIDTHS)
    out.update(arch_long=np.asarray(json.dumps(LONG)))


def gen_train(out):
    """three updates of the real reference (models/ranker.py:192-230; BCE, clip 10, Adam 1e-3, dropout 0) alternating over two batches, then
    the scores of the first batch; with the embedding table fixed and free"""
    for tag, fix in (("fix", True), ("free", False)):
        rng = np.random.default_rng(73)
        B, N = 4, 3
        bs = []
        for _ in range(2):
            q, ql, d, dl = batches(rng, B, N, QL, DL)
            lab = np.zeros((B, N), np.int64)
            lab[np.arange(B), rng.integers(0, N, size=B)] = 1
            bs.append(dict(que_rep=q, que_len=ql, doc_rep=d, doc_len=dl, label=lab))
        args = G.base_args("ARCII", dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0,
                           momentum=0, grad_clipping=10.0, fix_embeddings=fix, max_query_len=QL, max_doc_len=DL)
        r = G.Ranker(args, list(range(G.V)))
        G.load_det(r.network)
        r.init_optimizer()
        losses = [float(r.update({k: G.T(v) for k, v in bs[step % 2].items()})) for step in range(3)]
        r.network.eval()
        with torch.no_grad():
            s = r.network(*[G.T(bs[0][k]) for k in ("que_rep", "que_len", "doc_rep", "doc_len")])
        if tag == "fix":
            for bi, b in enumerate(bs):
                out.update({"train_b%d_%s" % (bi, k): v for k, v in b.items()})
        out.update({"train_losses_" + tag: np.asarray(losses, np.float64), "train_scores_" + tag: s.detach()})


@torch.no_grad()
def gen_arch():
    out = {}
    rng = np.random.default_rng(79)
    for tag, arch, (wq, wd), (B, N) in (("_asym", ASYM, ASYM_WIDTHS, (3, 4)), ("_wide", WIDE, WIDE_WIDTHS, (2, 3))):
        m = model(wq, wd, **arch)
        record(out, tag, m, rng, B, N, wq, wd)
        out.update({"arch" + tag: np.asarray(json.dumps(arch)), "widths" + tag: np.asarray((wq, wd))})
    G.save("arcii_arch", **out)


if __name__ == "__main__":
    torch.manual_seed(G.SEED)
    torch.set_num_threads(4)
    out = {}
    gen(out)
    gen_product(out)
    gen_long(out)
    gen_train(out)
    G.save("arcii", **out)
    gen_arch()
