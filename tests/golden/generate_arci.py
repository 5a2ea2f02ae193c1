#!/usr/bin/env python
"""Golden fixtures of the reference's ARC-I (neuroir/rankers/arci.py), run on CPU.

Reuses generate.py's compatibility shims, deterministic weights and helpers by import; like there, the fixtures carry ids and
outputs only -- every consumer regenerates the weights from their state-dict keys (context_attentive_ir_amd.detinit).

    python tests/golden/generate_arci.py          # rewrites tests/golden/arci.npz and arci_arch.npz

arci.npz: the default arch at max_query_len 9 / max_doc_len 23 (scores, a non-zero PAD row, the narrower widths the same model accepts and
the one it refuses), a long case (filters_1d [256, 8] at widths 10 / 200: several row tiles, a small head) and three Ranker.update steps
with the embedding table fixed and free.  arci_arch.npz: three layers with kernel sizes 3, 5, 1 and pools 2, 1, 2 at emsize 37.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate as G  # noqa: E402  (installs the shims, puts the reference on sys.path)

from neuroir.rankers.arci import ARCI  # noqa: E402

PAD_ROW_SCALE = 0.25     # the "loaded state dict with a non-zero PAD row" variant: row 0 = this x the row of id 1
QL, DL = 9, 23
ARCH = dict(filters_1d=[24, 40, 16], kernel_size_1d=[3, 5, 1], maxpool_size_1d=[2, 1, 2], emsize=37)
ARCH_WIDTHS = (5, 9)
LONG = dict(filters_1d=[256, 8], kernel_size_1d=[3, 3], maxpool_size_1d=[2, 2])
LONG_WIDTHS = (10, 200)


def batches(rng, B, N, ql, dl):
    """ragged PAD tails, one interior PAD run, one all-PAD document"""
    qlen = rng.integers(1, ql + 1, size=B)
    qlen[0] = ql
    dlen = rng.integers(1, dl + 1, size=(B, N))
    dlen[0, 0] = dl
    q = G.rand_ids(rng, (B, ql), qlen)
    d = G.rand_ids(rng, (B, N, dl), dlen)
    d[0, 0, 2:min(dl - 1, 6)] = 0          # interior PAD run
    d[1, min(N - 1, 2), :] = 0             # all-PAD document
    return q, qlen, d, dlen


@torch.no_grad()
def run(m, q, qlen, d, dlen):
    s = m(G.T(q), G.T(qlen), G.T(d), G.T(dlen))
    return s, torch.softmax(s, -1)


@torch.no_grad()
def gen(out):
    rng = np.random.default_rng(41)
    args = G.base_args("ARCI", dropout_emb=0.2, fix_embeddings=False, max_query_len=QL, max_doc_len=DL)
    m = G.load_det(ARCI(args))
    sd = m.state_dict()
    out.update(sd_keys=np.asarray(list(sd.keys())), sd_shapes=np.asarray(json.dumps([list(v.shape) for v in sd.values()])),
               n_params=np.asarray(sum(p.numel() for p in m.parameters() if p.requires_grad)),
               arch=np.asarray(json.dumps(G.hyparam.get_model_specific_params("ARCI", "arch"))),
               data=np.asarray(json.dumps(G.hyparam.get_model_specific_params("ARCI", "data"))),
               max_query_len=np.asarray(QL), max_doc_len=np.asarray(DL))
    q, ql, d, dl = batches(rng, 3, 4, QL, DL)
    s, p = run(m, q, ql, d, dl)
    out.update(que_rep=q, que_len=ql, doc_rep=d, doc_len=dl, scores=s, softmax=p)
    # widths other than the ones of construction: accepted when they pool to the same feature counts (arci.py:104)
    for tag, (wq, wd) in (("_w8_20", (8, 20)), ("_w9_21", (9, 21))):
        q2, ql2, d2, dl2 = batches(rng, 3, 4, wq, wd)
        s2, p2 = run(m, q2, ql2, d2, dl2)
        out.update({"que_rep" + tag: q2, "que_len" + tag: ql2, "doc_rep" + tag: d2, "doc_len" + tag: dl2, "scores" + tag: s2, "softmax" + tag: p2})
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
def gen_long(out):
    rng = np.random.default_rng(43)
    wq, wd = LONG_WIDTHS
    m = G.load_det(ARCI(G.base_args("ARCI", dropout_emb=0.2, fix_embeddings=False, max_query_len=wq, max_doc_len=wd, **LONG)))
    q, ql, d, dl = batches(rng, 2, 2, wq, wd)
    s, p = run(m, q, ql, d, dl)
    out.update(arch_long=np.asarray(json.dumps(LONG)), que_rep_long=q, que_len_long=ql, doc_rep_long=d, doc_len_long=dl, scores_long=s,
               softmax_long=p)


def gen_train(out):
    """three updates of the real reference (models/ranker.py:192-230; BCE, clip 10, Adam 1e-3, dropout 0) alternating over two batches, then
    the scores of the first batch; with the embedding table fixed and free"""
    for tag, fix in (("fix", True), ("free", False)):
        rng = np.random.default_rng(47)
        B, N = 4, 3
        bs = []
        for _ in range(2):
            q, ql, d, dl = batches(rng, B, N, QL, DL)
            lab = np.zeros((B, N), np.int64)
            lab[np.arange(B), rng.integers(0, N, size=B)] = 1
            bs.append(dict(que_rep=q, que_len=ql, doc_rep=d, doc_len=dl, label=lab))
        args = G.base_args("ARCI", dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0,
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
    rng = np.random.default_rng(53)
    wq, wd = ARCH_WIDTHS
    m = G.load_det(ARCI(G.base_args("ARCI", dropout_emb=0.2, fix_embeddings=False, max_query_len=wq, max_doc_len=wd, **ARCH)))
    q, ql, d, dl = batches(rng, 3, 4, wq, wd)
    s, p = run(m, q, ql, d, dl)
    emb = m.word_embeddings.word_lut.weight
    emb[0] = PAD_ROW_SCALE * emb[1]
    sp, pp = run(m, q, ql, d, dl)
    G.save("arci_arch", arch=np.asarray(json.dumps(ARCH)), widths=np.asarray(ARCH_WIDTHS), que_rep=q, que_len=ql, doc_rep=d, doc_len=dl, scores=s,
           softmax=p, scores_padrow=sp, softmax_padrow=pp, pad_row_scale=np.asarray(PAD_ROW_SCALE))


if __name__ == "__main__":
    torch.manual_seed(G.SEED)
    torch.set_num_threads(4)
    out = {}
    gen(out)
    gen_long(out)
    gen_train(out)
    G.save("arci", **out)
    gen_arch()
