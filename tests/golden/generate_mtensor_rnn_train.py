#!/usr/bin/env python
"""Golden fixture of the reference's MATCH_TENSOR TRAINING step with the encoder configurations hyparam does not pin but the constructor admits
(neuroir/rankers/mtensor.py:36-49 passes rnn_type / nlayers to neuroir/encoders/rnn_encoder.py): GRU with one layer, GRU with two layers, LSTM
with two layers -- Ranker.update of the real reference (models/ranker.py:192-230) on CPU.

Reuses generate.py's compatibility shims and helpers by import (base_args, load_det, rand_ids, save); like there, the fixture carries ids and
recorded numbers only -- every consumer regenerates the weights from their state-dict keys (context_attentive_ir_amd.detinit).

    python tests/golden/generate_mtensor_rnn_train.py          # rewrites tests/golden/match_tensor_rnn_train.npz

Per case the recipe of generate.gen_train: B 4, N 3, QL 5, DL 11, all dropouts 0, Adam lr 1e-3, gradient clipping 10, two batches; recorded are the
scores and the loss of the first forward in train mode, the gradients of the first backward (before clipping; tensors above 4096 elements as
every 37th element plus the norm: three cases in one file under the size limit for committed files), and five update losses alternating over
the two batches.  Keys are "<case>.<name>".
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate as G  # noqa: E402  (installs the shims, puts the reference on sys.path)

CASES = (("gru1", dict(rnn_type="GRU", nlayers=1)), ("gru2", dict(rnn_type="GRU", nlayers=2)), ("lstm2", dict(rnn_type="LSTM", nlayers=2)))
B, N, QL, DL = 4, 3, 5, 11
FULL = 4096        # gradients up to this many elements are recorded whole


def batches(seed):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(2):
        qlen = rng.integers(1, QL + 1, size=B); dlen = rng.integers(1, DL + 1, size=(B, N)); qlen[0] = QL; dlen[0, 0] = DL
        q = G.rand_ids(rng, (B, QL), qlen); d = G.rand_ids(rng, (B, N, DL), dlen)
        lab = np.zeros((B, N), np.int64)
        lab[np.arange(B), rng.integers(0, N, size=B)] = 1
        out.append(dict(que_rep=q, que_len=qlen, doc_rep=d, doc_len=dlen, label=lab))
    return out


def gen_case(tag, kw, out):
    bs = batches(29)
    args = G.base_args("MATCH_TENSOR", dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0,
                       momentum=0, grad_clipping=10.0, fix_embeddings=True, max_query_len=QL, max_doc_len=DL, **kw)
    r = G.Ranker(args, list(range(G.V)))
    G.load_det(r.network)
    r.init_optimizer()
    b0 = bs[0]
    r.network.train()
    s = r.network(G.T(b0["que_rep"]), G.T(b0["que_len"]), G.T(b0["doc_rep"]), G.T(b0["doc_len"]))
    loss0 = r.criterion(s, G.T(b0["label"]).float())
    r.optimizer.zero_grad()
    loss0.backward()
    for bi, b in enumerate(bs):
        for k, v in b.items():
            out["%s.b%d_%s" % (tag, bi, k)] = v
    for name, p in r.network.named_parameters():
        if p.grad is not None and p.numel() <= FULL:
            out["%s.grad_%s" % (tag, name)] = p.grad.detach().clone()
        elif p.grad is not None:
            out["%s.gradsub37_%s" % (tag, name)] = p.grad.detach().flatten()[::37].clone()
            out["%s.gradnorm_%s" % (tag, name)] = p.grad.detach().norm()
    out[tag + ".scores0"], out[tag + ".loss0"] = s.detach(), loss0.detach()
    r.optimizer.zero_grad()
    out[tag + ".losses"] = np.asarray([float(r.update({k: G.T(v) for k, v in bs[step % 2].items()})) for step in range(5)], np.float64)


if __name__ == "__main__":
    out = {"cases": np.asarray([t for t, _ in CASES])}
    for tag, kw in CASES:
        gen_case(tag, kw, out)
        print(tag, "loss0 %.6f" % float(out[tag + ".loss0"]), "losses", out[tag + ".losses"])
    G.save("match_tensor_rnn_train", **out)
