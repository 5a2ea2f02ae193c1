#!/usr/bin/env python
"""Golden fixtures of the reference's DSSM and CDSSM (neuroir/rankers/dssm.py, cdssm.py), run on CPU.

Reuses generate.py's compatibility shims, deterministic weights and helpers by import; like there, the fixtures carry ids and
outputs only -- every consumer regenerates the weights from their state-dict keys (context_attentive_ir_amd.detinit).

    python tests/golden/generate_dssm.py          # rewrites tests/golden/dssm.npz, cdssm.npz, dssm_arch.npz and cdssm_arch.npz

dssm_arch.npz / cdssm_arch.npz hold one case each at a non-default emsize / nhid / nout (recorded under "arch"): an emsize off the
64-column groups with nhid % 8 != 0 and nout > 160 for DSSM, an emsize past the 64 KiB LDS line with the largest nhid and nout for CDSSM.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate as G  # noqa: E402  (installs the shims, puts the reference on sys.path)

from neuroir.rankers.dssm import DSSM  # noqa: E402
from neuroir.rankers.cdssm import CDSSM  # noqa: E402

PAD_ROW_SCALE = 0.25     # the "loaded state dict with a non-zero PAD row" variant: row 0 = this x the row of id 1


def batches(rng, B, N, QL, DL):
    """ragged PAD tails, one interior PAD run, repeated n-grams, one all-PAD document"""
    qlen = rng.integers(1, QL + 1, size=B)
    qlen[0] = QL
    dlen = rng.integers(1, DL + 1, size=(B, N))
    dlen[0, 0] = DL
    q = G.rand_ids(rng, (B, QL), qlen)
    d = G.rand_ids(rng, (B, N, DL), dlen)
    d[0, 0, 2:8] = 0                       # interior PAD run (longer than the 5-row window)
    d[0, 1, :min(DL, 6)] = 7               # one n-gram repeated
    d[1, 2, :] = 0                         # all-PAD document
    return q, qlen, d, dlen


@torch.no_grad()
def run(model, q, qlen, d, dlen):
    m = model
    tq, td = G.T(q), G.T(d)
    s = m(tq, G.T(qlen), td, G.T(dlen))
    return s, torch.softmax(s, -1)


@torch.no_grad()
def gen(name, cls, seed):
    rng = np.random.default_rng(seed)
    args = G.base_args(name.upper(), dropout_emb=0.2, fix_embeddings=False)
    m = G.load_det(cls(args))
    sd = m.state_dict()
    out = dict(sd_keys=np.asarray(list(sd.keys())), sd_shapes=np.asarray(json.dumps([list(v.shape) for v in sd.values()])),
               n_params=np.asarray(sum(p.numel() for p in m.parameters() if p.requires_grad)),
               arch=np.asarray(json.dumps(G.hyparam.get_model_specific_params(name.upper(), "arch"))))
    q, ql, d, dl = batches(rng, 3, 4, 9, 23)
    s, p = run(m, q, ql, d, dl)
    out.update(que_rep=q, que_len=ql, doc_rep=d, doc_len=dl, scores=s, softmax=p)
    # the narrowest widths CDSSM accepts (one window)
    q5, ql5, d5, dl5 = batches(rng, 2, 3, 5, 5)
    s5, p5 = run(m, q5, ql5, d5, dl5)
    out.update(que_rep5=q5, que_len5=ql5, doc_rep5=d5, doc_len5=dl5, scores5=s5, softmax5=p5)
    # non-zero PAD row
    emb = m.word_embeddings.word_lut.weight
    emb[0] = PAD_ROW_SCALE * emb[1]
    sp, pp = run(m, q, ql, d, dl)
    out.update(scores_padrow=sp, softmax_padrow=pp, pad_row_scale=np.asarray(PAD_ROW_SCALE))
    G.save(name, **out)


# non-default sizes: (emsize, nhid, nout), widths (QL, DL); the CDSSM documents span two 32-window tiles
ARCH = {"dssm": (dict(emsize=37, nhid=257, nout=200), (9, 70)), "cdssm": (dict(emsize=416, nhid=320, nout=256), (9, 40))}


@torch.no_grad()
def gen_arch(name, cls, seed):
    rng = np.random.default_rng(seed)
    arch, (QL, DL) = ARCH[name]
    m = G.load_det(cls(G.base_args(name.upper(), dropout_emb=0.2, fix_embeddings=False, **arch)))
    q, ql, d, dl = batches(rng, 3, 4, QL, DL)
    s, p = run(m, q, ql, d, dl)
    emb = m.word_embeddings.word_lut.weight
    emb[0] = PAD_ROW_SCALE * emb[1]
    sp, pp = run(m, q, ql, d, dl)
    G.save(name + "_arch", arch=np.asarray(json.dumps(arch)), que_rep=q, que_len=ql, doc_rep=d, doc_len=dl, scores=s, softmax=p,
           scores_padrow=sp, softmax_padrow=pp, pad_row_scale=np.asarray(PAD_ROW_SCALE))


if __name__ == "__main__":
    torch.manual_seed(G.SEED)
    torch.set_num_threads(4)
    gen("dssm", DSSM, 11)
    gen("cdssm", CDSSM, 12)
    gen_arch("dssm", DSSM, 13)
    gen_arch("cdssm", CDSSM, 14)
