#!/usr/bin/env python
"""Golden fixture of teacher-forced scoring under the reference's ACG (neuroir/recommender/seq2seq.py with copy_attn,
modules/copy_generator.py), run on CPU in float64.

The reference has no scorer, so this file composes one from the reference's own modules: for the five cases of generate_acg.py (same batch,
same weight seeds, read from acg.npz) the reference's forward() runs in eval mode, teacher-forced on N = 4 candidates per source row, with a
hook on its copy_generator that keeps the extended distribution of every step; decode()'s two collapse lines (index_add_ of the blanked slots
onto their fill ids, index_fill_ of the slots with 1e-10; recommender/seq2seq.py:162-171) are applied to every step's row, and log P is read
at the candidate's canonical extended id -- a slot that collapses onto a target word is read at that word.

    python tests/golden/generate_acg_score.py          # rewrites tests/golden/acg_score.npz

Recorded: the candidates [B, 4, TL] (tests/acg_score_ref.candidates: a copied out-of-vocabulary word, words both generated and copied, words
absent from the source, a collapsed slot id; unequal lengths) and the ids fed to the decoder, per case logp_<tag> [B, 4, TL - 1] (0 at PAD),
for the general case rows_general [B, 4, TL - 1, VT + CV] (the full collapsed rows, 1e-10 at the collapsed slots), and per case
loss_<tag> / gold_p_<tag>: the eval-mode forward loss of the batch's gold target without force_copy and the criterion's per-token
probabilities before its log.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import generate_acg as GA  # noqa: E402  (installs the shims, puts the reference on sys.path)

G = GA.G
from neuroir.recommender.seq2seq import Seq2seq  # noqa: E402
from neuroir.utils.copy_utils import align, collapse_copy_scores, make_src_map  # noqa: E402

import acg_ref as AR  # noqa: E402
import acg_score_ref as R  # noqa: E402

VT, VS, TL = GA.VT, GA.VS, GA.TL


@torch.no_grad()
def teacher_forced_rows(m, d, rep_n, src_map):
    """the reference's forward on decoder inputs rep_n [B, TL] -> the extended distribution of every step [B, TL, VT + CV] (not collapsed)"""
    kept = []
    h = m.copy_generator.register_forward_hook(lambda mod, inp, out: kept.append(out.detach().clone()))
    zeros = torch.zeros_like(rep_n)
    try:
        m(source_rep=G.T(d["src"]), source_len=G.T(d["lens"]), target_rep=rep_n, target_len=torch.full((rep_n.shape[0],), rep_n.shape[1]),
          target_seq=zeros, source_map=src_map, alignment=zeros)
    finally:
        h.remove()
    return kept[0]


@torch.no_grad()
def gold(m, d, src_map, al):
    kept, crit = [], m.criterion                                               # (a plain callable, no module: wrapped, not hooked)

    def keeping(*a):
        rows = crit(*a)
        kept.append(torch.exp(-rows.detach().clone()))
        return rows
    m.criterion = keeping
    try:
        loss = m(source_rep=G.T(d["src"]), source_len=G.T(d["lens"]), target_rep=G.T(d["tw"]), target_len=G.T(d["tlen"]), target_seq=G.T(d["ts"]),
                 source_map=src_map, alignment=al)
    finally:
        m.criterion = crit
    return loss.detach(), kept[0].view(len(d["lens"]), -1)


if __name__ == "__main__":
    torch.manual_seed(G.SEED)
    torch.set_num_threads(4)
    g = np.load(os.path.join(HERE, "acg.npz"), allow_pickle=False)
    src_dict, tgt_dict = GA.dictionaries()
    d = GA.batch(np.random.default_rng(97), repeat_oov=True)                  # generate_acg.gen_decode's batch
    assert np.array_equal(d["src"], g["source_words"]) and np.array_equal(d["ts"], g["target_seq"])
    blank, fill = collapse_copy_scores(tgt_dict, d["vocabs"])
    src_map, al = make_src_map(d["maps"]).double(), align(d["als"])
    dd = AR.batch_inputs()
    e2t, e2s = AR.index_tensors(dd)
    assert all(sorted(int(x) - VT for x in blank[b]) == [c for c in range(e2t.shape[1]) if int(e2t[b, c]) >= 0] for b in range(len(blank)))
    cand = R.candidates(dd, e2t, VT, TL)
    tgt2src = torch.tensor([src_dict[tgt_dict[i]] for i in range(VT)])
    rep = R.default_rep(cand, tgt2src, e2s, VT, VS)
    B, N = cand.shape[:2]
    canon = R.canonical(cand.reshape(-1), e2t.repeat_interleave(N * TL, 0), VT).view(B, N, TL)   # (the ids of a source row share its ext2tgt row)
    out = dict(candidate_seq=cand.numpy(), candidate_rep=rep.numpy(), tgt2src=tgt2src.numpy())
    for tag, cfg in GA.CASES:
        seed = json.loads(str(g["cfg_" + tag]))["seed"]
        m = GA.load_seed(Seq2seq(GA.args_for(cfg)), seed).double()
        logp = torch.zeros(B, N, TL - 1, dtype=torch.float64)
        rows = []
        for n in range(N):
            P = teacher_forced_rows(m, d, rep[:, n], src_map)[:, :-1]         # step t against token t + 1
            for b in range(B):
                if blank[b]:
                    blank_b, fill_b = torch.LongTensor(blank[b]), torch.LongTensor(fill[b])
                    for t in range(TL - 1):
                        P[b, t].index_add_(0, fill_b, P[b, t].index_select(0, blank_b))
                        P[b, t].index_fill_(0, blank_b, 1e-10)
            tok = cand[:, n, 1:]
            lp = torch.log(P.gather(2, canon[:, n, 1:].unsqueeze(2)).squeeze(2))
            logp[:, n] = torch.where(tok != AR.PAD, lp, torch.zeros_like(lp))
            rows.append(P)
        loss, gp = gold(m, d, src_map, al)
        out.update({"logp_" + tag: logp, "loss_" + tag: loss, "gold_p_" + tag: gp})
        if tag == "general":
            out["rows_general"] = torch.stack(rows, 1)
        print(tag, "seed", seed, "loss %.9f" % float(loss), "logp range", float(logp.min()), float(logp[logp < 0].max()),
              "-inf:", int(torch.isinf(logp).sum()))
    G.save("acg_score", **out)
