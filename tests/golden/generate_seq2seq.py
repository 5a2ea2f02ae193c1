#!/usr/bin/env python
"""Golden fixtures of the reference's Seq2seq (neuroir/recommender/seq2seq.py) and Recommender (neuroir/models/recommender.py), run on CPU.

Reuses generate.py's compatibility shims and helpers by import; like there, the fixture carries ids and outputs only -- every consumer
regenerates the weights from their state-dict keys (context_attentive_ir_amd.detinit, seed recorded per case).

    python tests/golden/generate_seq2seq.py          # rewrites tests/golden/seq2seq.npz

Cases (nlayers = 1, tgt_vocab_size = 200): attn_type general / dot / mlp at nhid 64, a unidirectional encoder at nhid 96 and a general case
at nhid 512.  Decode: B = 5 sources of width 7 with pairwise distinct, unsorted lengths (a permutation of 1..7 cut to 5), max_len 6, a
permuted src_dict.  Recorded per case: predictions, attentions (max(source_len) wide, as the reference returns them), the top-1 minus top-2
logit of every step, the teacher-forced loss; for the general case three Recommender.update losses with the embedding table fixed and free;
the RuntimeError of nlayers = 2 (hyparam.SEQ2SEQ's own value).

The weight seed of a case is searched (1, 2, ..) until EVERY decode step's logit gap is >= 1e-3 -- ten times the project's 1e-4 score-parity
bar, so that no step has to be left out of a comparison of predicted tokens -- and the case predicts >= 4 distinct tokens.
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate as G  # noqa: E402  (installs the shims, puts the reference on sys.path)

from neuroir.models.recommender import Recommender  # noqa: E402
from neuroir.recommender.seq2seq import Seq2seq  # noqa: E402

VT, B, QL, MAXLEN, TL = 200, 5, 7, 6, 6
MIN_GAP, MIN_DISTINCT, MAX_SEED = 1e-3, 4, 64
CASES = (("general", dict(attn_type="general", nhid=64, bidirection=True)), ("dot", dict(attn_type="dot", nhid=64, bidirection=True)),
         ("mlp", dict(attn_type="mlp", nhid=64, bidirection=True)), ("uni", dict(attn_type="general", nhid=96, bidirection=False)),
         ("wide", dict(attn_type="general", nhid=512, bidirection=True)))


def args_for(cfg, **kw):
    a = dict(tgt_vocab_size=VT, nlayers=1, copy_attn=False, reuse_copy_attn=False, force_copy=False, max_query_len=MAXLEN)
    a.update(cfg)
    a.update(kw)
    return G.base_args("SEQ2SEQ", **a)


def load_seed(model, seed):
    sd = model.state_dict()
    model.load_state_dict(G.det_state_dict({k: v.shape for k, v in sd.items()}, seed))
    return model.eval()


@torch.no_grad()
def decode(m, src, lens, src_dict, tgt_dict):
    logits = []
    hook = m.generator.register_forward_hook(lambda mod, inp, out: logits.append(out.detach().clone()))
    try:
        dec = m.decode(source_rep=G.T(src), source_len=G.T(lens), max_len=MAXLEN, src_dict=src_dict, tgt_dict=tgt_dict, src_map=None,
                       alignment=None, blank=None, fill=None, source_vocabs=None)
    finally:
        hook.remove()
    top = torch.stack(logits, 1).topk(2, 2).values                     # [B, max_len, 2]
    return dec["predictions"], dec["attentions"], (top[..., 0] - top[..., 1])


def gen_decode(out):
    rng = np.random.default_rng(83)
    lens = (rng.permutation(QL)[:B] + 1).astype(np.int64)              # pairwise distinct, unsorted
    assert len(set(lens.tolist())) == B and list(lens) != sorted(lens, reverse=True)
    src = G.rand_ids(rng, (B, QL), lens)
    tgt2src = rng.permutation(G.V).astype(np.int64)                     # src_dict[tgt_dict[i]]: tgt_dict = identity, src_dict = a permutation
    tgt_dict, src_dict = list(range(VT)), [int(x) for x in tgt2src]
    tlen = rng.integers(3, TL + 1, size=B)
    tlen[0] = TL
    tw, ts = G.rand_ids(rng, (B, TL), tlen), G.rand_ids(rng, (B, TL), tlen)
    out.update(source_words=src, source_lens=lens, tgt2src=tgt2src, max_len=np.asarray(MAXLEN), vocab=np.asarray(G.V), tgt_vocab=np.asarray(VT),
               target_words=tw, target_seq=ts, target_lens=tlen, min_gap=np.asarray(MIN_GAP))
    seeds = {}
    for tag, cfg in CASES:
        found = None
        for seed in range(1, MAX_SEED + 1):
            m = load_seed(Seq2seq(args_for(cfg)), seed)
            preds, attns, gaps = decode(m, src, lens, src_dict, tgt_dict)
            if float(gaps.min()) >= MIN_GAP and len(set(preds.reshape(-1).tolist())) >= MIN_DISTINCT:
                found = seed
                break
        assert found is not None, "no seed up to %d gives gaps >= %g and >= %d distinct tokens for %s" % (MAX_SEED, MIN_GAP, MIN_DISTINCT, tag)
        assert float(gaps.min()) >= MIN_GAP and len(set(preds.reshape(-1).tolist())) >= MIN_DISTINCT
        seeds[tag] = found
        with torch.no_grad():
            loss = m(source_rep=G.T(src), source_len=G.T(lens), target_rep=G.T(tw), target_len=G.T(tlen), target_seq=G.T(ts), source_map=None,
                     alignment=None)
        sd = m.state_dict()
        out.update({"predictions_" + tag: preds, "attentions_" + tag: attns, "gaps_" + tag: gaps, "loss_" + tag: loss.detach(),
                    "cfg_" + tag: np.asarray(json.dumps(dict(cfg, seed=found))),
                    "sd_keys_" + tag: np.asarray(list(sd.keys())), "sd_shapes_" + tag: np.asarray(json.dumps([list(v.shape) for v in sd.values()]))})
        print(tag, "seed", found, "min gap %.3g" % float(gaps.min()), "distinct", len(set(preds.reshape(-1).tolist())))
    return seeds, (src, lens, tw, ts, tlen)


def gen_nlayers2(out, data):
    """hyparam.SEQ2SEQ's own nlayers = 2: the reference's forward and decode fail"""
    src, lens, tw, ts, tlen = data
    out.update(arch=np.asarray(json.dumps(G.hyparam.get_model_specific_params("SEQ2SEQ", "arch"))),
               data=np.asarray(json.dumps(G.hyparam.get_model_specific_params("SEQ2SEQ", "data"))))
    m = load_seed(Seq2seq(G.base_args("SEQ2SEQ", tgt_vocab_size=VT, nhid=64, copy_attn=False, reuse_copy_attn=False, force_copy=False)), 1)
    msgs = []
    for call in (lambda: m(source_rep=G.T(src), source_len=G.T(lens), target_rep=G.T(tw), target_len=G.T(tlen), target_seq=G.T(ts), source_map=None,
                           alignment=None),
                 lambda: m.decode(source_rep=G.T(src), source_len=G.T(lens), max_len=MAXLEN, src_dict=list(range(G.V)), tgt_dict=list(range(VT)),
                                  src_map=None, alignment=None, blank=None, fill=None, source_vocabs=None)):
        try:
            with torch.no_grad():
                call()
            msgs.append("")
        except RuntimeError as e:
            msgs.append(str(e))
    assert all(s.startswith("Expected hidden[0] size (2, %d, 64), got [1, %d, 64]" % (B, B)) for s in msgs), msgs
    out.update(nlayers2_error=np.asarray(msgs[0]), nlayers2_error_type=np.asarray("RuntimeError"))


def gen_train(out, seed):
    """three updates of the real reference (models/recommender.py:160-227; clip 10, Adam 1e-3, dropout 0) alternating over two batches, in
    the collate layout [B, 1, .]; with the embedding table fixed and free"""
    cfg = dict(CASES)["general"]
    for tag, fix in (("fix", True), ("free", False)):
        rng = np.random.default_rng(89)
        bs = []
        for _ in range(2):
            lens = (rng.permutation(QL)[:B] + 1).astype(np.int64)
            tlen = rng.integers(3, TL + 1, size=B)
            tlen[0] = TL
            bs.append(dict(source_words=G.rand_ids(rng, (B, QL), lens)[:, None], source_lens=lens[:, None],
                           target_words=G.rand_ids(rng, (B, TL), tlen)[:, None], target_seq=G.rand_ids(rng, (B, TL), tlen)[:, None],
                           target_lens=tlen[:, None]))
        args = args_for(cfg, dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0, momentum=0,
                        grad_clipping=10.0, fix_embeddings=fix)
        r = Recommender(args, list(range(G.V)), list(range(VT)))
        load_seed(r.network, seed)
        r.init_optimizer()
        losses = [float(r.update({k: G.T(v) for k, v in bs[step % 2].items()})) for step in range(3)]
        if tag == "fix":
            for bi, b in enumerate(bs):
                out.update({"train_b%d_%s" % (bi, k): v for k, v in b.items()})
        out["train_losses_" + tag] = np.asarray(losses, np.float64)
        print("update losses", tag, losses)


if __name__ == "__main__":
    torch.manual_seed(G.SEED)
    torch.set_num_threads(4)
    out = {}
    seeds, data = gen_decode(out)
    gen_nlayers2(out, data)
    gen_train(out, seeds["general"])
    G.save("seq2seq", **out)
