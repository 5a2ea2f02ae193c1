#!/usr/bin/env python
"""Golden fixtures of the reference's ACG -- Seq2seq with copy_attn (neuroir/recommender/seq2seq.py, modules/copy_generator.py,
utils/copy_utils.py) -- and of Recommender (neuroir/models/recommender.py) with model_type ACG, run on CPU.

Reuses generate.py's compatibility shims and helpers by import; like there, the fixture carries ids, maps and outputs only -- every consumer
regenerates the weights from their state-dict keys (context_attentive_ir_amd.detinit, seed recorded per case).

    python tests/golden/generate_acg.py          # rewrites tests/golden/acg.npz

Vocabularies: 260 source words ("w4" .. "w259" behind the four specials), of which the first 200 are target words too: a source word >= 200 is
<unk> in the target dictionary and can only be copied.  Every row has its own dynamic dictionary (a Vocabulary over its source words, as
objects/query.py:56-58 builds it), `src_map`, `blank` / `fill` (collapse_copy_scores) and `alignment` come from the reference's own helpers.
Decode: B = 5 sources of width 7 with pairwise distinct, unsorted lengths, one row with a repeated out-of-vocabulary word, max_len 6.

Cases (nlayers = 1): general / dot / mlp at nhid 64 with reuse_copy_attn, general at nhid 64 with a copy attention of its own, general at
nhid 512; one force_copy loss.  Recorded per case: predictions (extended ids), attentions, the relative gap (top1 - top2) / top1 of the
collapsed distribution of every step, the teacher-forced loss; for the general case three Recommender.update losses with the table fixed
and free.

The weight seed of a case is searched (1, 2, ..) until every step's relative gap is >= 1e-3 -- ten times the project's 1e-4 parity bar, so
no step has to be left out of a comparison of tokens -- and the decode holds at least one copied word (prediction >= VT), one collapsed
winner (a target word that wins only with its copy mass: prediction != arg-max of the logits) and one generator winner (prediction == arg-max
of the logits).  With detinit's weights the switch stays near 1/2 and the softmax over 200 words is flat, so a generator winner WITHOUT any copy
mass (its word absent from the row's source) did not occur for any seed up to 64 on three input draws; `classes_<tag>` records that count as
its fourth entry, and the class is planted at the C ABI instead (tests/test_gpu_acg_envelope.py).
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate as G  # noqa: E402  (installs the shims, puts the reference on sys.path)

from neuroir.inputters.vocabulary import Vocabulary  # noqa: E402
from neuroir.models.recommender import Recommender  # noqa: E402
from neuroir.recommender.seq2seq import Seq2seq  # noqa: E402
from neuroir.utils.copy_utils import align, collapse_copy_scores, make_src_map  # noqa: E402

VS, VT, B, QL, MAXLEN, TL = 260, 200, 5, 7, 6, 6
MIN_GAP, MAX_SEED = 1e-3, 64
CASES = (("general", dict(attn_type="general", nhid=64, reuse_copy_attn=True)), ("dot", dict(attn_type="dot", nhid=64, reuse_copy_attn=True)),
         ("mlp", dict(attn_type="mlp", nhid=64, reuse_copy_attn=True)), ("own", dict(attn_type="general", nhid=64, reuse_copy_attn=False)),
         ("wide", dict(attn_type="general", nhid=512, reuse_copy_attn=True)))


def word(i):
    return "w%d" % i


def dictionaries():
    src_dict, tgt_dict = Vocabulary(), Vocabulary()
    src_dict.add_tokens([word(i) for i in range(4, VS)])
    tgt_dict.add_tokens([word(i) for i in range(4, VT)])
    assert len(src_dict) == VS and len(tgt_dict) == VT and src_dict[word(VS - 1)] == VS - 1 and tgt_dict[word(VT)] == 1
    return src_dict, tgt_dict


def args_for(cfg, **kw):
    a = dict(src_vocab_size=VS, tgt_vocab_size=VT, nlayers=1, bidirection=True, copy_attn=True, force_copy=False, max_query_len=MAXLEN)
    a.update(cfg)
    a.update(kw)
    return G.base_args("ACG", **a)


def load_seed(model, seed):
    sd = model.state_dict()
    model.load_state_dict(G.det_state_dict({k: v.shape for k, v in sd.items()}, seed))
    return model.eval()


def batch(rng, repeat_oov):
    """one batch in the reference's collate layout (inputters/recommender/vector.py:59-128), rows [B, .] (the session axis is added by the
    caller): ids, lengths, the rows' dynamic dictionaries, src_map and alignment lists"""
    lens = (rng.permutation(QL)[:B] + 1).astype(np.int64)              # pairwise distinct, unsorted
    lens[np.argmax(lens)] = QL                                          # the batch is as wide as its longest row, as the reference's collate makes it
    assert len(set(lens.tolist())) == B and list(lens) != sorted(lens, reverse=True)
    src = G.rand_ids(rng, (B, QL), lens, hi=VS)
    if repeat_oov:
        r = int(np.argmax(lens))                                        # the longest row: one out-of-vocabulary word at two positions
        src[r, 0] = src[r, 2] = VS - 3
    tlen = rng.integers(3, TL + 1, size=B)
    tlen[0] = TL
    tw = np.zeros((B, TL), np.int64)
    for b in range(B):                                                  # targets: half of the words come from the row's own source
        for t in range(int(tlen[b])):
            tw[b, t] = src[b, rng.integers(0, lens[b])] if rng.random() < 0.5 else rng.integers(4, VS)
    if repeat_oov:
        tw[r, 1] = VS - 3                                               # the repeated word is a target too: its copy mass is a sum in the loss
    ts = np.where(tw < VT, tw, 1)                                       # the same words in the target dictionary
    vocabs, maps, als = [], [], []
    for b in range(B):
        v = Vocabulary()
        v.add_tokens([word(int(i)) for i in src[b, :lens[b]]])
        vocabs.append(v)
        maps.append(torch.LongTensor([v[word(int(i))] for i in src[b, :lens[b]]]))
        als.append(torch.LongTensor([v[word(int(i))] for i in tw[b, :tlen[b]]]))
    return dict(src=src, lens=lens, tw=tw, ts=ts, tlen=tlen, vocabs=vocabs, maps=maps, als=als)


def pad_lists(rows, width, fill):
    out = np.full((len(rows), width), fill, np.int64)
    for i, r in enumerate(rows):
        out[i, :len(r)] = np.asarray(r, np.int64)
    return out


def vocab_ids(vocabs, src_dict):
    """[B, CVmax] source id of the word at every slot of every row's dictionary, -1 behind its end"""
    return pad_lists([[src_dict[v[c]] for c in range(len(v))] for v in vocabs], max(len(v) for v in vocabs), -1)


@torch.no_grad()
def decode(m, d, src_dict, tgt_dict, blank, fill):
    logits, probs = [], []
    h1 = m.generator.register_forward_hook(lambda mod, inp, out: logits.append(out.detach().clone()))
    # the hook keeps the tensor decode() collapses IN PLACE (squeeze(1) is a view of it): after the call it holds the collapsed distribution
    h2 = m.copy_generator.register_forward_hook(lambda mod, inp, out: probs.append(out))
    try:
        dec = m.decode(source_rep=G.T(d["src"]), source_len=G.T(d["lens"]), max_len=MAXLEN, src_dict=src_dict, tgt_dict=tgt_dict,
                       src_map=make_src_map(d["maps"]), alignment=None, blank=blank, fill=fill, source_vocabs=d["vocabs"])
    finally:
        h1.remove()
        h2.remove()
    P = torch.cat(probs, 1)                                              # [B, max_len, VT + CV]
    top = P.topk(2, 2).values
    lg = torch.cat(logits, 1)
    lg[:, :, 0] = -1e-20
    return dec["predictions"], dec["attentions"], (top[..., 0] - top[..., 1]) / top[..., 0], lg.max(2)[1]


def classes(preds, gen_top, fill):
    """(copied, collapsed winner, generator winner, of these without any copy mass) counts of a decode"""
    cop = col = gen = pure = 0
    for b in range(preds.shape[0]):
        for s in range(preds.shape[1]):
            p = int(preds[b, s])
            if p >= VT:
                cop += 1
            elif p != int(gen_top[b, s]):
                col += 1
            else:
                gen += 1
                pure += p not in fill[b]
    return cop, col, gen, pure


def gen_decode(out):
    rng = np.random.default_rng(97)
    src_dict, tgt_dict = dictionaries()
    d = batch(rng, repeat_oov=True)
    blank, fill = collapse_copy_scores(tgt_dict, d["vocabs"])
    CV = max(len(v) for v in d["vocabs"])
    al = align(d["als"])
    out.update(source_words=d["src"], source_lens=d["lens"], target_words=d["tw"], target_seq=d["ts"], target_lens=d["tlen"],
               src_map=pad_lists([m.tolist() for m in d["maps"]], QL, 0), alignment=pad_lists([a.tolist() for a in d["als"]], TL, 0),
               src_vocab_ids=vocab_ids(d["vocabs"], src_dict), blank=pad_lists(blank, CV, -1), fill=pad_lists(fill, CV, -1),
               max_len=np.asarray(MAXLEN), vocab=np.asarray(VS), tgt_vocab=np.asarray(VT), min_gap=np.asarray(MIN_GAP))
    seeds = {}
    for tag, cfg in CASES:
        found = None
        for seed in range(1, MAX_SEED + 1):
            m = load_seed(Seq2seq(args_for(cfg)), seed)
            preds, attns, gaps, gen_top = decode(m, d, src_dict, tgt_dict, blank, fill)
            cls = classes(preds, gen_top, fill)
            if float(gaps.min()) >= MIN_GAP and min(cls[:3]) >= 1:
                found = seed
                break
        assert found is not None, "no seed up to %d gives gaps >= %g and every winner class for %s" % (MAX_SEED, MIN_GAP, tag)
        seeds[tag] = found
        src_map = make_src_map(d["maps"])
        with torch.no_grad():
            loss = m(source_rep=G.T(d["src"]), source_len=G.T(d["lens"]), target_rep=G.T(d["tw"]), target_len=G.T(d["tlen"]),
                     target_seq=G.T(d["ts"]), source_map=src_map, alignment=al)
        sd = m.state_dict()
        out.update({"predictions_" + tag: preds, "attentions_" + tag: attns, "gaps_" + tag: gaps, "gen_top_" + tag: gen_top, "loss_" + tag: loss.detach(),
                    "classes_" + tag: np.asarray(cls), "cfg_" + tag: np.asarray(json.dumps(dict(cfg, seed=found))),
                    "sd_keys_" + tag: np.asarray(list(sd.keys())), "sd_shapes_" + tag: np.asarray(json.dumps([list(v.shape) for v in sd.values()]))})
        print(tag, "seed", found, "min gap %.3g" % float(gaps.min()), "copied / collapsed / generator / of these pure", cls, "loss %.6f" % float(loss))
        if tag == "general":
            mf = load_seed(Seq2seq(args_for(cfg, force_copy=True)), found)
            with torch.no_grad():
                lf = mf(source_rep=G.T(d["src"]), source_len=G.T(d["lens"]), target_rep=G.T(d["tw"]), target_len=G.T(d["tlen"]),
                        target_seq=G.T(d["ts"]), source_map=src_map, alignment=al)
            out["loss_force_copy"] = lf.detach()
            print("force_copy loss %.6f" % float(lf))
    return seeds


def gen_train(out, seed):
    """three updates of the real reference (models/recommender.py:160-227; clip 10, Adam 1e-3, dropout 0) alternating over two batches, in
    the collate layout [B, 1, .] with src_map / alignment lists; with the embedding table fixed and free"""
    cfg = dict(CASES)["general"]
    for tag, fix in (("fix", True), ("free", False)):
        rng = np.random.default_rng(101)
        src_dict, tgt_dict = dictionaries()
        bs = [batch(rng, repeat_oov=False) for _ in range(2)]
        args = args_for(cfg, dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0, momentum=0,
                        grad_clipping=10.0, fix_embeddings=fix)
        r = Recommender(args, src_dict, tgt_dict)
        load_seed(r.network, seed)
        r.init_optimizer()
        losses = []
        for step in range(3):
            d = bs[step % 2]
            ex = dict(source_words=G.T(d["src"][:, None]), source_lens=G.T(d["lens"][:, None]), target_words=G.T(d["tw"][:, None]),
                      target_seq=G.T(d["ts"][:, None]), target_lens=G.T(d["tlen"][:, None]), src_map=d["maps"], alignment=d["als"])
            losses.append(float(r.update(ex)))
        if tag == "fix":
            for bi, d in enumerate(bs):
                out.update({"train_b%d_source_words" % bi: d["src"][:, None], "train_b%d_source_lens" % bi: d["lens"][:, None],
                            "train_b%d_target_words" % bi: d["tw"][:, None], "train_b%d_target_seq" % bi: d["ts"][:, None],
                            "train_b%d_target_lens" % bi: d["tlen"][:, None], "train_b%d_src_map" % bi: pad_lists([m.tolist() for m in d["maps"]], QL, 0),
                            "train_b%d_alignment" % bi: pad_lists([a.tolist() for a in d["als"]], TL, 0)})
        out["train_losses_" + tag] = np.asarray(losses, np.float64)
        print("update losses", tag, losses)


if __name__ == "__main__":
    torch.manual_seed(G.SEED)
    torch.set_num_threads(4)
    out = {}
    seeds = gen_decode(out)
    out.update(arch=np.asarray(json.dumps(G.hyparam.get_model_specific_params("ACG", "arch"))),
               data=np.asarray(json.dumps(G.hyparam.get_model_specific_params("ACG", "data"))))
    gen_train(out, seeds["general"])
    G.save("acg", **out)
