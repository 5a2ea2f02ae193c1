#!/usr/bin/env python
"""Golden fixtures of the reference's HredQS (neuroir/recommender/hredqs.py) and of Recommender with model_type HREDQS
(neuroir/models/recommender.py), run on CPU.

Reuses generate.py's compatibility shims and helpers by import; like there, the fixture carries ids and outputs only -- every consumer
regenerates the weights from their state-dict keys (context_attentive_ir_amd.detinit, seed recorded per case).

    python tests/golden/generate_hredqs.py          # rewrites tests/golden/hredqs.npz

Cases (rnn_type LSTM, bidirection False, nlayers 1, tgt_vocab_size 200), (nhid, nhid_session) = (64, 64), (64, 96), (128, 256) with B = 3
sessions of S = 4 queries and (512, 1024) with B = 2, S = 3; queries of width 7 with lengths in 1..7 (at least one full, at least one
shorter row), max_len 6, a permuted src_dict.  Recorded per case: predictions, the top-1 minus top-2 logit of every step, the states `encode`
returns (as the reference runs, in float32, and from the same classes cast to float64), the teacher-forced loss; for the first case three
Recommender.update losses with the embedding table fixed and free; the hyparam table; the error of bidirection = True (hyparam.HREDQS's own
value); what nlayers = 2 and rnn_type GRU do.

The weight seed of a case is searched over 1..64 until every decode step's logit gap is >= 1e-3, the case decodes >= 4 distinct rows and
>= 4 distinct tokens, and the tokens differ from those the natural (b, s) pairing of states and decode rows would give (the reference pairs
decode row r with the state of step r // B of session r % B).
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
from neuroir.recommender.hredqs import HredQS  # noqa: E402

VT, QL, MAXLEN, TL = 200, 7, 6, 6
MIN_GAP, MIN_DISTINCT, MAX_SEED = 1e-3, 4, 64
CASES = (("h64", dict(nhid=64, nhid_session=64, B=3, S=4)), ("h96", dict(nhid=64, nhid_session=96, B=3, S=4)),
         ("h256", dict(nhid=128, nhid_session=256, B=3, S=4)), ("h1024", dict(nhid=512, nhid_session=1024, B=2, S=3)))


def args_for(cfg, **kw):
    a = dict(tgt_vocab_size=VT, nlayers=1, bidirection=False, max_query_len=MAXLEN, nhid=cfg["nhid"], nhid_session=cfg["nhid_session"])
    a.update(kw)
    return G.base_args("HREDQS", **a)


def load_seed(model, seed):
    sd = model.state_dict()
    model.load_state_dict(G.det_state_dict({k: v.shape for k, v in sd.items()}, seed))
    return model.eval()


@torch.no_grad()
def decode(m, src, lens, src_dict, tgt_dict, natural=False):
    """-> (predictions [B,S,max_len], gaps [B,S,max_len]); natural: the states are handed over in (b, s) order instead"""
    B, S = src.shape[:2]
    logits = []
    hook = m.generator.register_forward_hook(lambda mod, inp, out: logits.append(out.detach().clone()))
    enc = m.encode
    if natural:
        m.encode = lambda *a, **k: tuple(s.view(1, S, B, -1).transpose(1, 2).reshape(1, B * S, -1) for s in enc(*a, **k))
    try:
        dec = m.decode(source_rep=G.T(src), source_len=G.T(lens), max_len=MAXLEN, src_dict=src_dict, tgt_dict=tgt_dict, src_map=None,
                       alignment=None, blank=None, fill=None, source_vocabs=None)
    finally:
        hook.remove()
        if natural:
            del m.encode
    top = torch.stack(logits, 1).topk(2, 2).values                     # [B S, max_len, 2]
    return dec["predictions"], (top[..., 0] - top[..., 1]).view(B, S, MAXLEN)


def batch(rng, B, S):
    lens = rng.integers(1, QL + 1, size=(B, S)).astype(np.int64)
    lens[0, 0], lens[-1, -1] = QL, 2
    src = G.rand_ids(rng, (B, S, QL), lens)
    tlen = rng.integers(3, TL + 1, size=(B, S))
    tlen[0, 0] = TL
    return dict(source_words=src, source_lens=lens, target_words=G.rand_ids(rng, (B, S, TL), tlen), target_seq=G.rand_ids(rng, (B, S, TL), tlen),
                target_lens=tlen)


def gen_decode(out):
    rng = np.random.default_rng(97)
    tgt2src = rng.permutation(G.V).astype(np.int64)                     # src_dict[tgt_dict[i]]: tgt_dict = identity, src_dict = a permutation
    tgt_dict, src_dict = list(range(VT)), [int(x) for x in tgt2src]
    out.update(tgt2src=tgt2src, max_len=np.asarray(MAXLEN), vocab=np.asarray(G.V), tgt_vocab=np.asarray(VT), min_gap=np.asarray(MIN_GAP),
               cases=np.asarray([t for t, _ in CASES]))
    data, seeds = {}, {}
    for tag, cfg in CASES:
        shape = (cfg["B"], cfg["S"])
        if shape not in data:
            data[shape] = batch(rng, *shape)
            assert (data[shape]["source_lens"] == QL).any() and (data[shape]["source_lens"] < QL).any()
            out.update({"%s_b%ds%d" % ((k,) + shape): v for k, v in data[shape].items()})
        d = data[shape]
        found = None
        for seed in range(1, MAX_SEED + 1):
            m = load_seed(HredQS(args_for(cfg)), seed)
            preds, gaps = decode(m, d["source_words"], d["source_lens"], src_dict, tgt_dict)
            rows = preds.reshape(-1, MAXLEN)
            if (float(gaps.min()) >= MIN_GAP and len(set(map(tuple, rows.tolist()))) >= MIN_DISTINCT
                    and len(set(rows.reshape(-1).tolist())) >= MIN_DISTINCT
                    and not torch.equal(decode(m, d["source_words"], d["source_lens"], src_dict, tgt_dict, natural=True)[0], preds)):
                found = seed
                break
        assert found is not None, "no seed up to %d meets the conditions for %s" % (MAX_SEED, tag)
        seeds[tag] = found
        B, S = shape
        with torch.no_grad():
            h, c = m.encode(G.T(d["source_words"]).view(B * S, QL), G.T(d["source_lens"]).view(-1), B, S)
            loss = m(source_rep=G.T(d["source_words"]), source_len=G.T(d["source_lens"]), target_rep=G.T(d["target_words"]),
                     target_len=G.T(d["target_lens"]), target_seq=G.T(d["target_seq"]), source_map=None, alignment=None)
            h64, c64 = load_seed(HredQS(args_for(cfg)), found).double().encode(G.T(d["source_words"]).view(B * S, QL),
                                                                               G.T(d["source_lens"]).view(-1), B, S)
        sd = m.state_dict()
        out.update({"predictions_" + tag: preds, "gaps_" + tag: gaps, "enc_h_" + tag: h, "enc_c_" + tag: c, "loss_" + tag: loss.detach(),
                    "enc_h64_" + tag: h64, "enc_c64_" + tag: c64,
                    "cfg_" + tag: np.asarray(json.dumps(dict(cfg, seed=found))),
                    "sd_keys_" + tag: np.asarray(list(sd.keys())), "sd_shapes_" + tag: np.asarray(json.dumps([list(v.shape) for v in sd.values()]))})
        print(tag, "seed", found, "min gap %.3g" % float(gaps.min()), "distinct rows", len(set(map(tuple, rows.tolist()))))
    return seeds, data


def outcome(call):
    try:
        with torch.no_grad():
            call()
        return "", ""
    except Exception as e:  # noqa: BLE001  (the type is what is being recorded)
        return type(e).__name__, str(e)


def gen_configs(out, data):
    """hyparam.HREDQS's own bidirection = True, nlayers = 2 and rnn_type GRU: what the reference's forward / decode do"""
    out.update(arch=np.asarray(json.dumps(G.hyparam.get_model_specific_params("HREDQS", "arch"))),
               data=np.asarray(json.dumps(G.hyparam.get_model_specific_params("HREDQS", "data"))))
    d = data[(3, 4)]
    cfg = dict(CASES)["h64"]
    for name, kw in (("bidirection", dict(bidirection=True)), ("nlayers2", dict(nlayers=2)), ("gru", dict(rnn_type="GRU"))):
        m = load_seed(HredQS(args_for(cfg, **kw)), 1)
        fwd = outcome(lambda: m(source_rep=G.T(d["source_words"]), source_len=G.T(d["source_lens"]), target_rep=G.T(d["target_words"]),
                                target_len=G.T(d["target_lens"]), target_seq=G.T(d["target_seq"]), source_map=None, alignment=None))
        dec = outcome(lambda: m.decode(source_rep=G.T(d["source_words"]), source_len=G.T(d["source_lens"]), max_len=MAXLEN,
                                       src_dict=list(range(G.V)), tgt_dict=list(range(VT)), src_map=None, alignment=None, blank=None, fill=None,
                                       source_vocabs=None))
        print(name, "forward:", fwd, "decode:", dec)
        out.update({name + "_error_type": np.asarray(fwd[0]), name + "_error": np.asarray(fwd[1]),
                    name + "_decode_error_type": np.asarray(dec[0]), name + "_decode_error": np.asarray(dec[1])})
        if name == "nlayers2":
            out["nlayers2_sd_keys"] = np.asarray(list(m.state_dict().keys()))


def gen_train(out, seed):
    """three updates of the real reference (models/recommender.py:160-227; clip 10, Adam 1e-3, dropout 0) alternating over two batches
    [B, S, .]; with the embedding table fixed and free"""
    cfg = dict(CASES)["h64"]
    for tag, fix in (("fix", True), ("free", False)):
        rng = np.random.default_rng(101)
        bs = [batch(rng, 3, 4) for _ in range(2)]
        args = args_for(cfg, dropout_emb=0.0, dropout=0.0, dropout_rnn=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0, momentum=0,
                        grad_clipping=10.0, fix_embeddings=fix, copy_attn=False)
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
    gen_configs(out, data)
    gen_train(out, seeds["h64"])
    G.save("hredqs", **out)
