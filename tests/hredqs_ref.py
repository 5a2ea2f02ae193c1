"""The acceptance criterion of the HredQS mirror (csrc/hredqs.hip, recommender/hredqs.py): a restatement of
neuroir/recommender/hredqs.py:46-230 in the reference's op order -- embedding, RNNEncoder over the valid part of every query (packed-sequence
semantics, the memory bank zero beyond each length and as wide as the input), the max over ALL positions of that bank, the unidirectional
session LSTM carrying (h, c) over the S queries of a session, its states of EVERY step concatenated in STEP-major order, the decoder rows in
(b, s) order started from those states as they lie (decode row r: step r // B of session r % B), and per step the decoder LSTM, generator,
arg-max, the token mapped back to its source id -- evaluated in float64 as the reference and in float32 on the CPU as the yardstick of what
fp32 arithmetic costs, plus the bound a result has to meet.

Bound (the form of tests/seq2seq_ref.py) on the session states `encode` returns: with s = max |ref64|, e = max |got - ref64| / s and e_chain
the same figure for the float32 chain,

    e <= MARGIN * max(e_chain, 2^-23) + n_split * FMT["fp16x2"]

n_split: the split products on the path of the last session state: the query encoder's gate product and its QL recurrent products, the
session LSTM's gate product and its S recurrent products -- QL + S + 2 when every one of them runs on fp16 term pairs (the format's own
figure, whichever of the encoder's kernels the size picks), 0 for an all-fp32 path.  The decoder's and the generator's split products decide
tokens, not states.
MARGIN: the largest (e - fmt) / max(e_chain, 2^-23) the GPU tests print on the MI355X, doubled, rounded up to a power of two, never above
gemm_ref.MARGIN_CAP.  2 is the rule's starting value; DESIGN.md section 16 says which ratios were measured.

`fault` plants one of five mistakes, to show on the CPU that the criterion rejects them (tests/test_hredqs_host.py):
    "natural_pairing"    decode row (b, s) starts from the state of step s of session b
    "pool_valid_only"    the max runs over the valid positions of a query only
    "no_session_carry"   the session LSTM starts every step from the zero state
    "no_decoder_carry"   the decoder state is not carried between steps (every step starts from the initial state)
    "mean_pool"          mean over the positions instead of max
"""
import json

import numpy as np
import torch

import gemm_ref
from conftest import T, load_golden
from seq2seq_ref import _cast, _cell, encode as encode_queries, figures

EMB = "embedder.word_embeddings.make_embedding.emb_luts.0.weight"
SES = "session_encoder.encoder.rnns.0."
DEC = "decoder.decoder.rnn."
MARGIN = 2.0
EPS = gemm_ref.EPS
FAULTS = ("natural_pairing", "pool_valid_only", "no_session_carry", "no_decoder_carry", "mean_pool")
BOS, PAD = 2, 0


def _lstm(sd, prefix):
    return [sd[prefix + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


def session_steps(sd, src, lens, fault=None):
    """src [B,S,QL], lens [B,S] -> (h, c) of every session step, [B,S,HS] each"""
    B, S, QL = src.shape
    bank, _, _ = encode_queries(sd, sd[EMB][src.reshape(B * S, QL)], lens.reshape(-1), False)          # [R,QL,nhid], zero beyond each length
    if fault == "mean_pool":
        pooled = bank.mean(1)
    elif fault == "pool_valid_only":
        valid = (torch.arange(QL).view(1, QL) < lens.reshape(-1, 1)).unsqueeze(2)
        pooled = bank.masked_fill(~valid, float("-inf")).max(1)[0]
    else:
        pooled = bank.max(1)[0]
    pooled = pooled.view(B, S, -1)
    p = _lstm(sd, SES)
    HS = p[1].shape[1]
    h, c = pooled.new_zeros(B, HS), pooled.new_zeros(B, HS)
    hs, cs = [], []
    for s in range(S):
        if fault == "no_session_carry":
            h, c = torch.zeros_like(h), torch.zeros_like(c)
        h, c = _cell(pooled[:, s], h, c, *p)
        hs.append(h)
        cs.append(c)
    return torch.stack(hs, 1), torch.stack(cs, 1)


def paired(hs, cs, fault=None):
    """the decoder's initial states, row r = b S + s: the states in STEP-major order, as they lie (natural_pairing: in (b, s) order)"""
    B, S, HS = hs.shape
    if fault == "natural_pairing":
        return hs.reshape(B * S, HS), cs.reshape(B * S, HS)
    return hs.transpose(0, 1).reshape(B * S, HS), cs.transpose(0, 1).reshape(B * S, HS)


@torch.no_grad()
def decode(sd, src, lens, max_len, tgt2src=None, dtype=torch.float64, fault=None, force=None):
    """greedy decode -> dict(predictions [B,S,max_len], gaps [B,S,max_len]: top-1 minus top-2 logit of every step, enc_h / enc_c
    [1, S B, HS]: what `encode` returns).  force [B,S,max_len] (optional): the tokens fed back are these instead of the chain's own."""
    sd = _cast(sd, dtype)
    B, S, _ = src.shape
    table = sd[EMB]
    hs, cs = session_steps(sd, src, lens, fault)
    h0, c0 = paired(hs, cs, fault)
    h, c = h0, c0
    p = _lstm(sd, DEC)
    tok = torch.full((B * S,), BOS, dtype=torch.long)
    preds, gaps = [], []
    for step in range(max_len):
        if fault == "no_decoder_carry":
            h, c = h0, c0
        h, c = _cell(table[tok], h, c, *p)
        logits = h @ sd["generator.weight"].t() + sd["generator.bias"]
        top = logits.topk(min(2, logits.shape[1]), 1).values
        pred = logits.max(1)[1]
        preds.append(pred)
        gaps.append(top[:, 0] - top[:, -1])
        fed = pred if force is None else force.reshape(B * S, -1)[:, step]
        tok = tgt2src[fed] if tgt2src is not None else fed
        tok = torch.where((tok >= 0) & (tok < table.shape[0]), tok, torch.ones_like(tok))
    HS = hs.shape[2]
    return dict(predictions=torch.stack(preds, 1).view(B, S, max_len), gaps=torch.stack(gaps, 1).view(B, S, max_len),
                enc_h=hs.transpose(0, 1).reshape(1, S * B, HS), enc_c=cs.transpose(0, 1).reshape(1, S * B, HS))


def loss(sd, src, lens, tgt, tseq):
    """hredqs.py:89-143 on the tensors of sd as they are (they may require grad) -> scalar loss"""
    B, S, _ = src.shape
    R = B * S
    table = sd[EMB]
    h, c = paired(*session_steps(sd, src, lens))
    p = _lstm(sd, DEC)
    emb = table[tgt.reshape(R, -1)]
    hs = []
    for t in range(emb.shape[1]):
        h, c = _cell(emb[:, t], h, c, *p)
        hs.append(h)
    logits = (torch.stack(hs, 1) @ sd["generator.weight"].t() + sd["generator.bias"])[:, :-1]
    target = tseq.reshape(R, -1)[:, 1:]
    ll = torch.log_softmax(logits, -1).gather(2, target.unsqueeze(2)).squeeze(2)
    return (-ll * (target != PAD).to(ll.dtype)).sum(1).mean()


def n_split(QL, S):
    """every product on the path of the last session state, taken as a split one (the module docstring)"""
    return QL + S + 2


def accept(got, ref, chain, nsplit, margin=None):
    """(ok, figures): the criterion of the module docstring on one state tensor"""
    margin = MARGIN if margin is None else margin
    assert margin <= gemm_ref.MARGIN_CAP
    r = figures(got, ref, chain, nsplit)
    r["bound"] = margin * max(r["e_chain"], EPS) + r["extra"]
    return r["e"] <= r["bound"], r


def accept_decode(got, ref, chain, nsplit, margin=None):
    """the whole criterion: the predicted tokens are the float64 restatement's, exactly (the fixtures keep every step's logit gap >= 1e-3),
    and both session states meet the bound -> (ok, figures of the worse state)"""
    same = bool(torch.equal(torch.as_tensor(np.asarray(got["predictions"].cpu())), ref["predictions"]))
    okh, fh = accept(got["enc_h"], ref["enc_h"], chain["enc_h"], nsplit, margin)
    okc, fc = accept(got["enc_c"], ref["enc_c"], chain["enc_c"], nsplit, margin)
    fig = fh if fh["e"] - fh["bound"] >= fc["e"] - fc["bound"] else fc
    fig["predictions_equal"] = same
    return okh and okc and same, fig


# ------------------------------------------------------------------ the fixture cases (tests/golden/generate_hredqs.py)
CASES = ("h64", "h96", "h256", "h1024")


def case_cfg(tag):
    return json.loads(str(load_golden("hredqs")["cfg_" + tag]))


def case_args(tag, **kw):
    from context_attentive_ir_amd.config import default_args
    g = load_golden("hredqs")
    c = case_cfg(tag)
    return default_args("HREDQS", **dict(dict(src_vocab_size=int(g["vocab"]), tgt_vocab_size=int(g["tgt_vocab"]), nlayers=1, nhid=c["nhid"],
                                              nhid_session=c["nhid_session"], bidirection=False, max_query_len=int(g["max_len"])), **kw))


def case(tag):
    """(network on the CPU with the fixture's weights, its config, the golden arrays of the case and of its batch under their plain names)"""
    from context_attentive_ir_amd.detinit import det_state_dict
    from context_attentive_ir_amd.recommender import HredQS
    g = load_golden("hredqs")
    c = case_cfg(tag)
    net = HredQS(case_args(tag))
    net.load_state_dict(det_state_dict({k: v.shape for k, v in net.state_dict().items()}, c["seed"]))
    net.eval()
    arrs = {k[:-len(tag) - 1]: v for k, v in g.items() if k.endswith("_" + tag)}
    sfx = "_b%ds%d" % (c["B"], c["S"])
    arrs.update({k[:-len(sfx)]: T(v) for k, v in g.items() if k.endswith(sfx)})
    arrs.update(tgt2src=g["tgt2src"], max_len=int(g["max_len"]))
    return net, c, arrs
