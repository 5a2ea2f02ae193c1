"""The acceptance criterion of the Seq2seq decoder (csrc/seq2seq.hip, recommender/seq2seq.py): a restatement of
neuroir/recommender/seq2seq.py:48-195 in the reference's op order -- embedding, RNNEncoder over the valid part of every source (packed-sequence
semantics), the decoder's initial state taken in the reference's LENGTH-SORTED order, and per step the decoder LSTM (no input feed),
GlobalAttention ('general' / 'dot' / 'mlp'; masked softmax, context, linear_out, tanh for general / dot only), generator, arg-max, the token
mapped back to its source id -- evaluated in float64 as the reference and in float32 on the CPU as the yardstick of what fp32 arithmetic costs,
plus the bound a result has to meet.

Bound (the form of tests/arcii_ref.py and tests/gemm_ref.py) on `attentions`: with s = max |ref64|, e = max |got - ref64| / s and e_chain the
same figure for the float32 chain,

    e <= MARGIN * max(e_chain, 2^-23) + n_split * FMT["fp16x2"]

n_split: the split products on the path of an attention row: one recurrent product per decoder step on the fp16-term step (max_len of them
for the last row), 0 on the fp32 step.  The generator's split product decides tokens, not attentions.
MARGIN: the largest (e - fmt) / max(e_chain, 2^-23) the GPU tests print on the MI355X, doubled, rounded up to a power of two, never above
gemm_ref.MARGIN_CAP.  2 is the rule's starting value (what arci_ref / arcii_ref ended on); DESIGN.md section 15 says which ratios were
measured and which were not.

`fault` plants one of four mistakes, to show on the CPU that the bound rejects them (tests/test_seq2seq_host.py):
    "orig_order"  the decoder starts from the encoder's final state in ORIGINAL row order
    "no_mask"     positions past the source length take part in the softmax
    "tanh_swap"   tanh applied behind linear_out for 'mlp', left out for 'general' / 'dot'
    "no_carry"    the decoder state is not carried between steps (every step starts from the initial state)
"""
import json

import numpy as np
import torch

import gemm_ref
from conftest import T, load_golden

EMB = "embedder.word_embeddings.make_embedding.emb_luts.0.weight"
ENC = "encoder.encoder.rnns.0."
DEC = "decoder.decoder.rnn."
ATT = "decoder.decoder.attn."
MARGIN = 2.0
EPS = gemm_ref.EPS
FAULTS = ("orig_order", "no_mask", "tanh_swap", "no_carry")
BOS, PAD = 2, 0


def _cell(x, h, c, wih, whh, bih, bhh):
    g = x @ wih.t() + bih + h @ whh.t() + bhh
    i, f, gg, o = g.chunk(4, 1)
    c2 = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c2), c2


def encode(sd, emb, lens, bidirection):
    """RNNEncoder (1 layer, use_last) -> (memory bank [B,T,nhid], zero past the length; h_n, c_n [ND,B,nhid/ND] in ORIGINAL row order)"""
    B, Tn, _ = emb.shape
    banks, hn, cn = [], [], []
    for sfx in (["", "_reverse"] if bidirection else [""]):
        p = [sd[ENC + n + "_l0" + sfx] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        H = p[1].shape[1]
        h = emb.new_zeros(B, H)
        c = emb.new_zeros(B, H)
        out = [None] * Tn
        for t in (range(Tn - 1, -1, -1) if sfx else range(Tn)):
            h2, c2 = _cell(emb[:, t], h, c, *p)
            m = (t < lens).unsqueeze(1)
            h, c = torch.where(m, h2, h), torch.where(m, c2, c)
            out[t] = h2 * m.to(h2.dtype)
        banks.append(torch.stack(out, 1))
        hn.append(h)
        cn.append(c)
    return torch.cat(banks, 2), torch.stack(hn, 0), torch.stack(cn, 0)


def initial_state(hn, cn, lens, fault=None):
    """decoders/decoder.py:160-177 on the encoder's final state AS THE REFERENCE'S ENCODER RETURNS IT: rows in length-sorted order"""
    order = torch.arange(lens.shape[0]) if fault == "orig_order" else torch.sort(lens, 0, True)[1]
    return tuple(torch.cat([s[d][order] for d in range(s.shape[0])], 1) for s in (hn, cn))


def attend(sd, attn_type, h, mem, lens, fault=None):
    """GlobalAttention on queries h [B,TL,H] -> (attn_h [B,TL,H], align_vectors [B,TL,QL])"""
    B, TL, H = h.shape
    QL = mem.shape[1]
    if attn_type == "mlp":
        wq = h @ sd[ATT + "linear_query.weight"].t() + sd[ATT + "linear_query.bias"]
        uh = mem @ sd[ATT + "linear_context.weight"].t()
        align = (torch.tanh(wq.unsqueeze(2) + uh.unsqueeze(1)) @ sd[ATT + "v.weight"].t()).squeeze(-1)
    else:
        q = h @ sd[ATT + "linear_in.weight"].t() if attn_type == "general" else h
        align = torch.bmm(q, mem.transpose(1, 2))
    if fault != "no_mask":
        mask = torch.arange(QL).unsqueeze(0) < lens.unsqueeze(1)
        align = align.masked_fill(~mask.unsqueeze(1), float("-inf"))
    a = torch.softmax(align, -1)
    cat = torch.cat([torch.bmm(a, mem), h], 2)
    o = cat @ sd[ATT + "linear_out.weight"].t()
    if attn_type == "mlp":
        o = o + sd[ATT + "linear_out.bias"]
    if (attn_type != "mlp") != (fault == "tanh_swap"):
        o = torch.tanh(o)
    return o, a


def _cast(sd, dtype):
    return {k: v.detach().to(dtype) for k, v in sd.items()}


@torch.no_grad()
def decode(sd, cfg, src, lens, max_len, tgt2src=None, dtype=torch.float64, fault=None, force=None):
    """greedy decode -> dict(predictions [B,max_len], attentions [B,max_len,QL], gaps [B,max_len]: top-1 minus top-2 logit of every step).
    force [B,max_len] (optional): the tokens fed back are these predictions instead of the chain's own (a float32 chain is then comparable
    position by position with the float64 one)."""
    sd = _cast(sd, dtype)
    table = sd[EMB]
    mem, hn, cn = encode(sd, table[src], lens, cfg["bidirection"])
    h0, c0 = initial_state(hn, cn, lens, fault)
    h, c = h0, c0
    p = [sd[DEC + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    tok = torch.full((src.shape[0],), BOS, dtype=torch.long)
    preds, attns, gaps = [], [], []
    for step in range(max_len):
        if fault == "no_carry":
            h, c = h0, c0
        h, c = _cell(table[tok], h, c, *p)
        o, a = attend(sd, cfg["attn_type"], h.unsqueeze(1), mem, lens, fault)
        logits = o.squeeze(1) @ sd["generator.weight"].t() + sd["generator.bias"]
        top = logits.topk(2, 1).values
        pred = logits.max(1)[1]
        preds.append(pred)
        attns.append(a.squeeze(1))
        gaps.append(top[:, 0] - top[:, 1])
        fed = pred if force is None else force[:, step]
        tok = tgt2src[fed] if tgt2src is not None else fed
        tok = torch.where((tok >= 0) & (tok < table.shape[0]), tok, torch.ones_like(tok))
    return dict(predictions=torch.stack(preds, 1), attentions=torch.stack(attns, 1), gaps=torch.stack(gaps, 1))


def loss(sd, cfg, src, lens, tgt, tseq):
    """seq2seq.py:48-103 on the tensors of sd as they are (they may require grad) -> scalar loss"""
    table = sd[EMB]
    mem, hn, cn = encode(sd, table[src], lens, cfg["bidirection"])
    h, c = initial_state(hn, cn, lens)
    p = [sd[DEC + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    emb = table[tgt]
    hs = []
    for t in range(tgt.shape[1]):
        h, c = _cell(emb[:, t], h, c, *p)
        hs.append(h)
    o, _ = attend(sd, cfg["attn_type"], torch.stack(hs, 1), mem, lens)
    logits = (o @ sd["generator.weight"].t() + sd["generator.bias"])[:, :-1]
    target = tseq[:, 1:]
    ll = torch.log_softmax(logits, -1).gather(2, target.unsqueeze(2)).squeeze(2)
    return (-ll * (target != PAD).to(ll.dtype)).sum(1).mean()


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


# ------------------------------------------------------------------ the fixture cases (tests/golden/generate_seq2seq.py)
CASES = ("general", "dot", "mlp", "uni", "wide")


def case_cfg(tag):
    return json.loads(str(load_golden("seq2seq")["cfg_" + tag]))


def case_args(tag, **kw):
    from context_attentive_ir_amd.config import default_args
    g = load_golden("seq2seq")
    c = case_cfg(tag)
    return default_args("SEQ2SEQ", **dict(dict(src_vocab_size=int(g["vocab"]), tgt_vocab_size=int(g["tgt_vocab"]), nlayers=1, nhid=c["nhid"],
                                               attn_type=c["attn_type"], bidirection=c["bidirection"], max_query_len=int(g["max_len"])), **kw))


def case(tag):
    """(network on the CPU with the fixture's weights, its config, the golden arrays of the case under their plain names)"""
    from context_attentive_ir_amd.detinit import det_state_dict
    from context_attentive_ir_amd.recommender import Seq2seq
    g = load_golden("seq2seq")
    c = case_cfg(tag)
    net = Seq2seq(case_args(tag))
    net.load_state_dict(det_state_dict({k: v.shape for k, v in net.state_dict().items()}, c["seed"]))
    net.eval()
    arrs = {k[:-len(tag) - 1]: v for k, v in g.items() if k.endswith("_" + tag)}
    arrs.update(tgt2src=g["tgt2src"], max_len=int(g["max_len"]))
    return net, c, arrs


def pad_attn(a, QL):
    """the reference's attentions are max(source_len) wide; the mirror's have the padded width QL with exact zeros behind"""
    a = T(np.asarray(a))
    return torch.nn.functional.pad(a, (0, QL - a.shape[-1]))


def accept_decode(got, ref, chain, n_split, margin=None):
    """the whole criterion of a decode: the predicted tokens are the float64 restatement's, exactly (the fixtures keep every step's logit gap
    >= 1e-3), and the attentions meet the bound -> (ok, figures)"""
    same = bool(torch.equal(torch.as_tensor(np.asarray(got["predictions"].cpu())), ref["predictions"]))
    ok, fig = accept(got["attentions"], ref["attentions"], chain["attentions"], n_split, margin)
    fig["predictions_equal"] = same
    return ok and same, fig
