"""The acceptance criterion of the GRU decoders (csrc/gru_step.hip, recommender/seq2seq_gru.py): a restatement of the reference's Seq2seq and
ACG with rnn_type = 'GRU' (decoders/decoder.py:175-177, decoders/rnn_decoder.py:46-47; everything behind the decoder step is
tests/seq2seq_ref.py's and tests/acg_ref.py's, imported) in the reference's op order -- GRU encoder over the valid part of every source, the
decoder's initial state from the single h_n in LENGTH-SORTED order, torch.nn.GRU's step (gate order r, z, n; b_hn inside the reset product)
-- in float64 as the reference and in float32 on the CPU as the yardstick of what fp32 arithmetic costs.  The bound is seq2seq_ref.accept's:

    e <= MARGIN * max(e_chain, 2^-23) + n_split * FMT["fp16x2"]

`fault` plants one of five mistakes in the decoder:
    "bhn_outside"  b_hn added outside the reset product (the textbook GRU): n = tanh(.. + r * (W_hn h) + b_hn)
    "gate_order"   the gate rows read as z, r, n
    "blend_swap"   h' = z n + (1 - z) h
    "no_carry"     the decoder state is not carried between steps
    "orig_order"   the decoder starts from the encoder's final state in ORIGINAL row order
"""
import json

import torch

import acg_ref as AR
import gemm_ref
import seq2seq_ref as S
from conftest import T, load_golden

FAULTS = ("bhn_outside", "gate_order", "blend_swap", "no_carry", "orig_order")
S2S_CASES = ("general", "dot", "mlp", "uni", "wide")
ACG_CASES = ("general", "mlp", "own")
MARGIN = 2.0
BOS, PAD = 2, 0
accept, accept_decode, figures, pad_attn = S.accept, S.accept_decode, S.figures, S.pad_attn


def cell(x, h, wih, whh, bih, bhh, fault=None):
    """torch.nn.GRU's step"""
    gi, gh = x @ wih.t() + bih, h @ whh.t()
    i_r, i_z, i_n = gi.chunk(3, 1)
    h_r, h_z, h_n = gh.chunk(3, 1)
    b_r, b_z, b_n = bhh.chunk(3, 0)
    if fault == "gate_order":
        i_r, i_z, h_r, h_z, b_r, b_z = i_z, i_r, h_z, h_r, b_z, b_r
    r = torch.sigmoid(i_r + h_r + b_r)
    z = torch.sigmoid(i_z + h_z + b_z)
    n = torch.tanh(i_n + r * h_n + b_n) if fault == "bhn_outside" else torch.tanh(i_n + r * (h_n + b_n))
    return z * n + (1 - z) * h if fault == "blend_swap" else (1 - z) * n + z * h


def encode(sd, emb, lens, bidirection):
    """RNNEncoder('GRU', 1 layer, use_last) -> (memory bank [B,T,nhid], zero past the length; h_n [ND,B,nhid/ND] in ORIGINAL row order)"""
    B, Tn, _ = emb.shape
    banks, hn = [], []
    for sfx in (["", "_reverse"] if bidirection else [""]):
        p = [sd[S.ENC + n + "_l0" + sfx] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        h = emb.new_zeros(B, p[1].shape[1])
        out = [None] * Tn
        for t in (range(Tn - 1, -1, -1) if sfx else range(Tn)):
            h2 = cell(emb[:, t], h, *p)
            m = (t < lens).unsqueeze(1)
            h = torch.where(m, h2, h)
            out[t] = h2 * m.to(h2.dtype)
        banks.append(torch.stack(out, 1))
        hn.append(h)
    return torch.cat(banks, 2), torch.stack(hn, 0)


def initial_state(hn, lens, fault=None):
    order = torch.arange(lens.shape[0]) if fault == "orig_order" else torch.sort(lens, 0, True)[1]
    return torch.cat([hn[d][order] for d in range(hn.shape[0])], 1)


def _dec_params(sd):
    return [sd[S.DEC + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]


@torch.no_grad()
def decode(sd, cfg, src, lens, max_len, tgt2src=None, dtype=torch.float64, fault=None, force=None):
    """seq2seq_ref.decode with the GRU cell -> dict(predictions, attentions, gaps)"""
    sd = S._cast(sd, dtype)
    table = sd[S.EMB]
    mem, hn = encode(sd, table[src], lens, cfg["bidirection"])
    h0 = initial_state(hn, lens, fault)
    h, p = h0, _dec_params(sd)
    tok = torch.full((src.shape[0],), BOS, dtype=torch.long)
    preds, attns, gaps = [], [], []
    for step in range(max_len):
        if fault == "no_carry":
            h = h0
        h = cell(table[tok], h, *p, fault=fault)
        o, a = S.attend(sd, cfg["attn_type"], h.unsqueeze(1), mem, lens)
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


def _teacher_forced(sd, cfg, src, lens, tgt, fault=None):
    table = sd[S.EMB]
    mem, hn = encode(sd, table[src], lens, cfg["bidirection"])
    h0 = initial_state(hn, lens, fault)
    h, p, emb, hs = h0, _dec_params(sd), table[tgt], []
    for t in range(tgt.shape[1]):
        if fault == "no_carry":
            h = h0
        h = cell(emb[:, t], h, *p, fault=fault)
        hs.append(h)
    return torch.stack(hs, 1), mem


def loss(sd, cfg, src, lens, tgt, tseq, fault=None):
    """seq2seq.py:48-103 with the GRU cell on the tensors of sd as they are (they may require grad) -> scalar loss"""
    hs, mem = _teacher_forced(sd, cfg, src, lens, tgt, fault)
    o, _ = S.attend(sd, cfg["attn_type"], hs, mem, lens)
    logits = (o @ sd["generator.weight"].t() + sd["generator.bias"])[:, :-1]
    target = tseq[:, 1:]
    ll = torch.log_softmax(logits, -1).gather(2, target.unsqueeze(2)).squeeze(2)
    return (-ll * (target != PAD).to(ll.dtype)).sum(1).mean()


@torch.no_grad()
def acg_decode(sd, cfg, src, lens, max_len, idx, e2t, e2s, tgt2src=None, dtype=torch.float64, fault=None):
    """acg_ref.decode with the GRU cell -> dict(predictions (extended ids), attentions, gaps (relative), gen_top, next)"""
    sd = S._cast(sd, dtype)
    table = sd[S.EMB]
    VT, CV = sd["generator.weight"].shape[0], e2t.shape[1]
    mem, hn = encode(sd, table[src], lens, cfg["bidirection"])
    h0 = initial_state(hn, lens, fault)
    h, p = h0, _dec_params(sd)
    tok = torch.full((src.shape[0],), BOS, dtype=torch.long)
    out = dict(predictions=[], attentions=[], gaps=[], gen_top=[], next=[])
    for _ in range(max_len):
        if fault == "no_carry":
            h = h0
        h = cell(table[tok], h, *p, fault=fault)
        o, a = S.attend(sd, cfg["attn_type"], h.unsqueeze(1), mem, lens)
        a_c = AR.copy_attention(sd, cfg, o, mem, lens, a)
        P, l = AR.extended(sd, o.squeeze(1), a_c.squeeze(1), idx, lens, CV)
        P = AR.collapse_(P, e2t, VT)
        top = P.topk(2, 1).values
        pred = P.max(1)[1]
        low = pred.clamp(max=VT - 1)
        word_src = tgt2src[low] if tgt2src is not None else low
        ext = e2s[torch.arange(src.shape[0]), (pred - VT).clamp(min=0)]
        tok = torch.where(pred < VT, word_src, ext)
        tok = torch.where((tok >= 0) & (tok < table.shape[0]), tok, torch.ones_like(tok))
        for k, v in (("predictions", pred), ("attentions", a.squeeze(1)), ("gaps", (top[:, 0] - top[:, 1]) / top[:, 0]), ("gen_top", l.max(1)[1]),
                     ("next", tok)):
            out[k].append(v)
    return {k: torch.stack(v, 1) for k, v in out.items()}


def acg_loss(sd, cfg, src, lens, tgt, tseq, idx, alignment, force_copy=False, fault=None):
    """acg_ref.loss with the GRU cell -> scalar loss"""
    hs, mem = _teacher_forced(sd, cfg, src, lens, tgt, fault)
    o, a = S.attend(sd, cfg["attn_type"], hs, mem, lens)
    a_c = AR.copy_attention(sd, cfg, o, mem, lens, a)[:, :-1]
    _, s, z = AR.gen_parts(sd, o[:, :-1])
    z = z.squeeze(-1)
    target, al = tseq[:, 1:], alignment[:, 1:]
    hit = (idx.unsqueeze(1) == al.unsqueeze(2)) & (torch.arange(idx.shape[1]).view(1, 1, -1) < lens.view(-1, 1, 1))
    mass = (a_c * hit.to(a_c.dtype)).sum(2)
    st = s.gather(2, target.unsqueeze(2)).squeeze(2)
    anu, au = (al != AR.UNK).to(s.dtype), (al == AR.UNK).to(s.dtype)
    w = au if force_copy else (target != AR.UNK).to(s.dtype) + au * (target == AR.UNK).to(s.dtype)
    out = anu * z * mass + AR.EPS_LOSS + w * (1 - z) * st
    return (-out.log() * (target != PAD).to(s.dtype)).sum(1).mean()


# ------------------------------------------------------------------ one step at the C ABI (tests/test_gpu_gru_step_envelope.py)
def step(ids, table, wih, bih, whh, bhh, h, dtype=torch.float64, fault=None):
    """nir_gru_step's contract: ids outside [0, V) read row 1"""
    ids = torch.where((ids >= 0) & (ids < table.shape[0]), ids, torch.ones_like(ids))
    c = lambda t: t.to(dtype)
    return cell(c(table)[ids], c(h), c(wih), c(whh), c(bih), c(bhh), fault=fault)


def split_pairs(h):
    """h [B,H] float32 -> the fp16 term pairs [B][H/8][2][8] the step writes (csrc/split2.hpp, both terms rounded to nearest), as float16"""
    h = h.float()
    h1 = h.half()
    h2 = ((h - h1.float()) * 2048.0).half()
    B, H = h.shape
    return torch.stack((h1.view(B, H // 8, 8), h2.view(B, H // 8, 8)), 2).contiguous()


def step_inputs(H, B, E, V=50, seed=5):
    """the input family of the one-step envelope: weights scaled for their reduction, a b_hn of order 1, a repeated id and ids outside [0, V)"""
    g = torch.Generator().manual_seed(seed * 1000 + H * 7 + B)
    table = gemm_ref.family("randn", g, V, E, "a")
    wih, whh = gemm_ref.family("randn", g, 3 * H, E, "w"), gemm_ref.family("randn", g, 3 * H, H, "w")
    bih, bhh = 0.1 * torch.randn(3 * H, generator=g), 0.1 * torch.randn(3 * H, generator=g)
    bhh[2 * H:] = 1.0 + 0.5 * torch.rand(H, generator=g)
    h = torch.tanh(torch.randn(B, H, generator=g))
    ids = torch.randint(0, V, (B,), generator=g)
    ids[B // 2] = ids[0]
    ids[-1] = V + 3
    if B > 2:
        ids[1] = -1
    return ids, table, wih, bih, whh, bhh, h


# ------------------------------------------------------------------ the fixture cases (tests/golden/generate_seq2seq_gru.py)
def golden(kind):
    """the arrays of one model kind ('s2s' / 'acg') of seq2seq_gru.npz under the key names of seq2seq.npz / acg.npz"""
    return {k[4:]: v for k, v in load_golden("seq2seq_gru").items() if k.startswith(kind + "_")}


def case_cfg(kind, tag):
    c = json.loads(str(golden(kind)["cfg_" + tag]))
    c.setdefault("bidirection", True)
    return c


def case_args(kind, tag, **kw):
    from context_attentive_ir_amd.config import default_args
    g, c = golden(kind), case_cfg(kind, tag)
    base = dict(src_vocab_size=int(g["vocab"]), tgt_vocab_size=int(g["tgt_vocab"]), nlayers=1, nhid=c["nhid"], attn_type=c["attn_type"],
                bidirection=c["bidirection"], max_query_len=int(g["max_len"]), rnn_type="GRU")
    if kind == "acg":
        base.update(reuse_copy_attn=c["reuse_copy_attn"])
    return default_args("ACG" if kind == "acg" else "SEQ2SEQ", **dict(base, **kw))


def case(kind, tag, **kw):
    """(network on the CPU with the fixture's weights, its config, the golden arrays of the case under their plain names)"""
    from context_attentive_ir_amd.detinit import det_state_dict
    from context_attentive_ir_amd.recommender import ACGGRU, Seq2seqGRU
    g, c = golden(kind), case_cfg(kind, tag)
    net = (ACGGRU if kind == "acg" else Seq2seqGRU)(case_args(kind, tag, **kw))
    net.load_state_dict(det_state_dict({k: v.shape for k, v in net.state_dict().items()}, c["seed"]))
    net.eval()
    arrs = {k[:-len(tag) - 1]: v for k, v in g.items() if k.endswith("_" + tag)}
    if kind == "s2s":
        arrs.update(tgt2src=g["tgt2src"], max_len=int(g["max_len"]))
    return net, c, arrs


def acg_batch(prefix=""):
    """acg_ref.batch_inputs on the GRU fixture's arrays"""
    g = golden("acg")
    sq = (lambda a: T(a).squeeze(1)) if prefix else T
    src, lens = sq(g[prefix + "source_words"]), sq(g[prefix + "source_lens"])
    tw, ts, tlen = sq(g[prefix + "target_words"]), sq(g[prefix + "target_seq"]), sq(g[prefix + "target_lens"])
    idx, al = T(g[prefix + "src_map"]), T(g[prefix + "alignment"])
    src_dict, tgt_dict = AR.dictionaries(int(g["vocab"]), int(g["tgt_vocab"]))
    return dict(src=src, lens=lens, tw=tw, ts=ts, tlen=tlen, idx=idx, al=al, maps=[idx[b, :int(lens[b])] for b in range(src.shape[0])],
                als=[al[b, :int(tlen[b])] for b in range(src.shape[0])], vocabs=AR.row_vocabs(src, lens), src_dict=src_dict, tgt_dict=tgt_dict)
