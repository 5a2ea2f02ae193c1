"""The acceptance criterion of teacher-forced candidate scoring (csrc/score.hip, include/neuroir_score.h; Seq2seq / Seq2seqGRU / HredQS
.score_candidates): a restatement in float64 (the reference) and float32 (the yardstick of what fp32 arithmetic costs).  The reference project
has no scorer beyond its training loss; the semantics are this project's:

    generator   logits = x W^T + b;  lse = logsumexp(logits);  logp[r] = logits[r, target[r]] - lse[r]
                0 where target[r] == pad or target[r] outside [0, VT)
    sequences   position j of a sequence counts iff target[j] != pad, target[j] >= 0 and no EARLIER position held EOS (the beam's "frozen at
                EOS" rule); scores = the sum of the counted log-probabilities, lengths = their number, uncounted positions read 0
    models      candidate_seq [.., N, TL] (BOS first): step t of the teacher-forced decoder, fed candidate_rep[t], is scored against
                candidate_seq[t + 1]; candidate_rep defaults to what the decodes feed: token 0 as it is, tgt2src[token] behind it; candidate
                (b, n) is row b N + n and decodes from the state and the memory bank of source b; the encoder, the initial state (the reference's length-sorted pairing; HredQS: its step-major pairing) and the cells are those of
                seq2seq_ref / gru_dec_ref / hredqs_ref.  For N = 1 and the gold target, -mean(scores) is the reference forward's loss.

Bound (the project's form).  s = max |logit_ref64| of the case -- the scale the generator's arithmetic works at; a log-probability is a
difference of two numbers of that size.  With e = max |got - ref64| / s and e_chain the same figure for the float32 chain,

    e <= MARGIN * max(e_chain, 2^-23) + n_split * FMT["fp16x2"]

n_split, the split-product results that enter a figure.  Generator level (nir_score_gen_target driven directly): a token log-probability on the
fused form is (target logit) - lse; the target logit is one split product, and lse moves by at most the largest error among the row's logits
(d lse / d logit_v = softmax_v, a convex weighting), one more: n_split = 2 per token.  A sequence sum adds at most T counted tokens: 2 T.  The
plain form computes the logits with the fp32 GEMM: 0.  Model level: the decoder outputs themselves come from the encoder and the teacher-forced
pass, whose products run on the library's fp32-class GEMMs and recurrences; following hredqs_ref.n_split every product on the path of the last
step's output is taken as a split one -- n_path(kind, QL, T[, S]) below -- so a token has n_path (+ 2 fused) and a sequence T times that.
MARGIN starts at 2 and moves only by the house rule (the largest measured ratio doubled, rounded up to a power of two, never above
gemm_ref.MARGIN_CAP); DESIGN.md section 26 quotes the measured ratios.

`fault` plants one of seven mistakes (tests/test_score_host.py shows on the CPU that the criterion rejects each):
    "raw_logit"   no - lse
    "no_bias"     the generator's bias is left out
    "pad_counts"  PAD targets are scored and counted
    "after_eos"   tokens behind the first EOS are counted
    "shift"       step t is scored against token t instead of t + 1
    "wrong_row"   candidate row i = b N + n reads source i % B (the beam's row layout) instead of i // N
    "orig_order"  the initial state is not in the reference's pairing (Seq2seq: original instead of length-sorted order; HredQS: natural pairing)
"""
import numpy as np
import torch

import gemm_ref
import gru_dec_ref as GR
import hredqs_ref as HQ
import seq2seq_ref as S

EOS, BOS, PAD, UNK = 3, 2, 0, 1
MARGIN = 4.0
EPS = gemm_ref.EPS
FMT = gemm_ref.FMT["fp16x2"]
FAULTS = ("raw_logit", "no_bias", "pad_counts", "after_eos", "shift", "wrong_row", "orig_order")
GEN_FAULTS = ("raw_logit", "no_bias", "pad_counts", "after_eos")                    # those a generator-level case can show


# ------------------------------------------------------------------ generator and sequences
def gen_target(x, w, b, target, pad=PAD, dtype=torch.float64, fault=None):
    """x [R, K], w [VT, K], b [VT] or None, target [R] -> (logp [R], lse [R], logits [R, VT], bad [R]: target outside the vocabulary)"""
    logits = x.to(dtype) @ w.to(dtype).t()
    if b is not None and fault != "no_bias":
        logits = logits + b.to(dtype)
    VT = logits.shape[1]
    lse = torch.logsumexp(logits, 1)
    bad = (target < 0) | (target >= VT)
    tl = logits.gather(1, target.clamp(0, VT - 1).unsqueeze(1)).squeeze(1)
    lp = tl if fault == "raw_logit" else tl - lse
    counts = ~bad if fault == "pad_counts" else ~bad & (target != pad)
    return torch.where(counts, lp, torch.zeros_like(lp)), lse, logits, bad


def sequences(lp, target, pad=PAD, eos=EOS, fault=None):
    """lp, target [nseq, T] -> (lp with the uncounted positions zeroed, scores [nseq], lengths [nseq])"""
    is_eos = (target == eos) if eos >= 0 else torch.zeros_like(target, dtype=torch.bool)
    before = (torch.cumsum(is_eos.long(), 1) - is_eos.long()) > 0                   # an EARLIER position held eos
    counts = target >= 0
    if fault != "pad_counts":
        counts = counts & (target != pad)
    if fault != "after_eos":
        counts = counts & ~before
    lp = torch.where(counts, lp, torch.zeros_like(lp))
    sc = torch.zeros(lp.shape[0], dtype=lp.dtype)
    for j in range(lp.shape[1]):                                                    # in position order, like the kernel
        sc = sc + lp[:, j]
    return lp, sc, counts.sum(1)


def sequences_brute(lp, target, pad, eos):
    """the same by loops over plain Python numbers"""
    out_lp, sc, ln = [], [], []
    for row_lp, row_t in zip(lp.tolist(), target.tolist()):
        ended, s, n, o = False, 0.0, 0, []
        for v, t in zip(row_lp, row_t):
            if not ended and t != pad and t >= 0:
                s, n = s + v, n + 1
                o.append(v)
            else:
                o.append(0.0)
            if eos >= 0 and t == eos:
                ended = True
        out_lp.append(o)
        sc.append(s)
        ln.append(n)
    return torch.tensor(out_lp, dtype=lp.dtype), torch.tensor(sc, dtype=lp.dtype), torch.tensor(ln)


def score_rows(x, w, b, cand, pad=PAD, eos=EOS, dtype=torch.float64, fault=None):
    """x [nseq, T, K]: the decoder outputs of the teacher-forced steps; cand [nseq, T + 1] -> dict(token_logprobs [nseq, T], scores, lengths,
    s = max |logit|)"""
    nseq, T, K = x.shape
    target = cand[:, :-1] if fault == "shift" else cand[:, 1:]
    lp, _, logits, _ = gen_target(x.reshape(nseq * T, K), w, b, target.reshape(-1), pad, dtype, fault)
    lp, sc, ln = sequences(lp.view(nseq, T), target, pad, eos, fault)
    return dict(token_logprobs=lp, scores=sc, lengths=ln, s=float(logits.abs().max()))


# ------------------------------------------------------------------ the models
def default_rep(cand, tgt2src, V):
    """what decode() / decode_beam() feed: the first token as it is (they start from BOS itself), tgt2src[token] behind it, <unk> outside the
    source vocabulary"""
    rep = cand if tgt2src is None else torch.cat((cand[..., :1], tgt2src[cand[..., 1:].clamp(0, tgt2src.shape[0] - 1)]), -1)
    return torch.where((rep >= 0) & (rep < V), rep, torch.full_like(rep, UNK))


def _rows(n_src, N, fault):
    i = torch.arange(n_src * N)
    return i % n_src if fault == "wrong_row" else i // N


@torch.no_grad()
def score(kind, sd, cfg, src, lens, cand, rep=None, tgt2src=None, dtype=torch.float64, fault=None):
    """kind 's2s' / 'gru': src [B, QL], lens [B], cand [B, N, TL]; 'hredqs': src [B, S, QL], lens [B, S], cand [B, S, N, TL]
    -> score_rows' dict with the outputs in cand's leading shape"""
    sd = S._cast(sd, dtype)
    table = sd[S.EMB]
    lead, TL = tuple(cand.shape[:-1]), cand.shape[-1]
    N, T = cand.shape[-2], TL - 1
    rep = default_rep(cand, tgt2src, table.shape[0]) if rep is None else rep
    flat = cand.reshape(-1, TL)
    emb = table[rep.reshape(-1, TL)[:, :-1]]                                         # [rows, T, E]
    if kind == "hredqs":
        h0, c0 = HQ.paired(*HQ.session_steps(sd, src, lens), fault="natural_pairing" if fault == "orig_order" else None)
        idx = _rows(h0.shape[0], N, fault)
        h, c, p, hs = h0[idx], c0[idx], HQ._lstm(sd, HQ.DEC), []
        for t in range(T):
            h, c = S._cell(emb[:, t], h, c, *p)
            hs.append(h)
        o = torch.stack(hs, 1)
    else:
        f = "orig_order" if fault == "orig_order" else None
        if kind == "gru":
            mem, hn = GR.encode(sd, table[src], lens, cfg["bidirection"])
            state, p = (GR.initial_state(hn, lens, f),), GR._dec_params(sd)
        else:
            mem, hn, cn = S.encode(sd, table[src], lens, cfg["bidirection"])
            state, p = S.initial_state(hn, cn, lens, f), [sd[S.DEC + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
        idx = _rows(src.shape[0], N, fault)
        state, hs = tuple(s[idx] for s in state), []
        for t in range(T):
            state = (GR.cell(emb[:, t], state[0], *p),) if kind == "gru" else S._cell(emb[:, t], state[0], state[1], *p)
            hs.append(state[0])
        o, _ = S.attend(sd, cfg["attn_type"], torch.stack(hs, 1), mem[idx], lens[idx])
    out = score_rows(o, sd["generator.weight"], sd["generator.bias"], flat, dtype=dtype, fault=fault)
    return dict(token_logprobs=out["token_logprobs"].view(lead + (T,)), scores=out["scores"].view(lead), lengths=out["lengths"].view(lead), s=out["s"])


def n_path(kind, QL, T, S_len=0):
    """every product on the path of the last teacher-forced step's decoder output, taken as a split one: the query encoder's gate product and
    its QL recurrent products; HredQS: the session LSTM's gate product and S recurrent ones; the decoder's gate product and T recurrent
    products; the attention's projection, context and output products (Seq2seq)"""
    if kind == "hredqs":
        return HQ.n_split(QL, S_len) + 1 + T
    return (QL + 1) + (1 + T) + 3


# ------------------------------------------------------------------ the bound
def _cpu(x):
    return x.detach().cpu() if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))


def figures(got, ref, chain, s, n_split):
    got, ref, chain = _cpu(got).double(), _cpu(ref).double(), _cpu(chain).double()
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "non-finite output"
    assert s > 0
    e = float((got - ref).abs().max()) / s if got.numel() else 0.0
    e_chain = float((chain - ref).abs().max()) / s if got.numel() else 0.0
    extra = n_split * FMT
    return dict(e=e, e_chain=e_chain, s=s, extra=extra, ratio=(e - extra) / max(e_chain, EPS))


def accept(got, ref, chain, n_split, margin=None):
    """got / ref / chain: dicts with token_logprobs [.., T], scores [..], lengths [..]; ref carries s.  n_split: per token (a sequence: T times
    that).  -> (ok, dict(tokens=figures, scores=figures, lengths_equal))"""
    margin = MARGIN if margin is None else margin
    assert margin <= gemm_ref.MARGIN_CAP
    T = ref["token_logprobs"].shape[-1]
    ft = figures(got["token_logprobs"], ref["token_logprobs"], chain["token_logprobs"], ref["s"], n_split)
    fs = figures(got["scores"], ref["scores"], chain["scores"], ref["s"], n_split * T)
    for f in (ft, fs):
        f["bound"] = margin * max(f["e_chain"], EPS) + f["extra"]
    same = bool(torch.equal(_cpu(got["lengths"]).long(), _cpu(ref["lengths"]).long()))
    return same and ft["e"] <= ft["bound"] and fs["e"] <= fs["bound"], dict(tokens=ft, scores=fs, lengths_equal=same)


def accept_rows(got_lp, ref, chain, n_split, margin=None):
    """generator level: token log-probabilities [R] alone against gen_target's (lp, lse, logits, bad) of float64 and float32"""
    margin = MARGIN if margin is None else margin
    assert margin <= gemm_ref.MARGIN_CAP
    f = figures(got_lp, ref[0], chain[0], float(ref[2].abs().max()), n_split)
    f["bound"] = margin * max(f["e_chain"], EPS) + f["extra"]
    return f["e"] <= f["bound"], f


# ------------------------------------------------------------------ candidates for the fixtures
def candidates(target_seq, N=4, VT=200, seed=0):
    """target_seq [.., TL] (the fixtures' gold targets) -> [.., N, TL] candidates of unequal lengths: n = 0 the gold row; n = 1 an EOS in the
    middle with a PAD tail; n = 2 EOS at once, then PAD; n = 3 an EOS in the middle with non-PAD tokens (EOS among them) behind it, the way a
    beam's predictions row looks; further n: random tokens without EOS.  The first token of every candidate is the gold row's."""
    g = torch.Generator().manual_seed(1000 + seed)
    lead, TL = tuple(target_seq.shape[:-1]), target_seq.shape[-1]
    gold = target_seq.reshape(-1, TL)
    out = torch.randint(4, VT, (gold.shape[0], N, TL), generator=g)
    out[:, :, 0] = gold[:, :1]
    out[:, 0] = gold
    mid = min(max(2, TL // 2), TL - 1)
    if N > 1:
        out[:, 1, mid] = EOS
        out[:, 1, mid + 1:] = PAD
    if N > 2:
        out[:, 2, 1] = EOS
        out[:, 2, 2:] = PAD
    if N > 3:
        out[:, 3, mid] = EOS
        if mid + 1 < TL:
            out[:, 3, TL - 1] = EOS
    return out.view(lead + (N, TL))
