"""The acceptance criterion of teacher-forced candidate scoring under the session models (CARS / M_MATCH_TENSOR / MNSRF .score_candidates,
Multitask.score_suggestions) and of the grouped attention underneath (csrc/tf_attend.hip, include/neuroir_teacher.h): restatements in float64
(the reference) and float32 (the yardstick of what fp32 arithmetic costs).  The reference project has no scorer beyond its training loss; the
semantics are this project's (DESIGN.md sections 26 and 27):

    attention   row r of h [ngroups G, H] belongs to group g = r // G and reads bank row src = rowmap[g] (g without a map; clamped into
                [0, rows_src)) and len = clamp(source_len[src], 0, QL):  align_j = h . score_bank[src, j];  j >= len masked;  a = softmax(align);
                cat[r] = [sum_j a_j memory_bank[src, j] ; h[r]];  masked positions of a are exactly 0; len 0: NaN
    models      candidate_seq [Bd, N, TL] (BOS first), Bd = B (S-1): step t of the teacher-forced decoder, fed candidate_rep[t], is scored against
                candidate_seq[t + 1].  Candidate (i, n) starts from row i of the decoder's initial states; under CARS it attends source row
                rowmap[i] and adds the session term of row i -- exactly the pairing of decode() and decode_beam(), the reference's step-major /
                batch-major quirk carried over.  The steps are session_beam_ref.model_step's, forced along the candidate's tokens (its beam
                axis is the candidate axis); the counting rule is score_ref.sequences'.

Bound (the project's form): e <= MARGIN * max(e_chain, 2^-23) + n_split * FMT["fp16x2"], e = max |got - ref64| / s.

Attention level.  delta ctx = sum_j (delta a_j) mem_j + (the context product's own error), so with m = max |memory bank| over the positions that
count and A = max over rows and positions of sum_k |h_k| |sb_jk| (the scale a score's product works at):  |delta s_j| <= FMT A for a split score
product, sum_j |delta a_j| <= 2 max_j |delta s_j| (the softmax moves by at most the spread of the perturbation), and the context product adds
FMT m: |delta ctx| <= m (2 A + 1) FMT.  With s = m max(1, 2 A) that is at most 2 FMT: n_split = 2 on the fused form (the score product and
the context product), 0 on the plain one.  The attention row is held to the same bound at s = max(1, 2 A); cat's second half is h, bit for bit.
Model level.  s = max |logit_ref64| (score_ref's).  The states, the encoded queries and the session pools are INPUTS of score_candidates, so
the path starts at the decoder: n_path = its gate product + the T recurrent products (+ for CARS the two bank products, linear_out,
token_prob_predictor1 and the session term: 5), every one taken as a split product as hredqs_ref / score_ref do; the fused attention adds 2
and the fused generator 2.  A sequence sum: T times the token's figure (score_ref.accept).
MARGIN starts at score_ref.MARGIN and moves only by the house rule (the largest ratio measured on the MI355X doubled, rounded up to a power of
two, never above gemm_ref.MARGIN_CAP); DESIGN.md section 27 quotes the measured ratios.

`fault` plants score_ref's seven mistakes, session_beam_ref's two, and four of this layout's own (tests/test_session_score_host.py shows on the
CPU that the criterion rejects each where the case can show it):
    "state_pairing"    the initial states are taken batch-major: decode row b (S-1) + j starts from states row j B + b
    "orig_order"       (score_ref's name) the same mistake on the cell state alone
    "neighbour_bank"   attention level: the rows of a group's last 64-row block read the NEXT group's banks
    "mask_len_of_row"  attention level: the length is taken at the group's own index instead of rowmap[group]
"no_bias" needs a generator bias (the plain decoders), "wrong_source_row" / "sess_dropped" are CARS's (session_beam_ref).
"""
import functools

import torch

import gemm_ref
import score_ref as R
import session_beam_ref as SB
from conftest import T, load_golden
from helpers import build_model, cpu_state_dict
from oracle import neuroir_cpu as O

EOS, BOS, PAD, UNK = R.EOS, R.BOS, R.PAD, R.UNK
MARGIN = R.MARGIN
EPS, FMT = gemm_ref.EPS, gemm_ref.FMT["fp16x2"]
TF_ROWS = 64                                                                  # rows of a workgroup of the fused form
TF_MIN_G = 128                                                                # rows per group from which nir_tf_attend takes its fused form
ATTEND_FAULTS = ("neighbour_bank", "mask_len_of_row")
PAIRING_FAULTS = ("state_pairing", "orig_order")
CASES = SB.CASES
TRAIN_CASES = [("cars", "cars_train"), ("mnsrf", "mnsrf_train"), ("mmt", "m_match_tensor_train")]


# ------------------------------------------------------------------ the grouped attention
def _src_rows(ngroups, rows_src, rowmap):
    src = torch.arange(ngroups) if rowmap is None else rowmap.long()
    return src.clamp(0, rows_src - 1)


@torch.no_grad()
def tf_attend(h, mem, sb, lens, rowmap, G, dtype=torch.float64, fault=None):
    """h [ngroups G, H], mem / sb [rows_src, QL, H], lens [rows_src], rowmap [ngroups] or None -> dict(cat [R, 2H], attn [R, QL], length [R],
    m, A: the two scales of the bound)"""
    Rn, H = h.shape
    rows_src, QL, _ = mem.shape
    ngroups = Rn // G
    src_g = _src_rows(ngroups, rows_src, rowmap)
    g = torch.arange(Rn) // G
    bank = src_g[g]
    if fault == "neighbour_bank":
        last = (torch.arange(Rn) % G) >= ((G - 1) // TF_ROWS) * TF_ROWS
        bank = torch.where(last, src_g[(g + 1) % ngroups], bank)
    len_rows = src_g[g] if fault != "mask_len_of_row" else g.clamp(0, rows_src - 1)
    ln = lens[len_rows].clamp(0, QL)
    hd, sbd, md = h.to(dtype), sb.to(dtype)[bank], mem.to(dtype)[bank]
    align = torch.einsum("rh,rjh->rj", hd, sbd)
    mask = torch.arange(QL).unsqueeze(0) < ln.unsqueeze(1)
    a = torch.softmax(align.masked_fill(~mask, float("-inf")), 1)               # a row of length 0: NaN, like the kernel's
    ctx = torch.einsum("rj,rjh->rh", torch.where(mask, a, torch.zeros_like(a)), md)
    ctx = torch.where((ln == 0).unsqueeze(1), torch.full_like(ctx, float("nan")), ctx)
    A = torch.einsum("rh,rjh->rj", hd.abs().double(), sbd.abs().double())
    A = float(A[mask].max()) if bool(mask.any()) else 0.0
    m = float(md.double().abs()[mask].max()) if bool(mask.any()) else 0.0
    return dict(cat=torch.cat((ctx, hd), 1), attn=a, length=ln, m=m, A=A)


def accept_attend(got_cat, got_attn, h, ref, chain, n_split, margin=None):
    """got_cat [R, 2H] (and got_attn [R, QL] or None) against tf_attend's float64 `ref` and float32 `chain` -> (ok, figures).  The rows of
    length 0 are compared by their NaN pattern alone; cat's second half must be h, bit for bit."""
    margin = MARGIN if margin is None else margin
    assert margin <= gemm_ref.MARGIN_CAP
    got_cat = got_cat.detach().cpu()
    H = h.shape[1]
    dead = ref["length"] == 0
    same_h = bool(torch.equal(got_cat[:, H:], h.float()))
    nan_ok = bool(torch.isnan(got_cat[dead, :H]).all()) and bool(torch.isfinite(got_cat[~dead, :H]).all())
    scale = max(1.0, 2.0 * ref["A"])
    fig = {"same_h": same_h, "nan_pattern": nan_ok}
    ok = same_h and nan_ok
    live = ~dead
    pairs = [("ctx", got_cat[:, :H], ref["cat"][:, :H], chain["cat"][:, :H], max(ref["m"], 1e-30) * scale)]
    if got_attn is not None:
        ga = got_attn.detach().cpu()
        masked = torch.arange(ga.shape[1]).unsqueeze(0) >= ref["length"].unsqueeze(1)
        zeros = bool((ga[live][masked[live]] == 0).all()) and bool(torch.isnan(ga[dead]).all())
        fig["masked_exactly_zero"] = zeros
        ok = ok and zeros
        pairs.append(("attn", ga, ref["attn"], chain["attn"], scale))
    for name, g_, r_, c_, s in pairs:
        if bool(live.any()):
            e = float((g_[live].double() - r_[live].double()).abs().max()) / s
            e_chain = float((c_[live].double() - r_[live].double()).abs().max()) / s
        else:
            e = e_chain = 0.0
        extra = n_split * FMT
        bound = margin * max(e_chain, EPS) + extra
        fig[name] = dict(e=e, e_chain=e_chain, s=s, extra=extra, bound=bound, ratio=(e - extra) / max(e_chain, EPS))
        ok = ok and e <= bound
    return ok, fig


# ------------------------------------------------------------------ the cases
def load_case(kind, tag):
    """session_beam_ref's five fixtures (golden weights, states, encoded queries; read-only, shared) + VT"""
    cs = SB.load_case(kind, tag)
    return cs


def vocab_tgt(cs):
    return int(cs["sd"][SB.PRED2 if cs["kind"] == "cars" else "generator.weight"].shape[0])


@functools.lru_cache(maxsize=None)
def train_case(kind, fixture):
    """the first batch of a `*_train` fixture as a case of model_step: the fixture network's weights, its decoder inputs restated by the oracle
    (float32: they are INPUTS of both restatements below), and the gold target_words / target_seq [Bd, TL]"""
    g = load_golden(fixture)
    V = int(g["meta_vocab"])
    q, ql = T(g["b0_source_words"]), T(g["b0_source_lens"])
    B, S, _ = q.shape
    Bd = B * (S - 1)
    gold = dict(target_words=T(g["b0_target_words"]).reshape(Bd, -1), target_seq=T(g["b0_target_seq"]).reshape(Bd, -1))
    if kind == "cars":
        sd = cpu_state_dict(build_model("CARS", vocab=V, tgt_vocab_size=V))
        pooled, enc = O.cars_encode(sd, q, ql)
        _, states, attns = O.cars_rank_document_full(sd, pooled, T(g["b0_document_words"]), T(g["b0_document_lens"]), T(g["b0_document_labels"]))
        cat = [a for a in attns if a is not None]
        cs = dict(kind=kind, tag="full", sd=sd, dec_h=states[0][0], dec_c=states[1][0], lut=None, B=B, SD=S - 1, V=V, enc=enc.float(), lens=ql.reshape(-1),
                  attns=list(attns), session_cat=torch.cat(cat, 2).reshape(B * S, -1))
    else:
        sd = cpu_state_dict(build_model("MNSRF" if kind == "mnsrf" else "M_MATCH_TENSOR", vocab=V, tgt_vocab_size=50))
        pooled = O.mnsrf_encode(sd, q, ql)[0] if kind == "mnsrf" else O.m_match_tensor_encode(sd, q, ql).max(1)[0].view(B, S, -1)
        _, hh, cc = O.session_decoder_states(O._strip_encoder_nesting(sd), "session_query_encoder", pooled)
        cs = dict(kind=kind, tag="", sd=sd, dec_h=hh[0], dec_c=cc[0], lut=None, B=B, SD=S - 1, V=V)
    cs.update(gold)
    return cs


def gold_like(cs):
    """[BOS] + the greedy fixture's predictions [Bd, max_len + 1]: the 'gold' row score_ref.candidates varies"""
    return torch.cat((torch.full_like(cs["greedy"][:, :1], BOS), cs["greedy"]), 1)


def candidates(cs, N=4, seed=0):
    """[Bd, N, TL]: unequal lengths, an EOS at once, a PAD tail, tokens behind an EOS -- score_ref.candidates on gold_like, with the EOS in
    front of candidate 1's PAD tail replaced by a word, so that PAD positions exist that no EOS has frozen already"""
    out = R.candidates(gold_like(cs), N, vocab_tgt(cs), seed)
    if N > 1:
        TL = out.shape[-1]
        mid = min(max(2, TL // 2), TL - 1)
        out[:, 1, mid] = out[:, 1, mid - 1].clamp(min=4)
    return out


def ranking_candidates(cs, N=6):
    """the candidates on which rankings are compared: tests/test_session_score_host.py asserts on the CPU that their float64 score gaps
    are at least ten times the bound, with and without length normalisation"""
    return candidates(cs, N, seed=3)


# ------------------------------------------------------------------ the scorers
def score_logits(lg, cand, fault=None):
    """lg [nseq, T, VT] logits of the teacher-forced steps, cand [nseq, TL] -> score_ref.score_rows' dict"""
    VT = lg.shape[2]
    target = cand[:, :-1] if fault == "shift" else cand[:, 1:]
    lse = torch.logsumexp(lg, 2)
    bad = (target < 0) | (target >= VT)
    tl = lg.gather(2, target.clamp(0, VT - 1).unsqueeze(2)).squeeze(2)
    lp = tl if fault == "raw_logit" else tl - lse
    counts = ~bad if fault == "pad_counts" else ~bad & (target != PAD)
    lp, sc, ln = R.sequences(torch.where(counts, lp, torch.zeros_like(lp)), target, PAD, EOS, fault)
    return dict(token_logprobs=lp, scores=sc, lengths=ln, s=float(lg.abs().max()))


def faults_of(cs):
    """the planted faults this case can show"""
    out = [f for f in R.FAULTS if f != "no_bias" or cs["kind"] != "cars"] + ["state_pairing"]
    if cs["kind"] == "cars":
        out.append("wrong_source_row")
        if cs.get("session_cat") is not None:
            out.append("sess_dropped")
    return out


@torch.no_grad()
def score(cs, sd, cand, rep=None, dtype=torch.float64, fault=None):
    """cand [Bd, N, TL] -> dict(token_logprobs [Bd, N, TL-1], scores [Bd, N], lengths [Bd, N], s)"""
    Bd, N, TL = cand.shape
    T_ = TL - 1
    rep = R.default_rep(cand, cs.get("lut"), cs["V"]) if rep is None else rep
    sd = dict(sd)
    if fault == "no_bias":
        sd["generator.bias"] = torch.zeros_like(sd["generator.bias"])
    if fault in PAIRING_FAULTS:
        i = torch.arange(Bd)
        perm = (i % cs["SD"]) * cs["B"] + i // cs["SD"]
        cs = dict(cs, dec_c=cs["dec_c"][perm], dec_h=cs["dec_h"][perm] if fault == "state_pairing" else cs["dec_h"])
    state0, step = SB.model_step(cs, sd, dtype, fault if fault in SB.SESSION_FAULTS else None)
    r = torch.arange(Bd * N)                                                       # model_step's rows: r = n Bd + i
    f = r if fault == "wrong_row" else (r % Bd) * N + r // Bd                      # the candidate a row is fed
    toks = rep.reshape(Bd * N, TL)[f]
    state, lg = tuple(s.repeat(N, 1) for s in state0), []
    for t in range(T_):
        state, logits, _ = step(state, toks[:, t])
        lg.append(logits)
    lg = torch.stack(lg, 1)
    out = torch.empty_like(lg)
    out[f] = lg
    res = score_logits(out, cand.reshape(Bd * N, TL), fault)
    return dict(token_logprobs=res["token_logprobs"].view(Bd, N, T_), scores=res["scores"].view(Bd, N), lengths=res["lengths"].view(Bd, N), s=res["s"])


@torch.no_grad()
def suggestion_nll(cs, sd, target_words, target_seq, dtype=torch.float64):
    """the suggestion loss of the models' train-mode forward without dropout and without the entropy term, in the forward's own batched form
    (cars.py:605-657, mmtensor.py:224-254, mnsrf.py:198-228): the decoder over all TL steps, attention as batched products, log-softmax, NLL
    masked at PAD, summed over time, averaged over rows -- written independently of score() above"""
    sd = {k: v.to(dtype) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
    p = [sd["decoder.decoder.rnn." + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    emb = sd[SB.TABLE][target_words]                                               # [Bd, TL, E]
    h, c, hs = cs["dec_h"].to(dtype), cs["dec_c"].to(dtype), []
    for t in range(emb.shape[1]):
        h, c = SB._cell(emb[:, t], h, c, *p)
        hs.append(h)
    h_all = torch.stack(hs, 1)                                                     # [Bd, TL, H]
    if cs["kind"] == "cars":
        B, SD = cs["B"], cs["SD"]
        QL = cs["enc"].shape[1]
        mem = cs["enc"].to(dtype).view(B, SD + 1, QL, -1)[:, :-1].reshape(B * SD, QL, -1) @ sd["dec_attn.weight"].t()
        mlen = cs["lens"].view(B, SD + 1)[:, :-1].reshape(-1)
        align = torch.bmm(h_all @ sd["decoder.decoder.attn.linear_in.weight"].t(), mem.transpose(1, 2))
        mask = torch.arange(QL).unsqueeze(0) < mlen.unsqueeze(1)
        a = torch.softmax(align.masked_fill(~mask.unsqueeze(1), float("-inf")), 2)
        out = torch.tanh(torch.cat((torch.bmm(a, mem), h_all), 2) @ sd["decoder.decoder.attn.linear_out.weight"].t())[:, :-1]
        po = out @ sd["token_prob_predictor1.weight"].t()
        csess = cs["session_cat"].to(dtype).view(B, SD + 1, -1)[:, :-1].reshape(B * SD, -1)
        po = po + (csess @ sd["shared_session_projector.linear.weight"].t() + csess @ sd["private_session_projector2.linear.weight"].t()).unsqueeze(1)
        logits = po @ sd[SB.PRED2].t()
    else:
        logits = h_all[:, :-1] @ sd["generator.weight"].t() + sd["generator.bias"]
    tgt = target_seq[:, 1:]
    nll = -torch.log_softmax(logits, 2).gather(2, tgt.unsqueeze(2)).squeeze(2)
    return (nll * (tgt != PAD).to(dtype)).sum(1).mean()


def n_path(kind, T_):
    """the products on the path of a teacher-forced step's generator input, each taken as a split one (see the module docstring)"""
    return 1 + T_ + (5 if kind == "cars" else 0)


def n_split(kind, T_, fused_attention, fused_generator):
    return n_path(kind, T_) + (2 if fused_attention and kind == "cars" else 0) + (2 if fused_generator else 0)


def accept(got, ref, chain, nsplit, margin=None):
    """score_ref.accept on [Bd, N, ..] outputs (got may be [B, S-1, N, ..]: reshaped)"""
    shaped = {k: (got[k].detach().cpu().reshape(ref[k].shape) if torch.is_tensor(got[k]) else got[k]) for k in ("token_logprobs", "scores", "lengths")}
    return R.accept(shaped, ref, chain, nsplit, MARGIN if margin is None else margin)


def score_bound_abs(fig):
    """the bound of a sequence score in absolute terms"""
    return fig["scores"]["bound"] * fig["scores"]["s"]
