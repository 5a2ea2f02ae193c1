"""The acceptance criterion of ACG's beam search (csrc/beam.hip: acg_beam_row_kernel, acg_beam_select_kernel; ACG.decode_beam): a restatement
in float64 (the reference) and float32 (the yardstick of what fp32 arithmetic costs) on top of acg_ref (extended, collapse_, copy_attention) and
beam_ref (repeat_state, reorder_state).  The reference ships no search; the semantics are this project's (DESIGN.md section 24,
include/neuroir_acg_beam.h) and extend beam_ref's:

    rows      R = B W, row = k B + b; the copy maps, ext2tgt, ext2src and the lengths are NOT repeated: beam row r reads source row r % B
    offers    live beam k: cum[b, k] + log P[e] for every extended id e of the COLLAPSED distribution except the collapsed slots themselves (the
              reference leaves 1e-10 there; the slot's word is already offered as its target id); log 0 = -inf is an offer like any other
    select    the W best per source row, score descending, ties to the smaller flat index k (VT + CV) + e
    finished  e == EOS; a finished beam offers (k, EOS) alone, at cum[b, k]
    feedback  tgt2src[e] below VT, ext2src[b, e - VT] from VT on, <unk> (1) outside the source vocabulary

The restatement forms the FULL collapsed distribution of every row, [R, VT + CV] -- what the HIP path never writes; that is what checks its
argument that W + CV candidates per row suffice.  The search core (`search`) takes the model as a step function and is tested against brute
force on its own (it cannot be beam_ref.search: that subtracts a log-sum-exp and feeds back through one table).

Bound on the scores: beam_ref's form, e <= MARGIN max(e_chain, 2^-23) + n_split FMT["fp16x2"], with the MARGIN below.

`fault` plants one of nine mistakes: beam_ref's four model-independent ones
    "no_reorder", "eos_grows", "all_live_step0"   as there
    "raw_logit"        the vocabulary part is left unnormalised: (1 - z) exp(l - max l), no division by the softmax's sum
and five of the copy generator's beam
    "maps_of_wrong_row"     beams k > 0 read the maps (src_map_idx, ext2tgt, ext2src) of source row (b + 1) % B
    "target_offered_twice"  a collapsed slot stays a candidate, with its mass, next to its target word
    "mass_only_on_argmax"   the collapsed mass of a row is added to the row's first logit (its arg-max word) only
    "slot_feedback_unk"     a selected slot feeds back <unk>
    "pad_raw"               the PAD logit is not replaced by -1e-20
"""
import json
import os

import torch

import acg_ref as AR
import beam_ref as BR
import gemm_ref
import gru_dec_ref as GR
import seq2seq_ref as S
from conftest import GOLDEN

EOS, BOS, UNK = 3, 2, 1
# beam_ref.MARGIN (2) moved by the house rule: the largest ratio measured on the MI355X is 1.62 (lstm wide, W = 4, both plain forms; DESIGN.md
# section 24); doubled and rounded up to a power of two that is 4, which is gemm_ref.MARGIN_CAP
MARGIN = 4.0
MIN_GAP = BR.MIN_GAP
FAULTS = ("no_reorder", "raw_logit", "eos_grows", "all_live_step0", "maps_of_wrong_row", "target_offered_twice", "mass_only_on_argmax",
          "slot_feedback_unk", "pad_raw")
NEG = float("-inf")


@torch.no_grad()
def search(step_fn, state0, B, W, max_len, feedback, fault=None, force=None, bos=BOS):
    """step_fn(state, tok [R]) -> (state', logp [R, N] (log P of every extended id), live [R, N] bool (False: no candidate), aux [R, A]);
    feedback(b, k, e) -> the source id fed back when beam k of source row b selects e.  state0: tuple of [B, .] tensors.
    force = (backptr [max_len, B, W], tokens [max_len, B, W]): the choices are these (scores still the chain's).
    -> dict(predictions [B, W, max_len], scores, lengths, aux [B, W, max_len, A], backptr / tokens / gaps [max_len, B, W] (gaps: adjacent, among the
    top W + 1 candidates), finished [B, W], finished_at: per step the flags the step began with, picked: every selection as (step, b, parent
    beam k, e))"""
    state = BR.repeat_state(state0, W)
    dt = state[0].dtype
    cum = torch.full((B, W), NEG, dtype=dt)
    cum[:, 0] = 0
    if fault == "all_live_step0":
        cum[:] = 0
    fin = torch.zeros(B, W, dtype=torch.bool)
    tok = torch.full((B * W,), bos, dtype=torch.long)
    bps, toks, auxs, gaps, picked, fins = [], [], [], [], [], []
    for t in range(max_len):
        fins.append(fin.clone())
        state, logp, live, aux = step_fn(state, tok)
        N = logp.shape[1]
        bp = torch.zeros(B, W, dtype=torch.long)
        v = torch.zeros(B, W, dtype=torch.long)
        new = torch.zeros(B, W, dtype=dt)
        g = torch.full((B, W), float("inf"), dtype=dt)
        for b in range(B):
            cand = []                                                      # (score, flat index)
            for k in range(W):
                if bool(fin[b, k]) and fault != "eos_grows":
                    cand.append((float(cum[b, k]), k * N + EOS))
                    continue
                row = cum[b, k] + logp[k * B + b]
                cand.extend((float(row[e]), k * N + e) for e in range(N) if bool(live[k * B + b, e]))
            cand.sort(key=lambda x: (-x[0], x[1]))
            if force is None:
                top = cand[:W]
            else:
                want = {int(force[0][t][b, j]) * N + int(force[1][t][b, j]): j for j in range(W)}
                top = sorted((c for c in cand if c[1] in want), key=lambda c: want[c[1]])
                assert len(top) == W, "forced choices are candidates of the chain"
            for j, (sc, flat) in enumerate(top):
                bp[b, j], v[b, j] = flat // N, flat % N
            if force is None:
                for j in range(min(W, len(cand) - 1)):
                    d = cand[j][0] - cand[j + 1][0]
                    g[b, j] = d if d == d else float("inf")               # (-inf) - (-inf): no order to lose
            # the scores in the chain's own dtype, not through a Python float
            for j in range(W):
                k, e = int(bp[b, j]), int(v[b, j])
                new[b, j] = cum[b, k] if (bool(fin[b, k]) and fault != "eos_grows") else cum[b, k] + logp[k * B + b, e]
        picked.append([(t, b, int(bp[b, j]), int(v[b, j])) for b in range(B) for j in range(W)])
        cum = new
        fin = (v == EOS) & (fault != "eos_grows")
        if fault != "no_reorder":
            state = BR.reorder_state(state, bp)
        tok = torch.tensor([feedback(b, int(bp[b, k]), int(v[b, k])) for k in range(W) for b in range(B)], dtype=torch.long)      # row k B + b
        bps.append(bp)
        toks.append(v)
        auxs.append(aux)
        gaps.append(g)
    A = auxs[0].shape[1]
    pred = torch.zeros(B, W, max_len, dtype=torch.long)
    aux_out = torch.zeros(B, W, max_len, A, dtype=auxs[0].dtype)
    k = torch.arange(W).unsqueeze(0).expand(B, W)
    ar = torch.arange(B).unsqueeze(1)
    for t in range(max_len - 1, -1, -1):
        pred[:, :, t] = toks[t].gather(1, k)
        src = bps[t].gather(1, k)
        aux_out[:, :, t] = auxs[t].view(W, B, A)[src, ar]
        k = src
    is_eos = pred == EOS
    first = torch.where(is_eos.any(2), is_eos.long().argmax(2) + 1, torch.full((B, W), max_len))
    return dict(predictions=pred, scores=cum, lengths=first, aux=aux_out, backptr=torch.stack(bps), tokens=torch.stack(toks), gaps=torch.stack(gaps),
                finished=fin, finished_at=fins, picked=[p for step in picked for p in step])


def collapsed_rows(sd, o, a_c, idx, lens, e2t, VT, fault=None):
    """the full collapsed distribution of R decode rows (maps already per row) -> (log P [R, VT + CV], live [R, VT + CV], mass [R, CV]: the copy
    part before the collapse)"""
    CV = e2t.shape[1]
    P, l = AR.extended(sd, o, a_c, idx, lens, CV, "no_pad" if fault == "pad_raw" else None)
    if fault == "raw_logit":
        z = 1 - P[:, :VT].sum(1, keepdim=True)                                    # (1 - z) softmax sums to 1 - z
        P[:, :VT] = (1 - z) * torch.exp(l - l.max(1, keepdim=True).values)
    mass = P[:, VT:].clone()
    live = torch.ones_like(P, dtype=torch.bool)
    collapsed = torch.zeros(P.shape[0], CV, dtype=torch.bool)
    collapsed[:, 2:] = e2t[:, 2:] >= 0
    if fault == "target_offered_twice":
        P = AR.collapse_(P, e2t, VT, "no_blank")
    elif fault == "mass_only_on_argmax":
        first = l.max(1)[1]
        for r in range(P.shape[0]):
            P[r, first[r]] += mass[r][collapsed[r]].sum()
        live[:, VT:] = ~collapsed
    else:
        P = AR.collapse_(P, e2t, VT)
        live[:, VT:] = ~collapsed
    return torch.log(P), live, mass


def model_step(sd, cfg, cell, src, lens, idx, e2t, e2s, dtype, fault=None):
    """(state0, step_fn, feedback) of a fixture network: cell 'LSTM' / 'GRU'; aux = the decoder's own attention row [QL].  step_fn records, per
    row, the copy mass before the collapse in step_fn.mass (the fixture conditions read it)"""
    sd = S._cast(sd, dtype)
    table = sd[S.EMB]
    B, VT = src.shape[0], sd["generator.weight"].shape[0]
    if cell == "GRU":
        mem, hn = GR.encode(sd, table[src], lens, cfg["bidirection"])
        state0 = (GR.initial_state(hn, lens),)
        p = GR._dec_params(sd)
    else:
        mem, hn, cn = S.encode(sd, table[src], lens, cfg["bidirection"])
        state0 = S.initial_state(hn, cn, lens)
        p = [sd[S.DEC + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]

    def maps_of(W):
        """(idx, e2t, e2s) per decode row k B + b"""
        rows = torch.arange(B).repeat(W)
        if fault == "maps_of_wrong_row":
            rows = torch.cat([rows[:B], (rows[B:] + 1) % B])
        return idx[rows], e2t[rows], e2s[rows]

    def step(state, tok):
        W = tok.shape[0] // B
        if cell == "GRU":
            state = (GR.cell(table[tok], state[0], *p),)
        else:
            state = S._cell(table[tok], state[0], state[1], *p)
        memr, lensr = mem.repeat(W, 1, 1), lens.repeat(W)
        o, a = S.attend(sd, cfg["attn_type"], state[0].unsqueeze(1), memr, lensr)
        a_c = AR.copy_attention(sd, cfg, o, memr, lensr, a)
        ridx, re2t, _ = maps_of(W)
        logp, live, mass = collapsed_rows(sd, o.squeeze(1), a_c.squeeze(1), ridx, lensr, re2t, VT, fault)
        step.mass.append(mass)
        return state, logp, live, a.squeeze(1)
    step.mass = []

    def feedback(b, k, e):
        if e < VT:
            nxt = e
        elif fault == "slot_feedback_unk":
            nxt = UNK
        else:
            row = (b + 1) % B if (fault == "maps_of_wrong_row" and k > 0) else b
            nxt = int(e2s[row, e - VT])
        return nxt if 0 <= nxt < table.shape[0] else UNK
    return state0, step, feedback


def decode(sd, cfg, cell, src, lens, max_len, W, idx, e2t, e2s, dtype=torch.float64, fault=None, force=None):
    """beam-search decode of a fixture network -> search()'s dict with `attentions` for aux, and `mass`: per step [R, CV] the copy mass"""
    state0, step, feedback = model_step(sd, cfg, cell, src, lens, idx, e2t, e2s, dtype, fault)
    out = search(step, state0, src.shape[0], W, max_len, feedback, fault, force)
    out["attentions"] = out.pop("aux")
    out["mass"] = step.mass
    return out


# ------------------------------------------------------------------ brute force over a table of next-token distributions
def table_step(logp, live):
    """a model whose state is the last token: the distribution of a row = logp[last token]; logp [N + 1, N], row N is the start symbol's"""
    def step(state, tok):
        return state, logp[tok], live[tok], tok.unsqueeze(1).to(logp.dtype)
    return step


def brute_force(logp, live, max_len):
    """every EOS-collapsed sequence of max_len steps over the live candidates with its score -> list of (score, tokens), score descending"""
    N = logp.shape[1]
    seqs = [((), 0.0, N, False)]
    for _ in range(max_len):
        nxt = []
        for toks, sc, last, done in seqs:
            if done:
                nxt.append((toks + (EOS,), sc, EOS, True))
            else:
                nxt.extend((toks + (e,), sc + float(logp[last, e]), e, e == EOS) for e in range(N) if bool(live[last, e]))
        seqs = nxt
    return sorted(((sc, toks) for toks, sc, _, _ in seqs), key=lambda x: -x[0])


# ------------------------------------------------------------------ the bound
def accept_decode(got, ref, chain, n_split, margin=None):
    return BR.accept_decode(got, ref, chain, n_split, MARGIN if margin is None else margin)


# ------------------------------------------------------------------ the fixtures: the acg.npz cases with a network of their own per seed
# (kind, tag) -> per width: [seed, smallest gap] (searched by tests/golden/generate_acg_beam.py, asserted by tests/test_acg_beam_host.py)
CASES = [("lstm", t) for t in AR.CASES] + [("gru", "general")]
WIDE_CASE = ("lstm", "general")                                                  # also runs W = 3 and W = 8
MAXLEN, MAXLEN_W8 = 6, 4                                                         # (W = 8 meets the gap condition on all rows at 4 steps)


def widths(kind, tag):
    return (1, 3, 4, 8) if (kind, tag) == WIDE_CASE else (1, 4)


def max_len(W):
    return MAXLEN_W8 if W == 8 else MAXLEN


def seeds():
    """{"<kind>_<tag>": {"<W>": [seed, smallest gap]}}: tests/golden/acg_beam_seeds.json"""
    return json.loads(open(os.path.join(GOLDEN, "acg_beam_seeds.json")).read())


def batch():
    """the decode batch of acg.npz with its index tensors: dict(src, lens, idx, e2t, e2s, src_dict, tgt_dict, vocabs, ...)"""
    d = AR.batch_inputs()
    d["e2t"], d["e2s"] = AR.index_tensors(d)
    return d


def case(kind, tag, W, seed=None):
    """(network on the CPU, cfg, cell): the shapes of the acg.npz case, weights det_state_dict(shapes, seed), generator.bias with
    beam_ref.noisy_bias(seed) -- noise and the EOS lift.  W = 1 shares the seed of W = 4."""
    from context_attentive_ir_amd.detinit import det_state_dict
    from context_attentive_ir_amd.recommender import ACG, ACGGRU
    if seed is None:
        seed = seeds()["%s_%s" % (kind, tag)][str(4 if W == 1 else W)][0]
    if kind == "gru":
        net, c = ACGGRU(GR.case_args("acg", tag)), GR.case_cfg("acg", tag)
    else:
        net, c = ACG(AR.case_args(tag)), AR.case_cfg(tag)
    net.load_state_dict(det_state_dict({k: v.shape for k, v in net.state_dict().items()}, seed))
    with torch.no_grad():
        net.generator.bias.copy_(BR.noisy_bias(net.generator.bias, seed))
    net.eval()
    return net, c, ("GRU" if kind == "gru" else "LSTM")


def conditions(ref, free32, W, VT, e2t):
    """the fixture conditions of a (case, W) on the float64 decode `ref` and the free-running float32 decode -> dict of booleans + min_gap.
    slot / fed: on a beam k > 0 at a step >= 1, a selected un-collapsed slot / a selected target word whose copy mass is nonzero"""
    B = e2t.shape[0]
    ident = torch.arange(W).view(1, 1, W).expand_as(ref["backptr"])
    slot = fed = False
    for t, b, k, e in ref["picked"]:
        if k == 0 or t == 0 or bool(ref["finished_at"][t][b, k]):
            continue
        if e >= VT:
            slot = True
        else:
            cs = [c for c in range(2, e2t.shape[1]) if int(e2t[b, c]) == e]
            fed = fed or (bool(cs) and float(ref["mass"][t][k * B + b, cs].sum()) > 0)
    return dict(min_gap=float(ref["gaps"].min()), gap=float(ref["gaps"].min()) >= MIN_GAP, eos=bool((ref["tokens"] == EOS).any()),
                mixed=bool(ref["finished"].any()) and bool((~ref["finished"]).any()), moved=bool((ref["backptr"] != ident).any()),
                f32=bool(torch.equal(ref["backptr"], free32["backptr"])) and bool(torch.equal(ref["tokens"], free32["tokens"])), slot=slot, fed=fed)


MARGIN_CAP = gemm_ref.MARGIN_CAP
