"""The acceptance criterion of ACG's sampling decode (csrc/sample.hip: sample_gen_kernel<.., PAD>, acg_sample_row_kernel; ACG.sample_extended):
a restatement in float64 (the reference) and float32 (the yardstick of what fp32 arithmetic costs) on top of acg_beam_ref (model_step,
collapsed_rows: the FULL collapsed distribution of every row, [R, VT + CV] -- what the HIP path never writes, and what checks its argument that
1 + CV candidates per row suffice) and sample_ref (Philox, Gumbel, the freeze rule).  The reference project has no sampler; the semantics are this
project's (the head of include/neuroir_acg_sample.h):

    rows      R = B N, row r = n B + b; the copy maps, ext2tgt, ext2src and the lengths are NOT repeated: row r reads source row r % B
    P(e)      acg_beam_ref's: the collapsed distribution by extended id e; a collapsed slot is no candidate
    noise     sample_ref's keyed by the EXTENDED id: counter (e >> 2, b, t, n), word e & 3
    choice    token = argmax_e (log P(e) / tau + g[e]) over the candidates, ties to the smaller e; top_k = K: over the K largest P (descending,
              the smaller id first among equals) with the same noise keyed by e
    logp      log P(token): tau = 1 over the full collapsed distribution, whatever tau and top_k are
    freeze    sample_ref's; feedback acg_beam_ref's (tgt2src[e] below VT, ext2src[b, e - VT] from VT on, <unk> outside the source vocabulary)

`fault` plants one of ten mistakes (tests/test_acg_sample_host.py shows on the CPU that the criteria reject each):
    "copy_mass_ignored"              a draw from the generator's softmax alone
    "noise_keyed_by_word_for_slots"  slot c takes the noise of id c, not of VT + c
    "collapsed_slot_drawn"           nothing is collapsed: a collapsed slot keeps its mass and stays a candidate, its target gets none
    "target_offered_twice"           a collapsed slot stays a candidate, with its mass, next to its target word (acg_beam_ref's)
    "tau_on_generator_only"          the temperature divides the words' log P alone; the slots are perturbed at tau = 1
    "maps_of_wrong_row"              samples n > 0 read the maps of source row (b + 1) % B (acg_beam_ref's)
    "slot_feedback_unk"              a drawn slot feeds back <unk> (acg_beam_ref's)
    "pad_raw"                        the PAD logit is not replaced by -1e-20 (acg_beam_ref's)
    "logp_at_tau"                    logp is the log-probability under P^(1/tau) normalised, not under P
    "eos_grows"                      rows go on sampling behind EOS (sample_ref's)
"""
import numpy as np
import torch

import acg_beam_ref as BRA
import beam_ref
import gemm_ref
import sample_ref as SR

EOS, BOS, UNK = 3, 2, 1
FAULTS = ("copy_mass_ignored", "noise_keyed_by_word_for_slots", "collapsed_slot_drawn", "target_offered_twice", "tau_on_generator_only",
          "maps_of_wrong_row", "slot_feedback_unk", "pad_raw", "logp_at_tau", "eos_grows")
STAT_FAULTS = FAULTS[:4]                                                          # also rejected by the chi-square on the restatement
NEG = float("-inf")
E_G = SR.E_G
MIN_GAP = SR.MIN_GAP
# acg_beam_ref.MARGIN's role.  The house rule on the largest ratio measured on the MI355X (DESIGN.md section 33,
# profiles/acg_sample_criterion_mi355x.log): doubled, rounded up to a power of two, never above gemm_ref.MARGIN_CAP.  The largest ratio over
# the 48 (case, setting, form) decodes is -30.3 -- every error lies inside the split-format term alone -- so the margin is the smallest power
# of two the rule can give, 2^0
MARGIN = 1.0
MARGIN_CAP = gemm_ref.MARGIN_CAP


# ------------------------------------------------------------------ one step
def _model_fault(fault):
    """the faults acg_beam_ref.collapsed_rows / model_step plant themselves"""
    return fault if fault in ("target_offered_twice", "maps_of_wrong_row", "slot_feedback_unk", "pad_raw") else None


def faulty_rows(logp, live, mass, e2t, VT, fault):
    """the distribution a fault draws from, on collapsed_rows' outputs (log P [R, NE], live, mass [R, CV]); e2t per row [R, CV].  Both faults take
    the collapsed mass off the targets again: what is left of a word is (1 - z) softmax(l)[v]"""
    P = torch.exp(logp)
    for r in range(P.shape[0]):
        for c in range(2, e2t.shape[1]):
            t = int(e2t[r, c])
            if 0 <= t < VT:
                P[r, t] -= mass[r, c]
                P[r, VT + c] = mass[r, c]
    P = P.clamp(min=0)
    if fault == "collapsed_slot_drawn":
        return torch.log(P), torch.ones_like(live)
    live = live.clone()                                                           # copy_mass_ignored: the words alone, renormalised -- the generator's softmax
    live[:, VT:] = False
    P[:, :VT] = P[:, :VT] / P[:, :VT].sum(1, keepdim=True)
    return torch.log(P), live


def choose(logp, live, seed, step, nsrc, inv_tau, VT, top_k=0, fault=None, dtype=torch.float64):
    """logp [R, NE] (log P of every extended id), live [R, NE] (False: no candidate) -> dict(token [R], logp [R] (log P of the token), p [R, NE]
    (the perturbed values, -inf where not a candidate), gap [R] (best - second best perturbed value; inf with fewer than two finite ones))"""
    R_, NE = logp.shape
    logp = logp.to(dtype)
    cand = live.clone()
    if top_k > 0:                                                                 # the K largest P among the candidates, the smaller id first
        masked = torch.where(cand, logp, torch.full_like(logp, NEG))
        order = torch.sort(masked, dim=1, descending=True, stable=True)[1][:, :top_k]
        keep = torch.zeros_like(cand)
        keep.scatter_(1, order, True)
        cand = cand & keep
    ids = np.broadcast_to(np.arange(NE), (R_, NE)).copy()
    if fault == "noise_keyed_by_word_for_slots":
        ids[:, VT:] -= VT
    g = torch.from_numpy(SR.gumbel(SR.words(seed, step, nsrc, R_, NE, ids)))
    scale = torch.full((NE,), float(inv_tau), dtype=torch.float64)
    if fault == "tau_on_generator_only":
        scale[VT:] = 1.0
    if dtype == torch.float64:
        p = logp * scale + g
    else:                                                                         # fma(log P, 1 / tau, g) on fp32 operands, one rounding
        p = (logp.double() * scale.float().double() + g.float().double()).float()
    p = torch.where(cand & (logp > NEG), p, torch.full_like(p, NEG))              # P = 0 is never chosen
    best = p.max(1, keepdim=True)[0]
    e = torch.arange(NE).unsqueeze(0).expand(R_, NE)
    tok = torch.where((p == best) & (best > NEG), e, torch.full_like(e, 1 << 40)).min(1)[0]
    tok = torch.where(tok < (1 << 40), tok, torch.zeros_like(tok))               # no candidate of positive probability: id 0
    srt = torch.sort(p.double(), dim=1, descending=True)[0]
    gap = srt[:, 0] - srt[:, 1]
    gap = torch.where(torch.isnan(gap), torch.full_like(gap, float("inf")), gap)
    lp = logp.gather(1, tok.unsqueeze(1)).squeeze(1)
    if fault == "logp_at_tau":
        lp = lp * inv_tau - torch.logsumexp(torch.where(live, logp * inv_tau, torch.full_like(logp, NEG)), 1)
    return dict(token=tok, logp=lp, p=p, gap=gap)


# ------------------------------------------------------------------ the decode
@torch.no_grad()
def sample(step_fn, state0, B, N, max_len, seed, feedback, VT, e2t, inv_tau=1.0, top_k=0, fault=None, force=None, dtype=torch.float64, bos=BOS):
    """step_fn / feedback: acg_beam_ref.model_step's.  force [max_len, R]: the tokens are these instead of the sampler's own -- log-probabilities
    still the chain's.  -> sample_ref.sample's dict (s: the largest finite |log P| of a candidate) + picked: every live draw as (step, b, n, e),
    mass: per step [R, CV] the copy mass"""
    state = beam_ref.repeat_state(state0, N)
    R_ = B * N
    tok = torch.full((R_,), bos, dtype=torch.long)
    fin = torch.zeros(R_, dtype=torch.bool)
    cum = torch.zeros(R_, dtype=dtype)
    length = torch.full((R_,), max_len, dtype=torch.long)
    toks, lps, auxs, gaps, picked, s = [], [], [], [], [], 0.0
    rows_b = torch.arange(B).repeat(N)
    for t in range(max_len):
        state, logp, live, aux = step_fn(state, tok)
        mass = step_fn.mass[-1]
        if fault in ("collapsed_slot_drawn", "copy_mass_ignored"):
            logp, live = faulty_rows(logp, live, mass, e2t[rows_b], VT, fault)
        s = max(s, float(logp[live & (logp > NEG)].abs().max()))
        c = choose(logp, live, seed, t, B, inv_tau, VT, top_k, fault, dtype)
        v = c["token"] if force is None else force[t].long()
        lp = c["logp"] if force is None else logp.to(dtype).gather(1, v.unsqueeze(1)).squeeze(1)
        gap = c["gap"]
        picked.extend((t, r % B, r // B, int(v[r])) for r in range(R_) if not bool(fin[r]))
        if fault != "eos_grows":
            v = torch.where(fin, torch.full_like(v, EOS), v)
            lp = torch.where(fin, torch.zeros_like(lp), lp)
            gap = torch.where(fin, torch.full_like(gap, float("inf")), gap)
        cum = cum + lp
        newly = (v == EOS) & ~fin
        length = torch.where(newly, torch.full_like(length, t + 1), length)
        if fault != "eos_grows":
            fin = fin | newly
        tok = torch.tensor([feedback(r % B, r // B, int(v[r])) for r in range(R_)], dtype=torch.long)
        toks.append(v)
        lps.append(lp)
        auxs.append(aux)
        gaps.append(gap)

    def out(x):                                                                    # [max_len, R, ...] -> [B, N, max_len, ...]
        x = torch.stack(x)
        return x.view((max_len, N, B) + tuple(x.shape[2:])).permute(2, 1, 0, *range(3, x.dim() + 1)).contiguous()
    return dict(predictions=out(toks), token_logprobs=out(lps), scores=cum.view(N, B).t().contiguous(), lengths=length.view(N, B).t().contiguous(),
                aux=out(auxs), tokens=torch.stack(toks), gaps=torch.stack(gaps), picked=picked, mass=step_fn.mass, s=s)


def decode(sd, cfg, cell, src, lens, max_len, N, seed, idx, e2t, e2s, tau=1.0, top_k=0, dtype=torch.float64, fault=None, force=None):
    """sampling decode of a fixture network -> sample()'s dict with `attentions` for aux"""
    state0, step, feedback = BRA.model_step(sd, cfg, cell, src, lens, idx, e2t, e2s, dtype, _model_fault(fault))
    VT = sd["generator.weight"].shape[0]
    out = sample(step, state0, src.shape[0], N, max_len, seed, feedback, VT, e2t, 1.0 / tau, top_k, fault, force, dtype)
    out["attentions"] = out.pop("aux")
    return out


# ------------------------------------------------------------------ the bounds
def token_bound(ref, chain, n_split, tau):
    """2 (E_y / tau + E_G), sample_ref.model_token_bound's form: E_y = s (MARGIN max(e_chain, 2^-23) + n_split FMT), e_chain the float32 chain's
    error of a token log-probability (forced along the float64 tokens) at the scale s.  s is the largest finite |log P| of a candidate in the
    float64 decode: log P[v] = l[v] - lse(l) + log(1 - z) moves one for one with the logit (less where copy mass is added), so the spread of log P
    is the spread of the logits, which is what the split products' error is relative to"""
    s = ref["s"]
    lp64, lp32 = ref["token_logprobs"], chain["token_logprobs"].double()
    ok = torch.isfinite(lp64) & torch.isfinite(lp32)
    e_chain = float((lp32 - lp64)[ok].abs().max()) / s
    e_y = s * (beam_ref.MARGIN * max(e_chain, beam_ref.EPS) + n_split * gemm_ref.FMT["fp16x2"])
    return 2 * (e_y / tau + E_G)


def accept_decode(got, ref, chain, n_split, margin=None):
    return SR.accept_decode(got, ref, chain, n_split, MARGIN if margin is None else margin)


# ------------------------------------------------------------------ the fixtures: acg_beam_ref's six cases at width 4 (networks with a noisy bias)
CASES = BRA.CASES
N = 4
SETTINGS = ((1.0, 0), (0.7, 0), (1.0, 3), (0.7, 3))                                 # (tau, top_k)
MAXLEN = 6
SEARCH_LIMIT = 64                                                                   # seeds tried per (case, setting)
N_SPLIT = 2                                                                         # split products per token on the fast path: the fp16-term step and the fused generator
# (kind_tag) -> one seed per setting, in SETTINGS' order: the first seed (from 1) that keeps every live step's float64 top-two gap of the perturbed
# values above max(10 x token bound, MIN_GAP) and whose free-running float32 sampler draws the float64 tokens; over a case's four settings the
# samples hold a drawn un-collapsed slot, a drawn target with nonzero copy mass and a drawn word with none (tests/test_acg_sample_host.py asserts
# that these are the search's)
SEEDS = {'lstm_general': [2, 2, 1, 1], 'lstm_dot': [1, 2, 1, 1], 'lstm_mlp': [2, 2, 1, 1], 'lstm_own': [1, 1, 1, 1], 'lstm_wide': [1, 1, 1, 1],
         'gru_general': [1, 1, 1, 2]}
# one seed per case at (tau 0.7, top_k 0) whose samples additionally hold no PAD in front of their first EOS: handed to score_extended
SCORE_SEEDS = {'lstm_general': 2, 'lstm_dot': 2, 'lstm_mlp': 2, 'lstm_own': 1, 'lstm_wide': 1, 'gru_general': 1}


def case(kind, tag):
    return BRA.case(kind, tag, 4)


def batch():
    return BRA.batch()


def seed_conditions(kind, tag, tau, top_k, seed, D=None, net=None):
    """-> (dict(gap, bound, gap_ok, f32: the free-running float32 sampler draws the float64 tokens), the float64 decode)"""
    D = batch() if D is None else D
    net, c, cell = case(kind, tag) if net is None else net
    args = (net.state_dict(), c, cell, D["src"], D["lens"], MAXLEN, N, seed, D["idx"], D["e2t"], D["e2s"], tau, top_k)
    ref = decode(*args)
    chain = decode(*args, dtype=torch.float32, force=ref["tokens"])
    free = decode(*args, dtype=torch.float32)
    bound = token_bound(ref, chain, N_SPLIT * MAXLEN, tau)
    gap = float(ref["gaps"].min())
    return dict(gap=gap, bound=bound, gap_ok=gap > max(10 * bound, MIN_GAP), f32=bool(torch.equal(free["tokens"], ref["tokens"]))), ref


def search_seed(kind, tag, tau, top_k, extra=None, D=None, net=None):
    """the first seed from 1 that meets seed_conditions (and extra(ref), where given), or None within SEARCH_LIMIT"""
    for seed in range(1, SEARCH_LIMIT + 1):
        cond, ref = seed_conditions(kind, tag, tau, top_k, seed, D, net)
        if cond["gap_ok"] and cond["f32"] and (extra is None or extra(ref)):
            return seed
    return None


def pad_free(ref):
    """no PAD in front of a sample's first EOS"""
    pred, ln = ref["predictions"], ref["lengths"]
    live = torch.arange(pred.shape[2]).view(1, 1, -1) < ln.unsqueeze(2)
    return not bool(((pred == 0) & live).any())


def drawn_kinds(ref, VT, e2t):
    """(a drawn un-collapsed slot, a drawn target with nonzero copy mass, a drawn word without) among a decode's live draws"""
    B = e2t.shape[0]
    slot = fed = word = False
    for t, b, n, e in ref["picked"]:
        if e >= VT:
            slot = True
            continue
        cs = [c for c in range(2, e2t.shape[1]) if int(e2t[b, c]) == e]
        m = float(ref["mass"][t][n * B + b, cs].sum()) if cs else 0.0
        fed, word = fed or m > 0, word or m == 0
    return slot, fed, word


# ------------------------------------------------------------------ the generator-level cases (nir_acg_sample_gen_select driven directly)
def gen_rows(d, nsrc, dtype=torch.float64, fault=None):
    """the full collapsed rows of a generator-level problem `d`: row r reads source row r % nsrc -> (log P [R, VT + CV], live, logits [R, VT]).
    A map entry outside [0, CV) contributes nothing; ext2tgt outside [0, VT) does not collapse"""
    import acg_score_ref as SC
    o, VT, CV = d["o"], d["gen_w"].shape[0], d["e2t"].shape[1]
    rows = torch.arange(o.shape[0]) % nsrc
    sd = SC._sd(d["gen_w"], d["gen_b"], d["copy_w"], d["copy_b"], dtype)
    idx, lens = d["smap"][rows], d["lens"][rows].clamp(0, d["smap"].shape[1])
    a = d["attn"].to(dtype).clone()
    a[(idx < 0) | (idx >= CV)] = 0
    P, l = SC.extended_rows(sd, o.to(dtype), a, idx.clamp(0, CV - 1), lens, CV, "no_pad" if fault == "pad_raw" else None)
    e2t = d["e2t"][rows]
    e2t = torch.where((e2t >= 0) & (e2t < VT), e2t, torch.full_like(e2t, -1))
    e2t[:, :2] = -1
    mass = P[:, VT:].clone()
    P = BRA.AR.collapse_(P, e2t, VT, "no_blank" if fault == "target_offered_twice" else None)
    live = torch.ones_like(P, dtype=torch.bool)
    if fault != "target_offered_twice":
        live[:, VT:] = e2t < 0
    return torch.log(P), live, l, mass


STAT_VT, STAT_CV = 37, 5


def stat_problem(rows=16384, K=32):
    """the statistical case: `rows` identical rows, nsrc = 1, VT 37, CV 5.  The five slots: 0 un-collapsed with mass (two positions), 1 empty (no
    position), 2 collapsed onto word 7, 3 and 4 sharing word 9.  The switch sits near 0.6, half of the attention on slot 0; the bias is lowered by 3.5 so that PAD's logit (about zero) is one of the larger: PAD and slot 0 both hold real mass,
    which is what shows a slot drawing with the noise of a word's id"""
    g, QL = torch.Generator().manual_seed(4100), 6
    x = torch.randn(1, K, generator=g)
    x[0, 0] = 0.0
    w = torch.randn(STAT_VT, K, generator=g) / K ** 0.5 * 1.06
    w[:, 0] = 0
    cw = torch.zeros(K)
    cw[0] = 1.0
    attn = torch.tensor([[0.30, 0.15, 0.15, 0.10, 0.20, 0.10]])
    return dict(o=x.expand(rows, K).contiguous(), gen_w=w, gen_b=1.06 * torch.randn(STAT_VT, generator=g) - 3.5, copy_w=cw, copy_b=torch.tensor([0.4]),
                attn=attn.expand(rows, QL).contiguous(), lens=torch.tensor([QL]), smap=torch.tensor([[0, 2, 3, 4, 0, 3]]),
                e2t=torch.tensor([[-1, -1, 7, 9, 9]]))


GEN_CLASSES = ("vocab", "slot", "enters", "raw_target", "shared", "pad_raw", "pad_target", "generic")
LIFT, SWITCH = 90.0, 85.0                                                           # the noise lies in (-2.9, 16.7): 85 / 4 > 16.7 + 2.9 at every tau <= 4


def gen_problem(rows, nsrc, K, VT, CV, QL, seed=0):
    """One problem of nir_acg_sample_gen_select with a class planted per row (cycled over the rows; a class that does not fit QL / CV / the source
    row gives way to "generic") -> dict(o, gen_w, gen_b, copy_w, copy_b, attn, lens, smap, e2t, cls [R] (index into GEN_CLASSES), want [R]: the
    extended id that must win whatever the noise is, -1 for generic rows).
    Five features of o are reserved (their generator weights are 0 except as said): f0 is the switch logit (copy_w = e_0); f1 lifts word w_none
    (no slot collapses onto it), f2 word T1 (the target of slot 5), f4 word T2 (the target of slots 3 and 4) by LIFT; f3 pushes EVERY logit down
    by LIFT, which leaves PAD's constant -1e-20 on top.  The map puts slots (5, 3, 4, 2, u) at the first positions (u: a slot that is not collapsed),
    rotated per source row; slot 2 collapses onto PAD's id on source rows b % 4 >= 2; slot CV - 1 has no position (mass 0); every fifth source row (from
    the fourth) has length 0; source rows b % 3 == 1 carry map entries outside [0, CV) in front of their length, under real attention.  Behind
    every length the map points at used slots and the attention holds 7.0.
    classes:  vocab       f1 lifted, switch -SWITCH                      -> w_none            slot     switch +SWITCH, attention on u's position -> VT + u
              enters      switch +SWITCH, attention on slot 5's position -> T1 (by its mass)   raw_target  f2 lifted, switch -SWITCH           -> T1
              shared      switch +SWITCH, attention on slots 3 and 4     -> T2                 pad_raw  f3 lifted, switch -SWITCH              -> 0
              pad_target  switch +SWITCH, attention on slot 2            -> 0                  generic  nothing planted"""
    g = torch.Generator().manual_seed(7000 + seed)
    assert VT >= 5 and CV >= 2 and QL >= 1 and K >= 32
    o = gemm_ref.family("randn", g, rows, K, "a")
    gen_w = gemm_ref.family("randn", g, VT, K, "w")
    gen_b = torch.randn(VT, generator=g)
    o[:, :5] = 0
    gen_w[:, :5] = 0
    w_none, T1, T2 = 1, VT - 2, VT - 1
    gen_w[w_none, 1], gen_w[T1, 2], gen_w[T2, 4] = 1.0, 1.0, 1.0
    gen_w[:, 3] = -1.0
    copy_w = torch.zeros(K)
    copy_w[0] = 1.0
    copy_b = torch.tensor([0.25])
    lens = torch.full((nsrc,), QL, dtype=torch.long)
    lens[3::5] = 0
    u = 6 if CV > 7 else 1
    e2t = torch.full((nsrc, CV), -1, dtype=torch.long)
    e2t[:, :2] = T1                                                                 # slots 0 and 1 are never collapsed, whatever their entry says
    if CV > 2:
        e2t[2::4, 2] = e2t[3::4, 2] = 0
    if CV > 4:
        e2t[:, 3] = e2t[:, 4] = T2
    if CV > 5:
        e2t[:, 5] = T1
    for c in range(7, CV - 1):
        if c % 3 == 0:
            e2t[:, c] = 2 + c % (VT - 4)                                            # further collapsed slots, never onto w_none, T1 or T2
        elif c % 3 == 1:
            e2t[:, c] = VT + 5                                                      # outside [0, VT): not collapsed
    free = max(1, CV - 1)
    smap = torch.randint(0, free, (nsrc, QL), generator=g)
    pos = torch.full((nsrc, CV), -1, dtype=torch.long)                              # the planted position of a slot
    for b in range(nsrc):
        n = int(lens[b])
        for j, c in enumerate([5, 3, 4, 2, u][:n]):
            if c < free:
                smap[b, (j + b) % n] = c
        if b % 3 == 1 and n > 6:                                                    # two positions the plan leaves alone
            smap[b, (5 + b) % n], smap[b, (6 + b) % n] = -1, CV + 3
        for j in range(n):
            c = int(smap[b, j])
            if 0 <= c < CV and int((smap[b, :n] == c).sum()) == 1:                  # a slot's one position
                pos[b, c] = j
        smap[b, n:] = torch.tensor([(5, 3, 2, 6, 0, 1)[j % 6] % CV for j in range(QL - n)], dtype=torch.long)
    rb = torch.arange(rows) % nsrc
    behind = torch.arange(QL).unsqueeze(0) >= lens[rb].unsqueeze(1)
    logit_a = torch.randn(rows, QL, generator=g)
    cls = torch.full((rows,), GEN_CLASSES.index("generic"), dtype=torch.long)
    want = torch.full((rows,), -1, dtype=torch.long)
    o[:, 0] = 1.5 * torch.randn(rows, generator=g)
    for r in range(rows):
        b, name = int(rb[r]), GEN_CLASSES[r % len(GEN_CLASSES)]
        collapses = lambda c: c >= 2 and c < CV and 0 <= int(e2t[b, c]) < VT          # noqa: E731
        at = lambda c: int(pos[b, c]) if c < CV else -1                              # noqa: E731
        if name == "vocab":
            o[r, 1], o[r, 0], want[r] = LIFT, -SWITCH, w_none
        elif name == "raw_target" and collapses(5):
            o[r, 2], o[r, 0], want[r] = LIFT, -SWITCH, T1
        elif name == "pad_raw":
            o[r, 3], o[r, 0], want[r] = LIFT, -SWITCH, 0
        elif name == "slot" and at(u) >= 0 and not collapses(u):
            o[r, 0], want[r] = SWITCH, VT + u
            logit_a[r, at(u)] += SWITCH
        elif name == "enters" and collapses(5) and at(5) >= 0:
            o[r, 0], want[r] = SWITCH, T1
            logit_a[r, at(5)] += SWITCH
        elif name == "shared" and collapses(3) and collapses(4) and at(3) >= 0 and at(4) >= 0:
            o[r, 0], want[r] = SWITCH, T2
            logit_a[r, at(3)] += SWITCH
            logit_a[r, at(4)] += SWITCH
        elif name == "pad_target" and collapses(2) and at(2) >= 0:
            o[r, 0], want[r] = SWITCH, 0
            logit_a[r, at(2)] += SWITCH
        else:
            continue
        cls[r] = r % len(GEN_CLASSES)
    attn = torch.softmax(logit_a.masked_fill(behind, NEG), 1)
    attn[behind] = 7.0
    return dict(o=o, gen_w=gen_w, gen_b=gen_b, copy_w=copy_w, copy_b=copy_b, attn=attn, lens=lens, smap=smap, e2t=e2t, cls=cls, want=want)


def gen_reference(d, nsrc, seed, step, tau, top_k, n_split):
    """the float64 choice of a generator-level problem and the bounds of a form -> dict(ref: choose()'s, e_y, e_p, logp64, live, s)"""
    VT = d["gen_w"].shape[0]
    logp, live, l64, _ = gen_rows(d, nsrc)
    _, _, l32, _ = gen_rows(d, nsrc, torch.float32)
    ref = choose(logp, live, seed, step, nsrc, 1.0 / tau, VT, top_k)
    e_y = SR.logit_bound(l64, l32, n_split)
    fin = ref["p"][ref["p"] > NEG]
    return dict(ref=ref, e_y=e_y, e_p=SR.perturbed_bound(e_y, 1.0 / tau, float(fin.abs().max())), logp64=logp, live=live, s=float(l64.abs().max()))


def accept_tokens(got, g):
    """got [R] against gen_reference's dict: the float64 token wherever its gap exceeds 2 e_p; elsewhere one of the candidates within 2 e_p of the
    best -> (ok, number of near-tie rows)"""
    ref, e_p = g["ref"], g["e_p"]
    got = torch.as_tensor(np.asarray(got.cpu() if torch.is_tensor(got) else got)).long()
    near = ref["gap"] <= 2 * e_p
    ok = bool(torch.equal(got[~near], ref["token"][~near]))
    best = ref["p"].max(1, keepdim=True)[0]
    for r in torch.nonzero(near).flatten().tolist():
        ok = ok and bool(ref["p"][r, got[r]] >= best[r] - 2 * e_p)
    return ok, int(near.sum())
