"""The acceptance criterion of teacher-forced scoring under ACG's collapsed extended distribution (csrc/score.hip, include/neuroir_acg_score.h;
ACG / ACGGRU.score_extended, CopyRecommender.score_extended): a restatement in float64 (the reference) and float32 (the yardstick of what fp32
arithmetic costs), on top of acg_ref (gen_parts, copy_attention, extended, collapse_) and score_ref (sequences, the bound).  The reference
project has no scorer; the semantics are this project's and mirror the beam's (acg_beam_ref):

    rows        the whole collapsed extended distribution of every teacher-forced row is WRITTEN here, [R, VT + CV], by the reference's own op
                order (acg_ref.extended, then decode()'s collapse) -- what the HIP path never forms -- and read at the row's canonical id
    canonical   a word id below VT is itself; a slot VT + c that collapses (c >= 2, ext2tgt[b, c] in [0, VT)) is its word -- one word has one
                probability, however it is spelled (the reference's matrix holds 1e-10 at such a slot); any other slot is itself
    masked      0 where the id is PAD, negative, or at / past VT + CV (that last case is flagged)
    row r       reads source row r // rows_per_src
    sequences   score_ref.sequences, unchanged: PAD and negative ids do not count, a sequence is frozen behind EOS
    models      score_ref.score's teacher-forced pass with ACG's default inputs (tgt2src below VT, ext2src[b, e - VT] from VT on)

Bound: score_ref's form.  s = max |logit_ref64| (PAD overridden); e <= MARGIN * max(e_chain, 2^-23) + n_split * FMT["fp16x2"].  d log P is at
most the logit error plus the lse error, because the generator's share of P is at most 1, and the copy share is fp32 arithmetic on the library's
side and the restatement's alike: n_split = 2 per token fused, 0 plain; a sequence T times that; model level + score_ref.n_path.  -inf must
match exactly and is left out of e.

`fault` plants one of eight mistakes (tests/test_acg_score_host.py shows on the CPU that the criterion rejects each at MARGIN_CAP):
    "no_pad_sub"          the PAD logit is not replaced by -1e-20
    "no_collapse_mass"    a word is scored without the mass of the slots that collapse onto it
    "one_slot_only"       of two slots sharing a word only the first is counted
    "slot_not_canonical"  a collapsed slot id reads the slot's own entry instead of its word's
    "swap_switch"         z and 1 - z exchanged
    "wrong_src_row"       row r reads source r % nsrc (the beam's layout) instead of r // rows_per_src
    "reads_past_len"      the copy attention and the map are read at every position, not at j < len
    "shift"               step t is scored against token t instead of t + 1
"""
import torch

import acg_ref as AR
import gemm_ref
import gru_dec_ref as GR
import score_ref as SR
import seq2seq_ref as S

PAD, UNK, BOS, EOS = AR.PAD, AR.UNK, AR.BOS, AR.EOS
FAULTS = ("no_pad_sub", "no_collapse_mass", "one_slot_only", "slot_not_canonical", "swap_switch", "wrong_src_row", "reads_past_len", "shift")
GEN_FAULTS = FAULTS[:-1]                                                        # those a generator-level case can show
MARGIN = 4.0                                                                    # the house rule on the ratios measured on the MI355X: DESIGN.md section 31
MARGIN_CAP = gemm_ref.MARGIN_CAP
EPS, FMT = SR.EPS, SR.FMT
NEG = float("-inf")


# ------------------------------------------------------------------ the rows
def _sd(gen_w, gen_b, copy_w, copy_b, dtype):
    return {"generator.weight": gen_w.to(dtype), "generator.bias": (torch.zeros(gen_w.shape[0]) if gen_b is None else gen_b).to(dtype),
            "copy_generator.linear_copy.weight": copy_w.reshape(1, -1).to(dtype), "copy_generator.linear_copy.bias": copy_b.reshape(1).to(dtype)}


def collapse(P, e2t, VT, fault=None):
    """decode()'s collapse per row (acg_ref.collapse_), with the two faults of the mass"""
    if fault == "no_collapse_mass":
        for r in range(P.shape[0]):
            P[r, [VT + c for c in range(2, e2t.shape[1]) if int(e2t[r, c]) >= 0]] = AR.BLANKED
        return P
    if fault == "one_slot_only":
        for r in range(P.shape[0]):
            seen = set()
            for c in range(2, e2t.shape[1]):
                t = int(e2t[r, c])
                if t >= 0:
                    if t not in seen:
                        P[r, t] += P[r, VT + c]
                    seen.add(t)
                    P[r, VT + c] = AR.BLANKED
        return P
    return AR.collapse_(P, e2t, VT)


def canonical(e, e2t_rows, VT, fault=None):
    """extended ids [R] -> the entry of the collapsed row that holds the id's probability (clamped where the id is masked)"""
    CV = e2t_rows.shape[1]
    c = (e - VT).clamp(0, CV - 1)
    t = e2t_rows.gather(1, c.unsqueeze(1)).squeeze(1)
    coll = (e >= VT) & (e < VT + CV) & (c >= 2) & (t >= 0) & (t < VT)
    if fault == "slot_not_canonical":
        coll = torch.zeros_like(coll)
    return torch.where(coll, t, e.clamp(0, VT + CV - 1))


def extended_rows(sd, o, a_c, idx, lens, CV, fault=None):
    """acg_ref.extended with the loop over the rows taken inside the tensor operations: per row the same operations in the same order (position
    j ascending, copy[c] = z a[j] + copy[c]), one pass over the positions for all rows (tests/test_acg_score_host.py: the copy part equal to the
    bit).  One difference, the project's (neuroir_acg_beam.h): 1 - z is sigmoid(-x), not 1 - sigmoid(x), so that a saturated switch keeps its
    small side -- at x = 40 the reference's form is exactly 0 even in float64."""
    l, s, z = AR.gen_parts(sd, o, fault)
    x = o @ sd["copy_generator.linear_copy.weight"].t() + sd["copy_generator.linear_copy.bias"]
    omz = torch.sigmoid(x if fault == "swap_switch" else -x)
    copy = torch.zeros(o.shape[0], CV, dtype=o.dtype)
    r = torch.arange(o.shape[0])
    for j in range(int(lens.max()) if lens.numel() else 0):
        live = j < lens
        c = idx[:, j]
        copy[r[live], c[live]] = z[live, 0] * a_c[live, j] + copy[r[live], c[live]]
    return torch.cat([omz * s, copy], 1), l


def gen_target(o, gen_w, gen_b, copy_w, copy_b, attn, lens, smap, e2t, target, rows_per_src, pad=PAD, dtype=torch.float64, fault=None, row_ids=None):
    """the C entry: o [R, K], attn [R, QL], lens [nsrc], smap [nsrc, QL], e2t [nsrc, CV], target [R] extended ids; row_ids [R]: the rows' numbers
    in the call where o / attn / target are a sample of it
    -> (logp [R], logits [R, VT] with the PAD override, flagged [R]: id at or past VT + CV, P [R, VT + CV]: the collapsed rows)"""
    R, VT, CV, nsrc = o.shape[0], gen_w.shape[0], e2t.shape[1], lens.shape[0]
    row_ids = torch.arange(R) if row_ids is None else row_ids
    rows = row_ids % nsrc if fault == "wrong_src_row" else row_ids // rows_per_src
    sd = _sd(gen_w, gen_b, copy_w, copy_b, dtype)
    lr = torch.full((R,), smap.shape[1], dtype=torch.long) if fault == "reads_past_len" else lens[rows].clamp(0, smap.shape[1])
    idx = smap[rows]
    a = attn.to(dtype).clone()
    ok = (idx >= 0) & (idx < CV)                                                    # a map entry outside [0, CV) contributes nothing
    a[~ok] = 0
    P, l = extended_rows(sd, o.to(dtype), a, idx.clamp(0, CV - 1), lr, CV, {"no_pad_sub": "no_pad", "swap_switch": "swap_switch"}.get(fault))
    P = collapse(P, e2t[rows], VT, fault)
    flagged = target >= VT + CV
    counts = (target >= 0) & ~flagged & (target != pad)
    lp = torch.log(P.gather(1, canonical(target, e2t[rows], VT, fault).unsqueeze(1)).squeeze(1))
    return torch.where(counts, lp, torch.zeros_like(lp)), l, flagged, P


def score_rows(o, a_c, w, lens, smap, e2t, cand, rows_per_src, dtype=torch.float64, fault=None):
    """o [nseq, T, K], a_c [nseq, T, QL]; cand [nseq, T + 1] extended ids -> dict(token_logprobs [nseq, T], scores, lengths, s)"""
    nseq, T, K = o.shape
    target = cand[:, :-1] if fault == "shift" else cand[:, 1:]
    lp, l, _, _ = gen_target(o.reshape(nseq * T, K), w["gen_w"], w["gen_b"], w["copy_w"], w["copy_b"], a_c.reshape(nseq * T, -1), lens, smap, e2t,
                             target.reshape(-1), rows_per_src, PAD, dtype, fault)
    lp, sc, ln = SR.sequences(lp.view(nseq, T), target)
    return dict(token_logprobs=lp, scores=sc, lengths=ln, s=float(l.abs().max()))


# ------------------------------------------------------------------ the models
def default_rep(cand, tgt2src, e2s, VT, V):
    """what the ACG decodes feed back for extended ids [B, N, TL]: the first token as it is, tgt2src[e] below VT, ext2src[b, e - VT] from VT
    on, <unk> outside [0, V)"""
    B, N, _ = cand.shape
    CV = e2s.shape[1]
    low = cand.clamp(0, VT - 1)
    word = low if tgt2src is None else tgt2src[low]
    ext = e2s.unsqueeze(1).expand(B, N, CV).gather(2, (cand - VT).clamp(0, CV - 1))
    rep = torch.cat((cand[..., :1], torch.where(cand < VT, word, ext)[..., 1:]), -1)
    return torch.where((rep >= 0) & (rep < V), rep, torch.full_like(rep, UNK))


def extended_targets(target_seq, alignment, VT):
    """the id under which CopyGeneratorCriterion finds a gold token's probability"""
    return torch.where((target_seq == UNK) & (alignment != UNK), alignment + VT, target_seq)


def weights(sd, dtype=torch.float64):
    return dict(gen_w=sd["generator.weight"].to(dtype), gen_b=sd["generator.bias"].to(dtype),
                copy_w=sd["copy_generator.linear_copy.weight"].reshape(-1).to(dtype), copy_b=sd["copy_generator.linear_copy.bias"].to(dtype))


@torch.no_grad()
def score(kind, sd, cfg, src, lens, cand, idx, e2t, e2s, rep=None, tgt2src=None, dtype=torch.float64, fault=None):
    """kind 'lstm' / 'gru': src [B, QL], lens [B], cand [B, N, TL] extended ids -> score_rows' dict in cand's leading shape"""
    sd = S._cast(sd, dtype)
    table = sd[S.EMB]
    B, N, TL = cand.shape
    T, VT = TL - 1, sd["generator.weight"].shape[0]
    rep = default_rep(cand, tgt2src, e2s, VT, table.shape[0]) if rep is None else rep
    emb = table[rep.reshape(-1, TL)[:, :-1]]
    if kind == "gru":
        mem, hn = GR.encode(sd, table[src], lens, cfg["bidirection"])
        state, p = (GR.initial_state(hn, lens),), GR._dec_params(sd)
    else:
        mem, hn, cn = S.encode(sd, table[src], lens, cfg["bidirection"])
        state, p = S.initial_state(hn, cn, lens), [sd[S.DEC + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    rows = torch.arange(B * N) // N                                                 # the teacher-forced pass itself is score_ref's, pinned there
    state, hs = tuple(s[rows] for s in state), []
    for t in range(T):
        state = (GR.cell(emb[:, t], state[0], *p),) if kind == "gru" else S._cell(emb[:, t], state[0], state[1], *p)
        hs.append(state[0])
    o, a = S.attend(sd, cfg["attn_type"], torch.stack(hs, 1), mem[rows], lens[rows])
    a_c = AR.copy_attention(sd, cfg, o, mem[rows], lens[rows], a)
    out = score_rows(o, a_c, weights(sd, dtype), lens, idx, e2t, cand.reshape(B * N, TL), N * T, dtype, fault)
    # (score_rows' rows are (sequence, step): row r of the flat call belongs to source r // (N T))
    return dict(token_logprobs=out["token_logprobs"].view(B, N, T), scores=out["scores"].view(B, N), lengths=out["lengths"].view(B, N), s=out["s"])


def n_path(QL, T):
    return SR.n_path("s2s", QL, T)


# ------------------------------------------------------------------ the bound
def _split_inf(got, ref):
    """-inf must match exactly and is left out of e -> (same, got, ref) with those entries zeroed"""
    got, ref = SR._cpu(got).double(), SR._cpu(ref).double()
    gi, ri = torch.isneginf(got), torch.isneginf(ref)
    same = bool(torch.equal(gi, ri))
    return same, torch.where(gi | ri, torch.zeros_like(got), got), torch.where(gi | ri, torch.zeros_like(ref), ref)


def accept_rows(got_lp, ref_lp, chain_lp, s, n_split, margin=None):
    """generator level: token log-probabilities [R] against the float64 and float32 restatements; s = max |logit_ref64|"""
    margin = MARGIN if margin is None else margin
    assert margin <= MARGIN_CAP
    same, g, r = _split_inf(got_lp, ref_lp)
    _, c, _ = _split_inf(chain_lp, ref_lp)
    f = SR.figures(g, r, c, s, n_split)
    f["bound"] = margin * max(f["e_chain"], EPS) + f["extra"]
    f["inf_equal"] = same
    return same and f["e"] <= f["bound"], f


def accept(got, ref, chain, n_split, margin=None):
    """dicts with token_logprobs [.., T], scores [..], lengths [..]; ref carries s.  n_split per token (a sequence: T times that)"""
    margin = MARGIN if margin is None else margin
    assert margin <= MARGIN_CAP
    T = ref["token_logprobs"].shape[-1]
    out, ok = {}, bool(torch.equal(SR._cpu(got["lengths"]).long(), SR._cpu(ref["lengths"]).long()))
    for key, n in (("token_logprobs", n_split), ("scores", n_split * T)):
        same, g, r = _split_inf(got[key], ref[key])
        _, c, _ = _split_inf(chain[key], ref[key])
        f = SR.figures(g, r, c, ref["s"], n)
        f["bound"] = margin * max(f["e_chain"], EPS) + f["extra"]
        f["inf_equal"] = same
        ok = ok and same and f["e"] <= f["bound"]
        out[key] = f
    out["lengths_equal"] = bool(torch.equal(SR._cpu(got["lengths"]).long(), SR._cpu(ref["lengths"]).long()))
    return ok, out


# ------------------------------------------------------------------ candidates of extended ids for the acg.npz batch
def candidates(d, e2t, VT, TL=6):
    """the decode batch of acg.npz -> [B, 4, TL] candidates of unequal length, BOS first.  Per source row: n = 0 walks the row's own source --
    a copied out-of-vocabulary word as its slot id where the row has one, words both generated and copied as their target ids -- and ends in
    EOS; n = 1 words absent from the source, an EOS in the middle, a PAD tail; n = 2 EOS at once, then PAD; n = 3 a collapsed slot id (scored as
    its word), an EOS in the middle and tokens (EOS among them) behind it, the way a beam's predictions row looks."""
    src, lens, idx = d["src"], d["lens"], d["idx"]
    B = src.shape[0]
    out = torch.full((B, 4, TL), PAD, dtype=torch.long)
    out[:, :, 0] = BOS
    mid = min(max(2, TL // 2), TL - 1)
    for b in range(B):
        n_b = int(lens[b])
        own = []
        for j in range(n_b):                                                        # the row's source as extended ids
            w, c = int(src[b, j]), int(idx[b, j])
            own.append(w if w < VT else VT + c)
        walk = (own * TL)[:TL - 2] + [EOS]
        out[b, 0, 1:1 + len(walk)] = torch.tensor(walk)
        absent = [w for w in range(4 + b, VT) if w not in src[b, :n_b].tolist()][:mid - 1]
        out[b, 1, 1:mid] = torch.tensor(absent)
        out[b, 1, mid] = EOS
        out[b, 2, 1] = EOS
        coll = [VT + c for c in range(2, e2t.shape[1]) if int(e2t[b, c]) >= 0]
        out[b, 3, 1:mid] = torch.tensor((coll + own + absent)[:mid - 1])
        out[b, 3, mid] = EOS
        out[b, 3, mid + 1:] = torch.tensor((own * TL)[:TL - mid - 1])
        out[b, 3, TL - 1] = EOS
    return out


# ------------------------------------------------------------------ a generator-level case with every target class planted
CLASSES = ("pad", "pad_word_via_slot", "word_no_mass", "word_one_slot_two_positions", "word_two_slots", "slot", "collapsed_slot", "slot0", "slot1",
           "slot_without_position", "past_the_end", "negative")


def planted(rows, rows_per_src, K, VT, CV, QL, seed=0, length="full", switch=0.0, dominant=False):
    """One vocabulary-wide row set for nir_acg_score_gen_target with every target class its shape can hold, cycling over the rows ->
    dict(o, gen_w, gen_b, copy_w, copy_b, attn, lens, smap, e2t, target, rows_per_src, classes [R] (index into CLASSES), n_inf).
    length 'full': every source row is QL long; 'one': length 1; 'mixed': every third source row has length 1.  Behind the length the map points at the slots the
    targets use and the attention holds 7.0: a kernel that reads there is off by whole units.  Slot CV - 1 has no position (log 0).
    switch: the copy switch's logit (0, +40, -40: a saturated switch keeps its small side).  dominant: the bias of word VT - 1 is lifted by
    80, with targets on it and below it."""
    g = torch.Generator().manual_seed(4000 + seed)
    nsrc = rows // rows_per_src
    assert nsrc * rows_per_src == rows and VT >= 5 and CV >= 2 and QL >= 1
    o = gemm_ref.family("randn", g, rows, K, "a")
    gen_w = gemm_ref.family("randn", g, VT, K, "w")
    gen_b = torch.randn(VT, generator=g)
    w_none, w_one, w_two = 1, VT - 2, VT - 1
    if dominant:
        gen_b[w_two] += 80.0
    copy_w = 1e-3 * torch.randn(K, generator=g)
    copy_b = torch.tensor([float(switch)])
    lens = torch.full((nsrc,), QL, dtype=torch.long)
    if length == "one":
        lens[:] = 1
    elif length == "mixed":
        lens[2::3] = 1
    free = max(1, CV - 1)                                                           # slot CV - 1 takes no position
    smap = torch.randint(0, free, (nsrc, QL), generator=g)
    e2t = torch.full((nsrc, CV), -1, dtype=torch.long)
    if CV > 2:
        e2t[:, 2] = 0                                                               # a slot that collapses onto PAD's id
    if CV > 4:
        e2t[:, 3] = e2t[:, 4] = w_two
    if CV > 5:
        e2t[:, 5] = w_one
    for c in range(7, CV - 1):                                                      # slot 6 stays un-collapsed; further ones: words 2 .. VT - 3, never w_none
        if c % 3 and VT > 5:
            e2t[:, c] = 2 + (c % (VT - 4))
    for b in range(nsrc):
        n = int(lens[b])
        plan = [5, 5, 3, 4, 2, 6][:n]
        for j, c in enumerate(plan):                                                # rotated per source row: a wrong source row shows
            if c < free:
                smap[b, (j + b) % n] = c
    behind = torch.arange(QL).unsqueeze(0) >= lens.repeat_interleave(rows_per_src).unsqueeze(1)
    attn = torch.softmax(torch.randn(rows, QL, generator=g).masked_fill(behind, NEG), 1)
    attn[behind] = 7.0
    for b in range(nsrc):                                                           # poison behind the length: the slots the targets use
        n = int(lens[b])
        smap[b, n:] = torch.tensor([(5, 3, 2, 6, 0, 1)[j % 6] % CV for j in range(QL - n)], dtype=torch.long)
    ids = {"pad": PAD, "pad_word_via_slot": VT + 2 if CV > 2 else None, "word_no_mass": w_none, "word_one_slot_two_positions": w_one if CV > 5 else None,
           "word_two_slots": w_two, "slot": VT + 6 if CV > 7 else None, "collapsed_slot": VT + 5 if CV > 5 else None, "slot0": VT, "slot1": VT + 1,
           "slot_without_position": VT + CV - 1, "past_the_end": VT + CV, "negative": -1}
    have = [k for k in CLASSES if ids[k] is not None]
    cls = torch.tensor([CLASSES.index(have[r % len(have)]) for r in range(rows)])
    target = torch.tensor([ids[have[r % len(have)]] for r in range(rows)], dtype=torch.long)
    last_collapses = CV > 2 and int(e2t[0, CV - 1]) >= 0                            # (it never does: the loops above stop in front of it)
    assert not last_collapses
    held = torch.zeros(nsrc, CV, dtype=torch.bool)                                  # slots with a position in front of the length
    front = torch.arange(QL).unsqueeze(0) < lens.unsqueeze(1)
    held[torch.arange(nsrc).unsqueeze(1).expand(-1, QL)[front], smap[front]] = True
    b, c = torch.arange(rows) // rows_per_src, (target - VT).clamp(0, CV - 1)
    is_slot = (target >= VT) & (target < VT + CV) & ~((c >= 2) & (e2t[b, c] >= 0))
    n_inf = int((is_slot & ~held[b, c]).sum())                                      # un-collapsed slots without a position: log 0
    return dict(o=o, gen_w=gen_w, gen_b=gen_b, copy_w=copy_w, copy_b=copy_b, attn=attn, lens=lens, smap=smap, e2t=e2t, target=target,
                rows_per_src=rows_per_src, classes=cls, n_inf=n_inf)


def planted_ref(c, dtype=torch.float64, fault=None, keep=None):
    """the restatement of a planted case, on the rows `keep` where given"""
    k = slice(None) if keep is None else keep
    return gen_target(c["o"][k], c["gen_w"], c["gen_b"], c["copy_w"], c["copy_b"], c["attn"][k], c["lens"], c["smap"], c["e2t"], c["target"][k],
                      c["rows_per_src"], PAD, dtype, fault, row_ids=keep)
