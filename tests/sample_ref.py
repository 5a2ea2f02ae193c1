"""The acceptance criterion of the sampling decode (csrc/sample.hip, include/neuroir_sample.h; Seq2seq / Seq2seqGRU .decode_sample): the noise
restated exactly in numpy (Philox4x32-10 in uint64 arithmetic), the Gumbel in float64 from the same word, and the sampler in float64 (the
reference) and float32 (the yardstick of what fp32 arithmetic costs) on top of seq2seq_ref / gru_dec_ref through beam_ref.model_step.  The
reference project has no sampler; the semantics are this project's (the head of include/neuroir_sample.h):

    rows      R = B N, row r = n B + b (the beam's layout); the banks are not repeated
    noise     Philox4x32-10, key = (seed & 0xffffffff, seed >> 32), counter = (v >> 2, b, t, n), word v & 3 belongs to v;
              u = ((word >> 9) + 0.5) 2^-23;  g = -log(-log u)
    choice    token = argmax_v fma(y_v, 1 / tau, g_v), ties to the smaller v; top_k = K: over the K largest y (descending, the smaller index
              first among equals) with the same noise keyed by v
    logp      y_token - lse(y): at tau = 1 over the full vocabulary, whatever tau and top_k are
    freeze    behind EOS (3) a row emits EOS at log-probability 0; scores = the sum in step order; lengths = first EOS + 1, else max_len
    feedback  tgt2src[token], <unk> (1) outside the source vocabulary

Bounds.  E_G bounds |g_device - g64|: the house rule on the measured maximum (doubled, rounded up to a power of two), under the DERIVED
condition E_G <= 2^-17 -- four fp32 ulps at the largest value the noise takes (16.6, ulp 2^-19); a noise built on a fast-math log does not
meet it.  With E_y the per-logit bound of score_ref's form (s (MARGIN max(e_chain, 2^-23) + n_split FMT), n_split = 1 fused, 0 plain), the
perturbed value fma(y, 1 / tau, g) of the device lies within E_p = E_y / tau + E_G (+ an fp32 rounding of the sum, 2^-24 |p|) of the float64
one, so the device token must be the float64 token wherever the float64 top-two gap exceeds 2 E_p, and one of the candidates within 2 E_p of
the best elsewhere.  Model level: tokens and lengths exactly (the fixtures keep every step's float64 gap above MIN_GAP, checked on the CPU
against 10 x the bound: tests/test_sample_host.py), scores / token_logprobs by beam_ref's form (n_split = 2 max_len fast, 0 plain),
attentions by seq2seq_ref.accept.

`fault` plants one of seven mistakes (tests/test_sample_host.py shows on the CPU that the criteria reject each):
    "no_noise"            g = 0: the greedy token
    "tau_ignored"         the choice perturbs y, not y / tau
    "row_shared_noise"    every row draws with the counter of (b, n) = (0, 0)
    "step_shared_noise"   every step draws with the counter of t = 0
    "raw_logit_logp"      logp = y_token (no - lse)
    "eos_grows"           rows go on sampling behind EOS
    "noise_on_topk_rank"  the top-k form keys the noise by the rank j, not by the vocabulary id
"""
import math

import numpy as np
import torch

import beam_ref
import gemm_ref
import score_ref

EOS, BOS, UNK = 3, 2, 1
FAULTS = ("no_noise", "tau_ignored", "row_shared_noise", "step_shared_noise", "raw_logit_logp", "eos_grows", "noise_on_topk_rank")
E_G_CAP = 2.0 ** -17                   # derived: four fp32 ulps at g = 16.6
E_G = 2.0 ** -18                       # the house rule on the measured maximum 2^-19.03; asserted <= E_G_CAP by the tests
MIN_GAP = 1e-3                         # the model fixtures: every step's float64 top-two gap of the perturbed values (beam_ref.MIN_GAP's role)
CHI2_THRESHOLD = 92.0                  # the 1 - 1e-6 quantile of chi-square at 36 degrees of freedom (Wilson-Hilferty)
MASK32 = np.uint64(0xFFFFFFFF)
M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)


# ------------------------------------------------------------------ the noise
def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (broadcastable leading shapes), any integer dtype holding 32-bit words -> uint32 [..., 4]"""
    c = [np.asarray(counter[..., i], dtype=np.uint64) & MASK32 for i in range(4)]
    k = [np.asarray(key[..., i], dtype=np.uint64) & MASK32 for i in range(2)]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]                                             # < 2^64: exact
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK32]
        k = [(k[0] + W0) & MASK32, (k[1] + W1) & MASK32]
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def wilson_hilferty(df, z):
    return df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3


def words(seed, step, nsrc, rows, VT, ids=None, fault=None):
    """the Philox word of every (row, v): uint32 [rows, VT]; ids [rows, W]: of these vocabulary ids alone -> [rows, W]"""
    seed = int(seed)
    key = np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64)
    r = np.arange(rows, dtype=np.uint64)
    b, n = r % np.uint64(nsrc), r // np.uint64(nsrc)
    if fault == "row_shared_noise":
        b, n = b * np.uint64(0), n * np.uint64(0)
    t = np.uint64(0 if fault == "step_shared_noise" else step)
    if ids is None:
        nq = (VT + 3) // 4
        ctr = np.zeros((rows, nq, 4), dtype=np.uint64)
        ctr[..., 0] = np.arange(nq, dtype=np.uint64)[None, :]
        ctr[..., 1], ctr[..., 2], ctr[..., 3] = b[:, None], t, n[:, None]
        return philox4x32_10(ctr, key).reshape(rows, nq * 4)[:, :VT]
    ids = np.asarray(ids).astype(np.uint64)
    ctr = np.zeros(ids.shape + (4,), dtype=np.uint64)
    ctr[..., 0] = ids >> np.uint64(2)
    ctr[..., 1], ctr[..., 2], ctr[..., 3] = b[:, None], t, n[:, None]
    out = philox4x32_10(ctr, key)
    return np.take_along_axis(out, (ids & np.uint64(3)).astype(np.int64)[..., None], -1)[..., 0]


def uniform(wd):
    """float64 (exact): u = ((word >> 9) + 0.5) 2^-23"""
    return ((np.asarray(wd, dtype=np.uint32) >> np.uint32(9)).astype(np.float64) + 0.5) * 2.0 ** -23


def gumbel(wd):
    """float64: g = -log(-log u)"""
    return -np.log(-np.log(uniform(wd)))


def gumbel_fast32(wd):
    """what a fast-math evaluation does -- -log(u) as an fp32 log2 of absolute accuracy times ln 2: the form E_G_CAP must reject"""
    u = uniform(wd).astype(np.float32)
    l2 = np.log2(u.astype(np.float64))
    l2 = (np.round(l2 * 2.0 ** 23) / 2.0 ** 23).astype(np.float32)                # an fp32 result with an absolute error of half an ulp of 1
    w = np.maximum(-(l2 * np.float32(math.log(2))), np.float32(2.0 ** -126))
    return -np.log(w.astype(np.float64))


# ------------------------------------------------------------------ one step
def _fma(y, inv_tau, g, dtype):
    """fma(y, 1 / tau, g): float64 as it is; float32: the fp32 operands, one rounding"""
    if dtype == torch.float64:
        return y * inv_tau + g
    it = float(np.float32(inv_tau))
    return (y.float().double() * it + g.float().double()).float()


def topk_lists(logits, K):
    """nir_beam_gen_topk's order: descending, the smaller index first among equals -> (values, indices) [R, K]"""
    val, idx = torch.sort(logits, dim=1, descending=True, stable=True)
    return val[:, :K], idx[:, :K]


def choose(logits, seed, step, nsrc, inv_tau, top_k=0, fault=None, dtype=torch.float64):
    """logits [R, VT] -> dict(token [R], y [R] (the token's logit), lse [R], p [R, C] (the perturbed values of the C candidates), ids [R, C],
    gap [R] (best - second best perturbed value; inf with one candidate))"""
    R, VT = logits.shape
    logits = logits.to(dtype)
    if top_k > 0:
        val, ids = topk_lists(logits, top_k)
        if fault == "noise_on_topk_rank":
            wd = words(seed, step, nsrc, R, VT, np.broadcast_to(np.arange(top_k), (R, top_k)), fault)
        else:
            wd = words(seed, step, nsrc, R, VT, ids.numpy(), fault)
    else:
        val, ids = logits, torch.arange(VT).unsqueeze(0).expand(R, VT)
        wd = words(seed, step, nsrc, R, VT, None, fault)
    g = torch.from_numpy(gumbel(wd))
    if fault == "no_noise":
        g = torch.zeros_like(g)
    p = _fma(val, 1.0 if fault == "tau_ignored" else inv_tau, g, dtype)
    # the best perturbed value, the smaller id among equals
    best = p.max(1, keepdim=True)[0]
    cand = torch.where(p == best, ids, torch.full_like(ids, 1 << 40))
    tok = cand.min(1)[0]
    pos = (ids == tok.unsqueeze(1)).long().argmax(1)
    y = val.gather(1, pos.unsqueeze(1)).squeeze(1)
    srt = torch.sort(p.double(), dim=1, descending=True)[0]
    gap = srt[:, 0] - srt[:, 1] if p.shape[1] > 1 else torch.full((R,), float("inf"), dtype=torch.float64)
    return dict(token=tok, y=y, lse=torch.logsumexp(logits, 1), p=p, ids=ids, gap=gap)


# ------------------------------------------------------------------ the decode
@torch.no_grad()
def sample(step_fn, state0, B, N, max_len, seed, inv_tau=1.0, top_k=0, lut=None, V=None, fault=None, force=None, dtype=torch.float64, bos=BOS):
    """step_fn(state, tok [R]) -> (state', logits [R, VT], aux [R, A]) (beam_ref.search's).  force [max_len, R]: the tokens are these (row order
    n B + b) instead of the sampler's own -- log-probabilities still the chain's.
    -> dict(predictions [B, N, max_len], token_logprobs, scores [B, N], lengths, aux [B, N, max_len, A], tokens [max_len, R] (the raw choices,
    EOS where frozen), gaps [max_len, R] (inf where frozen), s: max |logit|)"""
    state = beam_ref.repeat_state(state0, N)
    R = B * N
    tok = torch.full((R,), bos, dtype=torch.long)
    fin = torch.zeros(R, dtype=torch.bool)
    cum = torch.zeros(R, dtype=dtype)
    length = torch.full((R,), max_len, dtype=torch.long)
    toks, lps, auxs, gaps, s = [], [], [], [], 0.0
    for t in range(max_len):
        state, logits, aux = step_fn(state, tok)
        VT = logits.shape[1]
        s = max(s, float(logits.abs().max()))
        c = choose(logits, seed, t, B, inv_tau, top_k, fault, dtype)
        v = c["token"] if force is None else force[t].long()
        y = logits.to(dtype).gather(1, v.unsqueeze(1)).squeeze(1)
        lp = y if fault == "raw_logit_logp" else y - c["lse"]
        gap = c["gap"]
        if fault != "eos_grows":
            v = torch.where(fin, torch.full_like(v, EOS), v)
            lp = torch.where(fin, torch.zeros_like(lp), lp)
            gap = torch.where(fin, torch.full_like(gap, float("inf")), gap)
        cum = cum + lp
        newly = (v == EOS) & ~fin
        length = torch.where(newly, torch.full_like(length, t + 1), length)
        if fault != "eos_grows":
            fin = fin | newly
        nxt = lut[v] if lut is not None else v
        tok = torch.where((nxt >= 0) & (nxt < (V if V is not None else VT)), nxt, torch.ones_like(nxt))
        toks.append(v)
        lps.append(lp)
        auxs.append(aux)
        gaps.append(gap)
    def out(x):                                                                    # [max_len, R, ...] -> [B, N, max_len, ...]
        x = torch.stack(x)
        return x.view((max_len, N, B) + tuple(x.shape[2:])).permute(2, 1, 0, *range(3, x.dim() + 1)).contiguous()
    return dict(predictions=out(toks), token_logprobs=out(lps), scores=cum.view(N, B).t().contiguous(), lengths=length.view(N, B).t().contiguous(),
                aux=out(auxs), tokens=torch.stack(toks), gaps=torch.stack(gaps), s=s)


def decode(sd, cfg, cell, src, lens, max_len, N, seed, tau=1.0, top_k=0, lut=None, dtype=torch.float64, fault=None, force=None):
    """sampling decode of a fixture network -> sample()'s dict with `attentions` for aux"""
    state0, step, V = beam_ref.model_step(sd, cfg, cell, src, lens, dtype)
    out = sample(step, state0, src.shape[0], N, max_len, seed, 1.0 / tau, top_k, lut, V, fault, force, dtype)
    out["attentions"] = out.pop("aux")
    return out


# ------------------------------------------------------------------ the bounds
def logit_bound(logits64, logits32, n_split):
    """E_y: score_ref's per-logit bound (absolute)"""
    s = float(logits64.abs().max())
    e_chain = float((logits32.double() - logits64).abs().max()) / s
    return s * (score_ref.MARGIN * max(e_chain, score_ref.EPS) + n_split * score_ref.FMT)


def perturbed_bound(e_y, inv_tau, p_abs_max):
    """E_p: what the device's perturbed value may differ from the float64 one by"""
    return e_y * inv_tau + E_G + 2.0 ** -23 * p_abs_max


def accept_tokens(got, ref, e_p):
    """got [R] against choose()'s float64 dict: the float64 token wherever its gap exceeds 2 e_p; elsewhere one of the candidates within 2 e_p of
    the best -> (ok, number of near-tie rows)"""
    got = torch.as_tensor(np.asarray(got.cpu() if torch.is_tensor(got) else got)).long()
    near = ref["gap"] <= 2 * e_p
    ok = bool(torch.equal(got[~near], ref["token"][~near]))
    best = ref["p"].max(1, keepdim=True)[0]
    for r in torch.nonzero(near).flatten().tolist():
        allowed = ref["ids"][r][ref["p"][r] >= best[r] - 2 * e_p]
        ok = ok and bool((allowed == got[r]).any())
    return ok, int(near.sum())


def accept_decode(got, ref, chain, n_split, margin=None):
    """tokens and lengths exactly the float64 restatement's; scores, token_logprobs and attentions inside their bounds"""
    cpu = lambda x: torch.as_tensor(np.asarray(x.cpu() if torch.is_tensor(x) else x))      # noqa: E731
    same = bool(torch.equal(cpu(got["predictions"]).long(), ref["predictions"])) and bool(torch.equal(cpu(got["lengths"]).long(), ref["lengths"]))
    ok_s, fs = beam_ref.accept_scores(got["scores"], ref["scores"], chain["scores"], n_split, margin)
    # a token's log-probability is judged at the scale of the scores' criterion: one step's share of the split products
    ok_t, ft = beam_ref.accept_scores(got["token_logprobs"], ref["token_logprobs"], chain["token_logprobs"], n_split, margin)
    ok_a, fa = beam_ref.S.accept(got["attentions"], ref["attentions"], chain["attentions"], n_split // 2, margin)
    return same and ok_s and ok_t and ok_a, dict(same=same, scores=fs, token_logprobs=ft, attentions=fa)


def score_bound_abs(fig):
    return fig["bound"] * fig["s"]


def model_token_bound(ref, chain, n_split, tau):
    """the model-level token bound 2 (E_y / tau + E_G): E_y = s (MARGIN max(e_chain, 2^-23) + n_split FMT) with s the largest |logit| of the
    float64 decode and e_chain the float32 chain's error of a token log-probability (forced along the float64 tokens) at that scale -- the
    chain's logit error as far as the decode shows it.  The fixtures keep every step's float64 gap above 10 x this."""
    s = ref["s"]
    e_chain = float((chain["token_logprobs"].double() - ref["token_logprobs"]).abs().max()) / s
    e_y = s * (beam_ref.MARGIN * max(e_chain, beam_ref.EPS) + n_split * gemm_ref.FMT["fp16x2"])
    return 2 * (e_y / tau + E_G)


# ------------------------------------------------------------------ the statistical criterion
def chi_square(tokens, probs):
    """Pearson's statistic of the token counts against the expected probabilities [VT] (float64)"""
    tokens = np.asarray(tokens).astype(np.int64)
    probs = np.asarray(probs, dtype=np.float64)
    n = tokens.size
    counts = np.bincount(tokens, minlength=probs.size).astype(np.float64)
    return float((((counts - n * probs) ** 2) / (n * probs)).sum())


Z_1E6 = 4.753424                                                                    # the standard normal's 1 - 1e-6 quantile


def chi_square_pooled(tokens, probs, min_expected=5.0):
    """Pearson's statistic with the cells that expect fewer than `min_expected` draws pooled into one (a chi-square with expected counts
    below one is badly approximated by its nominal distribution) -> (statistic, degrees of freedom, threshold: the 1 - 1e-6 quantile at that
    many degrees of freedom by Wilson-Hilferty)"""
    tokens = np.asarray(tokens).astype(np.int64)
    probs = np.asarray(probs, dtype=np.float64)
    n = tokens.size
    counts = np.bincount(tokens, minlength=probs.size).astype(np.float64)
    rare = n * probs < min_expected
    if rare.any():
        counts, probs = np.append(counts[~rare], counts[rare].sum()), np.append(probs[~rare], probs[rare].sum())
    df = probs.size - 1
    return float((((counts - n * probs) ** 2) / (n * probs)).sum()), df, wilson_hilferty(df, Z_1E6)


def stat_problem(rows=16384, K=32, VT=37, seed=0):
    """the statistical case: `rows` identical rows x, logits about 1.5 randn -> (x [rows, K], w [VT, K], b [VT])"""
    g = torch.Generator().manual_seed(4000 + seed)
    x = torch.randn(1, K, generator=g)
    w = torch.randn(VT, K, generator=g) / math.sqrt(K) * 1.06
    b = 1.06 * torch.randn(VT, generator=g)
    return x.expand(rows, K).contiguous(), w, b


# ------------------------------------------------------------------ the fixtures
CASES = beam_ref.CASES                                                              # the five Seq2seq fixtures and the two GRU ones
N = 4
SETTINGS = ((1.0, 0), (0.7, 0), (1.0, 3), (0.7, 3))                                 # (tau, top_k)
# the seeds of the model-level GPU tests, searched on the CPU: every step's float64 gap >= 10 x the token bound and >= MIN_GAP in all four
# settings, the free-running float32 sampler draws the float64 tokens (tests/test_sample_host.py asserts both)
SEEDS = {"s2s_general": 1, "s2s_dot": 2, "s2s_mlp": 1, "s2s_uni": 1, "s2s_wide": 1, "gru_general": 1, "gru_mlp": 2}
OTHER_SEED = 1000                                                                   # added to a case's seed: another draw
# the seeds of the samples at (tau 0.7, top_k 0) that are handed to score_candidates, one per fixture, searched on the CPU like SEEDS with one
# more condition: no sample holds PAD (0), whose position score_candidates does not count (tests/test_sample_host.py asserts all of it).  The
# PAD case itself is checked with PAD_CASE: a fixture and seed whose samples do hold PAD in front of their first EOS.
SCORE_SEEDS = {"s2s_general": 2, "s2s_dot": 2, "s2s_mlp": 1, "s2s_uni": 2, "s2s_wide": 2, "gru_general": 2, "gru_mlp": 2}
PAD_CASE = ("s2s", "general", 1)


def case(kind, tag):
    """the beam fixture of width 4 (the greedy fixture with a noisy generator bias and a lift on EOS)"""
    return beam_ref.case(kind, tag, 4)


def appended_batch(lens):
    """(keep, more): the fixture batch without its shortest row, and the same with that row appended behind -- torch.sort(lengths,
    descending) pairs the rows of `keep` as before (the lengths are distinct), so only the (b, n) keying decides whether their samples move"""
    assert len(set(lens.tolist())) == lens.numel()
    short = int(lens.argmin())
    keep = torch.tensor([i for i in range(lens.numel()) if i != short])
    more = torch.cat((keep, torch.tensor([short])))
    o1, o2 = torch.sort(lens[keep], 0, True)[1], torch.sort(lens[more], 0, True)[1]
    assert torch.equal(o2[:-1], o1) and int(o2[-1]) == keep.numel()
    return keep, more


# ------------------------------------------------------------------ the generator-level cases (nir_sample_gen driven directly)
# (rows, K, VT, tau, bias, nsrc): rows at the row-tile and row-block edges, K at one k-step, the clamped chunk (288), the NBT switch (512 | 544),
# the largest and a plain-only one (48), VT from one tile with idle waves to several vocabulary ranges, the three temperatures, the bias
# ascending, descending, random, or with one logit dominant by +80 (the noise stays below 16.7: that token comes out at every tau <= 4).
GEN_CASES = [(1, 32, 5, 1.0, "rand", 1), (15, 288, 16, 0.25, "asc", 3), (16, 512, 17, 4.0, "desc", 1), (17, 544, 37, 1.0, "dom", 17),
             (63, 1024, 4099, 0.25, "rand", 3), (64, 48, 37, 1.0, "asc", 1), (65, 32, 4099, 4.0, "desc", 5), (129, 512, 4099, 1.0, "dom", 3),
             (129, 1024, 17, 0.25, "asc", 1), (64, 544, 5, 4.0, "dom", 64), (16, 288, 4099, 1.0, "rand", 1), (65, 48, 4099, 0.25, "dom", 13),
             (129, 512, 37, 4.0, "rand", 43), (17, 1024, 16, 1.0, "desc", 1)]
GEN_SEEDS = [100 + i for i in range(len(GEN_CASES))]
GEN_STEPS = [0, 1, 5, 1 << 20, 2, 3, 7, 19, 4, 6, 8, 9, 10, 11]


def gen_problem(ci):
    """-> (x [rows, K], w [VT, K], b [VT], dom: the dominant index or None)"""
    rows, K, VT, tau, bias, nsrc = GEN_CASES[ci]
    g = torch.Generator().manual_seed(rows * 31 + K * 7 + VT + ci)
    x, w = gemm_ref.family("randn", g, rows, K, "a"), gemm_ref.family("randn", g, VT, K, "w")
    if bias == "asc":
        b = torch.arange(VT).float() / 4
    elif bias == "desc":
        b = -torch.arange(VT).float() / 4
    else:
        b = torch.randn(VT, generator=g)
    dom = None
    if bias == "dom":
        dom = (VT * 2) // 3
        x, b = x * 0.05, torch.zeros(VT)                                            # the other logits within +-0.5: 80 / 4 - 2.8 > 0.5 / 4 + 16.7
        b[dom] = 80
    return x, w, b, dom


def gen_reference(ci, n_split):
    """the float64 choice of a generator-level case and the bounds of a form -> dict(ref: choose()'s, e_y, e_p, logits64, logits32)"""
    rows, K, VT, tau, bias, nsrc = GEN_CASES[ci]
    x, w, b, dom = gen_problem(ci)
    l64 = x.double() @ w.double().t() + b.double()
    l32 = x @ w.t() + b
    ref = choose(l64, GEN_SEEDS[ci], GEN_STEPS[ci], nsrc, 1.0 / tau)
    e_y = logit_bound(l64, l32, n_split)
    return dict(ref=ref, e_y=e_y, e_p=perturbed_bound(e_y, 1.0 / tau, float(ref["p"].abs().max())), logits64=l64, logits32=l32, dom=dom)
