"""The acceptance criterion of CARS attention pooling (nir_attn_pool_f32; csrc/cars.hip, csrc/cars_attn.hip): a float64 reference of
the whole operation on the operands as each kernel form receives them, numpy encoders / decoders of the row formats, seeded input
families, the bound a result has to meet and a numpy emulation of the kernel forms with single faults (tests/test_attn_criterion_host.py
shows on the CPU that the bound accepts the honest forms and rejects every fault).

Operation:  z = W0 h + b0;  logit_t = w3 . tanh(z_t) + b3;  p = softmax over t < clamp(len, 0, T);  pooled = sum_t p_t h_t;  len = 0 gives a
NaN row.

Forms (FORMS below) and the operands their reference sees:
    f32    the plain chain (fp32 GEMM, row-dot, attn_pool_kernel): rows and W0 as given.
    bf3    gemm3_kernel (three bf16 terms) + attn_pool2_kernel: as given.
    x2     two fp16 terms of rows and W0, the weighted sum over the fp32 rows (attn_pool_fused_kernel; gemm3h_kernel + attn_pool2_kernel): as given.
    pipe0  attn_pool_pipe_kernel<false,0>: as x2, but the weighted sum reads the rows back from their two term planes.
    pipe2  <false,2>: the rows ARE term pairs (the test encodes them, the reference decodes exactly those); W0 as given.
    row1   <false,1>: the rows ARE fp16 (decoded exactly); W0 as given.
    one0   <true,0>: fp32 rows and W0 each enter as ONE fp16 term, rounded toward zero at that site (split2_hi = v_cvt_pkrtz_f16_f32 in the
           kernel, split2_hi1_rtz in nir_split_f16x2): the reference rounds both the same way, in the GEMM and in the weighted sum (the kernel
           keeps no other copy of a row).
    one1   <true,1>: the rows ARE fp16; W0 is its leading term as above.

Bound (the project's form): with s = max |ref64| over the finite rows, e = max |got - ref64| / s and e32 the same figure for torch's CPU
fp32 chain on the same operands,

    e <= margin * max(e32, 2^-23) + fmt + act          (+ floor / s for the tiny families)

Every term besides margin comes from the formats.  A perturbation of every logit of a sequence by at most d multiplies each unnormalised
weight by a factor in [e^-d, e^d], so each p_t moves by at most (e^2d - 1) p_t and pooled by at most (e^2d - 1) max|h| ~ 2 d max|h|:
SENS(d) = 2 d max|h|.
  fmt   the GEMM result z is off by at most g * max|z| with g the format figure of tests/gemm_ref.py (FMT: 0 for f32, 2^-22 for bf16x3,
        3 * 2^-22 for the fp16 pair: each operand known to 2^-22, the dropped h2' w2' product another 2^-22; where the rows are handed over
        exactly -- pipe2, row1 -- their own 2^-22 is not spent: 2 * 2^-22; one0 / one1: 0, the reference holds the rounded operands).
        |tanh'| <= 1, and column n of z carries its own rounding residuals (row n of W0 against the row's terms): 256 errors of that size
        with independent signs meet in the logit, weighted by w3, so they add in quadrature: d_fmt = g max|z| ||w3||_2.  (The sum of
        magnitudes g max|z| sum|w3| would only be reached by residuals aligned with sign(w3) in every column; it is 13 x larger at 256
        columns and would hide a row carried as one fp16 term in the weighted sum, 2^-12 of pooled, behind the `peaked` family's w3.)
        This is a statistical argument, not a bound: it makes the criterion STRICTER than the worst case.  A failure at a few x fmt on
        an adversarial input (rows of W0 alike, w3 of one sign) would be a failure of this assumption, not of the kernel.
        Where the weighted sum reconstructs a row from its two planes (pipe0) the row is off by 2^-22 max|h| and so is pooled (the p_t sum
        to 1).  fmt = (SENS(d_fmt) + recon) / s.
  act   the kernels' tanh is 1 - 2 / (1 + 2^(2 log2(e) z)) on v_exp_f32 / v_rcp_f32 (fast_tanh in csrc/common.hpp documents ~1e-7
        absolute; twice that is allowed, as in gemm_ref): d_tanh = 2e-7 sum|w3|.  The softmax runs __expf(logit - max) = v_exp_f32 of
        the argument times log2(e), rounded to fp32: a relative error of 2^-24 * |logit - max| <= 2^-24 * 2 max|logit| in the weight, i.e. a
        logit error d_exp = 2^-23 max|logit|.  act = SENS(d_tanh + d_exp) / s.
  floor (tiny, tiny20 on the forms that split fp32 rows: x2, pipe0) the scaled residual of a row below 2^-13 is an fp16 subnormal, the row
        is known to 2^-35 absolute (gemm_ref.subnormal_floor): z moves by 2^-35 max_n sum_k |W0[n,k]|, the logit by that times ||w3||_2, and
        a reconstructed row by 2^-35.
  margin  per form: the largest measured (e - fmt - act) / max(e32, 2^-23) on the MI355X, doubled, rounded up to a power of two, at least 1
        and never above MARGIN_CAP = 4.  e32 is the error of the reference chain, never of the kernel.  Measured (DESIGN.md section 2 has
        the figures per kernel): the ratio is negative for every form but the fused kernel on `uniform` (w3 = 0, so fmt = 0 and act is the
        exp term alone), 0.23 there -> 1 everywhere.  The kernels' own error stays within 2.2 x max(e32, 2^-23) in every case outside
        the tiny families; what the bound leaves above that is the room the documented 1e-7 of the fast tanh takes through sum|w3|.

What pooled cannot show: softmax is shift invariant, so b3 -- and any error that shifts all logits of a sequence alike, a uniform offset
of tanh included -- leaves pooled unchanged.  No test here claims to cover b3."""
import numpy as np
import torch

import gemm_ref as G

EPS = 2.0 ** -23
MARGIN_CAP = 4.0
FORMS = ("f32", "bf3", "x2", "pipe0", "pipe2", "row1", "one0", "one1")
GEMM_FMT = {"f32": 0.0, "bf3": G.FMT["bf16x3"], "x2": G.FMT["fp16x2"], "pipe0": G.FMT["fp16x2"], "pipe2": 2 * 2.0 ** -22, "row1": 2 * 2.0 ** -22,
            "one0": 0.0, "one1": 0.0}
RECON = {"pipe0": 2.0 ** -22}
MARGIN = {f: 1.0 for f in FORMS}
FAMILIES = ("model", "peaked", "saturated", "uniform", "edge", "tiny", "tiny20")
D = 256


# ------------------------------------------------------------------ inputs
def family(name, seed, M, T, d=D):
    """dict(h [M,T,d], W0 [d,d], b0 [d], w3 [d], b3 [1]) of float32 CPU tensors; the rows are uniform in (-1, 1) unless the family says otherwise"""
    g = torch.Generator().manual_seed(seed)
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    h = torch.rand(M, T, d, generator=g, dtype=torch.float64) * 2 - 1
    W0, b0, w3, b3 = randn(d, d) / 16, randn(d) / 16, randn(d) / 16, randn(1)
    if name == "peaked":                                 # logits spread over tens: the softmax is close to one-hot, logit errors show
        w3 = randn(d)
    elif name == "saturated":                            # |z| far past 44 (2^(2 log2(e) z) overflows fp32), a few weights just below 2^15
        # (max|z| ~ 3e4 makes fmt ~ 0.1 of pooled: on this family the criterion asserts little more than a finite result of the right shape,
        # which is what the family is for -- overflow of exp2 in 1 - 2 / (1 + 2^z); the softmax and the weighted sum are pinned by the others)
        W0 = randn(d, d) * 40
        W0[3, 5], W0[100, 200], W0[255, 0] = 32767.0, -32767.5, 32000.0
    elif name == "uniform":
        w3 = torch.zeros(d, dtype=torch.float64)
    elif name == "edge":                                 # whole rows at the end of (-1, 1)
        h = torch.where(h >= 0, 1.0, -1.0) * (1 - 2.0 ** -24)
    elif name == "tiny":
        h = h * 2.0 ** -10
    elif name == "tiny20":
        h = h * 2.0 ** -20
    elif name != "model":
        raise ValueError(name)
    return dict(h=h.float(), W0=W0.float(), b0=b0.float(), w3=w3.float(), b3=b3.float())


def ragged_lens(seed, M, T):
    """seeded lengths in [1, T], not periodic in anything"""
    return torch.randint(1, T + 1, (M,), generator=torch.Generator().manual_seed(seed + 12345))


# ------------------------------------------------------------------ row formats
def encode_f16_rows(h):
    """fp32 [.., d] -> the fp16-row layout as int16 (round to nearest, as a recurrence's (_Float16) store)"""
    return np.ascontiguousarray(np.asarray(h, dtype=np.float32).astype(np.float16)).view(np.int16)


def decode_f16_rows(raw):
    return np.asarray(raw).view(np.float16).astype(np.float64)


def encode_pairs(h):
    """fp32 [.., d] -> the term-pair layout as int16 [.., 2 d]: per row and group of four columns the 4 leading fp16 terms, then the 4
    residual terms fp16(2^11 (x - h1)); both rounded toward zero, as split2() forms them"""
    h1, h2 = G.split_terms(np.asarray(h, dtype=np.float32), "fp16x2")
    lead = h1.astype(np.float16).reshape(h1.shape[:-1] + (-1, 1, 4))
    res = h2.astype(np.float16).reshape(lead.shape)
    return np.ascontiguousarray(np.concatenate([lead, res], -2).reshape(h1.shape[:-1] + (-1,))).view(np.int16)


def decode_pairs(raw):
    v = np.asarray(raw).view(np.float16).astype(np.float64)
    v = v.reshape(v.shape[:-1] + (-1, 2, 4))
    return (v[..., 0, :] + v[..., 1, :] / 2048.0).reshape(v.shape[:-3] + (-1,))


def w0_fragments(W0):
    """W0 [256, 256] fp32 on the GPU -> the fragment-ordered planes multitask/cars.py packs for the fused kernels"""
    from context_attentive_ir_amd import lib
    planes = torch.stack(lib.split_f16x2(W0, 256))
    return planes.view(2, 16, 16, 8, 4, 8).permute(3, 1, 0, 4, 2, 5).contiguous()


def _rtz16(x):
    return torch.from_numpy(G._f16_rtz(np.ascontiguousarray(x.numpy(), dtype=np.float32)).astype(np.float64))


def operands(form, h, W0):
    """(rows, W0) in float64 as the reference of `form` sees them.  h: fp32 tensor, or for pipe2 / row1 / one1 the int16 array handed to the kernel"""
    if form == "pipe2":
        rows = torch.from_numpy(decode_pairs(h))
    elif form in ("row1", "one1"):
        rows = torch.from_numpy(decode_f16_rows(h))
    elif form == "one0":
        rows = _rtz16(h)
    else:
        rows = h.double()
    return rows, (_rtz16(W0) if form in ("one0", "one1") else W0.double())


# ------------------------------------------------------------------ reference
def clamp_lens(lens, M, T):
    return torch.full((M,), T, dtype=torch.int64) if lens is None else lens.clamp(0, T)


def _pool(rows, W0, b0, w3, b3, lens, dt, parts=False):
    M, T, d = rows.shape
    rows, W0 = rows.to(dt), W0.to(dt)
    z = rows.reshape(M * T, d) @ W0.t() + b0.to(dt)
    lg = (torch.tanh(z) @ w3.to(dt) + b3.to(dt)).reshape(M, T)
    mask = torch.arange(T)[None, :] < clamp_lens(lens, M, T)[:, None]
    p = torch.softmax(lg.masked_fill(~mask, float("-inf")), -1)
    out = (p[:, :, None] * rows).sum(1)
    return (out, z, lg, mask) if parts else out


def ref64(rows, W0, b0, w3, b3, lens):
    """pooled [M, d] in float64; rows [M, T, d], W0 [d, d] float64 (operands()); a row of length 0 is NaN"""
    return _pool(rows, W0, b0, w3, b3, lens, torch.float64)


def measure(got, form, rows, W0, b0, w3, b3, lens, floor=False):
    """dict(e, e32, s, fmt, act, floor, ratio); NaN rows of the reference (length 0) must be NaN rows of got and are left out of e"""
    ref, z, lg, mask = _pool(rows, W0, b0, w3, b3, lens, torch.float64, parts=True)
    got = torch.as_tensor(np.asarray(got)) if not torch.is_tensor(got) else got.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    dead = torch.isnan(ref).all(1)
    assert bool((torch.isnan(ref).any(1) == dead).all())
    assert bool(torch.isnan(got[dead]).all()), "a length-0 row is not all NaN"
    live = ~dead
    ref, got = ref[live], got[live].double()
    assert bool(torch.isfinite(got).all()), "non-finite output"
    s = float(ref.abs().max())
    assert s > 0
    hmax = float(rows.abs().max())
    sw3 = float(w3.double().abs().sum())
    w3rss = float(w3.double().pow(2).sum().sqrt())
    sens = lambda d: 2.0 * d * hmax
    fmt = (sens(GEMM_FMT[form] * float(z.abs().max()) * w3rss) + RECON.get(form, 0.0) * hmax) / s
    lgmax = float(lg[mask].abs().max()) if bool(mask.any()) else 0.0
    act = sens(2e-7 * sw3 + 2.0 ** -23 * lgmax) / s
    fl = 0.0
    if floor:
        assert form in ("x2", "pipe0")
        fl = (sens(2.0 ** -35 * float(W0.abs().sum(1).max()) * w3rss) + (2.0 ** -35 if form == "pipe0" else 0.0)) / s
    e = float((got - ref).abs().max()) / s
    e32 = float((_pool(rows, W0, b0, w3, b3, lens, torch.float32)[live].double() - ref).abs().max()) / s
    return dict(e=e, e32=e32, s=s, fmt=fmt, act=act, floor=fl, ratio=(e - fmt - act - fl) / max(e32, EPS))


def accept(got, form, rows, W0, b0, w3, b3, lens, margin=None, floor=False):
    """(ok, figures): the criterion of the module docstring.  margin defaults to MARGIN[form] and may never exceed MARGIN_CAP."""
    margin = MARGIN[form] if margin is None else margin
    assert margin <= MARGIN_CAP
    r = measure(got, form, rows, W0, b0, w3, b3, lens, floor)
    r["bound"] = margin * max(r["e32"], EPS) + r["fmt"] + r["act"] + r["floor"]
    return r["e"] <= r["bound"], r


# ------------------------------------------------------------------ emulation of the kernel forms, with single faults
VARIANTS = {"x2": "pipe0", "row1": "row1", "one": "one0"}        # emulated variant -> the form it is judged as
MUTANTS = ("gemm_row1", "sum_row1", "w_res", "no_b0", "mask_long", "mask_short", "len_next", "len_ring", "den_2T", "wave_drop")


def emulate(variant, h, W0, b0, w3, b3, lens, mutant=None):
    """pooled [M, d] float64 as a fused kernel of `variant` forms it, sums in float64 (no fp32 accumulation error), with one fault:
    x2: two-term rows and W0, the h2' w2' product dropped, rows rebuilt from their planes for the weighted sum; row1: the rows are one fp16
    term (h: the int16 fp16 rows); one: rows and W0 one term each.  lens: int64 [M], every length in [1, T] (the faults move them)."""
    M, T, d = h.shape
    if variant == "row1":
        a1, a2 = decode_f16_rows(h), None
    else:
        a1, a2 = (t.astype(np.float64) for t in G.split_terms(h.numpy(), "fp16x2"))
        if variant == "one":
            a2 = None
    w1, w2 = (t.astype(np.float64) for t in G.split_terms(W0.numpy(), "fp16x2"))
    if variant == "one" or mutant == "w_res":
        w2 = None
    a1f = a1.reshape(M * T, d)
    z = a1f @ w1.T
    if a2 is not None and mutant != "gemm_row1":
        z = z + (a2.reshape(M * T, d) @ w1.T) / 2048.0
    if w2 is not None:
        z = z + (a1f @ w2.T) / 2048.0
    if mutant != "no_b0":
        z = z + b0.double().numpy()
    part = (np.tanh(z) * w3.double().numpy()).reshape(M * T, 4, d // 4).sum(-1)       # the four waves' partial logits
    if mutant == "wave_drop":
        part[:, 2] = 0.0
    lg = part.sum(-1).reshape(M, T) + float(b3)
    ln = lens.numpy().copy()
    if mutant == "mask_long":
        ln = np.minimum(ln + 1, T)
    elif mutant == "mask_short":
        ln = np.maximum(ln - 1, 1)
    elif mutant == "len_next":
        ln = np.roll(ln, -1)
    elif mutant == "len_ring":
        ln = np.roll(ln, -max(64 // T, 1))
    mask = np.arange(T)[None, :] < ln[:, None]
    mx = np.where(mask, lg, -np.inf).max(1, keepdims=True)
    ex = np.where(mask, np.exp(lg - mx), 0.0)
    den = ex.sum(1, keepdims=True)
    if mutant == "den_2T":                               # the group sum one step too wide: a pair of sequences shares its denominator
        den = den + den[np.arange(M) ^ 1 if M % 2 == 0 else np.r_[np.arange(M - 1) ^ 1, M - 1]]
    p = ex / den
    rows = a1 if a2 is None or mutant == "sum_row1" else a1 + a2 / 2048.0
    return torch.from_numpy((p[:, :, None] * rows).sum(1))
