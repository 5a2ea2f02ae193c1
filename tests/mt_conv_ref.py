"""The acceptance criterion of the train-mode MatchTensor convolutions (csrc/mt_conv_train.hip: mt_conv3_fwd_kernel, mt_conv3_pack_wt_kernel,
mt_conv3_bwd_data_kernel, mt_conv3_bwd_weight_kernel) and of the fixed-order column sum that reduces their gradients (nir_colsum_det_f32):
a float64 reference, seeded input families, the bound a result has to meet, the case list shared by the CPU and the GPU test, and a numpy
emulation of the kernels in their own summation order with single faults (tests/test_mt_conv_criterion_host.py shows on the CPU that the
bound accepts the honest emulation and rejects every fault).  The fall-back of the same head (nir_im2col_rows_f32 / nir_col2im_rows_f32)
has its reference and case list at the end.

Operation: T [M, C1 = 51, H, W] fp32, filters w_g [NF = 6, C1, 3, kw_g], kw_g = 3, 5, 7 (g = 0, 1, 2), biases b_g [NF];
    pre_g = conv2d(T, w_g, b_g, padding (1, g + 1));  forward rows out[(m, y, x), g NF + o] = relu(pre_g[m, o, y, x])       [M H W, 3 NF]
The backward entries take dpre [M H W, 3 NF], the gradient of the PRE-activation, so the ReLU mask is not part of what is judged:
    dT = d pre / d T . dpre,  dw_g = d pre / d w_g . dpre,  db_g = column sum of dpre.
Reference: torch.nn.functional.conv2d in float64 and its autograd.  Yardstick e32: the same computation by torch on the CPU in fp32.

Bound, per output tensor (KEYS: the forward rows, dT, dw1..3, db1..3 after the column sum): with s = max |ref64| (1 for an all-zero
reference), e = max |got - ref64| / s and e32 the same figure of the fp32 yardstick,

    e <= margin * max(e32, 2^-23)

No format term and no activation term: everything is fp32 FMA, ReLU is exact.  margin per kernel (KERNEL_OF maps a tensor to its kernel):
the largest measured e / max(e32, 2^-23) on the MI355X over CASES (profiles/mt_conv_criterion_mi355x.log), doubled, rounded up to a power of
two, at least 1 and never above MARGIN_CAP = 4 (the rule of gemm_ref.py).  e32 is the error of the yardstick, never of the kernel.

Inputs.  A non-impulse input goes to the GPU only if the in-order emulation stays within 0.8 of the bound at the cap on every tensor; a
seed that fails is skipped and the first passing seed is recorded in SEEDS -- the bound is not moved.  The `impulse` inputs have results
that are exactly representable (one product per output, or sums of small integers), so they are compared BIT-exactly with the float64
reference rounded to fp32: tap indexing is pinned independent of any tolerance."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS = 2.0 ** -23
MARGIN_CAP = 4.0
C1, NF, NCOL = 51, 6, 18
KW = (3, 5, 7)
TAP0 = (0, 9, 24)
NW = NF * C1 * 45
MT_XS, MT_CG = 2, 17
FWD_CHAINS = 1                                  # accumulators an output of mt_conv3_fwd_kernel is summed in (channel groups added at the end)
KEYS = ("fwd", "dT", "dw1", "dw2", "dw3", "db1", "db2", "db3")
KERNEL_OF = {"fwd": "fwd", "dT": "data", "dw1": "weight", "dw2": "weight", "dw3": "weight", "db1": "bias", "db2": "bias", "db3": "bias"}
KERNELS = ("fwd", "data", "weight", "bias")
# worst e / max(e32, 2^-23) over CASES on the MI355X (profiles/mt_conv_criterion_mi355x.log) -> margin_rule()
MEASURED = {"fwd": 3.059, "data": 3.191, "weight": 1.768, "bias": 1.730}
MARGIN = {"fwd": 4.0, "data": 4.0, "weight": 4.0, "bias": 4.0}      # the rule asks for 8 on fwd and data: the cap holds
MEASURED_COL2IM, MARGIN_COL2IM = 1.000, 2.0      # nir_col2im_rows_f32 (kh kw <= 21 plain additions per output), same rule
FAMILIES = ("randn", "mixed", "tiny", "positive", "dead")
FAULTS = ("a", "b", "c", "d", "e", "f", "g", "h1", "h2", "i1", "i2", "j", "k1", "k2", "l")
FAULT_KERNEL = dict(a="fwd", b="fwd", c="fwd", d="fwd", e="fwd", f="data", g="data", h1="data", h2="data", l="data", i1="weight", i2="weight",
                    j="weight", k1="weight", k2="weight")


def margin_rule(worst):
    """largest measured ratio -> margin: doubled, rounded up to a power of two, at least 1, never above the cap"""
    m = 1.0
    while m < 2.0 * worst:
        m *= 2.0
    return min(m, MARGIN_CAP)


# ------------------------------------------------------------------ kernel geometry (csrc/mt_conv_train.hip)
def data_lds(H, W):
    """dynamic LDS of mt_conv3_bwd_data_kernel: the sample's dpre rows [H W][3 NF + 1]"""
    return H * W * (NCOL + 1) * 4


def weight_lds(H, W, C=C1):
    """dynamic LDS of mt_conv3_bwd_weight_kernel: the sample's tile [C1][H (W + 1) made odd]"""
    return C * ((H * (W + 1)) | 1) * 4


def supported(nf, c1, H, W):
    """nir_mt_conv3_supported restated"""
    return int(nf == 6 and c1 == 51 and H >= 1 and W >= 1 and data_lds(H, W) <= 64 * 1024 and weight_lds(H, W, c1) <= 150 * 1024)


def xchunk(W):
    return (W + MT_XS - 1) // MT_XS


def colsum_slices(R):
    """(rows per slice, slices) of the column sum over R rows (colsum_mslice / colsum_slices of csrc/train.hip)"""
    ms = max(64, (R + 255) // 256)
    return ms, (R + ms - 1) // ms


def colsum_chain_depth(R, N):
    """the longest chain of fp32 additions behind one output of nir_colsum_det_f32: an a priori error bound of the sum is
    gamma * sum |x| with gamma = depth u / (1 - depth u), u = 2^-24 (the standard bound of a summation in which no operand passes through more
    than `depth` roundings)"""
    ms, S = colsum_slices(R)
    first = (ms + 15) // 16 + 16 if N <= 64 else ms
    return first + ((S + 15) // 16 + 16 if S > 1 else 0)


# (M, N, ld) of the direct column-sum test: the bias gradient of the C2 training step (320 rows a slice, 256 slices, lane-wise first pass) behind a
# wider row; a wide matrix with 79 rows a slice in 254 slices (row-order first pass); N = 64 | 65 on both sides of the kernel choice; one slice
COLSUM_CASES = [(81920, 18, 24), (20000, 100, 131), (130, 64, 70), (130, 65, 65), (64, 18, 19), (50, 300, 301)]


# ------------------------------------------------------------------ cases
def c(M, H, W, fam="randn", why=""):
    d = dict(M=M, H=H, W=W, fam=fam, why=why)
    d["id"] = "%s-M%d-H%d-W%d" % (fam, M, H, W)
    return d


SHAPES = [
    # block tails of the forward (256 positions a block)
    (1, 1, 255, "tail"), (1, 1, 256, "tail"), (1, 1, 257, "tail"),
    # every window column clipped on both sides; W = 1, 2: the second column range of the weight gradient is empty
    (1, 1, 1, "clip"), (1, 1, 2, "clip"), (1, 1, 3, "clip"), (2, 1, 7, "clip"), (3, 2, 4, "clip"), (1, 3, 1, "clip"), (2, 5, 6, "clip"),
    (2, 5, 7, "clip"), (2, 5, 8, "clip"),
    # the position loop of the data gradient: one pass exactly, two, three
    (2, 4, 64, "pass"), (1, 257, 1, "pass"), (2, 4, 65, "pass"), (1, 8, 64, "pass"), (1, 3, 171, "pass"),
    # the LDS opt-in of the weight gradient: (5, 63) is the last tile under 64 KB, (1, 321) the first above, (1, 750) the largest accepted
    (2, 5, 63, "lds"), (2, 1, 321, "lds"), (1, 8, 65, "lds"), (2, 10, 74, "lds"), (1, 11, 67, "lds"), (1, 1, 750, "lds"),
    # odd W: the column-range seam in the middle, xchunk rounds up
    (3, 4, 33, "oddW"), (3, 2, 9, "oddW"),
    # column-sum slices of the filter gradient: 2 M = 64 rows (one slice), 66 (two), 194 (four); the bias gradient sums M H W = 320 .. 970 rows
    (32, 2, 5, "slices"), (33, 2, 5, "slices"), (97, 2, 5, "slices"),
    # the workload: the C2 tile (4, 64), and a wide batch
    (40, 4, 16, "work"), (3, 4, 64, "work"), (33, 4, 64, "work"),
]
FAMILY_SHAPES = [(2, 5, 7), (2, 4, 65), (2, 10, 74), (40, 4, 16)]
REFUSED_SHAPES = [(1, 1, 751), (1, 2, 375), (1, 16, 46)]
CASES = [c(M, H, W, "randn", why) for M, H, W, why in SHAPES] + [c(M, H, W, fam, "family") for fam in FAMILIES[1:] for M, H, W in FAMILY_SHAPES]
BY_ID = {d["id"]: d for d in CASES}
assert len(BY_ID) == len(CASES)
# case id -> the first seed on which the in-order emulation stays within 0.8 of the bound at the cap (seed 0 where not listed)
SEEDS = {"randn-M1-H1-W256": 3, "tiny-M40-H4-W16": 2, "positive-M2-H5-W7": 2, "positive-M2-H4-W65": 1}
IMPULSE_SHAPES = [(4, 65), (2, 3), (1, 1), (3, 171)]


# ------------------------------------------------------------------ inputs
def family(d, seed=None):
    """dict of float32 CPU tensors: T [M, C1, H, W], w1..3, b1..3, dpre [M H W, 3 NF]"""
    M, H, W, fam = d["M"], d["H"], d["W"], d["fam"]
    seed = SEEDS.get(d["id"], 0) if seed is None else seed
    g = torch.Generator().manual_seed(100003 * seed + 1009 * M + 31 * H + W + 7 * FAMILIES.index(fam))
    randn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    rand = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    x = dict(T=randn(M, C1, H, W), dpre=randn(M * H * W, NCOL))
    for k in range(3):
        x["w%d" % (k + 1)], x["b%d" % (k + 1)] = randn(NF, C1, 3, KW[k]) * 0.2, randn(NF) * 0.2
    if fam == "mixed":                              # magnitudes 10^U(-3, 2) per channel of T and per filter
        x["T"] = x["T"] * 10.0 ** (rand(1, C1, 1, 1) * 5 - 3)
        for k in (1, 2, 3):
            x["w%d" % k] = x["w%d" % k] * 10.0 ** (rand(NF, 1, 1, 1) * 5 - 3)
    elif fam == "tiny":
        x["T"], x["dpre"] = x["T"] * 2.0 ** -10, x["dpre"] * 2.0 ** -10
        for k in (1, 2, 3):
            x["w%d" % k], x["b%d" % k] = x["w%d" % k] * 2.0 ** -10, x["b%d" % k] * 2.0 ** -20
    elif fam == "positive":                         # no cancellation anywhere: every sum is a sum of positive terms
        x["T"], x["dpre"] = rand(M, C1, H, W) + 0.5, rand(M * H * W, NCOL) + 0.5
        for k in range(3):
            K = C1 * 3 * KW[k]
            x["w%d" % (k + 1)], x["b%d" % (k + 1)] = (rand(NF, C1, 3, KW[k]) + 0.5) / K, (rand(NF) + 0.5) / K
    elif fam == "dead":                             # every ReLU is 0: the forward rows are exactly 0
        for k in (1, 2, 3):
            x["b%d" % k] = -1000.0 - x["b%d" % k].abs()
    elif fam != "randn":
        raise ValueError(fam)
    return {k: v.float().contiguous() for k, v in x.items()}


def impulse_positions(H, W):
    """(y0, x0) of the impulses: the four corners, the centre, both sides of the column-range seam, flat positions 255 and 256"""
    xc = xchunk(W)
    pos = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2), (H // 2, max(xc - 1, 0)), (H // 2, min(xc, W - 1))]
    pos += [(r // W, r % W) for r in (255, 256) if r < H * W]
    return sorted(set(pos))


IMPULSE_CHANNELS = (0, 16, 17, 33, 34, 50)          # both sides of the channel-group seams of MT_CG = 17


def impulse_fwd(H, W):
    """(inputs, list of (m, c, y0, x0)): sample m holds T = 1.0 at one (c, y0, x0), every position x every seam channel; sample 0 and M - 1
    included.  out[(m, y, x), g NF + o] = relu(fl32(w_g[o, c, y0 - y + 1, x0 - x + pw_g] + b_g[o])) inside the window, relu(b_g[o]) outside:
    one rounding, so the float64 reference rounded to fp32 is the exact answer."""
    pos = impulse_positions(H, W)
    where = [(m, IMPULSE_CHANNELS[m % 6], ) + pos[(m // 6) % len(pos)] for m in range(6 * len(pos))]
    x = family(c(len(where), H, W), seed=77)
    x["T"].zero_()
    for m, ch, y0, x0 in where:
        x["T"][m, ch, y0, x0] = 1.0
    return x, where


def impulse_bwd(H, W):
    """(inputs, list of (m, y0, x0, col)): sample m holds dpre = 1.0 at one ((y0, x0), col = g NF + o); T holds small integers.  Then
    dT[m, c, y, x] = w_g[o, c, y - y0 + 1, x - x0 + pw_g] inside the window and 0 elsewhere (one term), the partial row of (m, range of x0)
    holds T[m, c, y0 + dy - 1, x0 + dx - pw_g] (0 outside the tile) and the other range 0, the summed dw is a sum of small integers and db
    counts the impulses of a column: all exactly representable, in any order of summation."""
    pos = impulse_positions(H, W)
    M = 4 * NCOL
    where = [(m, ) + pos[(m + m // NCOL) % len(pos)] + (m % NCOL, ) for m in range(M)]
    x = family(c(M, H, W), seed=78)
    g = torch.Generator().manual_seed(79 + W)
    x["T"] = torch.randint(-8, 9, (M, C1, H, W), generator=g).float()
    x["dpre"].zero_()
    dp = x["dpre"].view(M, H, W, NCOL)
    for m, y0, x0, col in where:
        dp[m, y0, x0, col] = 1.0
    return x, where


# ------------------------------------------------------------------ reference
def _rows(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def chain(x, dt):
    """dict over KEYS of the operation in dtype dt (torch conv2d and its autograd), plus `pre` [M H W, 3 NF]"""
    T = x["T"].to(dt).clone().requires_grad_(True)
    ws = [x["w%d" % k].to(dt).clone().requires_grad_(True) for k in (1, 2, 3)]
    bs = [x["b%d" % k].to(dt).clone().requires_grad_(True) for k in (1, 2, 3)]
    pre = torch.cat([_rows(F.conv2d(T, ws[k], bs[k], padding=(1, k + 1))) for k in range(3)], 1)
    pre.backward(x["dpre"].to(dt))
    out = dict(fwd=torch.relu(pre.detach()), pre=pre.detach(), dT=T.grad)
    for k in range(3):
        out["dw%d" % (k + 1)], out["db%d" % (k + 1)] = ws[k].grad, bs[k].grad
    return out


def err(got, ref):
    """max |got - ref| / max |ref| (1 for an all-zero reference)"""
    got = torch.as_tensor(np.asarray(got)) if not torch.is_tensor(got) else got.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "non-finite result"
    s = float(ref.abs().max())
    return float((got.double() - ref).abs().max()) / (s if s > 0 else 1.0)


def prepare(x):
    """dict(ref = float64 results over KEYS, e32 = the yardstick's error per key)"""
    ref, y32 = chain(x, torch.float64), chain(x, torch.float32)
    return dict(ref=ref, e32={k: err(y32[k], ref[k]) for k in KEYS})


@functools.lru_cache(maxsize=None)
def _prepared(cid):
    x = family(BY_ID[cid])
    return x, prepare(x)


def prepared(d):
    """(inputs, dict(ref, e32)) of a case of CASES, computed once and shared by every test that needs it; treat as read-only"""
    return _prepared(d["id"])


def accept(got, key, p, margin=None):
    """(ok, figures) of tensor `key`: the criterion of the module docstring.  margin defaults to MARGIN of the tensor's kernel and may never
    exceed MARGIN_CAP."""
    margin = MARGIN[KERNEL_OF[key]] if margin is None else margin
    assert margin <= MARGIN_CAP
    e, e32 = err(got, p["ref"][key]), p["e32"][key]
    r = dict(e=e, e32=e32, ratio=e / max(e32, EPS), bound=margin * max(e32, EPS))
    return e <= r["bound"], r


def split_grads(dw, db):
    """the summed partial row [NW] and the column sum of dpre [3 NF] -> dict dw1..3, db1..3 in the filters' own layouts"""
    out, o = {}, 0
    for k in range(3):
        n = NF * C1 * 3 * KW[k]
        out["dw%d" % (k + 1)], out["db%d" % (k + 1)] = dw[o:o + n].reshape(NF, C1, 3, KW[k]), db[k * NF:(k + 1) * NF]
        o += n
    return out


# ------------------------------------------------------------------ numpy emulation in the kernels' order
def _f32(a):
    return a.astype(np.float32).astype(np.float64)


def _np(t):
    return t.double().numpy()


def emulate_fwd(x, fault=None, chains=None):
    """forward rows [M H W, 3 NF] float64: acc = bias, then channel outer, dy, dx, one rounding per FMA (a float64 product and add rounded to
    fp32); `chains` accumulators over equal channel groups, added to the first in order.  fault a..e of FAULTS."""
    chains = FWD_CHAINS if chains is None else chains
    T = _np(x["T"])
    M, C, H, W = T.shape
    Tp = np.zeros((M, C, H + 2, W + 6))
    Tp[:, :, 1:H + 1, 3:W + 3] = T
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    near = ((xs < 3) | (xs >= W - 3)) & (ys >= 0)
    out = np.zeros((M, H, W, NCOL))
    per = (C + chains - 1) // chains
    for g in range(3):
        kw, w = KW[g], _np(x["w%d" % (g + 1)])
        b = _np(x["b%d" % (1 if fault == "e" else g + 1)])
        accs = [np.zeros((M, NF, H, W)) for _ in range(chains)]
        accs[0] += b[None, :, None, None]
        for ch in range(C):
            k = ch // per
            for dy in range(3):
                for dx in range(kw):
                    col = dx if (fault == "c" and g < 2) else dx + 2 - g                      # column of the 3 x 7 window
                    v = Tp[:, ch, dy:dy + H, col:col + W]
                    if fault == "b":
                        inside = (ys + dy - 1 >= 0) & (ys + dy - 1 < H) & (xs + col - 3 >= 0) & (xs + col - 3 < W)
                        v = np.where(inside[None], v, T[:, ch])
                    if fault == "a" and g == 2 and dx in (0, 6):
                        v = np.where(near[None], 0.0, v)
                    accs[k] = _f32(accs[k] + v[:, None] * w[None, :, ch, dy, dx, None, None])
        acc = accs[0]
        for a in accs[1:]:
            acc = _f32(acc + a)
        out[..., g * NF:(g + 1) * NF] = acc.transpose(0, 2, 3, 1)
    out = np.maximum(out, 0.0).reshape(M * H * W, NCOL)
    if fault == "d" and (M * H * W) % 256:
        out[(M * H * W) // 256 * 256:] = 0.0
    return out


def pack_wt(x, bounds=(9, 24)):
    """mt_conv3_pack_wt_kernel: wt[tap][o][C1P = 52], tap -> (g, dy, dx) with the three filters back to back; an index past a filter's end
    reads as 0 here"""
    wt = np.zeros((45, NF, 52))
    flat = [_np(x["w%d" % k]).reshape(-1) for k in (1, 2, 3)]
    for tap in range(45):
        g = 0 if tap < bounds[0] else 1 if tap < bounds[1] else 2
        kw, tl = KW[g], tap - TAP0[g]
        dy, dx = tl // kw, tl % kw
        for o in range(NF):
            idx = ((o * C1 + np.arange(C1)) * 3 + dy) * kw + dx
            wt[tap, o, :C1] = np.where(idx < flat[g].size, flat[g][np.minimum(idx, flat[g].size - 1)], 0.0)
    return wt


def emulate_data(x, fault=None):
    """dT [M, C1, H, W] float64: one chain per channel over dy, dx, g, o (outer to inner).  fault f, g, h1, h2, l of FAULTS."""
    M, C, H, W = x["T"].shape
    dpp = np.zeros((M, H + 2, W + 6, NCOL))
    dpp[:, 1:H + 1, 3:W + 3] = _np(x["dpre"]).reshape(M, H, W, NCOL)
    wt = pack_wt(x, (10, 25) if fault == "l" else (9, 24))
    cidx = np.arange(C1)
    if fault == "h2":
        cidx = np.where(cidx == 50, 51, cidx)
    acc = np.zeros((M, C, H, W))
    for dy in range(3):
        for dx in range(7):
            r0, c0 = 2 - dy, (dx if fault == "g" else 6 - dx)             # source (y - dy + 1, x - dx + 3) in padded coordinates
            src = dpp[:, r0:r0 + H, c0:c0 + W]
            for g in range(3):
                kw, dxg = KW[g], dx - 2 + g
                if dxg < 0 or dxg >= kw:
                    continue
                tap = TAP0[g] + dy * kw + dxg
                for o in range(NF):
                    acc = _f32(acc + src[:, None, :, :, g * NF + o] * wt[tap, o, cidx][None, :, None, None])
    if fault == "h1":
        acc[:, 2 * MT_CG:] = 0.0
    if fault == "f":
        acc.reshape(M, C, H * W)[:, :, 256:] = 0.0
    return acc


def emulate_partial(x, fault=None):
    """the partial rows [M MT_XS, NW] float64 of the weight gradient: one chain per (m, column range) over y, then x.  fault i1, i2, j."""
    T, dp = _np(x["T"]), _np(x["dpre"])
    M, C, H, W = T.shape
    dp = dp.reshape(M, H, W, NCOL)
    Tp = np.zeros((M, C, H + 2, W + 6))
    Tp[:, :, 1:H + 1, 3:W + 3] = T
    if fault == "j":                                  # rows 0 and H - 1 meet dy = 0 / dy = 2 with a row of the tile instead of nothing
        Tp[:, :, 0], Tp[:, :, H + 1] = Tp[:, :, 1], Tp[:, :, H]
    xc = xchunk(W)
    acc = [np.zeros((M, MT_XS, NF, C, 3, kw)) for kw in KW]
    for y in range(H):
        for xx in range(W):
            js = [xx // xc]
            if fault == "i1" and js == [1]:
                continue
            if fault == "i2" and W % 2 and xx == xc - 1:
                js = [0, 1]
            win = Tp[:, :, y:y + 3, xx:xx + 7]
            for g in range(3):
                prod = dp[:, y, xx, g * NF:(g + 1) * NF][:, :, None, None, None] * win[:, None, :, :, 2 - g:2 - g + KW[g]]
                for j in js:
                    acc[g][:, j] = _f32(acc[g][:, j] + prod)
    return np.concatenate([a.reshape(M, MT_XS, -1) for a in acc], 2).reshape(M * MT_XS, NW)


def _lane_sum(rows):
    """colsum_lanes_kernel on one slice [R, N]: lane j adds rows j, j + 16, .. in order from 0, then the 16 lane sums are added in lane order from 0"""
    R, N = rows.shape
    n = (R + 15) // 16
    pad = np.zeros((n * 16, N))
    pad[:R] = rows
    pad = pad.reshape(n, 16, N)
    lanes = np.zeros((16, N))
    for i in range(n):
        lanes = _f32(lanes + pad[i])
    out = np.zeros(N)
    for j in range(16):
        out = _f32(out + lanes[j])
    return out


def _row_sum(rows):
    """colsum_kernel on one slice [R, N]: one thread per column, rows in order from 0"""
    out = np.zeros(rows.shape[1])
    for r in rows:
        out = _f32(out + r)
    return out


def emulate_colsum(rows, fault=None):
    """nir_colsum_det_f32 over rows [R, N]: slices of colsum_slices(R) rows, each summed by _row_sum (N > 64) or _lane_sum (N <= 64); more than
    one slice: _lane_sum over the slice sums; plain fp32 additions.  fault k1: rows beyond the first 64 dropped; k2: the last slice added twice."""
    R, N = rows.shape
    if fault == "k1":
        rows, R = rows[:64], min(R, 64)
    ms, S = colsum_slices(R)
    one = _lane_sum if N <= 64 else _row_sum
    part = np.stack([one(rows[s * ms:min(R, (s + 1) * ms)]) for s in range(S)])
    if S == 1:
        return part[0]
    return _lane_sum(np.concatenate([part, part[-1:]]) if fault == "k2" else part)


def emulate(x, kernels=KERNELS, fault=None):
    """dict over the KEYS of `kernels`, float64 torch tensors, as the kernels compute them (fault: one of FAULTS, applied to its own kernel)"""
    M, _, H, W = x["T"].shape
    out = {}
    if "fwd" in kernels:
        out["fwd"] = torch.from_numpy(emulate_fwd(x, fault))
    if "data" in kernels:
        out["dT"] = torch.from_numpy(emulate_data(x, fault))
    g = {}
    if "weight" in kernels:
        g["dw"] = emulate_colsum(emulate_partial(x, fault), fault)
    if "bias" in kernels:
        g["db"] = emulate_colsum(_np(x["dpre"]))
    if g:
        s = split_grads(g.get("dw", np.zeros(NW)), g.get("db", np.zeros(NCOL)))
        out.update({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in s.items() if ("dw" in g and k.startswith("dw")) or ("db" in g and k.startswith("db"))})
    return out


def honest_ok(x, p, kernels=KERNELS):
    """(ok, worst ratio): the 0.8 rule -- the in-order emulation within 0.8 of the bound at the cap on every tensor"""
    em = emulate(x, kernels)
    worst = max(accept(v, k, p, MARGIN_CAP)[1]["ratio"] for k, v in em.items())
    return worst <= 0.8 * MARGIN_CAP, worst


# ------------------------------------------------------------------ the fall-back: patch rows and their backward (csrc/train.hip)
def ic(M, C, H, W, kh, kw, why):
    return dict(M=M, C=C, H=H, W=W, kh=kh, kw=kw, why=why, id="M%d-C%d-H%d-W%d-k%dx%d" % (M, C, H, W, kh, kw))


IM2COL_CASES = [
    ic(2, 3, 2, 2, 3, 7, "W < kw"), ic(2, 4, 3, 9, 1, 3, "kh = 1"), ic(2, 2, 6, 5, 5, 3, "kh = 5"), ic(3, 5, 1, 11, 3, 5, "H = 1"),
    ic(2, 51, 3, 10, 3, 7, "K = 1071 > 256"), ic(1, 51, 2, 64, 3, 5, "channel groups 32 + 19"), ic(1, 3, 2, 2048, 1, 7, "CG = 1 at the widest row"),
]
IM2COL_REFUSED = [ic(1, 3, 2, 2049, 1, 7, "W = 2049"), ic(1, 3, 2, 8, 3, 4, "even kw")]


def im2col_family(d):
    g = torch.Generator().manual_seed(d["W"] * 13 + d["C"] + d["kh"])
    M, C, H, W, K = d["M"], d["C"], d["H"], d["W"], d["C"] * d["kh"] * d["kw"]
    return dict(x=torch.randn(M, C, H, W, generator=g), drows=torch.randn(M * H * W, K, generator=g))


def im2col_chain(d, v, dt):
    """(patch rows [M H W, C kh kw], din [M, C, H, W]) by F.unfold and its autograd in dtype dt"""
    M, C, H, W = v["x"].shape
    xin = v["x"].to(dt).clone().requires_grad_(True)
    rows = F.unfold(xin, (d["kh"], d["kw"]), padding=(d["kh"] // 2, d["kw"] // 2)).transpose(1, 2).reshape(M * H * W, -1)
    rows.backward(v["drows"].to(dt))
    return rows.detach(), xin.grad
