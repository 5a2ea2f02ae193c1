"""The acceptance criterion of the GEMM building blocks (nir_linear_ex_f32, nir_linear_planes_f32, nir_rowdot_f32): a float64
reference of the whole operation, the bound a kernel's result has to meet, seeded input families and a numpy emulation of the two
split-precision operand formats (used on the CPU to show that the bound rejects a kernel that loses one cross term).

Bound: with s = max |ref64|, e = max |got - ref64| / s and e_chain the same figure for torch's CPU fp32 chain on the same inputs,

    e <= margin * max(e_chain, 2^-23) + fmt(form) + act_term

fmt comes from the operand formats, not from a measurement:
    f32     0        fp32 MFMA: exact fp32 products, fp32 accumulation -- the error is accumulation order alone, which `margin` prices
    bf16x3  2^-22    three truncated 8-bit terms leave < 2^-23 of each operand; the dropped b1 b2 and b2 b1 products are 2 * 2^-24
    fp16x2  3*2^-22  each operand known to 2^-22 (11 + 11 mantissa bits), the dropped h2' h2' product another 2^-22 (csrc/split2.hpp)
act_term: fast_tanh is documented at ~1e-7 absolute (csrc/common.hpp); twice that is allowed, per tanh output (2e-7 / s) and per
row-dot output (2e-7 * sum of the 16 |add[n]| / s); 0 for none / ReLU / maxout.
MARGIN: from the largest measured (e - fmt - act_term) / max(e_chain, 2^-23) over the envelope cases on the MI355X, doubled and rounded up
to a power of two, and never above MARGIN_CAP = 4: the cap is what keeps a dropped cross term outside the bound
(tests/test_gemm_criterion_host.py).  Measured (DESIGN.md section 2 has the figures per kernel): 0.90 on the fp16 two-term kernels -> 2;
3.07 on the bf16 three-term kernel and 3.18 on the fp32-MFMA one, both at K = 900 -> the rule asks for 8, the cap holds, so 4 it is, with
1.26 x of headroom instead of 2 x.  Those two figures are accumulation order, not a lost term: the kernels add all K products of an output
into ONE fp32 accumulator (K / 2 resp. 6 K / 16 dependent additions) where the CPU BLAS of e_chain keeps dozens of partial sums, so the
ratio grows like sqrt(K) (1.2 - 1.5 at K = 300)."""
import numpy as np
import torch

ACT_NONE, ACT_TANH, ACT_RELU, ACT_MAXOUT2, ACT_TANH_ROWDOT16, ACT_BOUNDED = 0, 1, 2, 16, 17, 0x100
FMT = {"f32": 0.0, "bf16x3": 2.0 ** -22, "fp16x2": 3 * 2.0 ** -22}
EPS = 2.0 ** -23
MARGIN_CAP = 4.0
MARGIN = {"f32": 4.0, "bf16x3": 4.0, "fp16x2": 2.0}


# ------------------------------------------------------------------ inputs
def family(name, g, rows, K, role, cols=None):
    """One operand of the named input family as a float32 CPU tensor [rows, cols or K].  role "a": the A operand (or the embedding table it
    is gathered from); "w": the weight, scaled for a reduction of length K."""
    cols = K if cols is None else cols
    randn = lambda: torch.randn(rows, cols, generator=g, dtype=torch.float64)
    rand = lambda lo, hi: torch.rand(rows, cols, generator=g, dtype=torch.float64) * (hi - lo) + lo
    if role == "w":
        if name == "positive":
            x = rand(0.5, 1.5) / K
        elif name == "mixed":
            x = randn() / K ** 0.5 * 10.0 ** rand(-4, 2)
        else:                                        # randn / edge / tiny: the plain weight
            x = randn() / K ** 0.5
    elif name == "randn":
        x = randn()
    elif name == "positive":
        x = rand(0.5, 1.5)
    elif name == "mixed":
        x = (randn() * 10.0 ** rand(-4, 4)).clamp(-30000.0, 30000.0)
    elif name == "edge":                             # the documented 2^15 limit of the fp16 two-term format
        x = rand(-32767.9, 32767.9)
        x[rows // 3] = 32767.998
        x[(2 * rows) // 3] = -32767.998
    elif name == "tiny":
        x = randn() * 2.0 ** -10
    elif name == "tiny20":
        x = randn() * 2.0 ** -20
    else:
        raise ValueError(name)
    return x.float()


def gather_rows(table, ids, E, K, rows_per_seq, seq_stride, M):
    """The A operand of a gathered call as a dense [M, K] matrix: row m is the concatenation of the table rows of ids[base(m) + 0, 1, ..]."""
    taps = (K + E - 1) // E
    m = torch.arange(M)
    base = (m // rows_per_seq) * seq_stride + (m % rows_per_seq)
    idx = ids.reshape(-1)[base[:, None] + torch.arange(taps)[None]]
    return table[idx].reshape(M, taps * E)[:, :K]


# ------------------------------------------------------------------ reference
def _finish(v, add, act):
    act &= 0xff
    if act == ACT_TANH_ROWDOT16:
        return (torch.tanh(v) * add.to(v.dtype)).reshape(v.shape[0], -1, 16).sum(-1)
    if add is not None:
        v = v + add.to(v.dtype)
    if act == ACT_TANH:
        v = torch.tanh(v)
    elif act == ACT_RELU:
        v = torch.relu(v)
    elif act == ACT_MAXOUT2:
        v = v.reshape(v.shape[0], -1, 2).max(-1).values
    return v


def _chain(a, w, bias, bias2, add, act, dt):
    v = a.to(dt) @ w.to(dt).t()
    if bias is not None:
        v = v + bias.to(dt)
    if bias2 is not None:
        v = v + bias2.to(dt)
    return _finish(v, add, act)


def ref64(a, w, bias=None, bias2=None, add=None, act=0):
    """act(A W^T + bias + bias2 (+ add)) in float64 on the CPU; A [M, K] dense (gather_rows for a gathered call), W [N, K]."""
    return _chain(a, w, bias, bias2, add, act, torch.float64)


def act_term(act, add, s):
    act &= 0xff
    if act == ACT_TANH:
        return 2e-7 / s
    if act == ACT_TANH_ROWDOT16:
        return 2e-7 * float(add.double().abs().reshape(-1, 16).sum(-1).max()) / s
    return 0.0


def subnormal_floor(a, w):
    """fp16x2 below its lower range: the scaled residual is an fp16 subnormal, each operand is known to 2^-35 absolute, so output (m, n) may
    be off by 2^-35 * sum_k (|a[m,k]| + |w[n,k]|) on top of the ordinary bound."""
    return 2.0 ** -35 * (a.double().abs().sum(1)[:, None] + w.double().abs().sum(1)[None, :])


def measure(got, a, w, bias=None, bias2=None, add=None, act=0, form="f32", floor=None):
    """dict(e, e_chain, s, extra, ratio): ratio = (e - fmt - act_term) / max(e_chain, 2^-23), the figure MARGIN is chosen from."""
    ref = ref64(a, w, bias, bias2, add, act)
    got = torch.as_tensor(np.asarray(got)) if not torch.is_tensor(got) else got.detach().cpu()
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "non-finite output"
    s = float(ref.abs().max())
    assert s > 0
    err = (got.double() - ref).abs()
    if floor is not None:
        err = (err - floor).clamp_min(0.0)
    e = float(err.max()) / s
    e_chain = float((_chain(a, w, bias, bias2, add, act, torch.float32).double() - ref).abs().max()) / s
    extra = FMT[form] + act_term(act, add, s)
    return dict(e=e, e_chain=e_chain, s=s, extra=extra, ratio=(e - extra) / max(e_chain, EPS))


def accept(got, a, w, bias=None, bias2=None, add=None, act=0, form="f32", margin=None, floor=None):
    """(ok, figures): the criterion of the module docstring.  margin defaults to MARGIN[form] and may never exceed MARGIN_CAP."""
    margin = MARGIN[form] if margin is None else margin
    assert margin <= MARGIN_CAP
    r = measure(got, a, w, bias, bias2, add, act, form, floor)
    r["bound"] = margin * max(r["e_chain"], EPS) + r["extra"]
    return r["e"] <= r["bound"], r


# ------------------------------------------------------------------ emulation of the two split formats
def _trunc_bf16(x):
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _f16_rtz(x):
    """float32 -> float16 rounded toward zero (v_cvt_pkrtz_f16_f32), returned as float32"""
    h = x.astype(np.float16)
    over = np.abs(h.astype(np.float32)) > np.abs(x)
    h = np.where(over, np.nextafter(h, np.float16(0)), h)
    return h.astype(np.float32)


def split_terms(x, form):
    """The terms a kernel carries for the float32 array x, as float32 arrays.  bf16x3: (b0, b1, b2), each the top 16 bits of the running
    residual (exact fp32 residuals).  fp16x2: (h1, h2') with x ~ h1 + 2^-11 h2'."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if form == "bf16x3":
        b0 = _trunc_bf16(x)
        r = x - b0
        b1 = _trunc_bf16(r)
        r = r - b1
        return b0, b1, _trunc_bf16(r)
    h1 = _f16_rtz(x)
    return h1, _f16_rtz((x - h1) * np.float32(2048.0))


def emulate(a, w, form, drop=None):
    """A W^T as the split-precision kernels form it, products summed in float64 (so without the kernels' fp32 accumulation error).
    drop: one cross term left out, named by its A and W terms -- "b1b1", "b0b2", "b2b0" (bf16x3), "a2w1", "a1w2" (fp16x2)."""
    A = [t.astype(np.float64) for t in split_terms(a.numpy() if torch.is_tensor(a) else a, form)]
    W = [t.astype(np.float64) for t in split_terms(w.numpy() if torch.is_tensor(w) else w, form)]
    out = 0.0
    if form == "bf16x3":
        for i, j in ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)):
            if drop != "b%db%d" % (i, j):
                out = out + A[i] @ W[j].T
        return out
    cross = 0.0
    for i, j in ((1, 0), (0, 1)):
        if drop != "a%dw%d" % (i + 1, j + 1):
            cross = cross + A[i] @ W[j].T
    return A[0] @ W[0].T + cross / 2048.0
