"""The acceptance criterion of the train-mode recurrences and their BPTT up to 128 units per direction (nir_lstm_train_fwd, nir_lstm_train_fwd_split,
nir_lstm_train_bwd: csrc/train.hip, csrc/lstm_mfma.hip, csrc/lstm_fold.hip; nir_gru_train_fwd / _bwd: csrc/gru_train.hip) and of the streaming cell
kernels (nir_lstm_cell_*, nir_gru_cell_seq_*): a numpy restatement without autograd -- float64 the reference, float32 the yardstick --, the bound,
seeded input families, planted faults (the CPU evidence that the bound has teeth, tests/test_bptt_criterion_host.py) and a restatement of the
dispatchers that the case tables of tests/test_gpu_bptt_envelope.py are built with.

Contract (include/neuroir_hip.h).  Lengths are clamped to [0, T], a negative length counts as 0; the reverse direction walks t = len-1 .. 0.
LSTM forward: out [M,T,ndir*H] (zero at t >= len), act [M,T,ndir,4H] = (i,f,g,o) after their non-linearities and cst [M,T,ndir,H] = c_t of every
valid step (unspecified at t >= len), hn / cn [ndir,M,H] the state after the last valid step (h0 / c0 for len = 0).  LSTM BPTT: with dh = dout_t +
dh_rec, th = tanh(c_t), dc_t = dc_rec + dh o (1 - th^2) + dcst_t:
    di = dc_t g i (1-i)   df = dc_t c_{t-1} f (1-f)   dg = dc_t i (1-g^2)   do = dh th o (1-o)   dc_rec = dc_t f   dh_rec = dgates_t W_hh
dhn / dcn enter at a sequence's own last step (they are the initial dh_rec / dc_rec and are kept while the sequence has not started); a sequence of
length 0 hands them through to dh0 / dc0 unchanged; c_{t-1} of the first step is c0 (zero when NULL); dgates is zero at t >= len.
GRU (gate order r,z,n; q = W_hn h + b_hn inside the reset product): act = (r,z,n,q); BPTT with dh = dout_t + dh_rec:
    da_n = dh (1-z)(1-n^2)   da_r = da_n q r (1-r)   da_z = dh (h_{t-1} - n) z (1-z)   dq = da_n r   dh_rec = z dh + (da_r, da_z, dq) W_hh
dgx = (da_r, da_z, da_n), dq; h_{t-1} comes from `out` one row back (forward) / ahead (reverse), zero at the first step; no initial state.

The BPTT kernels are judged in isolation: their saved inputs are the float64 forward rounded to fp32 (NaN at t >= len of act / cst: the forward
leaves those unwritten, the backward may not depend on them), the yardstick runs the same BPTT in float32 from the same inputs.

Bound, for every output o and every direction separately (absolute errors against float64, e of the kernel, e32 of the yardstick):

    e(o) <= margin * max(e32(o), 2^-23 * s(o)) + e_act(o)   [+ n_split * gemm_ref.FMT["fp16x2"] for the split-fp16 forward]

s(o):   the largest magnitude of the float64 result of that output and direction (1 for an all-zero result: it compares at 2^-23 absolute).
        Gradients are not bounded by 1 (they scale with dout, dhn, dcst and T), hence the scale -- rnn_ref's bound is this one with s = 1.
e_act:  rnn_ref's DELTA = 2e-7 shift of every activation THE KERNEL UNDER TEST computes itself: the deviation of the float64 evaluation from itself
        with those activation outputs shifted by +DELTA and by -DELTA (the larger).  Every sigmoid / tanh in a forward; tanh(c_t) alone in the LSTM
        BPTT (i,f,g,o are inputs there); nothing in the GRU BPTT and in gru_cell_seq_bwd.
margin: per kernel family, MEASURED on the MI355X (tests/test_gpu_bptt_envelope.py prints (e - e_act) / max(e32, 2^-23 s) per case): the largest
        ratio of the family doubled and rounded up to a power of two, never below 1, never above gemm_ref.MARGIN_CAP = 4 (accept() asserts it).
        RATIO below holds the measured figures, DESIGN.md section 19 quotes them.
"""
import collections

import numpy as np

import gemm_ref as G
import rnn_ref as R

DELTA, EPS, MARGIN_CAP, POISON = R.DELTA, R.EPS, G.MARGIN_CAP, R.POISON
SPLIT_FMT = G.FMT["fp16x2"]
# kernel family -> the largest measured (e - e_act) / max(e32, 2^-23 s) over the family's cases (MI355X, 795 figures of 417 tests) and, below,
# the margin that follows from it.  Negative: no case's error reaches e_act alone.  lstm_bwd_mfma: the doubled figure asks for 8, the margin is the
# cap -- the kernel sums the 4H terms of dgates W_hh in ONE chain per unit tile, and so errs like the "sequential" fp32 evaluation (which sits at 3.3
# to 5.8 on the same inputs), not like the blocked sum of the yardstick; the figure is dh0's.
RATIO = {"lstm_fwd_valu": -0.343, "lstm_fwd_mfma16": 0.107, "lstm_fwd_split": -0.666, "lstm_bwd_valu": 1.433, "lstm_bwd_mfma": 3.436, "gru_fwd": -0.264,
         "gru_bwd_valu": 1.166, "gru_bwd_mfma": 1.343, "cell": 1.091}


def margin_from(ratio):
    """the project's rule (DESIGN.md sections 2 and 13): doubled, rounded up to a power of two, at least 1, at most the cap"""
    m = 1.0
    while m < 2.0 * ratio and m < MARGIN_CAP:
        m *= 2.0
    return m


MARGIN = {k: margin_from(r) for k, r in RATIO.items()}
assert MARGIN == {"lstm_fwd_valu": 1.0, "lstm_fwd_mfma16": 1.0, "lstm_fwd_split": 1.0, "lstm_bwd_valu": 4.0, "lstm_bwd_mfma": 4.0, "gru_fwd": 1.0,
                  "gru_bwd_valu": 4.0, "gru_bwd_mfma": 4.0, "cell": 4.0}


def family_of(kernel):
    base = kernel.split("<")[0]
    return {"lstm_train_fwd_kernel": "lstm_fwd_valu", "lstm_train_fwd_mfma16_kernel": "lstm_fwd_mfma16", "lstm16_pt_h2_kernel": "lstm_fwd_split",
            "lstm_train_bwd_kernel": "lstm_bwd_valu", "lstm_train_bwd_mfma_kernel": "lstm_bwd_mfma", "gru_train_fwd_kernel": "gru_fwd",
            "gru_train_bwd_kernel": "gru_bwd_valu", "gru_train_bwd_mfma_kernel": "gru_bwd_mfma"}.get(base, "cell")


def _jit(dt, shift, noise):
    def jit(v):
        if shift:
            v = v + dt(shift)
        if noise is not None:
            v = v + (noise.integers(0, 2, v.shape) * 2 - 1).astype(dt) * dt(1e-7)
        return v
    return jit


def _dot(h, W, order, dt):
    """h [M,K] W^T [K,N] in dtype dt, the orders of rnn_ref._dot ("blas": numpy's matmul; "seq": one accumulator, k ascending; "quad": four
    sequential partial sums over the quarters of K padded to a multiple of 16, combined as (p0 + p1) + (p2 + p3)), with the sequential sums as
    np.add.accumulate over the rounded products -- the same bits as rnn_ref's loop, fast enough for K = 4H = 512"""
    if order == "blas":
        return h @ W.T
    M, K = h.shape
    KQ = (K + 15) // 16 * 4
    spans = [(0, K)] if order == "seq" else [(q * KQ, min((q + 1) * KQ, K)) for q in range(4)]
    out = np.empty((M, W.shape[0]), dt)
    for r0 in range(0, M, 32):
        p = h[r0:r0 + 32, None, :] * W[None, :, :]
        part = [np.add.accumulate(p[:, :, a:b], axis=2)[:, :, -1] if b > a else np.zeros(p.shape[:2], dt) for a, b in spans]
        out[r0:r0 + 32] = part[0] if order == "seq" else (part[0] + part[1]) + (part[2] + part[3])
    return out


# ------------------------------------------------------------------ forward, in any precision
FWD_FAULTS = ("bhn_outside",)


def forward(cell, gin, w_hh, lengths=None, h0=None, c0=None, ndir=2, b_hh=None, dt=np.float64, shift=0.0, noise=None, order="blas", mut=None):
    """-> dict(out [M,T,ndir*H], act [M,T,ndir,4H], cst [M,T,ndir,H] (LSTM), hn, cn [ndir,M,H]) in dtype dt; act / cst are zero at t >= len here
    (unspecified in the contract).  shift / noise / order as rnn_ref.run; mut "bhn_outside": the GRU's b_hn added outside the reset product."""
    one = dt(1.0)
    gin = np.asarray(gin, dt)
    M, T, _ = gin.shape
    NG = 4 if cell == "lstm" else 3
    H = gin.shape[2] // (ndir * NG)
    assert gin.shape[2] == ndir * NG * H
    w = np.asarray(w_hh, dt).reshape(ndir, NG * H, H)
    lens = R.clamp_lengths(lengths, M, T)
    out, act = np.zeros((M, T, ndir * H), dt), np.zeros((M, T, ndir, 4 * H), dt)
    cst, hn, cn = np.zeros((M, T, ndir, H), dt), np.zeros((ndir, M, H), dt), np.zeros((ndir, M, H), dt)
    rows = np.arange(M)
    jit = _jit(dt, shift, noise)
    sig = lambda v: jit(one / (one + np.exp(-v)))
    tanh = lambda v: jit(np.tanh(v))
    with np.errstate(over="ignore"):
        for d in range(ndir):
            h = np.zeros((M, H), dt) if h0 is None else np.asarray(h0, dt).reshape(ndir, M, H)[d].copy()
            c = np.zeros((M, H), dt) if c0 is None else np.asarray(c0, dt).reshape(ndir, M, H)[d].copy()
            for step in range(int(lens.max()) if M else 0):
                t = np.full(M, step, np.int64) if d == 0 else lens - 1 - step
                live = step < lens
                tc = np.clip(t, 0, T - 1)
                g = gin[rows, tc, d * NG * H:(d + 1) * NG * H]
                hw = _dot(h, w[d], order, dt)
                if cell == "lstm":
                    a = g + hw
                    gi, gf, gg, go = sig(a[:, :H]), sig(a[:, H:2 * H]), tanh(a[:, 2 * H:3 * H]), sig(a[:, 3 * H:])
                    c2 = gf * c + gi * gg
                    h2 = go * tanh(c2)
                    a4 = np.concatenate((gi, gf, gg, go), 1)
                else:
                    bh = np.asarray(b_hh, dt).reshape(ndir, 3 * H)[d]
                    r = sig(g[:, :H] + (hw[:, :H] + bh[:H]))
                    z = sig(g[:, H:2 * H] + (hw[:, H:2 * H] + bh[H:2 * H]))
                    q = hw[:, 2 * H:] + bh[2 * H:]
                    n = tanh(g[:, 2 * H:] + (r * hw[:, 2 * H:] + bh[2 * H:] if mut == "bhn_outside" else r * q))
                    h2 = (one - z) * n + z * h
                    c2 = c
                    a4 = np.concatenate((r, z, n, q), 1)
                h = np.where(live[:, None], h2, h)
                c = np.where(live[:, None], c2, c)
                lr = rows[live]
                out[lr, tc[live], d * H:(d + 1) * H] = h2[live]
                act[lr, tc[live], d] = a4[live]
                cst[lr, tc[live], d] = c2[live]
            hn[d], cn[d] = h, c
    res = dict(out=out, act=act, hn=hn)
    if cell == "lstm":
        res.update(cst=cst, cn=cn)
    return res


# ------------------------------------------------------------------ BPTT, in any precision, faithful or with a planted fault
COMMON_FAULTS = ("no_dhn", "dhn_at_T", "idle_overwrite", "rev_T", "past_len", "no_hi_units", "b16")
LSTM_FAULTS = COMMON_FAULTS + ("no_dcn", "no_dcst", "c0_zero", "c_cur", "dc_no_f", "early_h0")
GRU_BWD_FAULTS = COMMON_FAULTS + ("dq_as_dan", "no_direct", "h_cur")        # rnn_train_ref's six: these three, past_len, rev_T ("rev_start") and
PRECISION_FAULTS = ("b16",)                                                 # the forward's "bhn_outside" (FWD_FAULTS)


def _walk(d, step, lens, M, T, mut):
    """(position t, clamped; rows the backward visits at this step)"""
    if d == 0:
        t = np.full(M, step, np.int64)
        return t, (np.ones(M, bool) if mut == "past_len" else step < lens)
    if mut == "rev_T":                                     # the reverse direction taken to start at T - 1: it walks the padding too
        return np.full(M, T - 1 - step, np.int64), np.ones(M, bool)
    t = lens - 1 - step
    return np.clip(t, 0, T - 1), t >= 0


def _product(dg, W, order, dt, mut, H, NG):
    """dh_rec = dg [M,NG*H] W [NG*H,H].  "no_hi_units": the units >= 64 of every gate left out; "b16": the B operand (dg) rounded to fp16"""
    if mut == "no_hi_units":
        W = W.copy()
        for g in range(NG):
            W[g * H + 64:(g + 1) * H] = 0
    if mut == "b16":
        with np.errstate(over="ignore"):
            dg = dg.astype(np.float16).astype(dt)
    return _dot(dg, np.ascontiguousarray(W.T), order, dt)


def _final_grad(a, d, dt, M, H, ndir, lens, T, mut, drop):
    if a is None or mut == drop:
        return np.zeros((M, H), dt)
    v = np.asarray(a, dt).reshape(ndir, M, H)[d].copy()
    if mut == "dhn_at_T":                                  # injected at step T - 1 instead of len - 1: lost for every shorter sequence
        v[lens < T] = 0
    return v


def lstm_bwd(dout, act, cst, w_hh, lengths=None, ndir=2, dhn=None, dcn=None, dcst=None, c0=None, dt=np.float64, shift=0.0, noise=None,
             order="blas", mut=None):
    """-> dict(dgates [M,T,ndir*4H], dh0, dc0 [ndir,M,H]) in dtype dt.  shift / noise act on tanh(c_t), the one activation the BPTT computes."""
    one = dt(1.0)
    dout = np.asarray(dout, dt)
    M, T, _ = dout.shape
    H = dout.shape[2] // ndir
    act, cst = np.asarray(act, dt).reshape(M, T, ndir, 4 * H), np.asarray(cst, dt).reshape(M, T, ndir, H)
    if mut is not None:                                    # a faulty walk may read t >= len: the unwritten positions count as zero there
        act, cst = np.nan_to_num(act), np.nan_to_num(cst)
    dcst = None if (dcst is None or mut == "no_dcst") else np.asarray(dcst, dt).reshape(M, T, ndir, H)
    c0 = None if (c0 is None or mut == "c0_zero") else np.asarray(c0, dt).reshape(ndir, M, H)
    w = np.asarray(w_hh, dt).reshape(ndir, 4 * H, H)
    lens = R.clamp_lengths(lengths, M, T)
    dgates, dh0, dc0 = np.zeros((M, T, ndir * 4 * H), dt), np.zeros((ndir, M, H), dt), np.zeros((ndir, M, H), dt)
    rows = np.arange(M)
    jit = _jit(dt, shift, noise)
    nsteps = T if mut in ("past_len", "rev_T") else (int(lens.max()) if M else 0)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(ndir):
            dhr = _final_grad(dhn, d, dt, M, H, ndir, lens, T, mut, "no_dhn")
            dc = _final_grad(dcn, d, dt, M, H, ndir, lens, T, mut, "no_dcn")
            early = (dhr.copy(), dc.copy())
            for step in range(nsteps - 1, -1, -1):
                t, on = _walk(d, step, lens, M, T, mut)
                if step == 0:
                    early = (dhr.copy(), dc.copy())
                a = act[rows, t, d]
                i_, f_, g_, o_ = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
                ct = cst[rows, t, d]
                if step > 0:
                    cprev = cst[rows, np.clip(t - 1 if d == 0 else t + 1, 0, T - 1), d]
                else:
                    cprev = np.zeros((M, H), dt) if c0 is None else c0[d]
                if mut == "c_cur":
                    cprev = ct
                th = jit(np.tanh(ct))
                dh = dout[rows, t, d * H:(d + 1) * H] + dhr
                dct = dc + dh * o_ * (one - th * th)
                if dcst is not None:
                    dct = dct + dcst[rows, t, d]
                dg = np.concatenate((dct * g_ * i_ * (one - i_), dct * cprev * f_ * (one - f_), dct * i_ * (one - g_ * g_),
                                     dh * th * o_ * (one - o_)), 1)
                dg = np.where(on[:, None], dg, dt(0))
                dgates[rows[on], t[on], d * 4 * H:(d + 1) * 4 * H] = dg[on]
                dc = np.where(on[:, None], dct if mut == "dc_no_f" else dct * f_, dc)
                prod = _product(dg, w[d], order, dt, mut, H, 4)
                dhr = prod if mut == "idle_overwrite" else np.where(on[:, None], prod, dhr)
            dh0[d], dc0[d] = early if mut == "early_h0" else (dhr, dc)
    return dict(dgates=dgates, dh0=dh0, dc0=dc0)


def gru_bwd(dout, act, out, w_hh, lengths=None, ndir=2, dhn=None, dt=np.float64, order="blas", mut=None):
    """-> dict(dgx [M,T,ndir*3H], dq [M,T,ndir*H]) in dtype dt (no activation is computed here: no shift)"""
    one = dt(1.0)
    dout = np.asarray(dout, dt)
    M, T, _ = dout.shape
    H = dout.shape[2] // ndir
    act, out = np.asarray(act, dt).reshape(M, T, ndir, 4 * H), np.asarray(out, dt).reshape(M, T, ndir * H)
    if mut is not None:
        act = np.nan_to_num(act)
    w = np.asarray(w_hh, dt).reshape(ndir, 3 * H, H)
    lens = R.clamp_lengths(lengths, M, T)
    dgx, dq = np.zeros((M, T, ndir * 3 * H), dt), np.zeros((M, T, ndir * H), dt)
    rows = np.arange(M)
    nsteps = T if mut in ("past_len", "rev_T") else (int(lens.max()) if M else 0)
    with np.errstate(invalid="ignore", over="ignore"):
        for d in range(ndir):
            dhr = _final_grad(dhn, d, dt, M, H, ndir, lens, T, mut, "no_dhn")
            for step in range(nsteps - 1, -1, -1):
                t, on = _walk(d, step, lens, M, T, mut)
                a = act[rows, t, d]
                r, z, n, q = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
                if mut == "h_cur":
                    hp = out[rows, t, d * H:(d + 1) * H]
                elif step > 0:
                    hp = out[rows, np.clip(t - 1 if d == 0 else t + 1, 0, T - 1), d * H:(d + 1) * H]
                else:
                    hp = np.zeros((M, H), dt)
                dh = dout[rows, t, d * H:(d + 1) * H] + dhr
                dan = dh * (one - z) * (one - n * n)
                da_r, da_z = dan * q * r * (one - r), dh * (hp - n) * z * (one - z)
                dqv = dan if mut == "dq_as_dan" else dan * r
                m = lambda v: np.where(on[:, None], v, dt(0))
                gx, gh = m(np.concatenate((da_r, da_z, dan), 1)), m(np.concatenate((da_r, da_z, dqv), 1))
                dgx[rows[on], t[on], d * 3 * H:(d + 1) * 3 * H] = gx[on]
                dq[rows[on], t[on], d * H:(d + 1) * H] = gh[on][:, 2 * H:]
                nxt = _product(gh, w[d], order, dt, mut, H, 3)
                if mut != "no_direct":
                    nxt = m(dh * z) + nxt
                dhr = nxt if mut == "idle_overwrite" else np.where(on[:, None], nxt, dhr)
    return dict(dgx=dgx, dq=dq)


# ------------------------------------------------------------------ the streaming cell kernels (element-wise)
def lstm_cell_fwd(gates, c_prev, dt=np.float64, shift=0.0):
    one, jit = dt(1.0), _jit(dt, shift, None)
    g = np.asarray(gates, dt)
    H = g.shape[1] // 4
    sig = lambda v: jit(one / (one + np.exp(-v)))
    i, f, gg, o = sig(g[:, :H]), sig(g[:, H:2 * H]), jit(np.tanh(g[:, 2 * H:3 * H])), sig(g[:, 3 * H:])
    c = f * (0 if c_prev is None else np.asarray(c_prev, dt)) + i * gg
    return dict(act=np.concatenate((i, f, gg, o), 1), c=c, h=o * jit(np.tanh(c)))


def lstm_cell_bwd(dh, dc, act, c, c_prev, dt=np.float64, shift=0.0):
    one, jit = dt(1.0), _jit(dt, shift, None)
    a, c = np.asarray(act, dt), np.asarray(c, dt)
    H = c.shape[1]
    i, f, g, o = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    th = jit(np.tanh(c))
    dh = np.zeros_like(c) if dh is None else np.asarray(dh, dt)
    dct = (0 if dc is None else np.asarray(dc, dt)) + dh * o * (one - th * th)
    cp = np.zeros_like(c) if c_prev is None else np.asarray(c_prev, dt)
    return dict(dgates=np.concatenate((dct * g * i * (one - i), dct * cp * f * (one - f), dct * i * (one - g * g), dh * th * o * (one - o)), 1),
                dc_prev=dct * f)


def gru_cell_fwd(gx, gh, h_prev, dt=np.float64, shift=0.0):
    """gh: [B,3H] (b_hh included) or the [3H] bias alone"""
    one, jit = dt(1.0), _jit(dt, shift, None)
    gx, gh = np.asarray(gx, dt), np.broadcast_to(np.asarray(gh, dt), np.shape(gx))
    H = gx.shape[1] // 3
    sig = lambda v: jit(one / (one + np.exp(-v)))
    r, z = sig(gx[:, :H] + gh[:, :H]), sig(gx[:, H:2 * H] + gh[:, H:2 * H])
    q = gh[:, 2 * H:]
    n = jit(np.tanh(gx[:, 2 * H:] + r * q))
    return dict(act=np.concatenate((r, z, n, q), 1), h=(one - z) * n + z * (0 if h_prev is None else np.asarray(h_prev, dt)))


def gru_cell_bwd(dh, act, h_prev, dt=np.float64):
    one = dt(1.0)
    a, dh = np.asarray(act, dt), np.asarray(dh, dt)
    H = dh.shape[1]
    r, z, n, q = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
    dan = dh * (one - z) * (one - n * n)
    da_r, da_z = dan * q * r * (one - r), dh * ((0 if h_prev is None else np.asarray(h_prev, dt)) - n) * z * (one - z)
    return dict(dgx=np.concatenate((da_r, da_z, dan), 1), dgh=np.concatenate((da_r, da_z, dan * r), 1), dh_dir=dh * z)


# ------------------------------------------------------------------ criterion
# how an output splits into directions: "cat" = direction blocks side by side in the last axis, "dim" = axis 2, "lead" = axis 0
LAYOUT = {"out": "cat", "dgates": "cat", "dgx": "cat", "dq": "cat", "act": "dim", "cst": "dim", "hn": "lead", "cn": "lead", "dh0": "lead", "dc0": "lead"}
PADDED_ZERO = ("out", "dgates", "dgx", "dq")              # exactly 0.0 at t >= len
VALID_ONLY = ("act", "cst")                               # unspecified at t >= len: judged at valid positions only


def _dir(name, a, d, ndir):
    lay = LAYOUT.get(name)
    if lay is None:                                        # element-wise outputs of the cell kernels: one block
        return a
    if lay == "cat":
        w = a.shape[-1] // ndir
        return a[..., d * w:(d + 1) * w]
    return a[:, :, d] if lay == "dim" else a[d]


def measure(got, fig):
    """got: {output: array or None}; fig: dict(ref, y32, shifted (list of dicts, may be empty), lens or None, ndir).
    -> dict(e, e32, e_act, s, ratio of the worst output, per = {(output, dir): (e, e32, e_act, s, ratio)}, tail, finite)"""
    ref, ndir, lens = fig["ref"], fig["ndir"], fig.get("lens")
    per, tail, finite = {}, 0, True
    for k, g in got.items():
        if g is None:
            continue
        g = np.asarray(g, np.float64).reshape(ref[k].shape)
        valid = None
        if lens is not None and k in PADDED_ZERO + VALID_ONLY:
            pad = np.arange(g.shape[1])[None, :] >= lens[:, None]
            if k in PADDED_ZERO:
                tail += int(np.count_nonzero(g[pad]))
            else:
                valid = ~pad
        for d in range(ndir if k in LAYOUT else 1):
            sel = (lambda a: _dir(k, a, d, ndir)[valid]) if valid is not None else (lambda a: _dir(k, a, d, ndir))
            gd, rd = sel(g), sel(ref[k])
            if not rd.size:
                continue
            fin = bool(np.isfinite(gd).all())
            finite = finite and fin
            err = lambda a: float(np.abs(np.asarray(a, np.float64) - rd).max())
            e, e32 = err(gd) if fin else float("inf"), err(sel(np.asarray(fig["y32"][k], np.float64)))
            e_act = max([err(sel(sh[k])) for sh in fig["shifted"]] or [0.0])
            s = float(np.abs(rd).max()) or 1.0
            per[(k, d)] = (e, e32, e_act, s, (e - e_act) / max(e32, EPS * s))
    worst = max(per, key=lambda kd: per[kd][4])
    e, e32, e_act, s, ratio = per[worst]
    return dict(e=e, e32=e32, e_act=e_act, s=s, ratio=ratio, worst="%s[%d]" % worst, per=per, tail=tail, finite=finite)


def accept(got, fig, margin=None, family=None, extra=0.0):
    """(ok, figures): the criterion of the module docstring; extra: the split-fp16 format term.  margin defaults to MARGIN[family], <= the cap."""
    margin = MARGIN[family] if margin is None else margin
    assert margin <= MARGIN_CAP
    r = measure(got, fig)
    r["miss"] = max(e / (margin * max(e32, EPS * s) + e_act + extra) for e, e32, e_act, s, _ in r["per"].values())      # > 1: outside the bound
    return r["finite"] and r["tail"] == 0 and r["miss"] <= 1.0, r


# ------------------------------------------------------------------ inputs
LENGTH_MODES = ("mixed", None, "ones", "zero", "over", "neg", "wg0", "ends")


def lengths_of(spec, M, T, S=4):
    """"mixed": random in 1..T with T first and 1 last; None: NULL; "ones"; "zero" / "over" / "neg": mixed with two sequences of length 0 /
    T + 5 / -3; "wg0": the first workgroup's S sequences 0, then mixed; "ends": mixed with 0, 1 and T all present; or an explicit list"""
    if spec is None:
        return None
    if not isinstance(spec, str):
        return np.asarray(spec, np.int64)
    rng = np.random.default_rng(M * 13 + T)
    if spec == "ones":
        return np.ones(M, np.int64)
    lens = R.mixed_lengths(rng, M, T)
    if spec in ("zero", "over", "neg"):
        bad = {"zero": 0, "over": T + 5, "neg": -3}[spec]
        lens[M // 2] = bad
        lens[min(1, M - 1)] = bad
    elif spec == "wg0":
        lens[:S] = 0
    elif spec == "ends":
        lens[M // 2] = 0
        if M > 3:
            lens[1] = -1
    return lens


def make(cell, fam, seed, M, T, H, ndir=2, lengths="mixed", h0=True, c0=True, dhn=True, dcn=True, dcst=True, dout0=False, S=4):
    """One seeded case: rnn_ref.make's forward inputs ("last" uses the "randn" gates) plus the incoming gradients as float32 -- dout [M,T,ndir*H]
    ("last": nonzero only at each direction's last step of every sequence, t = len-1 forward and t = 0 reverse; dout0: all zero), dhn / dcn
    [ndir,M,H], dcst [M,T,ndir,H].  dout and dcst hold +-1e4 at t >= len: a kernel that reads them is off by far more than any bound."""
    inp = R.make("randn" if fam == "last" else fam, seed, M, T, H, ndir, 0, cell, lengths_of(lengths, M, T, S), h0 and cell == "lstm", c0)
    rng = np.random.default_rng(seed + 77)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    lens = R.clamp_lengths(inp["lengths"], M, T)
    pad = np.arange(T)[None, :] >= lens[:, None]
    sign = np.where((np.arange(M)[:, None] + np.arange(T)[None, :]) % 2 == 0, POISON, -POISON)
    dout = rng.standard_normal((M, T, ndir, H))
    if fam == "last" or dout0:
        keep = np.zeros((M, T, ndir), bool)
        if not dout0:
            live = lens > 0
            keep[np.arange(M)[live], lens[live] - 1, 0] = True
            if ndir == 2:
                keep[live, 0, 1] = True
        dout = dout * keep[..., None]
    dout[pad] = sign[pad][:, None, None]
    dc = rng.standard_normal((M, T, ndir, H))
    dc[pad] = sign[pad][:, None, None]
    inp.update(fam=fam, lens=lens, dout=f32(dout.reshape(M, T, ndir * H)), dhn=f32(rng.standard_normal((ndir, M, H))) if dhn else None,
               dcn=f32(rng.standard_normal((ndir, M, H))) if (dcn and cell == "lstm") else None,
               dcst=f32(dc) if (dcst and cell == "lstm") else None)
    return inp


def fwd_eval(inp, dt=np.float64, **kw):
    return forward(inp["cell"], inp["gin"], inp["w_hh"], inp["lengths"], inp["h0"], inp["c0"], inp["ndir"], inp.get("b_hh"), dt=dt, **kw)


def fwd_figures(inp):
    """float64 reference, fp32 yardstick and the +-DELTA evaluations of the forward of a case (cached on the case)"""
    if "_fwd" not in inp:
        inp["_fwd"] = dict(ref=fwd_eval(inp), y32=fwd_eval(inp, np.float32), shifted=[fwd_eval(inp, shift=s) for s in (DELTA, -DELTA)],
                           lens=inp["lens"], ndir=inp["ndir"])
    return inp["_fwd"]


def saved_of(inp):
    """what the BPTT kernels are handed: the float64 forward rounded to fp32, act / cst NaN at t >= len (the GRU's out stays zero there)"""
    if "_saved" not in inp:
        ref = fwd_figures(inp)["ref"]
        pad = np.arange(inp["T"])[None, :] >= inp["lens"][:, None]
        s = {k: np.ascontiguousarray(ref[k], np.float32) for k in ("out", "act") + (("cst",) if inp["cell"] == "lstm" else ())}
        for k in ("act", "cst"):
            if k in s:
                s[k][pad] = np.nan
        inp["_saved"] = s
    return inp["_saved"]


def bwd_eval(inp, dt=np.float64, saved=None, **kw):
    s = saved or saved_of(inp)
    if inp["cell"] == "lstm":
        return lstm_bwd(inp["dout"], s["act"], s["cst"], inp["w_hh"], inp["lengths"], inp["ndir"], inp["dhn"], inp["dcn"], inp["dcst"], inp["c0"], dt=dt, **kw)
    kw.pop("shift", None)
    kw.pop("noise", None)
    return gru_bwd(inp["dout"], s["act"], s["out"], inp["w_hh"], inp["lengths"], inp["ndir"], inp["dhn"], dt=dt, **kw)


def bwd_figures(inp, saved=None, key="_bwd"):
    """the same for the BPTT from the saved inputs of saved_of() (or `saved`: the chained case hands over the kernel's own forward)"""
    if key not in inp:
        sh = [bwd_eval(inp, saved=saved, shift=s) for s in (DELTA, -DELTA)] if inp["cell"] == "lstm" else []
        inp[key] = dict(ref=bwd_eval(inp, saved=saved), y32=bwd_eval(inp, np.float32, saved=saved), shifted=sh, lens=inp["lens"], ndir=inp["ndir"])
    return inp[key]


def n_split(inp):
    """split products on the path of the last state of the longest sequence: one recurrent product per step"""
    return int(inp["lens"].max()) if inp["lens"].size else 0


def to_perm(gin, ndir, H):
    """gates_in [M,T,ndir*4H] (gate-major) -> the folded order [M*T][ndir][H][4] of nir_lstm_train_fwd_split"""
    M, T, _ = gin.shape
    return np.ascontiguousarray(gin.reshape(M * T, ndir, 4, H).transpose(0, 1, 3, 2))


# ------------------------------------------------------------------ the dispatchers, restated
Pred = collections.namedtuple("Pred", "kernel inst S")     # inst: the template arguments the profile name does not carry (documented, not observed)
GRU_AUTO, GRU_VALU, GRU_MFMA = 0, 1, 2
BWD_HP = (32, 64, 72, 96, 128)


def predict_lstm_fwd(M, T, H, ndir=2):
    """nir_lstm_train_fwd (csrc/train.hip) -> launch_bilstm_mfma16 with act != NULL (csrc/lstm_mfma.hip): always from H = 33"""
    if not (M >= 0 and T > 0 and ndir in (1, 2) and 1 <= H <= 128):
        raise ValueError("bad dims")
    if M == 0:
        return None
    if H >= 33 and 16 * T * ndir * 4 * H * 4 < R.OFF_LIMIT:
        g = (H + 15) // 16
        return Pred("lstm_train_fwd_mfma16_kernel<%d,%d>" % ((3 if g == 3 else 4, 1) if H <= 64 else (g, 2)), "", 16)
    return Pred("lstm_train_fwd_kernel", "<%d>" % (32 if H <= 32 else 64 if H <= 64 else 96 if H <= 96 else 128), 4)


def predict_lstm_split(M, T, H, ndir=2):
    """nir_lstm_train_fwd_split (csrc/lstm_fold.hip launch_lstm_train_split)"""
    if not (M >= 0 and 0 < T <= 512 and ndir in (1, 2) and 64 < H <= 128):
        raise ValueError("bad dims")
    return None if M == 0 else Pred("lstm16_pt_h2_kernel<3,2,false,true>" if H <= 96 else "lstm16_pt_h2_kernel<4,4,8,false,true>", "", 16)


def bwd_mfma_supported(H):
    """nir_gru_train_mfma_supported, and the same condition inside nir_lstm_train_bwd"""
    return 16 <= H <= 128 and (H + 3) // 4 * 4 in BWD_HP


def predict_lstm_bwd(M, T, H, ndir=2):
    if not (M >= 0 and T > 0 and ndir in (1, 2) and 1 <= H <= 128):
        raise ValueError("bad dims")
    if M == 0:
        return None
    hp = (H + 3) // 4 * 4
    if bwd_mfma_supported(H) and (H % 2 == 0 or M >= 1024):
        return Pred("lstm_train_bwd_mfma_kernel", "<%d>" % hp if hp <= 64 else "<%d,1>" % hp, 16)
    return Pred("lstm_train_bwd_kernel", "", 4)


def gru_pick_form(form, M, H):
    if form != GRU_AUTO:
        return form
    return GRU_MFMA if bwd_mfma_supported(H) and (H % 2 == 0 or M >= 1024) else GRU_VALU


def predict_gru_fwd(M, T, H, ndir=2):
    if not (M >= 0 and T > 0 and ndir in (1, 2) and 1 <= H <= 128):
        raise ValueError("bad dims")
    return None if M == 0 else Pred("gru_train_fwd_kernel", "<%d>" % (32 if H <= 32 else 64 if H <= 64 else 96 if H <= 96 else 128), 4)


def predict_gru_bwd(M, T, H, ndir=2, form=GRU_AUTO):
    if not (M >= 0 and T > 0 and ndir in (1, 2) and 1 <= H <= 128 and form in (GRU_AUTO, GRU_VALU, GRU_MFMA)):
        raise ValueError("bad dims")
    if form == GRU_MFMA and not bwd_mfma_supported(H):
        raise ValueError("the matrix-core form does not take H = %d" % H)
    if M == 0:
        return None
    if gru_pick_form(form, M, H) == GRU_MFMA:
        return Pred("gru_train_bwd_mfma_kernel", "<%d>" % ((H + 3) // 4 * 4), 16)
    return Pred("gru_train_bwd_kernel", "", 4)
