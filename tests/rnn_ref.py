"""The acceptance criterion of the eval-mode recurrences behind nir_bilstm_fwd, nir_bilstm_fused_fwd, nir_bilstm_steps_fwd and
nir_birnn_steps_fwd: float64 references of the whole operation (numpy), the bound a kernel's result has to meet, seeded input families,
fp32 emulations and mutants of the recurrence (the CPU evidence that the bound has teeth) and a restatement of the dispatchers of
csrc/lstm.hip and csrc/lstm_mfma.hip (which kernel, how many sequences per workgroup) that the case tables are built with.

Semantics (include/neuroir_hip.h): gates_in [M,T,ndir*4H] = x W_ih^T + b_ih + b_hh, gate order i,f,g,o, forward direction first; lengths are
clamped to [0, T]; the reverse direction walks t = len-1 .. 0; out is zero at t >= len; hn / cn are the state after the last valid step (the
initial state for len = 0); h0 / c0 optional and independent.  GRU (torch.nn.GRU): gate order r,z,n, gates_in carries b_ih, b_hh sits inside the
reset product, n = tanh(gin_n + r (W_hn h + b_hn)).

Bound: with e = max |got - ref64| over out, hn, cn (and the per-step cell states where asked for), absolute -- the outputs are bounded by 1
and the cell state by the sequence length, so no scale is divided out --

    e <= margin * max(e32, 2^-23) + e_act        and out == 0.0 exactly at t >= len

e32:   the error of a plain fp32 evaluation of the same recurrence on the same inputs (numpy float32, exact exp / tanh, the default dot order;
       the fused form starts from x and includes the input projection).
e_act: what the fast activations may cost: the larger deviation of the float64 recurrence from itself when EVERY sigmoid and tanh output is
       shifted by +DELTA and by -DELTA, DELTA = 2e-7 (the convention of gemm_ref.act_term: twice the ~1e-7 documented for fast_tanh in
       csrc/common.hpp).  fast_sigmoid(x) = v_rcp_f32(1 + v_exp_f32(-x log2 e)) is under the same figure.  With u = exp(-x) and
       sigma = 1 / (1 + u), a relative error r of u moves sigma by r u / (1 + u)^2 = r sigma (1 - sigma) <= r / 4:
         v_exp_f32, 1 ulp: r = 2^-23                                                            -> 3.0e-8
         the fp32 product x log2(e) is rounded: r = 2^-24 |x|, and |x| sigma (1 - sigma) <= 0.23    -> 1.4e-8
         the sum 1 + u is rounded (2^-24 relative, times sigma <= 1)                            -> 6.0e-8
         v_rcp_f32, 1 ulp of a result in [1/2, 1)                                               -> 6.0e-8
       together 1.6e-7 < DELTA.  Measured through every kernel template (test_activation_accuracy): sigmoid 9.4e-8, tanh 1.2e-7.
margin: per kernel family, from the largest measured (e - e_act) / max(e32, 2^-23) over the family's cases on the MI355X, doubled and
       rounded up, never above gemm_ref.MARGIN_CAP = 4 (accept() asserts it).  Measured: the ratio is NEGATIVE in all 359 cases of every
       family (largest -1.37, lstm_mfma_kernel and lstm_mfma16_kernel): no kernel's error reaches e_act alone (e <= 0.38 e_act), and
       e <= 1.98 max(e32, 2^-23) -- the kernels err like a plain fp32 evaluation, their activations well inside DELTA.  The rule then gives
       no positive number; 1 is used, the smallest margin that still means "an fp32 evaluation" (DESIGN.md section 2 has the figures).

The "remember" family (forget gate ~ 1) makes e_act itself large over long T (the shift accumulates in c): it tests state carry, not
precision; precision mutants are judged on "randn" and "sat" (tests/test_rnn_criterion_host.py)."""
import collections

import numpy as np

import gemm_ref as G

DELTA = 2e-7
EPS = 2.0 ** -23
MARGIN_CAP = G.MARGIN_CAP
# kernel family -> margin (see the module docstring; the figures are in DESIGN.md section 2)
MARGIN = {"rec": 1.0, "rec_fused": 1.0, "mfma_gin": 1.0, "mfma16_gin": 1.0, "mfma": 1.0, "mfma16": 1.0, "steps_lstm": 1.0, "steps_gru": 1.0}
POISON = 1e4


def family_of(kernel):
    base = kernel.split("<")[0]
    return {"lstm_rec_kernel": "rec", "lstm_rec_kernel[fused]": "rec_fused", "lstm_mfma_gin_kernel": "mfma_gin",
            "lstm_mfma16_gin_kernel": "mfma16_gin", "lstm_mfma_kernel": "mfma", "lstm_mfma16_kernel": "mfma16",
            "lstm_step_cell_kernel": "steps_lstm", "gru_step_cell_kernel": "steps_gru"}[base]


# ------------------------------------------------------------------ the recurrence, in any precision, faithful or mutated
def _dot(h, W, order, dt):
    """h [M,H] W^T [H,N] in dtype dt.  "blas": numpy's matmul; "seq": one accumulator, k ascending; "quad": the quad kernel of csrc/lstm.hip --
    four sequential partial sums over the quarters of K padded to a multiple of 16, combined as (p0 + p1) + (p2 + p3)."""
    if order == "blas":
        return h @ W.T
    M, H = h.shape
    if order == "seq":
        acc = np.zeros((M, W.shape[0]), dt)
        for k in range(H):
            acc = acc + h[:, k:k + 1] * W[None, :, k]
        return acc
    KQ = (H + 15) // 16 * 4
    part = []
    for q in range(4):
        acc = np.zeros((M, W.shape[0]), dt)
        for k in range(q * KQ, min((q + 1) * KQ, H)):
            acc = acc + h[:, k:k + 1] * W[None, :, k]
        part.append(acc)
    return (part[0] + part[1]) + (part[2] + part[3])


def clamp_lengths(lengths, M, T):
    return np.full(M, T, np.int64) if lengths is None else np.clip(np.asarray(lengths, np.int64), 0, T)


def run(cell, gin, w_hh, lengths=None, h0=None, c0=None, ndir=2, b_hh=None, dt=np.float64, shift=0.0, noise=None, order="blas", mut=None):
    """The recurrence over gates_in -> dict(out, hn, cn, cst) in dtype dt.  shift: added to every sigmoid / tanh output; noise: a
    numpy Generator -> +-1e-7 with a random sign on every activation output; order: see _dot; mut: one of MUTANTS (None = faithful)."""
    one = dt(1.0)
    gin = np.asarray(gin, dt)
    M, T, _ = gin.shape
    NG = 4 if cell == "lstm" else 3
    H = gin.shape[2] // (ndir * NG)
    assert gin.shape[2] == ndir * NG * H
    w = np.asarray(w_hh, dt).reshape(ndir, NG * H, H)
    lens = clamp_lengths(lengths, M, T)
    if mut == "nbr_len":                                   # one sequence walks with its neighbour's length
        m = next(i for i in range(M) if lens[i] != lens[(i + 1) % M])
        lens = lens.copy()
        lens[m] = lens[(m + 1) % M]
    out = np.zeros((M, T, ndir * H), dt)
    cst = np.zeros((M, T, ndir * H), dt)
    hn = np.zeros((ndir, M, H), dt)
    cn = np.zeros((ndir, M, H), dt)
    rows = np.arange(M)

    def jit(v):
        if shift:
            v = v + dt(shift)
        if noise is not None:
            v = v + (noise.integers(0, 2, v.shape) * 2 - 1).astype(dt) * dt(1e-7)
        return v

    sig = lambda v: jit(one / (one + np.exp(-v)))
    tanh = lambda v: jit(np.tanh(v))
    with np.errstate(over="ignore"):
        for d in range(ndir):
            h = np.zeros((M, H), dt) if h0 is None or mut == "no_h0" else np.asarray(h0, dt).reshape(ndir, M, H)[d].copy()
            c = np.zeros((M, H), dt) if c0 is None or mut == "no_c0" else np.asarray(c0, dt).reshape(ndir, M, H)[d].copy()
            W = w[d]
            if mut == "drop_col":                          # the last k of the recurrent product lost (the padding edge of K)
                W = W.copy()
                W[:, H - 1] = 0
            nsteps = T if mut == "final_T" else int(lens.max()) if M else 0
            for step in range(nsteps):
                if d == 0:
                    t = np.full(M, step, np.int64)
                else:
                    t = (T - 1 - step) if mut == "rev_T" else (lens - 1 - step)
                    t = np.broadcast_to(t, (M,))
                live = step < lens
                tc = np.clip(t, 0, T - 1)
                g = gin[rows, tc, d * NG * H:(d + 1) * NG * H]
                hw = _dot(h, W, order, dt)
                if cell == "lstm":
                    a = g + hw
                    gi, gf, gg, go = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
                    if mut == "swap_fg":
                        gf, gg = gg, gf
                    c2 = sig(gf) * c + sig(gi) * tanh(gg)
                    h2 = sig(go) * tanh(c2)
                else:
                    bh = np.asarray(b_hh, dt).reshape(ndir, 3 * H)[d]
                    r = sig(g[:, :H] + (hw[:, :H] + bh[:H]))
                    z = sig(g[:, H:2 * H] + (hw[:, H:2 * H] + bh[H:2 * H]))
                    if mut == "bhh_outside":
                        n = tanh(g[:, 2 * H:] + r * hw[:, 2 * H:] + bh[2 * H:])
                    else:
                        n = tanh(g[:, 2 * H:] + r * (hw[:, 2 * H:] + bh[2 * H:]))
                    h2 = (one - z) * n + z * h
                    c2 = c
                if mut == "h16":                           # the state rounded to fp16 between steps
                    h2 = h2.astype(np.float16).astype(dt)
                upd = np.ones(M, bool) if mut == "final_T" else live      # final_T: the state keeps moving after the last valid step
                h = np.where(upd[:, None], h2, h)
                c = np.where(upd[:, None], c2, c)
                lr = rows[live]
                out[lr, tc[live], d * H:(d + 1) * H] = h2[live]
                cst[lr, tc[live], d * H:(d + 1) * H] = c2[live]
            hn[d], cn[d] = h, c
    return dict(out=out, hn=hn, cn=cn, cst=cst)


MUTANTS_LSTM = ("h16", "shift3", "rev_T", "final_T", "no_h0", "no_c0", "swap_fg", "drop_col", "nbr_len")
MUTANTS_GRU = ("h16", "shift3", "rev_T", "final_T", "no_h0", "drop_col", "nbr_len", "bhh_outside")
PRECISION_MUTANTS = ("h16", "shift3")


def gates_of(inp, dt=np.float64):
    """gates_in of a case in dtype dt; the fused form projects x first (the whole chain in dt)."""
    if inp.get("x") is None:
        return np.asarray(inp["gin"], dt)
    x, wih = np.asarray(inp["x"], dt), np.asarray(inp["w_ih"], dt)
    return x @ wih.T + np.asarray(inp["b_ih"], dt) + np.asarray(inp["b_hh_in"], dt)


def evaluate(inp, dt=np.float64, **kw):
    """run() on a case dict (make()); mut "shift3" is the uniform activation shift of 3 DELTA"""
    if kw.get("mut") == "shift3":
        kw = dict(kw, mut=None, shift=3 * DELTA)
    return run(inp["cell"], gates_of(inp, dt), inp["w_hh"], inp["lengths"], inp["h0"], inp["c0"], inp["ndir"], inp.get("b_hh"), dt=dt, **kw)


def lstm_ref(gates_in, w_hh, lengths=None, h0=None, c0=None, ndir=2):
    return run("lstm", gates_in, w_hh, lengths, h0, c0, ndir)


def gru_ref(gates_in, w_hh, b_hh, lengths=None, h0=None, ndir=2):
    return run("gru", gates_in, w_hh, lengths, h0, None, ndir, b_hh=b_hh)


def fused_ref(x, w_ih, b_ih, b_hh, w_hh, lengths=None, h0=None, c0=None, ndir=2):
    return evaluate(dict(cell="lstm", x=x, w_ih=w_ih, b_ih=b_ih, b_hh_in=b_hh, w_hh=w_hh, lengths=lengths, h0=h0, c0=c0, ndir=ndir))


# ------------------------------------------------------------------ criterion
def _keys(inp, got):
    keys = ["out", "hn"] + (["cn"] if inp["cell"] == "lstm" else [])
    return [k for k in keys + ["cst"] if got.get(k) is not None]


def _err(got, ref, keys):
    return max(float(np.abs(np.asarray(got[k], np.float64) - ref[k]).max()) if ref[k].size else 0.0 for k in keys)


def figures(inp, keys=("out", "hn", "cn")):
    """dict(ref, e32, e_act) of a case over the outputs `keys` (those the result under judgement has), computed once per key set"""
    cache = inp.get("_fig") or {}
    inp["_fig"] = cache
    if "ref" not in cache:
        cache["ref"] = evaluate(inp)
    keys = tuple(k for k in ("out", "hn", "cn", "cst") if k in keys and (k != "cn" or inp["cell"] == "lstm"))
    if keys not in cache:
        ref = cache["ref"]
        cache[keys] = dict(ref=ref, e32=_err(evaluate(inp, np.float32), ref, keys),
                           e_act=max(_err(evaluate(inp, shift=s), ref, keys) for s in (DELTA, -DELTA)))
    return cache[keys]


def measure(got, inp):
    """got: dict with out and any of hn, cn, cst (None = not produced).  -> dict(e, e32, e_act, ratio, tail, finite)"""
    keys = _keys(inp, got)
    f = figures(inp, keys)
    finite = all(bool(np.isfinite(np.asarray(got[k])).all()) for k in keys)
    M, T = np.asarray(got["out"]).shape[:2]
    pad = np.arange(T)[None, :] >= clamp_lengths(inp["lengths"], M, T)[:, None]
    tail = sum(int(np.count_nonzero(np.asarray(got[k])[pad])) for k in ("out", "cst") if got.get(k) is not None)
    e = _err(got, f["ref"], keys) if finite else float("inf")
    return dict(e=e, e32=f["e32"], e_act=f["e_act"], ratio=(e - f["e_act"]) / max(f["e32"], EPS), tail=tail, finite=finite)


def accept(got, inp, margin=None, family=None):
    """(ok, figures): the criterion of the module docstring.  margin defaults to MARGIN[family] and may never exceed MARGIN_CAP."""
    margin = MARGIN[family] if margin is None else margin
    assert margin <= MARGIN_CAP
    r = measure(got, inp)
    r["bound"] = margin * max(r["e32"], EPS) + r["e_act"]
    return r["finite"] and r["tail"] == 0 and r["e"] <= r["bound"], r


# ------------------------------------------------------------------ inputs
def mixed_lengths(rng, M, T):
    """random lengths in 1..T that include T (first) and 1 (last)"""
    lens = rng.integers(1, T + 1, M)
    lens[0] = T
    if M > 1:
        lens[-1] = 1
    return lens.astype(np.int64)


def make(fam, seed, M, T, H, ndir=2, I=0, cell="lstm", lengths="mixed", h0=True, c0=True):
    """One seeded case as float32 arrays: gin [M,T,ndir*NG*H] (I == 0) or x [M,T,I], w_ih, b_ih, b_hh_in (I > 0: the fused entry), w_hh
    uniform in +-1/sqrt(H), b_hh (GRU), lengths (None, "mixed" or a sequence), h0 / c0 [ndir,M,H] or None.  Families: "randn" unit-normal
    gates; "sat" gates scaled 3x; "remember" forget-gate bias +4; "tiny" gates scaled 2^-10.  Padded positions (t >= len) of
    gin / x hold +-1e4: a reference never reads them, a kernel that does is off by far more than any bound."""
    rng = np.random.default_rng(seed)
    NG = 4 if cell == "lstm" else 3
    scale = {"randn": 1.0, "sat": 3.0, "remember": 1.0, "tiny": 2.0 ** -10}[fam]
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    k = 1.0 / np.sqrt(H)
    inp = dict(cell=cell, ndir=ndir, fam=fam, M=M, T=T, H=H, I=I, gin=None, x=None)
    inp["w_hh"] = f32(rng.uniform(-k, k, (ndir, NG * H, H)))
    if cell == "gru":
        inp["b_hh"] = f32(rng.uniform(-k, k, (ndir, 3 * H)))
    if lengths is None:
        inp["lengths"] = None
    elif isinstance(lengths, str):
        inp["lengths"] = mixed_lengths(rng, M, T)
    else:
        inp["lengths"] = np.asarray(lengths, np.int64)
        assert inp["lengths"].shape == (M,)
    lens = clamp_lengths(inp["lengths"], M, T)
    pad = np.arange(T)[None, :] >= lens[:, None]
    sign = np.where((np.arange(M)[:, None] + np.arange(T)[None, :]) % 2 == 0, POISON, -POISON)
    if I:
        x = rng.standard_normal((M, T, I)) * scale
        x[pad] = sign[pad][:, None]
        inp["x"] = f32(x)
        inp["w_ih"] = f32(rng.uniform(-1, 1, (ndir * 4 * H, I)) * np.sqrt(3.0 / I))
        b = rng.uniform(-k, k, (ndir, 4, H)) * scale
        if fam == "remember":
            b[:, 1] += 4.0
        inp["b_ih"] = f32(b.reshape(-1))
        inp["b_hh_in"] = f32(rng.uniform(-k, k, ndir * 4 * H) * scale)
    else:
        g = rng.standard_normal((M, T, ndir, NG, H)) * scale
        if fam == "remember":
            g[:, :, :, 1] += 4.0
        g[pad] = sign[pad][:, None, None, None]
        inp["gin"] = f32(g.reshape(M, T, ndir * NG * H))
    inp["h0"] = f32(rng.uniform(-1, 1, (ndir, M, H))) if h0 else None
    inp["c0"] = f32(rng.standard_normal((ndir, M, H))) if (c0 and cell == "lstm") else None
    return inp


# ------------------------------------------------------------------ the dispatchers of csrc/lstm.hip and csrc/lstm_mfma.hip, restated
Pred = collections.namedtuple("Pred", "kernel S IP")       # S: sequences per workgroup; IP: padded input width of the fused VALU kernel
OFF_LIMIT = 0x7FFFFFF0
MFMA_TABLE = [(1, 8), (1, 12), (1, 16), (1, 20), (2, 12), (2, 16), (2, 20), (2, 24), (3, 16), (3, 20), (3, 24), (3, 28),
              (4, 20), (4, 24), (4, 28), (4, 32), (5, 24), (5, 28), (5, 32), (5, 36)]
REC_KP = (16, 32, 48, 64, 80, 96, 112, 128)
TUNABLES = {"lstm_mfma16": -1, "lstm_s": 0}


def pick_s(seqdirs, fused, lstm_s=0):
    best, best_cost = 1, 1e30
    for S in (1, 2, 3, 4, 8):
        if fused and S > 4:
            continue
        wgs = (seqdirs + S - 1) // S
        slots = 256 * (2 if S == 1 else 1)
        cost = float((wgs + slots - 1) // slots) * (0.85 + 0.29 * S)
        if cost < best_cost - 1e-9:
            best_cost, best = cost, S
    if lstm_s in (1, 2, 3, 4, 8):
        best = lstm_s
    if fused and best > 4:
        best = 4
    return best


def predict(entry, M, T, H, I=0, ndir=2, tunables=None, batches_in_flight=1):
    """The kernel nir_bilstm_fwd (entry "fwd") / nir_bilstm_fused_fwd ("fused") launches, named as the profile report prints it (without
    the [M=,N=,K=] part), with the sequences per workgroup (not in the name: documented, not observed).  ValueError where the entry
    refuses the arguments; None for the M == 0 early return."""
    tn = dict(TUNABLES, **(tunables or {}))
    f16, ls = tn["lstm_mfma16"], tn["lstm_s"]
    if not (M >= 0 and T > 0 and ndir in (1, 2)):
        raise ValueError("bad dims")
    KP = (H + 15) // 16 * 16
    if entry == "fwd":
        if not 1 <= H <= 128:
            raise ValueError("hidden size")
        if 8 * T * ndir * 4 * H * 4 >= OFF_LIMIT:
            raise ValueError("32-bit tile offsets")
        if M == 0:
            return None
        if (f16 != 0 if f16 >= 0 else ((M + 15) // 16) * ndir >= 128) and 33 <= H <= 128 and 16 * T * ndir * 4 * H * 4 < OFF_LIMIT:
            g = (H + 15) // 16
            return Pred("lstm_mfma16_gin_kernel<%d,%d>" % ((3 if g == 3 else 4, 1) if H <= 64 else (g, 2)), 16, 0)
        if ((H + 15) // 16) % 4 != 0 and H >= 17 and 4 * T * ndir * 4 * H * 4 < OFF_LIMIT:
            return Pred("lstm_mfma_gin_kernel<%s>" % ("4,16,1" if H <= 64 else "3,24,2" if H <= 96 else "4,32,2"), 4, 0)
        return Pred("lstm_rec_kernel<%d>" % KP, pick_s(M * ndir, False, ls), 0)
    assert entry == "fused"
    if not (1 <= H <= 128 and 1 <= I <= 64):
        raise ValueError("H / I")
    if M == 0:
        return None
    if 4 * T * max(I, ndir * H) * 4 < OFF_LIMIT:
        if (f16 != 0 if f16 >= 0 else ((M + 15) // 16) * ndir >= 160) and 16 * T * max(I, ndir * H) * 4 < OFF_LIMIT and (H + I + 15) // 16 <= 10:
            return Pred("lstm_mfma16_kernel<%d,%d>" % ((H + I + 15) // 16, 2 if (H + 3) // 4 > 16 else 1), 16, 0)
        NG, KQ = (4 * H + 63) // 64, (H + I + 15) // 16 * 4
        if (NG, KQ) in MFMA_TABLE:
            if NG <= 4 and 4 * H <= 256:
                return Pred("lstm_mfma_kernel<%d,%d,4,1>" % (NG, KQ), 4, 0)
            three = False
            if batches_in_flight <= 1:
                wg4, wg3 = ((M + 3) // 4) * ndir, ((M + 2) // 3) * ndir
                three = float((wg3 + 255) // 256) * 0.85 < float((wg4 + 255) // 256)
            return Pred("lstm_mfma_kernel<%d,%d,%s>" % (NG, KQ, "3,1" if three else "4,2"), 3 if three else 4, 0)
    S = pick_s(M * ndir, True, ls)
    IP = 48 if I <= 48 else 64
    while S > 1 and S * T * IP * 4 > 96 * 1024:
        S >>= 1
    if S * T * IP * 4 > 140 * 1024:
        raise ValueError("LDS x tile")
    return Pred("lstm_rec_kernel[fused]<%d>" % KP, S, IP)


def compiled():
    """Every (kernel name, S, IP) the two source files instantiate for the eval-mode entries (launch_kp / launch_s, the NIR_MFMA_CASE and
    NIR_M16_CASE lists, launch_bilstm_mfma, launch_bilstm_mfma16)."""
    out = set()
    for kp in REC_KP:
        out |= {Pred("lstm_rec_kernel<%d>" % kp, s, 0) for s in (1, 2, 3, 4, 8)}
        out |= {Pred("lstm_rec_kernel[fused]<%d>" % kp, s, ip) for s in (1, 2, 3, 4) for ip in (48, 64)}
    out |= {Pred("lstm_mfma_gin_kernel<%s>" % a, 4, 0) for a in ("4,16,1", "3,24,2", "4,32,2")}
    out |= {Pred("lstm_mfma16_gin_kernel<%d,%d>" % a, 16, 0) for a in ((3, 1), (4, 1), (5, 2), (6, 2), (7, 2), (8, 2))}
    for ng, kq in MFMA_TABLE:
        forms = ((3, 1), (4, 2)) + (((4, 1),) if ng <= 4 else ())
        out |= {Pred("lstm_mfma_kernel<%d,%d,%d,%d>" % (ng, kq, s, tpt), s, 0) for s, tpt in forms}
    out |= {Pred("lstm_mfma16_kernel<%d,%d>" % (g, nt), 16, 0) for g in range(1, 11) for nt in (1, 2)}
    return out


def predict_linear(M, N, K, vec=True):
    """launch_linear_ex (csrc/gemm.hip) for a dense, un-gathered call without epilogue: the step GEMM of the streaming recurrences"""
    cd = lambda a, b: (a + b - 1) // b
    if vec and N >= 96 and K >= 32 and cd(M, 128) * cd(N, 128) >= 96:
        return "gemm3_kernel"
    if N <= 64 and vec and M >= 4096 and 16 * cd(N, 16) * (cd(K, 16) * 16 + 4) * 4 <= 128 * 1024:
        return "gemm_skinny_kernel"
    if cd(M, 64) * cd(N, 64) < 160:
        return "gemm32_kernel" if vec and K % 16 == 0 and cd(M, 32) * cd(N, 32) >= 200 else "gemm16_kernel"
    return "gemm_kernel"


FP32_GEMMS = ("gemm_kernel", "gemm16_kernel", "gemm32_kernel")


def predict_steps(cell, M, T, H, ndir, has_h0):
    """[(name, launches)] of nir_birnn_steps_fwd in the order of the profile report (sorted by name): T cell launches per direction and the
    step GEMM h W_hh^T (skipped at the first step of a zero initial state).  The state of direction 1 starts 6 M H floats into the
    workspace and its weights G H H floats into w_hh: 16-byte alignment (the vectorised loads) follows from M, H."""
    Gn = 3 if cell == "gru" else 4
    names = collections.Counter()
    for d in range(ndir):
        vec = H % 4 == 0 and (d * 6 * M * H) % 4 == 0 and (d * Gn * H * H) % 4 == 0
        n = T - (0 if has_h0 else 1)
        if n > 0:
            names[predict_linear(M, Gn * H, H, vec)] += n
    names["gru_step_cell_kernel" if cell == "gru" else "lstm_step_cell_kernel"] += T * ndir
    return sorted(names.items())
