"""GPU (-m gpu): every dispatch path of the in-kernel recurrences (nir_bilstm_fwd, nir_bilstm_fused_fwd: csrc/lstm.hip, csrc/lstm_mfma.hip)
and the streaming ones (nir_bilstm_steps_fwd, nir_birnn_steps_fwd: csrc/mnsrf.hip), called through the C ABI, against float64.  Each case
asserts three things:
  * the profile report names exactly the kernel tests/rnn_ref.py predicts, once per call (the streaming entries: the cell kernel T times per
    direction and the step GEMM, an fp32-form kernel) -- a shape that lands elsewhere is moved, not the assertion;
  * the result meets the criterion of tests/rnn_ref.py (the error of a plain fp32 evaluation times a margin <= 4, plus what the fast
    activations may cost), out is exactly zero at padded positions, a sequence of length 0 returns its initial state bit for bit;
  * out, hn, cn (and the workspace of the streaming entries) sit between guard regions that are intact afterwards, and are prefilled with
    NaN: an element the kernel forgot fails the criterion.
The kernel's name does not carry the sequences per workgroup S (nor the padded input width of the fused VALU kernel): the tables state the S
the dispatcher's restatement gives, tests/test_rnn_criterion_host.py checks tables and restatement against each other on the CPU.
Every case prints one "RNNENV" line with its figures before it asserts (pytest -s); DESIGN.md section 2 quotes the largest per family."""
import contextlib
import ctypes as C
import re

import numpy as np
import pytest
import torch

import rnn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0
GUARD = 64            # floats in front of and behind every output
WS_GUARD = 256        # bytes behind the streaming workspace
FIGURES = []


def c(kernel, S, entry, M, T, H, I=0, fam="randn", ndir=2, lens="mixed", h0=True, c0=True, hn=True, cn=True, tun=None, bif=0, cst=False, tag=""):
    """One case.  entry: "fwd" / "fused" (kernel, S: what rnn_ref.predict gives), "steps" (nir_bilstm_steps_fwd), "birnn_lstm" / "birnn_gru"
    (nir_birnn_steps_fwd; kernel = the cell kernel).  lens: "mixed" (random, with T first and 1 last), None (NULL), "ones", "wg1" (the first
    workgroup's S sequences 1, the others T), "zero" / "over" (mixed with two sequences of length 0 / T + 5) or a list.  h0 / c0: given or
    NULL; hn / cn: asked for or NULL; tun: tunables; bif: batches-in-flight hint (0 = none); cst: per-step cell states (birnn_lstm)."""
    d = dict(kernel=kernel, S=S, entry=entry, M=M, T=T, H=H, I=I, fam=fam, ndir=ndir, lens=lens, h0=h0, c0=c0, hn=hn, cn=cn, tun=tun or {},
             bif=bif, cst=cst)
    tags = [entry, kernel, "S%s" % S, "M%dT%dH%d" % (M, T, H)] + (["I%d" % I] if I else []) + ([fam] if fam != "randn" else [])
    tags += ["ndir1"] * (ndir == 1) + (["lens=%s" % (lens if isinstance(lens, (str, type(None))) else "list")] if lens != "mixed" else [])
    tags += ["no-h0"] * (not h0) + ["no-c0"] * (not c0) + ["no-hn"] * (not hn) + ["no-cn"] * (not cn) + ["cst"] * cst
    tags += ["%s=%d" % kv for kv in sorted(d["tun"].items())] + (["bif%d" % bif] if bif else []) + ([tag] if tag else [])
    d["id"] = "-".join(tags)
    return d


F16 = {"lstm_mfma16": 1}
REC, RECF, GIN, GIN16, MF, MF16 = ("lstm_rec_kernel<%d>", "lstm_rec_kernel[fused]<%d>", "lstm_mfma_gin_kernel<%s>", "lstm_mfma16_gin_kernel<%d,%d>",
                                   "lstm_mfma_kernel<%d,%d,%d,%d>", "lstm_mfma16_kernel<%d,%d>")

# ---- every (kernel, S) the dispatchers reach on their own: ragged M, mixed lengths with 1 and T, both directions -- and the thresholds from
# both sides: H 16/17, 32/33, 48/49, 64/65, 96/97, 112/113, 128; ceil(M/16) ndir 127/128 (unfused) and 159/160 (fused); H + I at 160;
# I 48/49/64; 4H 256/257; the 3- / 4-sequence choice of launch_mfma
DISPATCH = [
    # unfused VALU kernel: KP = 16, 64, 128 with S = 1, 3, 4, 8 from pick_s (M ndir in 1..512, 513..768, 769..1024, 1537..2048)
    c(REC % 16, 1, "fwd", 7, 6, 16), c(REC % 16, 1, "fwd", 5, 9, 1), c(REC % 16, 3, "fwd", 262, 6, 15), c(REC % 16, 4, "fwd", 390, 6, 16),
    c(REC % 16, 8, "fwd", 771, 6, 9),
    c(REC % 64, 1, "fwd", 7, 11, 64), c(REC % 64, 3, "fwd", 262, 6, 49), c(REC % 64, 4, "fwd", 390, 6, 64), c(REC % 64, 8, "fwd", 771, 5, 50),
    c(REC % 128, 1, "fwd", 9, 12, 128), c(REC % 128, 3, "fwd", 262, 5, 113), c(REC % 128, 4, "fwd", 390, 5, 128),
    c(REC % 128, 8, "fwd", 771, 5, 120),
    # 4x4x1-MFMA kernel, gates from memory: the unbalanced sizes
    c(GIN % "4,16,1", 4, "fwd", 7, 9, 17), c(GIN % "4,16,1", 4, "fwd", 10, 7, 32), c(GIN % "4,16,1", 4, "fwd", 6, 8, 33),
    c(GIN % "4,16,1", 4, "fwd", 10, 7, 48), c(GIN % "3,24,2", 4, "fwd", 7, 9, 65), c(GIN % "3,24,2", 4, "fwd", 33, 20, 70),
    c(GIN % "3,24,2", 4, "fwd", 10, 7, 96), c(GIN % "4,32,2", 4, "fwd", 6, 8, 97), c(GIN % "4,32,2", 4, "fwd", 10, 7, 112),
    c(GIN % "4,16,1", 4, "fwd", 1011, 4, 32), c(GIN % "3,24,2", 4, "fwd", 1008, 4, 70),
    # 16-sequence MFMA kernel, gates from memory: from ceil(M/16) ndir = 128
    c(GIN16 % (3, 1), 16, "fwd", 1011, 4, 33), c(GIN16 % (3, 1), 16, "fwd", 1011, 4, 48), c(GIN16 % (4, 1), 16, "fwd", 1011, 4, 49),
    c(GIN16 % (4, 1), 16, "fwd", 1011, 4, 64), c(GIN16 % (5, 2), 16, "fwd", 1011, 4, 65), c(GIN16 % (5, 2), 16, "fwd", 1011, 4, 80),
    c(GIN16 % (6, 2), 16, "fwd", 1011, 4, 81), c(GIN16 % (6, 2), 16, "fwd", 1011, 4, 96), c(GIN16 % (7, 2), 16, "fwd", 1011, 4, 97),
    c(GIN16 % (7, 2), 16, "fwd", 1011, 4, 112), c(GIN16 % (8, 2), 16, "fwd", 1011, 4, 113), c(GIN16 % (8, 2), 16, "fwd", 1011, 4, 128),
    c(REC % 128, 8, "fwd", 1008, 4, 128), c(REC % 128, 8, "fwd", 2032, 3, 128, ndir=1), c(GIN16 % (8, 2), 16, "fwd", 2033, 3, 128, ndir=1),
    c(REC % 64, 8, "fwd", 2032, 3, 64, ndir=1), c(GIN16 % (4, 1), 16, "fwd", 2033, 3, 64, ndir=1),
    # 4x4x1-MFMA kernel, input projection fused: the (NG, KQ) table; NG <= 4 always 4 sequences and one cell task per thread, NG = 5 three
    # sequences (one batch in flight, few workgroups) or four with two tasks
    c(MF % (1, 8, 4, 1), 4, "fused", 11, 7, 16, 16), c(MF % (1, 8, 4, 1), 4, "fused", 6, 7, 1, 16), c(MF % (1, 12, 4, 1), 4, "fused", 11, 7, 16, 32),
    c(MF % (1, 16, 4, 1), 4, "fused", 11, 7, 5, 59), c(MF % (1, 20, 4, 1), 4, "fused", 11, 7, 16, 64),
    c(MF % (2, 12, 4, 1), 4, "fused", 11, 7, 17, 16), c(MF % (2, 16, 4, 1), 4, "fused", 11, 7, 32, 32), c(MF % (2, 20, 4, 1), 4, "fused", 11, 7, 32, 48),
    c(MF % (2, 24, 4, 1), 4, "fused", 11, 7, 32, 64),
    c(MF % (3, 16, 4, 1), 4, "fused", 11, 7, 48, 16), c(MF % (3, 20, 4, 1), 4, "fused", 11, 7, 40, 40), c(MF % (3, 24, 4, 1), 4, "fused", 11, 7, 33, 63),
    c(MF % (3, 28, 4, 1), 4, "fused", 11, 7, 48, 64),
    c(MF % (4, 20, 4, 1), 4, "fused", 11, 7, 64, 16), c(MF % (4, 24, 4, 1), 4, "fused", 11, 7, 49, 47), c(MF % (4, 28, 4, 1), 4, "fused", 11, 7, 64, 48),
    c(MF % (4, 32, 4, 1), 4, "fused", 11, 7, 64, 64), c(MF % (4, 32, 4, 1), 4, "fused", 11, 7, 64, 49, bif=4),
    c(MF % (5, 24, 3, 1), 3, "fused", 11, 7, 65, 16), c(MF % (5, 28, 3, 1), 3, "fused", 34, 20, 70, 40), c(MF % (5, 32, 3, 1), 3, "fused", 11, 7, 80, 48),
    c(MF % (5, 36, 3, 1), 3, "fused", 11, 7, 80, 64),
    c(MF % (5, 24, 4, 2), 4, "fused", 11, 7, 80, 16, bif=4), c(MF % (5, 28, 4, 2), 4, "fused", 33, 20, 70, 40, bif=4),
    c(MF % (5, 32, 4, 2), 4, "fused", 11, 7, 65, 49, bif=4), c(MF % (5, 36, 4, 2), 4, "fused", 11, 7, 80, 64, bif=4),
    c(MF % (5, 28, 3, 1), 3, "fused", 384, 4, 70, 40), c(MF % (5, 28, 4, 2), 4, "fused", 385, 4, 70, 40), c(MF % (5, 28, 4, 2), 4, "fused", 2544, 3, 70, 40, ndir=1),
    # fused VALU kernel: H + I <= KP below the table, every H above 80, H + I > 160; S = 1, 3, 4 from pick_s, 2 once T outgrows the LDS x tile
    c(RECF % 16, 1, "fused", 7, 6, 8, 8), c(RECF % 16, 1, "fused", 3, 4, 1, 1), c(RECF % 16, 1, "fused", 7, 6, 15, 1),
    c(RECF % 32, 1, "fused", 7, 6, 17, 15), c(RECF % 32, 3, "fused", 262, 5, 20, 5), c(RECF % 48, 1, "fused", 7, 6, 33, 15),
    c(RECF % 64, 1, "fused", 7, 6, 49, 15), c(RECF % 64, 4, "fused", 390, 5, 60, 4), c(RECF % 80, 1, "fused", 7, 6, 65, 15),
    c(RECF % 96, 1, "fused", 7, 6, 81, 40), c(RECF % 96, 1, "fused", 5, 8, 96, 64), c(RECF % 96, 3, "fused", 262, 5, 96, 49),
    c(RECF % 112, 1, "fused", 7, 6, 97, 48), c(RECF % 112, 1, "fused", 7, 6, 112, 49), c(RECF % 112, 4, "fused", 390, 5, 100, 48),
    c(RECF % 128, 1, "fused", 7, 6, 113, 40), c(RECF % 128, 1, "fused", 7, 6, 128, 64), c(RECF % 128, 3, "fused", 262, 5, 128, 64),
    c(RECF % 128, 4, "fused", 390, 5, 128, 24), c(RECF % 112, 2, "fused", 391, 130, 100, 40), c(RECF % 128, 1, "fused", 2545, 3, 128, 33, ndir=1),
    # 16-sequence MFMA kernel, input projection fused: from ceil(M/16) ndir = 160; G = ceil((H + I) / 16), two tiles per wave above H = 64
    c(MF16 % (1, 1), 16, "fused", 1267, 3, 8, 8), c(MF16 % (2, 1), 16, "fused", 1267, 3, 16, 16), c(MF16 % (3, 1), 16, "fused", 1267, 3, 33, 15),
    c(MF16 % (4, 1), 16, "fused", 1267, 3, 48, 16), c(MF16 % (5, 1), 16, "fused", 1267, 3, 64, 16), c(MF16 % (6, 1), 16, "fused", 1267, 3, 64, 32),
    c(MF16 % (7, 1), 16, "fused", 1267, 3, 49, 63), c(MF16 % (8, 1), 16, "fused", 1267, 3, 64, 64), c(MF16 % (5, 2), 16, "fused", 1267, 3, 65, 15),
    c(MF16 % (6, 2), 16, "fused", 1267, 3, 70, 26), c(MF16 % (7, 2), 16, "fused", 1267, 3, 70, 40), c(MF16 % (8, 2), 16, "fused", 1267, 3, 80, 48),
    c(MF16 % (9, 2), 16, "fused", 1267, 3, 96, 48), c(MF16 % (10, 2), 16, "fused", 1267, 3, 128, 32), c(MF16 % (10, 2), 16, "fused", 1267, 3, 97, 63),
    c(MF16 % (7, 2), 16, "fused", 2545, 3, 70, 40, ndir=1), c(MF16 % (10, 2), 16, "fused", 2545, 3, 128, 32, ndir=1),
]

# the fused VALU kernel's S = 2, 3, 4 at every KP (S = 2: pick_s gives 4 and T = 130 (IP = 48) / 100 (IP = 64) halves it)
_RECF_HI = {16: (8, 8), 32: (20, 5), 48: (33, 15), 64: (60, 4), 80: (65, 15), 96: (96, 49), 112: (100, 48), 128: (128, 64)}
DISPATCH += [c(RECF % kp, s, "fused", m, (130 if i <= 48 else 100) if s == 2 else 5, h, i)
             for kp, (h, i) in _RECF_HI.items() for s, m in ((2, 391), (3, 263), (4, 391))]

# ---- forms the library picks for large M only, forced on small ragged batches
FORCED = [c(GIN16 % a, 16, "fwd", 37, 9, h, tun=F16) for a, h in (((3, 1), 40), ((4, 1), 64), ((5, 2), 70), ((6, 2), 96), ((7, 2), 100), ((8, 2), 128))]
FORCED += [c(MF16 % a, 16, "fused", 37, 9, h, i, tun=F16) for a, h, i in (((1, 1), 9, 5), ((2, 1), 15, 16), ((5, 1), 40, 40), ((8, 1), 64, 64), ((7, 2), 70, 40),
                                                                            ((9, 2), 96, 33), ((10, 2), 128, 24), ((10, 2), 100, 60))]
FORCED += [c(REC % kp, s, "fwd", 21, 8, h, tun={"lstm_s": s}) for kp, h in ((16, 11), (64, 64), (128, 128)) for s in (2, 3, 4, 8)]
FORCED += [c(RECF % kp, s, "fused", 21, 8, h, i, tun={"lstm_s": s}) for kp, h, i in ((96, 90, 64), (128, 128, 40)) for s in (2, 3, 4)]
FORCED += [c(RECF % 128, 4, "fused", 21, 8, 128, 40, tun={"lstm_s": 8}, tag="s8-caps-at-4"),
           c(REC % 128, 1, "fwd", 1011, 4, 128, tun={"lstm_mfma16": 0, "lstm_s": 1}, tag="mfma16-off")]

# ---- one representative of each of the eight kernel templates and of the two streaming forms
REPS = {
    "rec": dict(kernel=REC % 64, S=3, entry="fwd", M=10, T=12, H=64, tun={"lstm_s": 3}),
    "rec_fused": dict(kernel=RECF % 112, S=3, entry="fused", M=10, T=12, H=100, I=40, tun={"lstm_s": 3}),
    "mfma_gin": dict(kernel=GIN % "3,24,2", S=4, entry="fwd", M=10, T=12, H=70),
    "mfma16_gin": dict(kernel=GIN16 % (5, 2), S=16, entry="fwd", M=37, T=12, H=70, tun=F16),
    "mfma_s4": dict(kernel=MF % (3, 20, 4, 1), S=4, entry="fused", M=10, T=12, H=40, I=40),
    "mfma_s3": dict(kernel=MF % (5, 28, 3, 1), S=3, entry="fused", M=10, T=12, H=70, I=40),
    "mfma_tpt2": dict(kernel=MF % (5, 28, 4, 2), S=4, entry="fused", M=10, T=12, H=70, I=40, bif=4),
    "mfma16": dict(kernel=MF16 % (7, 2), S=16, entry="fused", M=37, T=12, H=70, I=40, tun=F16),
    "steps_lstm": dict(kernel="lstm_step_cell_kernel", S=1, entry="steps", M=10, T=12, H=129),
    "steps_gru": dict(kernel="gru_step_cell_kernel", S=1, entry="birnn_gru", M=10, T=12, H=130),
}


def _variants():
    out = []
    for name, r in REPS.items():
        def mk(r=r, **kw):
            a = dict(r, **kw)
            if a["entry"] in ("fwd", "fused"):                 # S of the variant's own shape (a long T halves it in the fused VALU kernel)
                a["S"] = R.predict(a["entry"], a["M"], a["T"], a["H"], a.get("I", 0), a.get("ndir", 2), a.get("tun"), a.get("bif", 0) or 1).S
            return c(**a)
        M, T = r["M"], r["T"]
        m1 = dict(M=1)
        out += [mk(ndir=1, tag=name), mk(lens=None, tag=name), mk(h0=True, c0=False, tag=name), mk(h0=False, c0=True, tag=name),
                mk(h0=False, c0=False, tag=name), mk(hn=False, cn=False, tag=name), mk(hn=True, cn=False, tag=name), mk(T=1, tag=name),
                mk(tag=name, **m1), mk(lens="ones", tag=name), mk(lens="wg1", M=max(M, 2 * r["S"] + 1), tag=name),
                mk(fam="remember", T=256, M=min(M, 10), tag=name), mk(fam="sat", tag=name), mk(fam="tiny", tag=name),
                mk(lens="zero", tag=name), mk(lens="zero", h0=False, c0=False, tag=name), mk(lens="over", tag=name)]
    return out


VARIANTS = _variants()

# ---- nir_birnn_steps_fwd / nir_bilstm_steps_fwd: H beyond the in-kernel recurrences and one below; the cell state of every step; the form
# multitask/suggest.py calls (ndir = 1, lengths, b_hh, h0, hn, cn all NULL); M small, so the step GEMM stays an fp32-form kernel
LSTEP, GSTEP = "lstm_step_cell_kernel", "gru_step_cell_kernel"
STEPS = [c(LSTEP, 1, "birnn_lstm", 9, 7, h, cst=True) for h in (70, 129, 200, 256, 1024)]
STEPS += [c(LSTEP, 1, "birnn_lstm", 6, 9, h, ndir=1, lens=None, h0=False, c0=False, hn=False, cn=False, cst=True, tag="suggest") for h in (129, 256)]
STEPS += [c(LSTEP, 1, "steps", 9, 7, h) for h in (100, 200, 1024)] + [c(LSTEP, 1, "birnn_lstm", 20, 5, 256, cst=True, lens="zero")]
STEPS += [c(GSTEP, 1, "birnn_gru", 9, 7, h, h0=h0) for h in (70, 129, 200, 256, 1024) for h0 in (True, False)]
STEPS += [c(GSTEP, 1, "birnn_gru", 9, 7, 131, ndir=1, lens=None), c(GSTEP, 1, "birnn_gru", 40, 5, 256, fam="sat")]


def _unique(cases):
    seen = {}
    for d in cases:
        n = seen[d["id"]] = seen.get(d["id"], 0) + 1
        if n > 1:
            d["id"] += "-%d" % n
    return cases


ALL_CASES = _unique(DISPATCH + FORCED + VARIANTS + STEPS)


# ------------------------------------------------------------------ running one case
def _profiled(L, fn):
    """[(kernel name without its [M=,N=,K=] part, launches)] of the library's launches inside fn(), sorted by name"""
    buf = C.create_string_buffer(1 << 16)
    L.nir_profile_report(buf, len(buf))                     # drop what earlier tests left
    L.nir_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.nir_profile_enable(0)
    L.nir_profile_report(buf, len(buf))
    out = {}
    for ln in buf.value.decode().strip().splitlines():
        name, launches, _ = ln.rsplit(",", 2)
        name = re.sub(r"\[M=[^\]]*\]$", "", name)
        out[name] = out.get(name, 0) + int(launches)
    return sorted(out.items())


def _guarded(n):
    """n floats of NaN between two guards of GUARD sentinels -> (buffer, view of the payload)"""
    buf = torch.full((n + 2 * GUARD,), float("nan"), device=DEV)
    buf[:GUARD] = SENT
    buf[GUARD + n:] = SENT
    return buf, buf[GUARD:GUARD + n]


def _payload(buf, n, what):
    h = buf.cpu()
    assert bool((h[:GUARD] == SENT).all()) and bool((h[GUARD + n:] == SENT).all()), "wrote outside %s" % what
    return h[GUARD:GUARD + n].numpy()


def lengths_of(d):
    """the lengths argument of a case: None, "mixed" (made by rnn_ref.make) or an int64 array"""
    M, T, spec = d["M"], d["T"], d["lens"]
    if spec is None or spec == "mixed":
        return spec
    rng = np.random.default_rng(M * 13 + T)
    if spec == "ones":
        return np.ones(M, np.int64)
    if spec == "wg1":
        return np.array([1] * d["S"] + [T] * (M - d["S"]), np.int64)
    lens = R.mixed_lengths(rng, M, T)
    bad = 0 if spec == "zero" else T + 5
    lens[M // 2] = bad
    lens[min(1, M - 1)] = bad
    return lens


@contextlib.contextmanager
def _steered(d):
    """the tunables and the batches-in-flight hint of a case, restored on the way out"""
    from context_attentive_ir_amd import lib
    with contextlib.ExitStack() as st:
        for k, v in d["tun"].items():
            st.enter_context(lib.tunable(k, v, restore=R.TUNABLES[k]))
        try:
            if d["bif"]:
                lib.set_batches_in_flight(d["bif"])
            yield
        finally:
            if d["bif"]:
                lib.set_batches_in_flight(0)


def _call(d, inp, out, hn, cn, cst, ws=None, ws_bytes=0):
    """the C-ABI call of a case -> its return code"""
    from context_attentive_ir_amd import lib
    L = lib.load()
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = {k: dev(inp.get(k)) for k in ("gin", "x", "w_ih", "b_ih", "b_hh_in", "w_hh", "b_hh", "lengths", "h0", "c0")}
    p = lambda k: lib.ptr(t[k])
    M, T, H, ndir, e = d["M"], d["T"], d["H"], d["ndir"], d["entry"]
    if e == "fwd":
        rc = L.nir_bilstm_fwd(p("gin"), p("lengths"), p("w_hh"), p("h0"), p("c0"), lib.ptr(out), lib.ptr(hn), lib.ptr(cn), M, T, H, ndir, lib.stream())
    elif e == "fused":
        rc = L.nir_bilstm_fused_fwd(p("x"), d["I"], p("w_ih"), p("b_ih"), p("b_hh_in"), p("lengths"), p("w_hh"), p("h0"), p("c0"), lib.ptr(out),
                                    lib.ptr(hn), lib.ptr(cn), M, T, H, ndir, lib.stream())
    elif e == "steps":
        rc = L.nir_bilstm_steps_fwd(p("gin"), p("lengths"), p("w_hh"), p("h0"), p("c0"), lib.ptr(out), lib.ptr(hn), lib.ptr(cn), M, T, H, ndir,
                                    lib.ptr(ws), ws_bytes, lib.stream())
    else:
        rc = L.nir_birnn_steps_fwd(1 if e == "birnn_gru" else 0, p("gin"), p("lengths"), p("w_hh"), p("b_hh"), p("h0"), p("c0"), lib.ptr(out),
                                   lib.ptr(cst), lib.ptr(hn), lib.ptr(cn), M, T, H, ndir, lib.ptr(ws), ws_bytes, lib.stream())
    torch.cuda.synchronize()                                 # the inputs of this call stay alive until it has run
    return rc


def _run(d):
    from context_attentive_ir_amd import lib
    L = lib.load()
    M, T, H, ndir, e = d["M"], d["T"], d["H"], d["ndir"], d["entry"]
    cell = "gru" if e == "birnn_gru" else "lstm"
    inp = R.make(d["fam"], M * 1009 + T * 131 + H * 7 + d["I"] + ndir, M, T, H, ndir, d["I"], cell, lengths_of(d), d["h0"], d["c0"])
    n_out, n_st = M * T * ndir * H, ndir * M * H
    obuf, out = _guarded(n_out)
    hbuf, hn = _guarded(n_st) if d["hn"] else (None, None)
    cbuf, cn = _guarded(n_st) if (d["cn"] and cell == "lstm") else (None, None)
    sbuf, cst = _guarded(n_out) if d["cst"] else (None, None)
    ws, ws_bytes = None, 0
    if e not in ("fwd", "fused"):
        ws_bytes = L.nir_bilstm_steps_workspace_bytes(M, H)
        ws = torch.full((ws_bytes + WS_GUARD,), 0x5A, dtype=torch.uint8, device=DEV)
    with _steered(d):
        ran = _profiled(L, lambda: lib.check(_call(d, inp, out, hn, cn, cst, ws, ws_bytes), e))
    if e in ("fwd", "fused"):
        assert ran == [(d["kernel"], 1)], ran
    else:
        want = R.predict_steps(cell, M, T, H, ndir, d["h0"])
        assert ran == want and all(n in R.FP32_GEMMS for n, _ in want if "gemm" in n), (ran, want)
        assert bool((ws[ws_bytes:] == 0x5A).all()), "wrote behind the workspace"
    got = dict(out=_payload(obuf, n_out, "out").reshape(M, T, ndir * H),
               hn=None if hbuf is None else _payload(hbuf, n_st, "hn").reshape(ndir, M, H),
               cn=None if cbuf is None else _payload(cbuf, n_st, "cn").reshape(ndir, M, H),
               cst=None if sbuf is None else _payload(sbuf, n_out, "c_steps").reshape(M, T, ndir * H))
    fam = R.family_of(d["kernel"])
    ok, r = R.accept(got, inp, family=fam)
    line = "RNNENV,%s,%s,e=%.3g,e32=%.3g,e_act=%.3g,ratio=%.3f,bound=%.3g,tail=%d" % (d["id"], fam, r["e"], r["e32"], r["e_act"], r["ratio"],
                                                                                    r["bound"], r["tail"])
    print(line)
    FIGURES.append(line)
    assert ok, line
    for m in np.flatnonzero(R.clamp_lengths(inp["lengths"], M, T) == 0):      # length 0: the initial state comes back bit for bit
        for g, k0 in ((got["hn"], "h0"), (got["cn"], "c0")):
            if g is not None:
                want = np.zeros((ndir, H), np.float32) if inp[k0] is None else inp[k0][:, m]
                assert np.array_equal(g[:, m], want), (k0, m)


@pytest.mark.parametrize("d", DISPATCH, ids=[d["id"] for d in DISPATCH])
def test_recurrence_dispatch(d):
    _run(d)


@pytest.mark.parametrize("d", FORCED, ids=[d["id"] for d in FORCED])
def test_recurrence_forced_forms(d):
    _run(d)


@pytest.mark.parametrize("d", VARIANTS, ids=[d["id"] for d in VARIANTS])
def test_recurrence_variants(d):
    _run(d)


@pytest.mark.parametrize("d", STEPS, ids=[d["id"] for d in STEPS])
def test_streaming_recurrence(d):
    _run(d)


# ------------------------------------------------------------------ the fast activations, per kernel template
@pytest.mark.parametrize("name", list(REPS))
def test_activation_accuracy(name):
    """T = 1 from a zero state over a dense sweep of gate values in [-30, 30]: with g saturated cn = sigmoid(i), with i saturated cn = tanh(g)
    (LSTM); the GRU gives h = (1 - sigmoid(z)) tanh(n).  Maximum absolute error against float64 <= DELTA.  The fused entries get the gate
    value of (sequence m, unit j) as x[m] * 1 + b_ih[j], both multiples of 2^-10: the fp32 sum is exact."""
    r = REPS[name]
    M, H, I, e = 61, r["H"], r.get("I", 0), r["entry"]
    gru = e == "birnn_gru"
    NG = 3 if gru else 4
    worst = {}
    for which in ("sigmoid", "tanh"):
        d = c(**dict(r, M=M, T=1, ndir=2, lens=None, h0=False, c0=False, tag="act"))
        # value of (m, j): a grid over [-30, 30) in steps of 60 / (M H), rounded to 2^-10
        base = np.round((np.arange(M) * 60.0 / M - 30.0) * 1024) / 1024                       # per sequence
        fine = np.round((np.arange(H) * 60.0 / (M * H)) * 1024) / 1024                       # per unit
        v = (base[:, None] + fine[None, :]).astype(np.float32)                              # [M, H], exact in fp32
        gates = np.zeros((M, 2, NG, H), np.float32)
        if gru:                      # r irrelevant (b_hh = 0); h = (1 - s(z)) tanh(n)
            gates[:, :, 1] = v[:, None] if which == "sigmoid" else -30.0
            gates[:, :, 2] = 30.0 if which == "sigmoid" else v[:, None]
            ref = (1.0 - 1.0 / (1.0 + np.exp(-gates[:, :, 1].astype(np.float64)))) * np.tanh(gates[:, :, 2].astype(np.float64))
        else:                        # i, f, g, o
            gates[:, :, 0] = v[:, None] if which == "sigmoid" else 30.0
            gates[:, :, 2] = 30.0 if which == "sigmoid" else v[:, None]
            gates[:, :, 3] = 30.0
            ref = 1.0 / (1.0 + np.exp(-gates[:, :, 0].astype(np.float64))) * np.tanh(gates[:, :, 2].astype(np.float64))
        inp = dict(cell="gru" if gru else "lstm", ndir=2, lengths=None, h0=None, c0=None, gin=None, x=None,
                   w_hh=np.zeros((2, NG * H, H), np.float32), b_hh=np.zeros((2, 3 * H), np.float32))
        if I:                        # gate = x[m, 0] * w + b: w = 1 on the swept gate's rows, the unit's offset and the constants in b_ih
            x = np.zeros((M, 1, I), np.float32)
            x[:, 0, 0] = base
            w = np.zeros((2, 4, H, I), np.float32)
            b = np.zeros((2, 4, H), np.float32)
            sw = 0 if which == "sigmoid" else 2
            w[:, sw, :, 0] = 1.0
            b[:, sw] = fine
            b[:, 2 - sw] = 30.0
            b[:, 3] = 30.0
            inp.update(x=x, w_ih=w.reshape(2 * 4 * H, I), b_ih=b.reshape(-1), b_hh_in=np.zeros(2 * 4 * H, np.float32))
        else:
            inp["gin"] = gates.reshape(M, 1, 2 * NG * H)
        n_out, n_st = M * 2 * H, 2 * M * H
        obuf, out = _guarded(n_out)
        hbuf, hn = _guarded(n_st)
        cbuf, cn = (None, None) if gru else _guarded(n_st)
        ws, ws_bytes = None, 0
        from context_attentive_ir_amd import lib
        L = lib.load()
        if e not in ("fwd", "fused"):
            ws_bytes = L.nir_bilstm_steps_workspace_bytes(M, H)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
        with _steered(d):
            ran = _profiled(L, lambda: lib.check(_call(d, inp, out, hn, cn, None, ws, ws_bytes), e))
        assert (r["kernel"], 1 if e in ("fwd", "fused") else 2) in ran, ran
        got = (_payload(hbuf, n_st, "hn") if gru else _payload(cbuf, n_st, "cn")).reshape(2, M, H).transpose(1, 0, 2)
        worst[which] = float(np.abs(got.astype(np.float64) - ref).max())
    line = "RNNACT,%s,%s,sigmoid=%.3g,tanh=%.3g,delta=%.3g" % (name, r["kernel"], worst["sigmoid"], worst["tanh"], R.DELTA)
    print(line)
    FIGURES.append(line)
    assert max(worst.values()) <= R.DELTA, line


# ------------------------------------------------------------------ refused arguments
def test_argument_errors_touch_nothing():
    from context_attentive_ir_amd import lib
    L = lib.load()
    assert [L.nir_bilstm_supported(h) for h in (0, 1, 128, 129)] == [0, 1, 1, 0]
    buf, dummy = _guarded(64)
    dummy.fill_(1.0)
    dp, st = lib.ptr(dummy), lib.stream()
    fwd = lambda M, T, H, ndir: L.nir_bilstm_fwd(dp, None, dp, None, None, dp, dp, dp, M, T, H, ndir, st)
    fused = lambda M, T, H, I, ndir=2: L.nir_bilstm_fused_fwd(dp, I, dp, dp, dp, None, dp, None, None, dp, dp, dp, M, T, H, ndir, st)
    for args in ((2, 3, 0, 2), (2, 3, 129, 2), (2, 3, 64, 3), (2, 3, 64, 0), (2, 0, 64, 2), (2, 1 << 20, 128, 2)):
        with pytest.raises(ValueError):
            R.predict("fwd", *args[:3], ndir=args[3])
        assert fwd(*args) != 0, args
    assert 8 * (1 << 20) * 2 * 4 * 128 * 4 >= R.OFF_LIMIT
    for args in ((2, 3, 64, 0), (2, 3, 64, 65), (2, 3, 0, 8), (2, 3, 129, 8), (2, 0, 64, 8)):
        with pytest.raises(ValueError):
            R.predict("fused", args[0], args[1], args[2], args[3])
        assert fused(*args) != 0, args
    assert fused(2, 3, 64, 8, ndir=3) != 0
    # the fused VALU kernel stages the whole x tile in LDS: a T beyond it is refused (real buffers: the refusal is behind the MFMA dispatch)
    M, T, H, I = 1, 750, 100, 40
    with pytest.raises(ValueError, match="LDS"):
        R.predict("fused", M, T, H, I)
    x = torch.zeros(M * T * I, device=DEV)
    w = torch.zeros(8 * H * max(H, I), device=DEV)
    obuf, out = _guarded(M * T * 2 * H)
    assert L.nir_bilstm_fused_fwd(lib.ptr(x), I, lib.ptr(w), lib.ptr(w), lib.ptr(w), None, lib.ptr(w), None, None, lib.ptr(out), None, None,
                                  M, T, H, 2, st) != 0
    assert b"LDS" in L.nir_last_error_string()
    torch.cuda.synchronize()
    assert bool(torch.isnan(obuf[GUARD:-GUARD]).all())
    # streaming entries
    need = L.nir_bilstm_steps_workspace_bytes(2, 64)
    steps = lambda ws_bytes, T=3, ndir=2: L.nir_bilstm_steps_fwd(dp, None, dp, None, None, dp, dp, dp, 2, T, 64, ndir, dp, ws_bytes, st)
    birnn = lambda cell, bhh, ws_bytes=need, H=64, M=2: L.nir_birnn_steps_fwd(cell, dp, None, dp, bhh, None, None, dp, None, dp, dp, M, 3, H, 2, dp, ws_bytes, st)
    assert steps(need - 1) != 0 and steps(need, T=0) != 0 and steps(need, ndir=3) != 0
    assert birnn(1, None) != 0 and birnn(2, dp) != 0 and birnn(0, None, need - 1) != 0 and birnn(0, None, H=0) != 0
    # M = 0: success, nothing launched, nothing written
    ran = _profiled(L, lambda: [lib.check(birnn(1, dp, M=0), "M = 0"), lib.check(fwd(0, 3, 64, 2), "M = 0"), lib.check(fused(0, 3, 64, 8), "M = 0"),
                                lib.check(L.nir_bilstm_steps_fwd(dp, None, dp, None, None, dp, dp, dp, 0, 3, 64, 2, dp, need, st), "M = 0")])
    assert ran == [] and R.predict("fwd", 0, 3, 64) is None and R.predict("fused", 0, 3, 64, 8) is None
    torch.cuda.synchronize()
    assert bool((_payload(buf, 64, "the dummy") == 1.0).all())


def test_every_kernel_family_sees_every_input_family():
    for fam in R.MARGIN:
        seen = {d["fam"] for d in ALL_CASES if R.family_of(d["kernel"]) == fam}
        assert {"randn", "sat", "tiny", "remember"} <= seen, (fam, seen)
