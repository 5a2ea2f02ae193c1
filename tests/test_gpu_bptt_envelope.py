"""GPU (-m gpu): the train-mode recurrences and their BPTT up to 128 units per direction (nir_lstm_train_fwd, nir_lstm_train_fwd_split,
nir_lstm_train_bwd, nir_gru_train_fwd, nir_gru_train_bwd) and the streaming cell kernels (nir_lstm_cell_*, nir_gru_cell_seq_*), called through the
C ABI only, against float64 (tests/bptt_ref.py).  Each case asserts:
  * the profile report names exactly the kernel the table states, once (tests/test_bptt_criterion_host.py checks the tables against the
    restated dispatchers on the CPU) -- a shape that lands elsewhere is moved, not the assertion;
  * every output meets the criterion of tests/bptt_ref.py, per output and direction; out, dgates, dgx, dq are exactly 0.0 at t >= len; hn / cn
    are the last valid state bit for bit (h0 / c0 for length 0); a second identical call gives the same bits;
  * every output buffer sits between guard regions that are intact afterwards and is prefilled with NaN.
The BPTT kernels are judged in isolation: their saved act / cst are the float64 forward rounded to fp32 and hold NaN at every t >= len (the
forward leaves those unwritten); one chained forward -> backward case per BPTT form is kept on top.  The cell-IO forms of the matrix-core BPTT
kernels (16-byte, 8-byte, scalar) are reached by offsetting exactly the buffers the kernels test for alignment and must agree bit for bit.  Before a
matrix-core BPTT case one large BPTT over NaN gradients leaves NaN in LDS (_stale_lds): a kernel that reads LDS it has not written shows.
Every case prints one "BPTTENV" line with its figures before it asserts (pytest -s); DESIGN.md section 19 quotes the largest per family."""
import numpy as np
import pytest
import torch

import bptt_ref as B
from test_gpu_rnn_envelope import _profiled

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0
GUARD = 64            # floats in front of and behind every output (256 bytes: the payload keeps the allocator's alignment)
SLACK = 4             # floats of room for the alignment offsets
FIGURES = []

LFV, LF16, LBV, LBM = "lstm_train_fwd_kernel", "lstm_train_fwd_mfma16_kernel<%d,%d>", "lstm_train_bwd_kernel", "lstm_train_bwd_mfma_kernel"
LSP3, LSP4 = "lstm16_pt_h2_kernel<3,2,false,true>", "lstm16_pt_h2_kernel<4,4,8,false,true>"
GF, GBV, GBM = "gru_train_fwd_kernel", "gru_train_bwd_kernel", "gru_train_bwd_mfma_kernel"
FWD_OPT = dict(h0=True, c0=True, hn=True, cn=True)
BWD_OPT = dict(dhn=True, dcn=True, dcst=True, c0=True, dh0=True, dc0=True, dout0=False)


def c(op, kernel, M, T, H, fam="randn", ndir=2, lens="ends", form=B.GRU_AUTO, off=0, tag="", reseed=0, **opt):
    """One case.  op: "lstm_fwd", "lstm_split", "gru_fwd", "lstm_bwd", "gru_bwd", "lstm_chain", "gru_chain" (kernel: the BPTT kernel; the forward is
    whatever the library picks).  lens: a mode of bptt_ref.lengths_of.  form: the GRU BPTT's form argument.  off: the cell-IO buffers of a BPTT start
    this many floats past 16-byte alignment.  opt: optional arguments handed over (True) or NULL (False); dout0: dout all zero."""
    base = FWD_OPT if op in ("lstm_fwd", "lstm_split", "gru_fwd") else BWD_OPT
    assert set(opt) <= set(base), opt
    o = dict(base, **opt)
    if op == "lstm_split":
        o.update(h0=False, c0=False, hn=False, cn=False)
    d = dict(op=op, kernel=kernel, M=M, T=T, H=H, fam=fam, ndir=ndir, lens=lens, form=form, off=off, opt=o, reseed=reseed)
    tags = [op, kernel, "M%dT%dH%d" % (M, T, H)] + ([fam] if fam != "randn" else []) + ["ndir1"] * (ndir == 1)
    tags += ["lens=%s" % (lens if isinstance(lens, (str, type(None))) else "list")] if lens != "ends" else []
    tags += ["form%d" % form] * (form != 0) + ["off%d" % off] * (off != 0) + ["%s%s" % ("" if v else "no-", k) for k, v in sorted(opt.items())]
    d["id"] = "-".join(tags + ([tag] if tag else []))
    return d


# ---- BPTT dispatch, both sides of every edge.  hp = H rounded up to 4 in {32, 64, 72, 96, 128} and H >= 16: the matrix cores for even H at any M, for
# odd H from 1024 sequences on (the GRU: the same rule under form = AUTO; forced forms take odd H at any M)
MFMA_H = (29, 30, 31, 32, 61, 62, 63, 64, 69, 70, 71, 72, 93, 94, 95, 96, 125, 126, 127, 128)
VALU_H = (15, 16, 28, 33, 60, 65, 68, 73, 92, 97, 124)
EVEN, ODD = [h for h in MFMA_H if h % 2 == 0], [h for h in MFMA_H if h % 2]
LSTM_BWD = [c("lstm_bwd", LBM, 17, 6, h) for h in EVEN] + [c("lstm_bwd", LBV, 17, 6, h) for h in ODD] + [c("lstm_bwd", LBV, 17, 6, h) for h in VALU_H]
LSTM_BWD += [c("lstm_bwd", LBV, 1023, 2, h) for h in (31, 71, 127)] + [c("lstm_bwd", LBM, 1024, 2, h) for h in ODD]
LSTM_BWD += [c("lstm_bwd", LBV, 1024, 2, h) for h in (15, 33, 73)] + [c("lstm_bwd", LBV, 5, 7, h) for h in (1, 2, 7, 14)]
GRU_BWD = [c("gru_bwd", GBM, 17, 6, h) for h in EVEN] + [c("gru_bwd", GBV, 17, 6, h) for h in ODD] + [c("gru_bwd", GBV, 17, 6, h) for h in VALU_H]
GRU_BWD += [c("gru_bwd", GBV, 1023, 2, h) for h in (31, 71, 127)] + [c("gru_bwd", GBM, 1024, 2, h) for h in (31, 69, 127)]
GRU_BWD += [c("gru_bwd", GBV, 17, 6, h, form=B.GRU_VALU) for h in MFMA_H] + [c("gru_bwd", GBM, 17, 6, h, form=B.GRU_MFMA) for h in MFMA_H]
GRU_BWD += [c("gru_bwd", GBV, 5, 7, h) for h in (1, 2, 7)]
# HP = 72 is the one size whose k-steps are padded (GRU: 54 -> 56, zero A fragments against LDS columns no step writes): every family, both cells
HP72 = [c("gru_bwd", GBM, 33, 9, h, fam=fam, form=B.GRU_MFMA) for fam in ("randn", "sat", "remember", "last") for h in (69, 70, 71, 72)]
HP72 += [c("lstm_bwd", LBM, 33, 9, h, fam=fam) for fam in ("sat", "remember", "last") for h in (70, 72)]

# ---- forward dispatch
def _g16(h):
    g = (h + 15) // 16
    return LF16 % ((3 if g == 3 else 4, 1) if h <= 64 else (g, 2))


FWD = [c("lstm_fwd", LFV, 5, 7, h) for h in (1, 17, 32)]
FWD += [c("lstm_fwd", _g16(h), 17, 6, h, **kw) for h in (33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128)
        for kw in ({}, dict(h0=False, c0=False, hn=False, cn=False))]
FWD += [c("lstm_split", LSP3 if h <= 96 else LSP4, 17, 6, h) for h in (65, 70, 96, 97, 128)]
FWD += [c("gru_fwd", GF, 5, 7, h) for h in (1, 32, 33, 64, 65, 96, 97, 128)]

# ---- one representative per kernel form: workgroup raggedness (16- and 4-sequence kernels), an all-idle workgroup, lens NULL, T = 1, one
# direction, the other length modes, every family
REPS = {
    "lstm_fwd_valu": dict(op="lstm_fwd", kernel=LFV, M=5, T=8, H=20),
    "lstm_fwd_mfma16": dict(op="lstm_fwd", kernel=LF16 % (5, 2), M=17, T=8, H=70),
    "lstm_fwd_split": dict(op="lstm_split", kernel=LSP3, M=17, T=8, H=70),
    "gru_fwd": dict(op="gru_fwd", kernel=GF, M=5, T=8, H=70),
    "lstm_bwd_valu": dict(op="lstm_bwd", kernel=LBV, M=5, T=8, H=33),
    "lstm_bwd_mfma": dict(op="lstm_bwd", kernel=LBM, M=17, T=8, H=70),
    "lstm_bwd_mfma2": dict(op="lstm_bwd", kernel=LBM, M=17, T=8, H=64),          # four waves x two unit tiles
    "gru_bwd_valu": dict(op="gru_bwd", kernel=GBV, M=5, T=8, H=33),
    "gru_bwd_mfma": dict(op="gru_bwd", kernel=GBM, M=17, T=8, H=70),
}
S_OF = {k: (4 if r["kernel"] in (LFV, GF, LBV, GBV) else 16) for k, r in REPS.items()}


def _variants():
    out = []
    for name, r in REPS.items():
        mk = lambda r=r, **kw: c(**dict(r, tag=name, **kw))
        S = S_OF[name]
        out += [mk(M=m, lens="mixed") for m in ((1, 4, 5) if S == 4 else (1, 15, 16, 17, 33))]
        out += [mk(M=2 * S + 1, lens="wg0"), mk(lens=None), mk(T=1), mk(ndir=1), mk(lens="ones"), mk(lens="zero"), mk(lens="over"), mk(lens="neg")]
        out += [mk(fam=f) for f in ("sat", "remember") + (("last",) if "bwd" in name else ("tiny",))]
    return out


VARIANTS = _variants()

# ---- final-state and initial-state arguments, in both BPTT forms of both cells: each alone, none, and dout == 0 with the final-state gradient alone
NONE = dict(dhn=False, dcn=False, dcst=False, c0=False, dh0=False, dc0=False)
STATE = []
for _name in ("lstm_bwd_valu", "lstm_bwd_mfma", "lstm_bwd_mfma2"):
    _mk = lambda **kw: c(**dict(REPS[_name], M=21, tag=_name, **kw))
    STATE += [_mk(**NONE)] + [_mk(**dict(NONE, **{k: True})) for k in ("dhn", "dcn", "dcst", "c0")] + [_mk(**dict(NONE, dhn=True, dh0=True)),
              _mk(**dict(NONE, dcn=True, dc0=True)), _mk(**dict(NONE, dh0=True, dc0=True)), _mk(dout0=True, dcst=False), _mk(dout0=True, dcst=False, dcn=False),
              _mk(dout0=True, dcst=False, dhn=False), _mk(dh0=False), _mk(dc0=False)]
for _name in ("gru_bwd_valu", "gru_bwd_mfma"):
    _mk = lambda **kw: c(**dict(REPS[_name], M=21, tag=_name, **kw))
    STATE += [_mk(dhn=False), _mk(dout0=True), _mk(dout0=True, ndir=1)]

# ---- state carry over many steps: the gradient is carried at O(1) ("remember") or reaches the early steps through the recurrent path alone ("last")
CARRY = [c(**dict(REPS[n], M=5, T=64, fam=f, lens="mixed", tag=n)) for n in REPS if "bwd" in n for f in ("remember", "last")]
# ---- one chained forward -> backward case per BPTT form
CHAIN = [c("lstm_chain", LBV, 5, 8, 33), c("lstm_chain", LBM, 17, 8, 70), c("lstm_chain", LBM, 17, 8, 64), c("lstm_chain", LBV, 5, 8, 20),
         c("gru_chain", GBV, 5, 8, 33), c("gru_chain", GBM, 17, 8, 70)]
# ---- the cell-IO forms by alignment: (cell, H, offsets in floats) -- +8 bytes takes the 8-byte form, +4 bytes the scalar one
CELL_IO = [(cell, h, (0, 2, 1)) for cell in ("lstm", "gru") for h in (32, 64, 128)] + [("lstm", 70, (0, 1)), ("gru", 70, (0, 1))]


def _unique(cases):
    seen = {}
    for d in cases:
        n = seen[d["id"]] = seen.get(d["id"], 0) + 1
        if n > 1:
            d["id"] += "-%d" % n
    return cases


ALL_CASES = _unique(LSTM_BWD + GRU_BWD + HP72 + FWD + VARIANTS + STATE + CARRY + CHAIN)
# inputs on which an honest fp32 evaluation (one sequential chain over the 4H terms of dgates W_hh, as the matrix-core kernel sums them) misses the
# bound at the cap by itself: replaced by the first reseed at which every honest evaluation stays within 0.8 of it -- found and checked on the CPU
# (tests/test_bptt_criterion_host.py::test_replaced_inputs_are_the_ones_an_honest_evaluation_fails_on)
_P = "lstm_bwd-lstm_train_bwd_mfma_kernel-"
RESEED = {_P + "M16T8H70-lens=mixed-lstm_bwd_mfma": 1, _P + "M17T8H70-lens=mixed-lstm_bwd_mfma": 2, _P + "M17T8H70-lens=None-lstm_bwd_mfma": 2,
          _P + "M17T8H70-lens=over-lstm_bwd_mfma": 2, _P + "M16T8H64-lens=mixed-lstm_bwd_mfma2": 1, _P + "M5T64H64-last-lens=mixed-lstm_bwd_mfma2": 2}
for _d in ALL_CASES:
    if _d["id"] in RESEED:
        _d["reseed"] = RESEED[_d["id"]]
        _d["id"] += "-reseed%d" % _d["reseed"]
assert sum(1 for _d in ALL_CASES if _d["reseed"]) == len(RESEED)


# ------------------------------------------------------------------ buffers
def _guarded(n, off=0):
    """n floats of NaN, `off` floats past 16-byte alignment, between two guards of sentinels -> (buffer, view of the payload)"""
    buf = torch.full((n + 2 * GUARD + SLACK,), float("nan"), device=DEV)
    buf[:GUARD + off] = SENT
    buf[GUARD + off + n:] = SENT
    view = buf[GUARD + off:GUARD + off + n]
    assert view.data_ptr() % 16 == 4 * off
    return buf, view


def _payload(buf, n, what, off=0):
    h = buf.cpu()
    assert bool((h[:GUARD + off] == SENT).all()) and bool((h[GUARD + off + n:] == SENT).all()), "wrote outside %s" % what
    return h[GUARD + off:GUARD + off + n].numpy()


def _dev(a, off=0):
    """a host array on the device (None stays None), its first element `off` floats past 16-byte alignment"""
    if a is None:
        return None
    a = np.ascontiguousarray(a)
    if a.dtype != np.float32:
        return torch.from_numpy(a).to(DEV)
    t = torch.empty(a.size + SLACK, device=DEV)
    v = t[off:off + a.size]
    v.copy_(torch.from_numpy(a.reshape(-1)))
    assert v.data_ptr() % 16 == 4 * off
    return v


def _bits_equal(a, b):
    return all((x is None and y is None) or torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a, b))


def _make(d):
    o = d["opt"]
    cell = "gru" if d["op"].startswith("gru") else "lstm"
    S = 16 if d["kernel"] in (LBM, GBM, LSP3, LSP4) or d["kernel"].startswith("lstm_train_fwd_mfma16") else 4
    seed = d["M"] * 1009 + d["T"] * 131 + d["H"] * 7 + d["ndir"] + 100003 * d["reseed"]
    return B.make(cell, d["fam"], seed, d["M"], d["T"], d["H"], d["ndir"], d["lens"], o.get("h0", True), o.get("c0", True), o.get("dhn", True),
                  o.get("dcn", True), o.get("dcst", True), o.get("dout0", False), S)


def _report(d, fam, r, what=""):
    line = "BPTTENV,%s%s,%s,worst=%s,e=%.3g,e32=%.3g,e_act=%.3g,s=%.3g,ratio=%.3f,miss=%.3f,tail=%d" % (
        d["id"], what, fam, r["worst"], r["e"], r["e32"], r["e_act"], r["s"], max(v[4] for v in r["per"].values()), r["miss"], r["tail"])
    print(line)
    FIGURES.append(line)
    return line


# ------------------------------------------------------------------ forward
def _forward_once(d, inp, L, lib):
    """one guarded call of the case's forward entry -> (profile, {name: (buffer, n, view)})"""
    M, T, H, ndir, o = d["M"], d["T"], d["H"], d["ndir"], d["opt"]
    lstm = inp["cell"] == "lstm"
    n_out, n_st = M * T * ndir * H, ndir * M * H
    bufs = dict(out=_guarded(n_out), act=_guarded(4 * n_out))
    if lstm:
        bufs["cst"] = _guarded(n_out)
    if o["hn"]:
        bufs["hn"] = _guarded(n_st)
    if o["cn"] and lstm:
        bufs["cn"] = _guarded(n_st)
    p = lambda k: lib.ptr(bufs[k][1]) if k in bufs else None
    t = {k: _dev(inp.get(k)) for k in ("gin", "w_hh", "b_hh", "lengths", "h0", "c0")}
    q = lambda k: lib.ptr(t[k])
    if d["op"] == "lstm_split":
        gp = _dev(B.to_perm(inp["gin"], ndir, H))
        ids = torch.arange(M * T, dtype=torch.int64, device=DEV)
        err = torch.zeros(4, dtype=torch.int32, device=DEV)
        call = lambda: L.nir_lstm_train_fwd_split(lib.ptr(gp), lib.ptr(ids), q("lengths"), q("w_hh"), p("out"), p("act"), p("cst"), lib.ptr(err), M, T, H,
                                                  ndir, lib.stream())
    elif lstm:
        err = None
        call = lambda: L.nir_lstm_train_fwd(q("gin"), q("lengths"), q("w_hh"), q("h0"), q("c0"), p("out"), p("act"), p("cst"), p("hn"), p("cn"), M, T, H,
                                            ndir, lib.stream())
    else:
        err = None
        call = lambda: L.nir_gru_train_fwd(q("gin"), q("lengths"), q("w_hh"), q("b_hh"), p("out"), p("act"), p("hn"), M, T, H, ndir, lib.stream())
    ran = _profiled(L, lambda: lib.check(call(), d["op"]))
    torch.cuda.synchronize()
    assert err is None or int(err.cpu()[0]) == 0
    return ran, bufs


def _shape(k, M, T, H, ndir):
    return {"out": (M, T, ndir * H), "act": (M, T, ndir, 4 * H), "cst": (M, T, ndir, H), "dgates": (M, T, ndir * 4 * H), "dgx": (M, T, ndir * 3 * H),
            "dq": (M, T, ndir * H)}.get(k, (ndir, M, H))


def _collect(bufs, M, T, H, ndir, off_keys=(), off=0):
    return {k: _payload(b, v.numel(), k, off if k in off_keys else 0).reshape(_shape(k, M, T, H, ndir)) for k, (b, v) in bufs.items()}


def _run_forward(d, judge=True):
    from context_attentive_ir_amd import lib
    L = lib.load()
    M, T, H, ndir = d["M"], d["T"], d["H"], d["ndir"]
    inp = _make(d)
    ran, bufs = _forward_once(d, inp, L, lib)
    got = _collect(bufs, M, T, H, ndir)
    if not judge:
        return inp, ran, got
    assert ran == [(d["kernel"], 1)], ran
    fam = B.family_of(d["kernel"])
    ok, r = B.accept(got, B.fwd_figures(inp), family=fam, extra=B.n_split(inp) * B.SPLIT_FMT if d["op"] == "lstm_split" else 0.0)
    line = _report(d, fam, r)
    assert ok, line
    lens = inp["lens"]
    for k, k0, src in (("hn", "h0", got["out"]), ("cn", "c0", got.get("cst"))):     # the last valid state, bit for bit
        if k not in got:
            continue
        for dd in range(ndir):
            for m in range(M):
                if lens[m] == 0:
                    want = np.zeros(H, np.float32) if inp.get(k0) is None else inp[k0][dd, m]
                else:
                    t = lens[m] - 1 if dd == 0 else 0
                    want = src[m, t, dd * H:(dd + 1) * H] if k == "hn" else src[m, t, dd]
                assert np.array_equal(got[k][dd, m], want), (k, dd, m)
    _, again = _forward_once(d, inp, L, lib)
    assert _bits_equal([bufs[k][1] for k in sorted(bufs)], [again[k][1] for k in sorted(again)]), "a second identical call gave other bits"


# ------------------------------------------------------------------ BPTT
LSTM_IO, GRU_IO = ("act", "cst", "dout", "dgates", "dcst", "c0"), ("act", "out", "dout", "dgx", "dq")      # the buffers the kernels test for alignment


_LDS = {}


def _stale_lds(L, lib):
    """Leave NaN behind in the LDS of every CU: one matrix-core LSTM BPTT over NaN gradients (8192 sequences, H = 128: its B-operand buffer covers
    the whole LDS footprint of the smaller instantiations).  LDS is not cleared between kernels, so a BPTT kernel that multiplies LDS it has not
    written itself (the padded k-steps of HP = 72 against the row padding) meets NaN instead of whatever the previous test left there.  Best effort:
    nothing is asserted about the poison itself."""
    M, T, H = 8192, 2, 128
    if not _LDS:
        _LDS.update(nan=torch.full((M * T * H,), float("nan"), device=DEV), half=torch.full((M * T * 4 * H,), 0.5, device=DEV),
                    w=torch.zeros(4 * H * H, device=DEV), dg=torch.empty(M * T * 4 * H, device=DEV))
    p = lambda k: lib.ptr(_LDS[k])
    lib.check(L.nir_lstm_train_bwd(p("nan"), None, None, None, p("half"), p("half"), None, None, p("w"), p("dg"), None, None, M, T, H, 1, lib.stream()), "stale LDS")


def _backward_once(d, inp, saved, L, lib):
    M, T, H, ndir, o, off = d["M"], d["T"], d["H"], d["ndir"], d["opt"], d["off"]
    lstm = inp["cell"] == "lstm"
    io = LSTM_IO if lstm else GRU_IO
    of = lambda k: off if k in io else 0
    n_out, n_st = M * T * ndir * H, ndir * M * H
    if lstm:
        bufs = dict(dgates=_guarded(4 * n_out, of("dgates")))
        bufs.update({k: _guarded(n_st) for k in ("dh0", "dc0") if o[k]})
    else:
        bufs = dict(dgx=_guarded(3 * n_out, of("dgx")), dq=_guarded(n_out, of("dq")))
    src = dict(dout=inp["dout"], dhn=inp["dhn"], dcn=inp["dcn"], dcst=inp["dcst"], c0=inp["c0"] if lstm else None, lengths=inp["lengths"],
               w_hh=inp["w_hh"], act=saved["act"], cst=saved.get("cst"), out=saved["out"])
    t = {k: _dev(v, of(k)) for k, v in src.items()}
    p = lambda k: lib.ptr(bufs[k][1]) if k in bufs else None
    q = lambda k: lib.ptr(t[k])
    if lstm:
        call = lambda: L.nir_lstm_train_bwd(q("dout"), q("dhn"), q("dcn"), q("dcst"), q("act"), q("cst"), q("c0"), q("lengths"), q("w_hh"), p("dgates"),
                                            p("dh0"), p("dc0"), M, T, H, ndir, lib.stream())
    else:
        call = lambda: L.nir_gru_train_bwd(q("dout"), q("dhn"), q("act"), q("out"), q("lengths"), q("w_hh"), p("dgx"), p("dq"), M, T, H, ndir, d["form"],
                                           lib.stream())
    if d["kernel"] in (LBM, GBM):
        _stale_lds(L, lib)
    ran = _profiled(L, lambda: lib.check(call(), d["op"]))
    torch.cuda.synchronize()
    return ran, bufs


def _run_backward(d):
    """-> the raw outputs (for the bit comparison of the cell-IO forms)"""
    from context_attentive_ir_amd import lib
    L = lib.load()
    M, T, H, ndir = d["M"], d["T"], d["H"], d["ndir"]
    chain = d["op"].endswith("chain")
    if chain:
        fd = dict(d, op="lstm_fwd" if d["op"] == "lstm_chain" else "gru_fwd", opt=dict(FWD_OPT, c0=d["opt"]["c0"]))
        inp, fran, fgot = _run_forward(fd, judge=False)
        pf = (B.predict_lstm_fwd if inp["cell"] == "lstm" else B.predict_gru_fwd)(M, T, H, ndir)
        assert fran == [(pf.kernel, 1)], fran
        saved = {k: fgot[k] for k in ("out", "act", "cst") if k in fgot}           # the kernel's own forward (NaN where it wrote nothing)
        f64, f32 = B.fwd_figures(inp)["ref"], B.fwd_figures(inp)["y32"]
        sh = [B.bwd_eval(inp, saved=s, shift=x) for s, x in zip(B.fwd_figures(inp)["shifted"], (B.DELTA, -B.DELTA))]
        fig = dict(ref=B.bwd_eval(inp, saved=f64), y32=B.bwd_eval(inp, np.float32, saved=f32), shifted=sh, lens=inp["lens"], ndir=ndir)
    else:
        inp = _make(d)
        saved, fig = B.saved_of(inp), B.bwd_figures(inp)
    ran, bufs = _backward_once(d, inp, saved, L, lib)
    io = LSTM_IO if inp["cell"] == "lstm" else GRU_IO
    got = _collect(bufs, M, T, H, ndir, io, d["off"])
    assert ran == [(d["kernel"], 1)], ran
    fam = B.family_of(d["kernel"])
    ok, r = B.accept(got, fig, family=fam)
    line = _report(d, fam, r)
    assert ok, line
    for m in np.flatnonzero(inp["lens"] == 0):             # length 0: the final-state gradient is handed through unchanged
        for k, k0 in (("dh0", "dhn"), ("dc0", "dcn")):
            if k in got:
                want = np.zeros((ndir, H), np.float32) if inp[k0] is None else inp[k0][:, m]
                assert np.array_equal(got[k][:, m], want), (k, m)
    _, again = _backward_once(d, inp, saved, L, lib)
    assert _bits_equal([bufs[k][1] for k in sorted(bufs)], [again[k][1] for k in sorted(again)]), "a second identical call gave other bits"
    return got


def _run(d):
    return _run_forward(d) if d["op"] in ("lstm_fwd", "lstm_split", "gru_fwd") else _run_backward(d)


def _ids(cases):
    return [d["id"] for d in cases]


@pytest.mark.parametrize("d", LSTM_BWD + GRU_BWD + HP72, ids=_ids(LSTM_BWD + GRU_BWD + HP72))
def test_bptt_dispatch(d):
    _run(d)


@pytest.mark.parametrize("d", FWD, ids=_ids(FWD))
def test_train_forward_dispatch(d):
    _run(d)


@pytest.mark.parametrize("d", VARIANTS, ids=_ids(VARIANTS))
def test_workgroup_raggedness_and_length_modes(d):
    _run(d)


@pytest.mark.parametrize("d", STATE, ids=_ids(STATE))
def test_final_and_initial_state_arguments(d):
    _run(d)


@pytest.mark.parametrize("d", CARRY, ids=_ids(CARRY))
def test_state_carry(d):
    _run(d)


@pytest.mark.parametrize("d", CHAIN, ids=_ids(CHAIN))
def test_chained_forward_backward(d):
    _run(d)


@pytest.mark.parametrize("cell,H,offs", CELL_IO, ids=["%s-H%d" % (a, h) for a, h, _ in CELL_IO])
def test_cell_io_forms_agree_bit_for_bit(cell, H, offs):
    """the matrix-core BPTT with its cell-IO buffers at 16-byte alignment, +8 bytes (8-byte pieces) and +4 bytes (scalar): each meets the criterion,
    all give the same bits"""
    res = [_run_backward(c(cell + "_bwd", LBM if cell == "lstm" else GBM, 17, 6, H, off=o, form=B.GRU_MFMA if cell == "gru" else 0)) for o in offs]
    for other in res[1:]:
        for k in res[0]:
            assert np.array_equal(res[0][k].view(np.int32), other[k].view(np.int32)), (cell, H, k)


# ------------------------------------------------------------------ the streaming cell kernels (element-wise; leading dimensions above the minimum)
PADC = 5               # padding columns of every strided buffer


def _strided(Bn, w, ld, fill=None):
    """[Bn, ld] between guards: the first w columns NaN (or `fill`: an input), the padding columns a sentinel -> (buffer, 2-D view)"""
    buf = torch.full((Bn * ld + 2 * GUARD,), SENT, device=DEV)
    v = buf[GUARD:GUARD + Bn * ld].view(Bn, ld)
    v[:, :w] = float("nan") if fill is None else torch.from_numpy(np.ascontiguousarray(fill, np.float32)).to(DEV)
    return buf, v


def _unstride(buf, Bn, w, ld, what):
    h = buf.cpu()
    body = h[GUARD:GUARD + Bn * ld].view(Bn, ld)
    assert bool((h[:GUARD] == SENT).all()) and bool((h[GUARD + Bn * ld:] == SENT).all()) and bool((body[:, w:] == SENT).all()), "wrote outside %s" % what
    return body[:, :w].numpy().copy()


def _judge_cell(name, got, ref, y32, shifted):
    ok, r = B.accept(got, dict(ref=ref, y32=y32, shifted=shifted, lens=None, ndir=1), family="cell")
    line = _report(dict(id=name), "cell", r)
    assert ok, line


CELL_SHAPES = [(b, h) for b in (1, 5, 257) for h in (1, 70, 200)]


@pytest.mark.parametrize("Bn,H", CELL_SHAPES)
def test_lstm_cell_kernels(Bn, H):
    from context_attentive_ir_amd import lib
    L = lib.load()
    rng = np.random.default_rng(Bn * 1000 + H)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    gx, gh, bias, cp = f32(rng.standard_normal((Bn, 4 * H))), f32(rng.standard_normal((Bn, 4 * H))), f32(rng.standard_normal(4 * H)), f32(rng.standard_normal((Bn, H)))
    dh1, dh2, dc1, dc2 = (f32(rng.standard_normal((Bn, H))) for _ in range(4))
    st = lib.stream()
    pre = lambda r: {"cell_" + k: v for k, v in r.items()}
    # ---- contiguous entries: c_prev given / NULL; (dh, dc) both, either NULL
    for has_cp in (True, False):
        gates = gx
        ref, y32 = B.lstm_cell_fwd(gates, cp if has_cp else None), B.lstm_cell_fwd(gates, cp if has_cp else None, np.float32)
        sh = [pre(B.lstm_cell_fwd(gates, cp if has_cp else None, shift=s)) for s in (B.DELTA, -B.DELTA)]
        ob = {k: _guarded(n) for k, n in (("act", Bn * 4 * H), ("c", Bn * H), ("h", Bn * H))}
        tg, tc = _dev(gates), _dev(cp if has_cp else None)
        lib.check(L.nir_lstm_cell_fwd(lib.ptr(tg), lib.ptr(tc), lib.ptr(ob["act"][1]), lib.ptr(ob["c"][1]), lib.ptr(ob["h"][1]), Bn, H, st), "lstm_cell_fwd")
        torch.cuda.synchronize()
        got = {"cell_" + k: _payload(b, v.numel(), k).reshape(ref[k].shape) for k, (b, v) in ob.items()}
        _judge_cell("lstm_cell_fwd-B%dH%d-cp%d" % (Bn, H, has_cp), got, pre(ref), pre(y32), sh)
        act32, c32 = f32(ref["act"]), f32(ref["c"])
        for has_dh, has_dc in ((True, True), (True, False), (False, True)):
            a = (dh1 if has_dh else None, dc1 if has_dc else None, act32, c32, cp if has_cp else None)
            rb, yb = B.lstm_cell_bwd(*a), B.lstm_cell_bwd(*a, dt=np.float32)
            shb = [pre(B.lstm_cell_bwd(*a, shift=s)) for s in (B.DELTA, -B.DELTA)]
            ob = {k: _guarded(n) for k, n in (("dgates", Bn * 4 * H), ("dc_prev", Bn * H))}
            t = [_dev(x) for x in a]
            lib.check(L.nir_lstm_cell_bwd(*[lib.ptr(x) for x in t], lib.ptr(ob["dgates"][1]), lib.ptr(ob["dc_prev"][1]), Bn, H, st), "lstm_cell_bwd")
            torch.cuda.synchronize()
            got = {"cell_" + k: _payload(b, v.numel(), k).reshape(rb[k].shape) for k, (b, v) in ob.items()}
            _judge_cell("lstm_cell_bwd-B%dH%d-cp%d-dh%d-dc%d" % (Bn, H, has_cp, has_dh, has_dc), got, pre(rb), pre(yb), shb)
    # ---- inside sequence buffers: gh / bias / neither, c_prev NULL, every NULL combination of the four gradient inputs
    ldg, lda, ldc = 4 * H + PADC, 4 * H + PADC + 2, H + PADC
    for mode, has_cp in (("gh", True), ("bias", False), ("none", True), ("bias", True)):
        add = gh if mode == "gh" else (np.broadcast_to(bias, gx.shape) if mode == "bias" else 0)
        cpv = cp if has_cp else None
        ev = lambda dt, s=0.0: B.lstm_cell_fwd(np.asarray(gx, dt) + np.asarray(add, dt), cpv, dt, s)
        ref, y32, sh = ev(np.float64), ev(np.float32), [pre(ev(np.float64, s)) for s in (B.DELTA, -B.DELTA)]
        bx, vx = _strided(Bn, 4 * H, ldg, gx)
        bc, vc = _strided(Bn, H, ldc, cp)
        oa, oc, oh = _strided(Bn, 4 * H, lda), _strided(Bn, H, ldc), _strided(Bn, H, ldc + 1)
        tgh, tb = _dev(gh if mode == "gh" else None), _dev(bias if mode != "none" else None)
        lib.check(L.nir_lstm_cell_seq_fwd(lib.ptr(vx), ldg, lib.ptr(tgh), lib.ptr(tb), lib.ptr(vc) if has_cp else None, ldc, lib.ptr(oa[1]), lda, lib.ptr(oc[1]),
                                          ldc, lib.ptr(oh[1]), ldc + 1, Bn, H, st), "lstm_cell_seq_fwd")
        torch.cuda.synchronize()
        got = dict(cell_act=_unstride(oa[0], Bn, 4 * H, lda, "act"), cell_c=_unstride(oc[0], Bn, H, ldc, "c"), cell_h=_unstride(oh[0], Bn, H, ldc + 1, "h"))
        _judge_cell("lstm_cell_seq_fwd-B%dH%d-%s-cp%d" % (Bn, H, mode, has_cp), got, pre(ref), pre(y32), sh)
        assert bool((_unstride(bx, Bn, 4 * H, ldg, "gx") == gx).all())
    act32, c32 = f32(ref["act"]), f32(ref["c"])            # of the last forward above (gates + bias, c_prev given)
    ba, va = _strided(Bn, 4 * H, lda, act32)
    bc, vc = _strided(Bn, H, ldc, c32)
    bp, vp = _strided(Bn, H, ldc + 2, cp)
    for mask in range(16):
        for has_cp in ((True, False) if mask == 15 else (True,)):
            on = [bool(mask >> i & 1) for i in range(4)]           # dh_step, dh_rec, dc_step, dc_rec
            res = {}
            for key, dt, s in (("ref", np.float64, 0.0), ("y32", np.float32, 0.0), ("p", np.float64, B.DELTA), ("m", np.float64, -B.DELTA)):
                dh = (np.asarray(dh1, dt) if on[0] else dt(0)) + (np.asarray(dh2, dt) if on[1] else dt(0))
                dc = (np.asarray(dc1, dt) if on[2] else dt(0)) + (np.asarray(dc2, dt) if on[3] else dt(0))
                res[key] = pre(B.lstm_cell_bwd(np.broadcast_to(dh, (Bn, H)), np.broadcast_to(dc, (Bn, H)), act32, c32, cp if has_cp else None, dt, s))
            s1, s3 = _strided(Bn, H, ldc, dh1), _strided(Bn, H, ldc + 3, dc1)
            t2, t4 = _dev(dh2), _dev(dc2)
            og, od = _strided(Bn, 4 * H, ldg), _guarded(Bn * H)
            lib.check(L.nir_lstm_cell_seq_bwd(lib.ptr(s1[1]) if on[0] else None, ldc, lib.ptr(t2) if on[1] else None, lib.ptr(s3[1]) if on[2] else None, ldc + 3,
                                              lib.ptr(t4) if on[3] else None, lib.ptr(va), lda, lib.ptr(vc), ldc, lib.ptr(vp) if has_cp else None, ldc + 2,
                                              lib.ptr(og[1]), ldg, lib.ptr(od[1]), Bn, H, st), "lstm_cell_seq_bwd")
            torch.cuda.synchronize()
            got = dict(cell_dgates=_unstride(og[0], Bn, 4 * H, ldg, "dgates"), cell_dc_prev=_payload(od[0], Bn * H, "dc_prev").reshape(Bn, H))
            _judge_cell("lstm_cell_seq_bwd-B%dH%d-mask%d-cp%d" % (Bn, H, mask, has_cp), got, res["ref"], res["y32"], [res["p"], res["m"]])


@pytest.mark.parametrize("Bn,H", CELL_SHAPES)
def test_gru_cell_kernels(Bn, H):
    from context_attentive_ir_amd import lib
    L = lib.load()
    rng = np.random.default_rng(Bn * 1000 + H + 1)
    f32 = lambda a: np.ascontiguousarray(a, np.float32)
    gx, gh, bhh, hp = f32(rng.standard_normal((Bn, 3 * H))), f32(rng.standard_normal((Bn, 3 * H))), f32(rng.standard_normal(3 * H)), f32(rng.uniform(-1, 1, (Bn, H)))
    d1, d2, d3 = (f32(rng.standard_normal((Bn, H))) for _ in range(3))
    st = lib.stream()
    pre = lambda r: {"cell_" + k: v for k, v in r.items()}
    ldg, lda, ldh = 3 * H + PADC, 4 * H + PADC + 2, H + PADC
    for has_gh, has_hp in ((True, True), (False, True), (False, False), (True, False)):
        g2, hv = gh if has_gh else bhh, hp if has_hp else None
        ref, y32 = B.gru_cell_fwd(gx, g2, hv), B.gru_cell_fwd(gx, g2, hv, np.float32)
        sh = [pre(B.gru_cell_fwd(gx, g2, hv, shift=s)) for s in (B.DELTA, -B.DELTA)]
        bx, vx = _strided(Bn, 3 * H, ldg, gx)
        bh_, vh = _strided(Bn, H, ldh + 1, hp)
        oa, oh = _strided(Bn, 4 * H, lda), _strided(Bn, H, ldh)
        tgh, tb = _dev(gh if has_gh else None), _dev(bhh)
        lib.check(L.nir_gru_cell_seq_fwd(lib.ptr(vx), ldg, lib.ptr(tgh), lib.ptr(tb), lib.ptr(vh) if has_hp else None, ldh + 1, lib.ptr(oa[1]), lda,
                                         lib.ptr(oh[1]), ldh, Bn, H, st), "gru_cell_seq_fwd")
        torch.cuda.synchronize()
        got = dict(cell_act=_unstride(oa[0], Bn, 4 * H, lda, "act"), cell_h=_unstride(oh[0], Bn, H, ldh, "h"))
        _judge_cell("gru_cell_seq_fwd-B%dH%d-gh%d-hp%d" % (Bn, H, has_gh, has_hp), got, pre(ref), pre(y32), sh)
    act32 = f32(ref["act"])
    ba, va = _strided(Bn, 4 * H, lda, act32)
    bp, vp = _strided(Bn, H, ldh + 1, hp)
    for mask in range(8):
        for has_hp in ((True, False) if mask == 7 else (True,)):
            on = [bool(mask >> i & 1) for i in range(3)]           # dh_step, dh_rec, dh_dir
            res = {}
            for key, dt in (("ref", np.float64), ("y32", np.float32)):
                dh = ((np.asarray(d1, dt) if on[0] else dt(0)) + (np.asarray(d2, dt) if on[1] else dt(0))) + (np.asarray(d3, dt) if on[2] else dt(0))
                res[key] = pre(B.gru_cell_bwd(np.broadcast_to(dh, (Bn, H)), act32, hp if has_hp else None, dt))
            s1 = _strided(Bn, H, ldh + 2, d1)
            t2, t3 = _dev(d2), _dev(d3)
            ox, og, od = _strided(Bn, 3 * H, ldg), _strided(Bn, 3 * H, ldg + 1), _guarded(Bn * H)
            lib.check(L.nir_gru_cell_seq_bwd(lib.ptr(s1[1]) if on[0] else None, ldh + 2, lib.ptr(t2) if on[1] else None, lib.ptr(t3) if on[2] else None,
                                             lib.ptr(va), lda, lib.ptr(vp) if has_hp else None, ldh + 1, lib.ptr(ox[1]), ldg, lib.ptr(og[1]), ldg + 1,
                                             lib.ptr(od[1]), Bn, H, st), "gru_cell_seq_bwd")
            torch.cuda.synchronize()
            got = dict(cell_dgx=_unstride(ox[0], Bn, 3 * H, ldg, "dgx"), cell_dgh=_unstride(og[0], Bn, 3 * H, ldg + 1, "dgh"),
                       cell_dh_dir=_payload(od[0], Bn * H, "dh_dir_out").reshape(Bn, H))
            _judge_cell("gru_cell_seq_bwd-B%dH%d-mask%d-hp%d" % (Bn, H, mask, has_hp), got, res["ref"], res["y32"], [])


# ------------------------------------------------------------------ refused arguments
def test_argument_errors_touch_nothing():
    from context_attentive_ir_amd import lib
    L = lib.load()
    assert [L.nir_gru_train_mfma_supported(h) for h in range(0, 131)] == [int(B.bwd_mfma_supported(h)) for h in range(0, 131)]
    buf, dummy = _guarded(64)
    dummy.fill_(1.0)
    dp, st = lib.ptr(dummy), lib.stream()
    for M, T, H, ndir in ((2, 3, 0, 2), (2, 3, 129, 2), (2, 3, 64, 3), (2, 0, 64, 2)):
        assert L.nir_lstm_train_fwd(dp, None, dp, None, None, dp, dp, dp, None, None, M, T, H, ndir, st) != 0
        assert L.nir_lstm_train_bwd(dp, None, None, None, dp, dp, None, None, dp, dp, None, None, M, T, H, ndir, st) != 0
        assert L.nir_gru_train_fwd(dp, None, dp, dp, dp, dp, None, M, T, H, ndir, st) != 0
        assert L.nir_gru_train_bwd(dp, None, dp, dp, None, dp, dp, dp, M, T, H, ndir, 0, st) != 0
    assert L.nir_gru_train_bwd(dp, None, dp, dp, None, dp, dp, dp, 2, 3, 33, 2, B.GRU_MFMA, st) != 0        # the matrix-core form does not take H = 33
    assert L.nir_gru_train_bwd(dp, None, dp, dp, None, dp, dp, dp, 2, 3, 32, 2, 3, st) != 0
    assert L.nir_lstm_train_fwd_split(dp, dp, None, dp, dp, dp, dp, dp, 2, 3, 64, 2, st) != 0               # 64 < H <= 128
    ran = _profiled(L, lambda: [lib.check(L.nir_lstm_train_fwd(dp, None, dp, None, None, dp, dp, dp, None, None, 0, 3, 64, 2, st), "M = 0"),
                                lib.check(L.nir_lstm_train_bwd(dp, None, None, None, dp, dp, None, None, dp, dp, None, None, 0, 3, 64, 2, st), "M = 0"),
                                lib.check(L.nir_gru_train_bwd(dp, None, dp, dp, None, dp, dp, dp, 0, 3, 64, 2, 0, st), "M = 0")])
    assert ran == []
    torch.cuda.synchronize()
    assert bool((_payload(buf, 64, "the dummy") == 1.0).all())
