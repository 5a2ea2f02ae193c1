"""GPU (-m gpu): every kernel form of CARS attention pooling, called through the C ABI (nir_attn_pool_f32: the dispatch nir_cars_encode and
nir_cars_encode_folded end in), against float64 on inputs the encoder never produces -- peaked logits, garbage in the padded tails, lengths
0 / out of range / NULL.  Each case asserts three things:
  * the profile report names the expected kernels, once each, and no other (a shape that lands elsewhere is moved, not the assertion);
  * the result meets the criterion of tests/attn_ref.py (fp32-chain error times a margin <= 4, plus what the formats and the fast
    transcendentals cost), a length-0 row is all NaN;
  * pooled sits between guard rows filled with a sentinel, and they stay untouched.
Tile counts are written against the CU count of the device (`ncu`), read from its properties: "3ncu+5" tiles give workgroups 4 and 3 tiles
of the pipeline (both plane buffers twice, the length ring fully cycled).  Every case prints one "ATTNENV" line before it asserts."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

import attn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0
D = R.D
ONE_TERM, PLAIN = 1, 2

# kernel form -> (expected launches, form of attn_ref, row_format, flags, tunables, bit 0 of `bounded`)
PIPE = {"attn_unfused_pipe": 2}
KERNELS = {
    "fused": (["attn_pool_fused_kernel"], "x2", 0, 0, {}, 1),
    "pipe<false,0>": (["attn_pool_pipe_kernel<false,0>"], "pipe0", 0, 0, PIPE, 1),
    "pipe<true,0>": (["attn_pool_pipe_kernel<true,0>"], "one0", 0, ONE_TERM, PIPE, 1),
    "pipe<true,1>": (["attn_pool_pipe_kernel<true,1>"], "one1", 1, 0, PIPE, 1),
    "pipe<false,1>": (["attn_pool_pipe_kernel<false,1>"], "row1", 3, 0, PIPE, 1),
    "pipe<false,2>": (["attn_pool_pipe_kernel<false,2>"], "pipe2", 2, 0, PIPE, 1),
    "pool2h": (["gemm3h_kernel", "attn_pool2_kernel"], "x2", 0, 0, {"attn_unfused": 1}, 1),
    "pool2b": (["gemm3_kernel", "attn_pool2_kernel"], "bf3", 0, 0, {"attn_unfused": 1}, 0),
    "plain": (["gemm_kernel", "rowdot_kernel", "attn_pool_kernel"], "f32", 0, PLAIN, {}, 1),
    "plain3": (["gemm3_kernel", "rowdot_kernel", "attn_pool_kernel"], "bf3", 0, PLAIN, {}, 1),     # a large plain launch: the bf16 three-term GEMM
    # selection by size alone
    "fused@size": (["attn_pool_fused_kernel"], "x2", 0, 0, {}, 1),
    "pipe@size": (["attn_pool_pipe_kernel<false,0>"], "pipe0", 0, 0, {}, 1),
    "fused@never": (["attn_pool_fused_kernel"], "x2", 0, 0, {"attn_unfused_pipe": 1}, 1),
}
PIPES = [k for k in KERNELS if k.startswith("pipe<")]


def c(kernel, T, tiles=None, M=None, fam="model", lens="ragged", floor=False):
    """One case.  tiles = (a, b, single_last): n = a * ncu + b tiles of 64 rows, all full (M * T = 64 n) or the last one holding a single
    sequence (M * T = 64 (n - 1) + T; a "+" in the id).  M: given directly instead (the unfused chains take any T)."""
    d = dict(kernel=kernel, T=T, tiles=tiles, M=M, fam=fam, lens=lens, floor=floor)
    d["id"] = "-".join([kernel, "T%d" % T, ("tiles=" + _tile_id(tiles)) if tiles else "M%d" % M, fam] + ["lens=" + lens] * (lens != "ragged") + ["floor"] * floor)
    return d


def _tile_id(t):
    a, b, last = t
    return (("%dncu" % a if a > 1 else "ncu") + ("%+d" % b if b else "") if a else "%d" % b) + ("+" if last else "")


def _rows(d, ncu):
    if d["M"] is not None:
        return d["M"]
    a, b, last = d["tiles"]
    n = a * ncu + b
    return (n - 1) * 64 // d["T"] + 1 if last else n * 64 // d["T"]


CASES = []
# ---- the single-role fused kernel: every T at one tile, two tiles, five tiles with a single sequence in the last; M = 1; every family
for T in (4, 8, 16, 32, 64):
    CASES += [c("fused", T, (0, 1, False)), c("fused", T, (0, 2, False), fam="peaked"), c("fused", T, (0, 5, True), fam="peaked" if T in (8, 32) else "model")]
CASES += [c("fused", 4, M=1), c("fused", 64, M=1, fam="peaked")]
for fam in R.FAMILIES:
    CASES += [c("fused", T, (0, 5, True), fam=fam, floor=fam.startswith("tiny")) for T in (16, 64) if (fam, T) != ("model", 16) and (fam, T) != ("model", 64)]
# ---- the pipeline, every instantiation: nk = 1 (one full tile of 16 ragged sequences); 3 tiles; workgroup 0 with two tiles; nk = 4 and 3; from 3 tiles on a last tile with one sequence
for k in PIPES:
    CASES += [c(k, 4, (0, 1, False)), c(k, 64, (0, 3, True), fam="peaked"), c(k, 4, (1, 1, True), fam="peaked"), c(k, 64, (1, 1, True)), c(k, 16, (3, 5, True), fam="peaked")]
for k in ("pipe<false,2>", "pipe<false,0>"):
    CASES += [c(k, 8, (0, 3, True)), c(k, 16, (0, 3, True), fam="peaked"), c(k, 32, (0, 3, True)), c(k, 32, (1, 1, True), fam="peaked")]
CASES += [c("pipe<false,2>", 16, (0, 3, True), fam=fam) for fam in R.FAMILIES if fam not in ("model", "peaked")]
CASES += [c("pipe<false,0>", 16, (0, 3, True), fam="tiny20", floor=True), c("pipe<false,0>", 64, (0, 3, True), fam="tiny", floor=True)]
# ---- selection by size, no tunable: the pipeline from 2 ncu tiles on
CASES += [c("fused@size", 16, (2, -1, False)), c("pipe@size", 16, (2, 0, False), fam="peaked"), c("fused@never", 16, (2, 0, False), fam="peaked")]
# ---- the unfused chains: T the fused kernels do not take (5, 21, 70 > a wave's 64 lanes: the strided loops run twice) and 16; M % 4 != 0;
# >= 6 017 rows reach the split-precision GEMMs (48 x 2 tiles of 128 x 128), 2 560 .. 6 016 rows the fp32-MFMA gemm_kernel
for T, Mbig, Msmall in ((5, 1205, 601), (21, 287, 143), (70, 87, 43), (16, 377, 189)):
    CASES += [c("pool2h", T, M=Mbig, fam="peaked" if T in (5, 70) else "model"), c("pool2b", T, M=Mbig, fam="model" if T in (5, 70) else "peaked"),
              c("plain", T, M=Msmall, fam="peaked" if T in (21, 16) else "model")]
CASES += [c("plain3", 16, M=377, fam="peaked")]
# ---- lengths: NULL, all T, all 1, out of range (clamped; -3 is a length of 0), one length 0 between ordinary ones
for k, T, tiles, M in (("fused", 16, (0, 5, True), None), ("pipe<false,2>", 16, (0, 3, True), None), ("pool2h", 21, None, 287), ("plain", 21, None, 143)):
    CASES += [c(k, T, tiles, M, fam="peaked", lens=mode) for mode in ("null", "full", "ones", "clamp", "zero")]


def _lens(mode, seed, M, T):
    if mode == "null":
        return None
    if mode in ("full", "ones"):
        return torch.full((M,), T if mode == "full" else 1, dtype=torch.int64)
    lens = R.ragged_lens(seed, M, T)
    if mode == "clamp":
        lens[1], lens[M - 2] = T + 5, -3
    elif mode == "zero":
        lens[M // 2 - 1], lens[M // 2], lens[M // 2 + 1] = max(T // 2, 1), 0, T
    return lens


def _profiled(L, fn):
    buf = C.create_string_buffer(1 << 16)
    L.nir_profile_report(buf, len(buf))                     # drop what earlier tests left
    L.nir_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.nir_profile_enable(0)
    L.nir_profile_report(buf, len(buf))
    out = []
    for ln in buf.value.decode().strip().splitlines():
        name, launches, _ = ln.rsplit(",", 2)
        out.append((re.sub(r"\[M=[^\]]*\]$", "", name), int(launches)))
    return out


class _Tunables(object):
    def __init__(self, tun):
        from context_attentive_ir_amd import lib
        self.ctx = [lib.tunable(k, v, 0) for k, v in tun.items()]

    def __enter__(self):
        for t in self.ctx:
            t.__enter__()

    def __exit__(self, *exc):
        for t in reversed(self.ctx):
            t.__exit__(*exc)
        return False


def _stage(form, h):
    """(what the kernel is handed, as a CPU tensor; what attn_ref.operands decodes)"""
    if form == "pipe2":
        raw = R.encode_pairs(h.numpy())
    elif form in ("row1", "one1"):
        raw = R.encode_f16_rows(h.numpy())
    else:
        return h, h
    return torch.from_numpy(raw), raw


class _Call(object):
    """nir_attn_pool_f32 on one set of weights: device copies, the weights struct, a guarded pooled"""

    def __init__(self, w, M, T, kernel, d=D):
        from context_attentive_ir_amd import lib
        self.lib, self.L = lib, lib.load()
        self.names, self.form, self.rf, self.flags, self.tun, bounded = KERNELS[kernel]
        self.M, self.T, self.d = M, T, d
        self.keep = {k: w[k].to(DEV) for k in ("W0", "b0", "w3", "b3")}
        if d == D:
            self.keep["frag"] = R.w0_fragments(self.keep["W0"])
        self.ws = lib.CarsEncoderWeights()
        self.ws.attn0_w, self.ws.attn0_b = self.keep["W0"].data_ptr(), self.keep["b0"].data_ptr()
        self.ws.attn3_w, self.ws.attn3_b = self.keep["w3"].data_ptr(), self.keep["b3"].data_ptr()
        self.ws.H, self.ws.bounded = d // 2, bounded
        self.ws.attn_frag = self.keep["frag"].data_ptr() if d == D else None
        nbytes = int(self.L.nir_attn_pool_workspace_bytes(M, T, d))
        self.work = torch.empty(nbytes, dtype=torch.uint8, device=DEV) if len(self.names) > 1 else None
        self.nbytes = nbytes if self.work is not None else 0

    def run(self, rows_cpu, lens, rf=None, flags=None):
        """(launches, pooled [M, d] on the CPU); the guard rows are checked"""
        lib = self.lib
        rd = rows_cpu.to(DEV).contiguous()
        ld = None if lens is None else lens.to(DEV)
        buf = torch.full((self.M + 3, self.d), SENT, device=DEV)
        out = buf[1:]
        self.buf = buf
        with _Tunables(self.tun):
            ran = _profiled(self.L, lambda: lib.check(self.L.nir_attn_pool_f32(
                lib.ptr(rd), self.rf if rf is None else rf, C.byref(self.ws), lib.ptr(ld), self.M, self.T, self.d, self.flags if flags is None else flags,
                lib.ptr(self.work), self.nbytes, lib.ptr(out), lib.stream()), "nir_attn_pool_f32"))
        g = buf.cpu()
        assert bool((g[0] == SENT).all()) and bool((g[1 + self.M:] == SENT).all()), "wrote outside pooled [M, D]"
        return ran, g[1:1 + self.M].clone()


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _run(d):
    ncu = _ncu()
    M, T = _rows(d, ncu), d["T"]
    seed = 1000 * T + M % 997 + len(d["fam"]) + len(d["kernel"])
    w = R.family(d["fam"], seed, M, T)
    lens = _lens(d["lens"], seed, M, T)
    call = _Call(w, M, T, d["kernel"])
    handed, raw = _stage(call.form, w["h"])
    ran, got = call.run(handed, lens)
    assert ran == sorted((n, 1) for n in call.names), (ran, M, T, ncu)      # (the report is sorted by name)
    assert d["tiles"] is None or (M * T + 63) // 64 == d["tiles"][0] * ncu + d["tiles"][1]
    rows, W0 = R.operands(call.form, raw, w["W0"])
    ok, r = R.accept(got, call.form, rows, W0, w["b0"], w["w3"], w["b3"], lens, floor=d["floor"])
    line = "ATTNENV,%s,M=%d,%s,e=%.3g,e32=%.3g,fmt=%.3g,act=%.3g,floor=%.3g,ratio=%.3f,bound=%.3g" % (
        d["id"], M, "+".join(call.names), r["e"], r["e32"], r["fmt"], r["act"], r["floor"], r["ratio"], r["bound"])
    print(line)
    assert ok, line
    if d["fam"] == "uniform":                                # w3 = 0: the plain mean over the valid steps, whatever the GEMM and tanh did
        n = R.clamp_lens(lens, M, T)
        mean = torch.stack([rows[m, :n[m]].mean(0) for m in range(M)])
        assert float((got.double() - mean).abs().max()) <= (T + 2) * 2.0 ** -24 * float(rows.abs().max()), line     # 1 / len and T fp32 FMAs


@pytest.mark.parametrize("d", CASES, ids=[d["id"] for d in CASES])
def test_attn_pool(d):
    _run(d)


PADDED = [("fused", 16, (0, 5, True), None), ("pipe<false,0>", 8, (1, 1, True), None), ("pipe<true,0>", 16, (0, 3, True), None), ("pipe<true,1>", 32, (0, 3, True), None),
          ("pipe<false,1>", 4, (0, 3, True), None), ("pipe<false,2>", 16, (1, 1, True), None), ("pool2h", 21, None, 287), ("pool2b", 70, None, 87),
          ("plain", 5, None, 601)]


@pytest.mark.parametrize("kernel,T,tiles,M", PADDED, ids=[p[0] for p in PADDED])
def test_padded_rows_never_reach_pooled(kernel, T, tiles, M):
    """rows at t >= len filled with seeded finite garbage in (-1, 1) against zero tails: bit for bit the same pooled (a masked row has
    probability exactly 0 and its own logit is never read)"""
    d = c(kernel, T, tiles, M, fam="peaked")
    M = _rows(d, _ncu())
    w = R.family("peaked", 77 + T, M, T)
    lens = R.ragged_lens(T, M, T)
    lens[0] = 1
    mask = (torch.arange(T)[None, :] < lens[:, None])[:, :, None]
    garbage = torch.rand(M, T, D, generator=torch.Generator().manual_seed(5)) * 1.998 - 0.999
    call = _Call(w, M, T, kernel)
    ran0, zero = call.run(_stage(call.form, torch.where(mask, w["h"], torch.zeros(())))[0], lens)
    ran1, junk = call.run(_stage(call.form, torch.where(mask, w["h"], garbage))[0], lens)
    assert ran0 == ran1 == sorted((n, 1) for n in call.names), (ran0, ran1)
    assert bool(torch.isfinite(zero).all()) and float(zero.abs().max()) > 0
    assert torch.equal(zero.view(torch.int32), junk.view(torch.int32)), "padded rows moved pooled by %g" % float((zero - junk).abs().max())


def test_refused_arguments_leave_pooled_untouched():
    from context_attentive_ir_amd import lib
    L = lib.load()
    M, T = 8, 16
    w = R.family("model", 3, M, T)

    def refused(match, kernel="fused", rows="h", rf=None, flags=None, tun=None, d=D, patch=None):
        wd = w if d == D else R.family("model", 3, M, T, d)
        call = _Call(wd, M, T, kernel, d)
        if tun is not None:
            call.tun = tun
        if patch:
            patch(call)
        form = {1: "one1", 2: "pipe2", 3: "row1"}.get(rf, "x2")
        with pytest.raises(RuntimeError, match=match):
            call.run(_stage(form, wd["h"])[0], None, rf=rf, flags=flags)
        assert bool((call.buf == SENT).all()), "a refused call wrote pooled"

    for rf in (1, 2, 3):                                                   # fp16 rows / term pairs, the pipeline not selected
        refused("pipelined kernel", rf=rf)
    refused("term-pair rows", rf=2, flags=ONE_TERM, tun=PIPE)
    refused("only taken by the fused pipeline", rf=1, d=128, tun=PIPE)      # D != 256: no fused kernel to take them
    refused("only taken by the fused pipeline", rf=2, tun={"attn_unfused": 1})
    refused("needs D % 64 == 0", d=48)                                      # attn_pool2_kernel reads D / 16 partials four at a time
    refused("unknown row format", rf=4)
    refused("null attention weight", patch=lambda call: setattr(call.ws, "attn3_w", None))
    refused("workspace too small", kernel="plain", patch=lambda call: setattr(call, "nbytes", 64))
    call = _Call(w, M, T, "fused")
    buf = torch.full((M, D), SENT, device=DEV)
    rows = w["h"].to(DEV)
    for args in ((None, C.byref(call.ws), lib.ptr(buf)), (lib.ptr(rows), None, lib.ptr(buf)), (lib.ptr(rows), C.byref(call.ws), None)):
        rc = L.nir_attn_pool_f32(args[0], 0, args[1], None, M, T, D, 0, None, 0, args[2], lib.stream())
        assert rc != 0 and b"null pointer" in L.nir_last_error_string()
    assert L.nir_attn_pool_f32(lib.ptr(rows), 0, C.byref(call.ws), None, 0, T, D, 0, None, 0, lib.ptr(buf), lib.stream()) == 0    # M = 0
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())
    ran, got = call.run(w["h"], None)                                       # and the library is still usable
    assert ran == [("attn_pool_fused_kernel", 1)] and bool(torch.isfinite(got).all())


@pytest.mark.parametrize("d,kernel,names", [(128, "pool2h", ["gemm16_kernel", "attn_pool2_kernel"]),
                                            (48, "plain", ["gemm16_kernel", "rowdot_kernel", "attn_pool_kernel"])])
def test_small_d_takes_an_unfused_chain(d, kernel, names):
    """D = 128: no fused kernel applies, the call lands on the tanh-rowdot GEMM plus attn_pool2_kernel without any tunable.  D = 48 (no
    multiple of 64: refused without the flag, test_refused_arguments) is taken by the plain chain."""
    M, T = 37, 9
    w = R.family("peaked", 11, M, T, d)
    lens = R.ragged_lens(2, M, T)
    call = _Call(w, M, T, kernel, d)
    call.tun, call.names = {}, names
    ran, got = call.run(w["h"], lens)
    assert ran == sorted((n, 1) for n in call.names), ran
    ok, r = R.accept(got, "f32", w["h"].double(), w["W0"].double(), w["b0"], w["w3"], w["b3"], lens)
    print("ATTNENV,D%d,e=%.3g,e32=%.3g,act=%.3g,ratio=%.3f,bound=%.3g" % (d, r["e"], r["e32"], r["act"], r["ratio"], r["bound"]))
    assert ok, r
