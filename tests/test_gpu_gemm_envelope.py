"""GPU (-m gpu): every dispatch path of nir_linear_ex_f32 (csrc/gemm.hip: launch_linear_ex) and every epilogue of gemm_store, called through the
C ABI, against float64.  Each case asserts three things:
  * the profile report names the expected kernel, once, and no other (a shape that lands elsewhere is moved, not the assertion);
  * the result meets the criterion of tests/gemm_ref.py (fp32-chain error times a margin <= 4, plus what the operand format costs);
  * C is allocated with ldc = N_out + 3 and guard rows in front and behind, filled with a sentinel: nothing outside [M, N_out] is written.
The name does not tell the one- from the two-k-tiles-per-stage form of the fp16 kernel: that follows from K >= 64 and the mode alone.
Every case prints one "GEMMENV" line with its figures before it asserts (pytest -s); DESIGN.md section 2 quotes the largest per family."""
import ctypes as C
import re

import pytest
import torch

import gemm_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0
LSEQ = 41             # seq_stride of the gathered cases; rows_per_seq = LSEQ - taps + 1 (< seq_stride once there are two taps)
VOCAB = 500


def _form(kernel):
    base = kernel.split("[")[0]
    return "bf16x3" if base == "gemm3_kernel" else "fp16x2" if base in ("gemm3h_kernel", "gemm_h2p_kernel") else "f32"


def c(kernel, M, N, K, fam="randn", act=0, bounded=False, E=0, bias="b", add=False, lda=0, woff=0, exact=False, floor=False):
    """One case.  E > 0: A is gathered from a [VOCAB, E] table (taps = ceil(K / E)); bias "b" / "bb" / "": bias, bias + bias2, both NULL;
    add: the addend [M, N + 5] (the [N] weight row under ACT_TANH_ROWDOT16); lda: extra floats per A row; woff: W starts that many floats
    past an aligned address; exact: under the exact_f32 tunable; floor: judged with the subnormal floor of the fp16 format."""
    d = dict(kernel=kernel, M=M, N=N, K=K, fam=fam, act=act, bounded=bounded, E=E, bias=bias, add=add, lda=lda, woff=woff, exact=exact,
             floor=floor)
    tags = [kernel, "%dx%dx%d" % (M, N, K), fam] + (["E%d" % E] if E else []) + (["act%d" % act] if act else [])
    tags += ["bias=%s" % (bias or "none")] * (bias != "b") + ["add"] * bool(add) + ["lda+%d" % lda] * bool(lda) + ["w+%d" % woff] * bool(woff)
    tags += ["exact"] * exact + ["floor"] * floor
    d["id"] = "-".join(tags)
    return d


H = dict(bounded=True)
DISPATCH = [
    # ---- gemm3_kernel, dense: the threshold edges of the dispatcher (96 tiles of 128 x 128, N >= 96, K >= 32), K tails, ragged M and N
    c("gemm3_kernel", 12161, 128, 64), c("gemm_kernel", 12160, 128, 64),
    c("gemm3_kernel", 12161, 96, 64, "positive"), c("gemm_kernel", 12161, 95, 64, "positive"),
    c("gemm3_kernel", 12161, 128, 32, "mixed"), c("gemm_kernel", 12161, 128, 28, "mixed"),
    c("gemm3_kernel", 12289, 129, 36), c("gemm3_kernel", 12161, 128, 136, "positive"), c("gemm3_kernel", 12161, 130, 300, "mixed"),
    c("gemm3_kernel", 12161, 128, 900, "positive"), c("gemm3_kernel", 12161, 128, 300, "tiny"), c("gemm3_kernel", 12161, 128, 1024),
    # ---- gemm3_kernel[gather]: mode 1 (K = E, K < E), mode 2 (2 and 3 taps, the third one partial), E = 300 and 64
    c("gemm3_kernel[gather]", 12289, 128, 300, E=300), c("gemm3_kernel[gather]", 12289, 128, 256, "positive", E=300),
    c("gemm3_kernel[gather]", 12289, 128, 64, "mixed", E=64), c("gemm3_kernel[gather]", 12289, 128, 600, "mixed", E=300),
    c("gemm3_kernel[gather]", 12289, 130, 900, "positive", E=300), c("gemm3_kernel[gather]", 12289, 128, 128, E=64),
    c("gemm3_kernel[gather]", 12289, 128, 192, "positive", E=64), c("gemm3_kernel[gather]", 12289, 128, 160, "tiny", E=64),
    # ---- gemm3h_kernel (0x100): one k-tile per stage (K < 64), two per stage (80: odd tile count; 72, 136: partial last tile), every family
    c("gemm3h_kernel", 12161, 128, 32, **H), c("gemm3h_kernel", 12161, 128, 48, "positive", **H), c("gemm3h_kernel", 12161, 128, 60, "mixed", **H),
    c("gemm3h_kernel", 12161, 128, 64, "edge", **H), c("gemm3h_kernel", 12161, 128, 72, "tiny", **H), c("gemm3h_kernel", 12161, 128, 80, **H),
    c("gemm3h_kernel", 12161, 128, 96, "positive", **H), c("gemm3h_kernel", 12289, 129, 136, "mixed", **H),
    c("gemm3h_kernel", 12161, 128, 300, "edge", **H), c("gemm3h_kernel", 3073, 512, 1024, **H), c("gemm3h_kernel", 12161, 128, 136, "tiny", **H),
    c("gemm3h_kernel", 12161, 128, 300, "tiny20", floor=True, **H), c("gemm3h_kernel", 12161, 128, 48, "tiny20", floor=True, **H),
    c("gemm3h_kernel[gather]", 12289, 128, 300, "edge", E=300, **H), c("gemm3h_kernel[gather]", 12289, 128, 64, E=64, **H),
    c("gemm3h_kernel[gather]", 12289, 128, 48, "positive", E=64, **H),
    # mode 2 stays on the one-tile form at any K
    c("gemm3h_kernel[gather]", 12289, 128, 128, "mixed", E=64, **H), c("gemm3h_kernel[gather]", 12289, 130, 900, "positive", E=300, **H),
    c("gemm3h_kernel[gather]", 12289, 128, 600, "tiny", E=300, **H),
    # ---- gemm_kernel: vectorised above (12160 x 128 x 64, K = 28); scalar loads: K % 4, lda = K + 1, W one float off, E % 4; gathers the
    # split kernels do not take: five taps (K > 3E), N < 96 with 2 and 3 taps
    c("gemm_kernel", 2000, 330, 301), c("gemm_kernel", 2000, 330, 300, "positive", lda=1), c("gemm_kernel", 2000, 330, 300, "mixed", woff=1),
    c("gemm_kernel[gather]", 20000, 70, 30, E=30), c("gemm_kernel[gather]", 12161, 130, 320, "positive", E=64),
    c("gemm_kernel[gather]", 12161, 130, 150, "mixed", E=30), c("gemm_kernel[gather]", 12161, 80, 192, E=64),
    c("gemm_kernel[gather]", 12161, 80, 128, "positive", E=64),
    # ---- gemm16_kernel: K < 512, K >= 512 (look-ahead branch), scalar loads, degenerate sizes, gathers with taps
    c("gemm16_kernel", 37, 40, 300), c("gemm16_kernel", 100, 50, 768, "positive"), c("gemm16_kernel", 33, 200, 1040, "mixed"),
    c("gemm16_kernel", 16, 2048, 768), c("gemm16_kernel", 130, 50, 30), c("gemm16_kernel", 5, 1, 7), c("gemm16_kernel", 40, 70, 515, "positive"),
    c("gemm16_kernel", 4095, 40, 300), c("gemm16_kernel[gather]", 200, 33, 60, E=20), c("gemm16_kernel[gather]", 200, 33, 90, "mixed", E=30),
    c("gemm16_kernel[gather]", 300, 50, 64, "positive", E=64),
    # ---- gemm32_kernel: 2, 3 and 5 row tiles per workgroup at 256 CUs (test_gemm32_row_tile_choice), K = 256 forces 2
    c("gemm32_kernel", 2114, 96, 512), c("gemm32_kernel", 2723, 96, 512, "positive"), c("gemm32_kernel", 4097, 98, 512, "mixed"),
    c("gemm32_kernel", 1120, 512, 1024), c("gemm32_kernel", 1101, 250, 256, "positive"),
    c("gemm32_kernel", 4096, 64, 512),                      # one float too many for the skinny kernel's 128 KB of LDS
    # ---- gemm_skinny_kernel: 1 .. 4 column tiles, the M and LDS thresholds, gathered, with an addend
    c("gemm_skinny_kernel", 4096, 7, 300), c("gemm_skinny_kernel", 5000, 17, 140, "positive"), c("gemm_skinny_kernel", 4096, 40, 300, "mixed"),
    c("gemm_skinny_kernel", 4100, 64, 300), c("gemm_skinny_kernel", 4096, 64, 496, "positive"),
    c("gemm_skinny_kernel[gather]", 20608, 40, 300, E=300), c("gemm_skinny_kernel[gather]", 4099, 64, 64, "positive", E=64),
    c("gemm_skinny_kernel[gather]", 9000, 7, 300, "mixed", E=300), c("gemm_skinny_kernel[gather]", 5000, 33, 128, E=300),
    c("gemm_skinny_kernel", 4096, 40, 300, add=True), c("gemm_skinny_kernel", 4100, 64, 300, act=1, add=True, bias="bb"),
    # ---- the exact_f32 tunable sends gemm3 shapes to the fp32-MFMA kernel: format term 0
    c("gemm_kernel", 12161, 128, 300, exact=True), c("gemm_kernel[gather]", 12289, 128, 900, E=300, exact=True),
]

# kernel -> (M, N) of the epilogue cases, (M, [N ...]) of the row-dot ones: ragged M everywhere, N = 130 is even with N / 2 odd and no
# multiple of any tile; the split kernels need N >= 96, so only N = 272 reaches them with the row-dot epilogue
EPI_BASE = {
    "gemm3_kernel": dict(M=6200, N=130, rd=[(4200, 272)]),
    "gemm3h_kernel": dict(M=6200, N=130, rd=[(4200, 272)]),
    "gemm_kernel": dict(M=3500, N=130, rd=[(12000, 16), (12001, 48), (2100, 272)]),
    "gemm16_kernel": dict(M=45, N=130, rd=[(45, 16), (45, 48), (45, 272)]),
    "gemm32_kernel": dict(M=1300, N=130, rd=[(6401, 16), (3201, 48), (801, 272)]),
}


def _epilogues():
    out = []
    for kernel, b in EPI_BASE.items():
        kw = dict(bounded=kernel == "gemm3h_kernel")
        M, N, K = b["M"], b["N"], 64
        out += [c(kernel, M, N, K, "positive", **kw), c(kernel, M, N, K, bias="bb", **kw), c(kernel, M, N, K, "positive", bias="", **kw),
                c(kernel, M, N, K, act=R.ACT_TANH, **kw), c(kernel, M, N, K, act=R.ACT_RELU, **kw),
                c(kernel, M, N, K, act=R.ACT_MAXOUT2, **kw), c(kernel, M, N, K, "positive", act=R.ACT_MAXOUT2, bias="bb", add=True, **kw),
                c(kernel, M, N, K, bias="", add=True, **kw), c(kernel, M, N, K, act=R.ACT_TANH, add=True, **kw),
                c(kernel, M, N, 48, "tiny", act=R.ACT_TANH, bias="bb", **kw)]
        out += [c(kernel, m, n, K, act=R.ACT_TANH_ROWDOT16, add=True, **kw) for m, n in b["rd"]]
    return out


EPILOGUES = _epilogues()
FIGURES = []


def _profiled(L, fn):
    """[(kernel name with its [gather] part, launches)] of the library's launches inside fn()"""
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


def _guarded(M, n_out):
    """C with ldc = n_out + 3, one guard row in front and two behind, all sentinel; returns (buffer, view of the rows the call may write)"""
    buf = torch.full((M + 3, n_out + 3), SENT, device=DEV)
    return buf, buf[1:]


def _check_guard(buf, M, n_out):
    g = buf.cpu().clone()
    inside = g[1:1 + M, :n_out].clone()
    g[1:1 + M, :n_out] = SENT
    assert bool((g == SENT).all()), "wrote outside [M, N_out]: %d elements" % int((g != SENT).sum())
    return inside


def _judge(case_id, kernel, got, a, w, bias, bias2, add, act, floor=None):
    ok, r = R.accept(got, a, w, bias, bias2, add, act, form=_form(kernel), floor=floor)
    line = "GEMMENV,%s,%s,e=%.3g,e_chain=%.3g,extra=%.3g,ratio=%.3f,bound=%.3g" % (case_id, kernel, r["e"], r["e_chain"], r["extra"], r["ratio"],
                                                                                  r["bound"])
    print(line)
    FIGURES.append(line)
    assert ok, line


def _run(d):
    from context_attentive_ir_amd import lib
    L = lib.load()
    M, N, K, E, act, fam = d["M"], d["N"], d["K"], d["E"], d["act"], d["fam"]
    g = torch.Generator().manual_seed(M * 1000 + N * 7 + K + len(fam))
    w = R.family(fam, g, N, K, "w")
    ids = table = None
    rps = ss = 0
    if E:
        taps = (K + E - 1) // E
        rps, ss = LSEQ - taps + 1, LSEQ
        table = R.family(fam, g, VOCAB, K, "a", cols=E)
        ids = torch.randint(0, VOCAB, ((M + rps - 1) // rps, LSEQ), generator=g)
        a = R.gather_rows(table, ids, E, K, rps, ss, M)
    else:
        a = R.family(fam, g, M, K, "a")
    scale = float((a[:256].double() @ w[:256].double().t()).std()) or 1.0      # bias and addend on the scale of the products
    bias = torch.randn(N, generator=g) * scale if d["bias"] else None
    bias2 = torch.randn(N, generator=g) * scale if d["bias"] == "bb" else None
    add = None
    if d["add"]:
        add = torch.randn(N, generator=g) / 4 if act == R.ACT_TANH_ROWDOT16 else torch.randn(M, N, generator=g) * scale
    n_out = N // 2 if act == R.ACT_MAXOUT2 else N // 16 if act == R.ACT_TANH_ROWDOT16 else N

    dev = lambda t: None if t is None else t.to(DEV)
    lda = K + d["lda"]
    ad = None
    if not E:
        ad = torch.full((M, lda), 3.0, device=DEV)
        ad[:, :K] = a.to(DEV)
    wbuf = torch.zeros(N * K + 8, device=DEV)
    wd = wbuf[d["woff"]:d["woff"] + N * K].view(N, K)
    wd.copy_(w)
    assert wd.data_ptr() % 16 == 4 * d["woff"]
    idd, td, bd, b2d = dev(ids), dev(table), dev(bias), dev(bias2)
    ldadd = 0
    addd = dev(add)
    if add is not None and add.dim() == 2:
        ldadd = N + 5
        addd = torch.full((M, ldadd), 1e30, device=DEV)
        addd[:, :N] = add.to(DEV)
    buf, cv = _guarded(M, n_out)

    def call():
        lib.check(L.nir_linear_ex_f32(lib.ptr(ad), lda if not E else 0, lib.ptr(idd), lib.ptr(td), E, rps, ss, lib.ptr(wd), K, lib.ptr(bd),
                                      lib.ptr(b2d), lib.ptr(cv), n_out + 3, M, N, K, act | (R.ACT_BOUNDED if d["bounded"] else 0),
                                      lib.ptr(addd), ldadd, lib.stream()), "nir_linear_ex_f32")

    if d["exact"]:
        with lib.tunable("exact_f32", 1, 0):
            ran = _profiled(L, call)
    else:
        ran = _profiled(L, call)
    assert ran == [(d["kernel"], 1)], ran
    got = _check_guard(buf, M, n_out)
    _judge(d["id"], d["kernel"], got, a, w, bias, bias2, add, act, R.subnormal_floor(a, w) if d["floor"] else None)


@pytest.mark.parametrize("d", DISPATCH, ids=[d["id"] for d in DISPATCH])
def test_linear_ex_dispatch(d):
    _run(d)


@pytest.mark.parametrize("d", EPILOGUES, ids=[d["id"] for d in EPILOGUES])
def test_linear_ex_epilogue(d):
    _run(d)


def test_every_split_kernel_sees_every_input_family():
    for kernel in ("gemm3_kernel", "gemm3h_kernel"):
        fams = {d["fam"] for d in DISPATCH if d["kernel"].split("[")[0] == kernel}
        want = {"randn", "positive", "mixed", "tiny"} | ({"edge", "tiny20"} if kernel == "gemm3h_kernel" else set())
        assert want <= fams, (kernel, want - fams)


def test_gemm32_row_tile_choice_covers_2_3_5():
    """The row tiles per workgroup are not in the kernel's name: recompute the launcher's choice (fewest rounds of workgroups over the CUs
    times the rows per workgroup, 2 .. 6, 2 alone under K = 512) for the gemm32 cases above on this device."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    chosen = set()
    for d in DISPATCH:
        if d["kernel"] != "gemm32_kernel":
            continue
        ncol = (d["N"] + 31) // 32
        cost = {ra: (((d["M"] + 16 * ra - 1) // (16 * ra)) * ncol + ncu - 1) // ncu * ra for ra in range(2, (6 if d["K"] >= 512 else 2) + 1)}
        chosen.add(min(cost, key=lambda ra: (cost[ra], ra)))        # first strict minimum, as the launcher's loop
    assert {2, 3, 5} <= chosen, (ncu, chosen)


def test_epilogue_argument_errors_leave_the_library_usable():
    with pytest.raises(RuntimeError, match="even N"):
        _run(c("gemm16_kernel", 45, 131, 64, act=R.ACT_MAXOUT2))
    with pytest.raises(RuntimeError, match="tanh-rowdot"):
        _run(c("gemm16_kernel", 45, 48, 64, act=R.ACT_TANH_ROWDOT16))               # no weight row
    with pytest.raises(RuntimeError, match="tanh-rowdot"):
        _run(c("gemm16_kernel", 45, 40, 64, act=R.ACT_TANH_ROWDOT16, add=True))     # N % 16 != 0
    _run(c("gemm16_kernel", 45, 48, 64, act=R.ACT_TANH_ROWDOT16, add=True))


@pytest.mark.parametrize("taps,M,N,fam,act", [(1, 5000, 130, "randn", 1), (3, 5000, 130, "positive", 0), (3, 4099, 256, "edge", 0),
                                              (1, 13000, 300, "mixed", 2), (3, 700, 96, "tiny", 1)])
def test_linear_planes_gathered(taps, M, N, fam, act):
    """nir_linear_planes_f32 with plane TABLES gathered by token id over 1 and 3 taps (E = 300 -> EP = 304: every tap ends in a partial
    16-byte chunk of zero padding, K = taps * 304 in a partial k-tile) against float64."""
    from context_attentive_ir_amd import lib
    L = lib.load()
    E, EP = 300, 304
    K = taps * E
    g = torch.Generator().manual_seed(M + N + taps)
    w = R.family(fam, g, N, K, "w")                                                 # [N][taps][E]
    table = R.family(fam, g, VOCAB, K, "a", cols=E)
    rps = LSEQ - taps + 1
    ids = torch.randint(0, VOCAB, ((M + rps - 1) // rps, LSEQ), generator=g)
    a = R.gather_rows(table, ids, E, K, rps, LSEQ, M)
    scale = float((a[:256].double() @ w[:256].double().t()).std()) or 1.0
    bias = torch.randn(N, generator=g) * scale
    t1, t2 = lib.split_f16x2(table.to(DEV), EP)
    w1, w2 = lib.split_f16x2(w.reshape(N * taps, E).to(DEV), EP)                    # [N * taps, EP] == [N, taps * EP]
    idd, bd = ids.to(DEV), bias.to(DEV)
    buf, cv = _guarded(M, N)
    ran = _profiled(L, lambda: lib.check(L.nir_linear_planes_f32(lib.ptr(t1), lib.ptr(t2), EP, lib.ptr(idd), rps, LSEQ, EP, taps, lib.ptr(w1),
                                                                 lib.ptr(w2), taps * EP, lib.ptr(bd), lib.ptr(cv), N + 3, M, N, taps * EP, act,
                                                                 lib.stream()), "nir_linear_planes_f32"))
    assert ran == [("gemm_h2p_kernel[gather]", 1)], ran
    got = _check_guard(buf, M, N)
    _judge("planes-%dtaps-%dx%d-%s-act%d" % (taps, M, N, fam, act), "gemm_h2p_kernel[gather]", got, a, w, bias, None, None, act)


@pytest.mark.parametrize("K", [1, 7, 256, 900])
@pytest.mark.parametrize("M", [1, 3, 4, 4099])
def test_rowdot(M, K):
    """nir_rowdot_f32 (one wave per row, four rows per workgroup): M around the workgroup, K below / at / above a wave's 64 lanes, ldx > K,
    with and without bias, plain and tanh."""
    from context_attentive_ir_amd import lib
    L = lib.load()
    g = torch.Generator().manual_seed(M * 31 + K)
    act = R.ACT_TANH if (M + K) % 2 else R.ACT_NONE
    fam = ("randn", "positive", "mixed")[(M + K) % 3] if act == R.ACT_NONE else "randn"
    x = R.family(fam, g, M, K, "a")
    w = R.family(fam, g, 1, K, "w")
    b = torch.randn(1, generator=g) if K != 7 else None
    ldx = K + (5 if M != 3 else 0)
    xd = torch.full((M, ldx), 1e30, device=DEV)
    xd[:, :K] = x.to(DEV)
    wd, bd = w.to(DEV), None if b is None else b.to(DEV)
    buf = torch.full((M + 8,), SENT, device=DEV)
    out = buf[4:]
    ran = _profiled(L, lambda: lib.check(L.nir_rowdot_f32(lib.ptr(xd), ldx, lib.ptr(wd), lib.ptr(bd), lib.ptr(out), M, K, act, lib.stream()),
                                         "nir_rowdot_f32"))
    assert ran == [("rowdot_kernel", 1)], ran
    h = buf.cpu()
    assert bool((h[:4] == SENT).all()) and bool((h[4 + M:] == SENT).all())
    _judge("rowdot-%dx%d-%s-act%d" % (M, K, fam, act), "rowdot_kernel", h[4:4 + M].reshape(M, 1), x, w, b, None, None, act)
