"""GPU (-m gpu): the 8-wave form of the fp16 two-term GEMM (csrc/gemm.hip: gemm3_kernel<.., NW = 8>) and the ranknet feature mode
(nir_linear_feats_f32), at the C ABI.

  * 8-wave against 4-wave, each forced through the debug tunable gemm3_wide (1 / 2) on the same inputs: torch.equal.  The tile is split
    along M and N only, so every accumulator sees the same MFMA sequence in both forms.  Without ACT_BOUNDED the tunable has no say (the
    bf16 three-term and fp32 kernels keep their one form); those cases show that it leaves such calls alone.
  * which form ran is read from nir_debug_gemm3_launches (the two forms share the profile label gemm3h_kernel, which existing tests pin);
    the dispatcher's own rule (at most one workgroup per CU -> eight waves) is checked on both sides of the CU count.
  * the 8-wave form against the float64 criterion of tests/gemm_ref.py, in its own right.
  * the feature mode against the arithmetic it replaces: the feature matrix [q', d, |q' - d|, q' * d] built in torch with the same fp32
    operations and given to nir_linear_ex_f32 -- torch.equal on every dispatch path the dispatcher can pick for it and on both forced forms.
  * nir_cars_rank_session click scores at B = 2, S = 3, N = 5 (all candidates, and a slice of NR = 2 through rank_docs) against the scores
    the commit before this change produced on the same seeded inputs (tests/golden/cars_session_b2s3n5_*.npy): bit-equal."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import cars_session_ref as SR
import gemm_ref as R
from context_attentive_ir_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SENT = -7777.0

MS, NS, KS = (1, 127, 130, 257), (2, 96, 128, 512), (16, 48, 300, 1024)
EPILOGUES = {"none": (0, False), "bias": (0, True), "tanh": (R.ACT_TANH, True), "maxout2": (R.ACT_MAXOUT2, True),
             "tanh_rowdot16": (R.ACT_TANH_ROWDOT16, True)}


def _n_out(N, act):
    return N // 2 if act == R.ACT_MAXOUT2 else N // 16 if act == R.ACT_TANH_ROWDOT16 else N


def _forms():
    """(four-wave, eight-wave) launches of the split-precision kernel so far: the two forms share a profile label"""
    a, b = C.c_longlong(0), C.c_longlong(0)
    lib.load().nir_debug_gemm3_launches(C.byref(a), C.byref(b))
    return a.value, b.value


def _linear(a, lda, w, bias, add, M, N, K, act, wide):
    """nir_linear_ex_f32 under gemm3_wide = wide -> (C [M, n_out] on the CPU, kernels the profile names)"""
    L = lib.load()
    n_out = _n_out(N, act & 0xff)
    out = torch.full((M + 2, n_out + 3), SENT, device=DEV)
    buf = C.create_string_buffer(1 << 14)
    with lib.tunable("gemm3_wide", wide, 0):
        L.nir_profile_report(buf, len(buf))
        L.nir_profile_enable(1)
        try:
            lib.check(L.nir_linear_ex_f32(lib.ptr(a), lda, None, None, 0, 0, 0, lib.ptr(w), K, lib.ptr(bias), None, lib.ptr(out[1:]), n_out + 3, M, N, K,
                                          act, lib.ptr(add), 0, lib.stream()), "nir_linear_ex_f32")
            torch.cuda.synchronize()
        finally:
            L.nir_profile_enable(0)
        L.nir_profile_report(buf, len(buf))
    names = [ln.rsplit(",", 2)[0].split("[")[0] for ln in buf.value.decode().strip().splitlines()]
    g = out.cpu()
    got = g[1:1 + M, :n_out].clone()
    g[1:1 + M, :n_out] = SENT
    assert bool((g == SENT).all()), "wrote outside [M, N_out]"
    return got, names


@pytest.mark.parametrize("bounded", [True, False], ids=["bounded", "unbounded"])
@pytest.mark.parametrize("ep", list(EPILOGUES))
def test_wide_form_is_bit_equal_to_the_four_wave_form(ep, bounded):
    """M: one row, one partial tile, a masked tail tile behind full ones; K: shorter than one stage, shorter than the two-stage prefetch,
    a tail that is no multiple of the k-step, the headline's 1024; every second shape with strided A (lda = K + 4)"""
    act, has_bias = EPILOGUES[ep]
    g = torch.Generator().manual_seed(77 + len(ep))
    i = 0
    for M in MS:
        for N in NS:
            if act == R.ACT_TANH_ROWDOT16 and N % 16:
                continue
            for K in KS:
                i += 1
                lda = K + 4 * (i % 2)
                a = torch.full((M, lda), 3.0)
                a[:, :K] = torch.rand(M, K, generator=g) * 2 - 1
                w = torch.randn(N, K, generator=g) / K ** 0.5
                bias = torch.randn(N, generator=g) if has_bias else None
                add = torch.randn(N, generator=g) / 4 if act == R.ACT_TANH_ROWDOT16 else None
                dev = [None if t is None else t.to(DEV) for t in (a, w, bias, add)]
                flag = R.ACT_BOUNDED if bounded else 0
                f0 = _forms()
                got8, n8 = _linear(dev[0], lda, dev[1], dev[2], dev[3], M, N, K, act | flag, 1)
                f1 = _forms()
                got4, n4 = _linear(dev[0], lda, dev[1], dev[2], dev[3], M, N, K, act | flag, 2)
                f2 = _forms()
                if bounded:
                    assert n8 == ["gemm3h_kernel"] and n4 == ["gemm3h_kernel"], (M, N, K, n8, n4)
                    assert (f1[0] - f0[0], f1[1] - f0[1]) == (0, 1), "gemm3_wide = 1 did not launch the 8-wave form"
                    assert (f2[0] - f1[0], f2[1] - f1[1]) == (1, 0), "gemm3_wide = 2 did not launch the 4-wave form"
                else:
                    assert f2 == f0, "an unbounded call of this size reached the split-precision kernel"
                    assert n8 == n4 and not n8[0].startswith("gemm3h_kernel"), (M, N, K, n8, n4)
                assert torch.equal(got8, got4), (ep, M, N, K, lda, float((got8 - got4).abs().max()))


def test_wide_form_meets_the_fp64_criterion():
    M, N, K = 257, 130, 300
    g = torch.Generator().manual_seed(5)
    a = R.family("randn", g, M, K, "a")
    w = R.family("randn", g, N, K, "w")
    bias = torch.randn(N, generator=g)
    f0 = _forms()
    got, names = _linear(a.to(DEV), K, w.to(DEV), bias.to(DEV), None, M, N, K, R.ACT_BOUNDED, 1)
    assert names == ["gemm3h_kernel"] and _forms() == (f0[0], f0[1] + 1)
    ok, r = R.accept(got, a, w, bias, None, None, 0, form="fp16x2")
    print("GEMM3WIDE e=%.3g e_chain=%.3g extra=%.3g ratio=%.3f bound=%.3g" % (r["e"], r["e_chain"], r["extra"], r["ratio"], r["bound"]))
    assert ok, r


# (BS, candidates, D, expected kernel by the dispatcher's own rule): the issue's shapes (a 128-row tile straddles several query rows, R is
# no multiple of the tile), then one shape per further path a feature-mode call can take
FEAT_CASES = [(3, 1, 256, "gemm16_kernel"), (3, 10, 256, "gemm16_kernel"), (3, 7, 256, "gemm16_kernel"),
              (3, 7, 64, "gemm16_kernel"),            # K = 256: the k-loop without look-ahead
              (60, 7, 256, "gemm32_kernel"), (130, 10, 256, "gemm_kernel"), (441, 7, 256, "gemm3h_kernel[feats]")]


def test_dispatch_rule_by_workgroups_per_cu():
    """left to the rule (gemm3_wide = 0): at most one 128 x 128 workgroup per CU -> eight waves, more -> four"""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    K = 64
    w = torch.randn(128, K, device=DEV) / 8
    for tiles, want in ((96, (0, 1)), (ncu, (0, 1)), (ncu + 1, (1, 0))):
        M = 128 * tiles
        a = torch.rand(M, K, device=DEV) * 2 - 1
        f0 = _forms()
        _, names = _linear(a, K, w, None, None, M, 128, K, R.ACT_BOUNDED, 0)
        f1 = _forms()
        assert names == ["gemm3h_kernel"] and (f1[0] - f0[0], f1[1] - f0[1]) == want, (tiles, names, f0, f1)


def test_unbounded_feature_mode_is_bit_equal_to_the_feature_matrix():
    """rank_bounded bit 0 clear at a large R: the bf16 three-term kernel (four waves) forms the features in its loader as well"""
    L = lib.load()
    BS, NC, D = 441, 7, 256
    g = torch.Generator().manual_seed(9)
    M = BS * NC
    qp = ((torch.rand(BS, D, generator=g) * 2 - 1) * 0.95).to(DEV)
    docs = ((torch.rand(M, D, generator=g) * 2 - 1) * 0.95).to(DEV)
    w = (torch.randn(512, 4 * D, generator=g) / (4 * D) ** 0.5).to(DEV)
    bias = torch.randn(512, generator=g).to(DEV)
    q = qp.repeat_interleave(NC, 0)
    feats = torch.cat([q, docs, (q - docs).abs(), q * docs], 1).contiguous()
    want, names = _linear(feats, 4 * D, w, bias, None, M, 512, 4 * D, R.ACT_MAXOUT2, 0)
    assert names == ["gemm3_kernel"]
    out = torch.full((M, 256), SENT, device=DEV)
    f0 = _forms()
    lib.check(L.nir_linear_feats_f32(lib.ptr(qp), lib.ptr(docs), D, NC, D, lib.ptr(w), 4 * D, lib.ptr(bias), lib.ptr(out), 256, M, 512, R.ACT_MAXOUT2,
                                     lib.stream()), "nir_linear_feats_f32")
    torch.cuda.synchronize()
    assert _forms() == (f0[0] + 1, f0[1])
    assert torch.equal(out.cpu(), want)


@pytest.mark.parametrize("BS,NC,D,kernel", FEAT_CASES, ids=["bs%d_n%d_d%d" % c[:3] for c in FEAT_CASES])
def test_feature_mode_is_bit_equal_to_the_feature_matrix(BS, NC, D, kernel):
    L = lib.load()
    g = torch.Generator().manual_seed(BS * 100 + NC)
    M = BS * NC
    qp = ((torch.rand(BS, D, generator=g) * 2 - 1) * 0.95).to(DEV)
    docs = ((torch.rand(M, D, generator=g) * 2 - 1) * 0.95).to(DEV)
    w = (torch.randn(512, 4 * D, generator=g) / (4 * D) ** 0.5).to(DEV)
    bias = torch.randn(512, generator=g).to(DEV)
    q = qp.repeat_interleave(NC, 0)
    feats = torch.cat([q, docs, (q - docs).abs(), q * docs], 1).contiguous()       # rank_feats' fp32 expressions
    act = R.ACT_MAXOUT2 | R.ACT_BOUNDED
    buf = C.create_string_buffer(1 << 14)
    for wide in (0, 1, 2):
        want, _ = _linear(feats, 4 * D, w, bias, None, M, 512, 4 * D, act, wide)
        out = torch.full((M + 2, 256 + 3), SENT, device=DEV)
        with lib.tunable("gemm3_wide", wide, 0):
            L.nir_profile_report(buf, len(buf))
            L.nir_profile_enable(1)
            try:
                lib.check(L.nir_linear_feats_f32(lib.ptr(qp), lib.ptr(docs), D, NC, D, lib.ptr(w), 4 * D, lib.ptr(bias), lib.ptr(out[1:]), 256 + 3, M, 512,
                                                 act, lib.stream()), "nir_linear_feats_f32")
                torch.cuda.synchronize()
            finally:
                L.nir_profile_enable(0)
            L.nir_profile_report(buf, len(buf))
        names = [ln.rsplit(",", 2)[0].split("[M=")[0] for ln in buf.value.decode().strip().splitlines()]
        assert names == [kernel if wide == 0 else "gemm3h_kernel[feats]"], names
        o = out.cpu()
        got = o[1:1 + M, :256].clone()
        o[1:1 + M, :256] = SENT
        assert bool((o == SENT).all()), "wrote outside [M, 256]"
        assert torch.equal(got, want), (wide, float((got - want).abs().max()))


# ------------------------------------------------------------------ end to end: the session tail against the recorded scores
GOLD_SEED = 20261                     # inputs and weights of the recorded scores: session_scores() below, run on the commit before this change
GOLD_SHAPE = dict(B=2, S=3, N=5, D=256, HS=256, HDEC=64)
GOLD_SLICE = (1, 2)                   # rank_docs: candidates 1..2 (NR = 2 < N)


def session_scores(cols=None):
    """click scores [B, S, N] (or [B, S, NR] for the candidate slice `cols` = (first, NR), through rank_docs) of nir_cars_rank_session /
    nir_cars_rank_session_shard on the seeded inputs"""
    L = lib.load()
    c = SR._case("gold", seed=GOLD_SEED, **GOLD_SHAPE)
    B, S, N, D = c["B"], c["S"], c["N"], c["D"]
    g = torch.Generator().manual_seed(GOLD_SEED)
    sd = SR.make_sd(D, c["HS"], c["HDEC"], GOLD_SEED + 1, True, True)
    pq = ((torch.rand(B, S, D, generator=g) * 2 - 1) * 0.95).to(DEV)
    docs = ((torch.rand(B, S, N, D, generator=g) * 2 - 1) * 0.95).to(DEV)
    lab, _ = SR.make_labels(c, g)
    lab = lab.to(DEV)
    w, keep = SR.device_weights(sd, c, DEV)
    need = L.nir_cars_session_workspace_bytes(B, S, N, C.byref(w))
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=DEV)
    wsp = C.c_void_p((ws.data_ptr() + 255) // 256 * 256)
    NR = cols[1] if cols else N
    scores = torch.full((B, S, NR), SENT, device=DEV)
    head = (lib.ptr(pq), lib.ptr(docs), lib.ptr(lab), B, S, N, C.byref(w), wsp, need, lib.ptr(scores), None, None)
    if cols:
        rdocs = docs[:, :, cols[0]:cols[0] + NR].contiguous()
        lib.check(L.nir_cars_rank_session_shard(*head, lib.ptr(rdocs), NR, lib.stream()), "nir_cars_rank_session_shard")
    else:
        lib.check(L.nir_cars_rank_session(*head, lib.stream()), "nir_cars_rank_session")
    torch.cuda.synchronize()
    del keep
    return scores.cpu().numpy()


@pytest.mark.parametrize("which,cols", [("all", None), ("slice", GOLD_SLICE)])
def test_session_scores_equal_the_recorded_ones(which, cols):
    want = np.load(os.path.join(GOLDEN, "cars_session_b2s3n5_%s.npy" % which))
    got = session_scores(cols)
    assert got.shape == want.shape and not (got == SENT).any()
    assert np.array_equal(got, want), float(np.abs(got - want).max())
