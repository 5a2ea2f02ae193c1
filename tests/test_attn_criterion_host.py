"""CPU: the teeth of the attention-pooling criterion (tests/attn_ref.py).  At the cap of its margin it accepts a numpy emulation of every
kernel variant (two-term rows and W0 without the h2' w2' product; one-term rows; one term each) and rejects the same emulation with any
single fault of attn_ref.MUTANTS -- so a kernel with one of these faults cannot pass tests/test_gpu_attn_envelope.py.  Every mutant prints
by how many times it exceeds the bound (pytest -s); DESIGN.md quotes the tightest factor."""
import numpy as np
import pytest
import torch

import attn_ref as R

M = 96
FACTORS = {}


def _inputs(fam, T):
    w = R.family(fam, 100 + T + len(fam), M, T)
    lens = R.ragged_lens(T, M, T)
    lens[::7] = T                                                                # mask_long needs room, mask_short needs len > 1
    lens = lens.clamp(min=2)
    return w, lens


def _judge(variant, w, lens, mutant=None):
    h = R.encode_f16_rows(w["h"].numpy()) if variant == "row1" else w["h"]
    got = R.emulate(variant, h, w["W0"], w["b0"], w["w3"], w["b3"], lens, mutant)
    form = R.VARIANTS[variant]
    rows, W0 = R.operands(form, h, w["W0"])
    return R.accept(got, form, rows, W0, w["b0"], w["w3"], w["b3"], lens, margin=R.MARGIN_CAP)


@pytest.mark.parametrize("fam", ["model", "peaked", "uniform", "edge", "saturated"])
@pytest.mark.parametrize("T", [4, 16, 64])
@pytest.mark.parametrize("variant", sorted(R.VARIANTS))
def test_criterion_accepts_every_honest_variant(variant, T, fam):
    w, lens = _inputs(fam, T)
    ok, r = _judge(variant, w, lens)
    print("honest %s T=%d %s: e=%.3g e32=%.3g fmt=%.3g act=%.3g bound=%.3g" % (variant, T, fam, r["e"], r["e32"], r["fmt"], r["act"], r["bound"]))
    assert ok, r


@pytest.mark.parametrize("fam", ["model", "peaked"])
@pytest.mark.parametrize("T", [4, 16, 64])
def test_criterion_rejects_every_single_fault(T, fam):
    w, lens = _inputs(fam, T)
    for mutant in R.MUTANTS:
        ok, r = _judge("x2", w, lens, mutant)
        f = r["e"] / r["bound"]
        FACTORS[(mutant, fam, T)] = f
        print("mutant %-10s T=%-2d %-6s: e=%.3g = %.2f x bound (%.0f x max(e32, 2^-23))" % (mutant, T, fam, r["e"], f, r["e"] / max(r["e32"], R.EPS)))
        assert not ok, (mutant, r)
        assert f > 1.3, (mutant, r)                      # not a near miss: e32 moves with the BLAS's summation order


def test_margin_is_capped_and_the_format_terms_are_ordered():
    assert set(R.MARGIN) == set(R.FORMS) == set(R.GEMM_FMT) and all(1.0 <= m <= R.MARGIN_CAP == 4.0 for m in R.MARGIN.values())
    assert R.GEMM_FMT["f32"] == R.GEMM_FMT["one0"] == 0.0 < R.GEMM_FMT["bf3"] < R.GEMM_FMT["pipe2"] < R.GEMM_FMT["x2"] == 3 * 2.0 ** -22
    w, lens = _inputs("model", 4)
    with pytest.raises(AssertionError):
        R.accept(torch.zeros(M, R.D), "f32", w["h"].double(), w["W0"].double(), w["b0"], w["w3"], w["b3"], lens, margin=8.0)


def test_row_formats_round_trip():
    h = R.family("model", 5, 3, 4)["h"].numpy()
    raw = R.encode_pairs(h)
    assert raw.shape == (3, 4, 2 * R.D) and raw.dtype == np.int16
    assert float(np.abs(R.decode_pairs(raw) - h).max()) <= 2.0 ** -21
    h1, h2 = R.G.split_terms(h, "fp16x2")
    v = raw.view(np.float16).reshape(3, 4, R.D // 4, 2, 4)                     # 16 bytes per group of four columns: leading terms, then residuals
    assert np.array_equal(v[..., 0, :].reshape(h.shape), h1.astype(np.float16)) and np.array_equal(v[..., 1, :].reshape(h.shape), h2.astype(np.float16))
    f = R.encode_f16_rows(h)
    assert f.shape == h.shape and np.array_equal(R.decode_f16_rows(f), h.astype(np.float16).astype(np.float64))


def test_length_zero_is_a_nan_row_and_uniform_is_the_mean():
    w = R.family("uniform", 9, 5, 8)
    lens = torch.tensor([3, 0, 8, 11, -2])
    ref = R.ref64(w["h"].double(), w["W0"].double(), w["b0"], w["w3"], w["b3"], lens)
    assert bool(torch.isnan(ref[[1, 4]]).all()) and bool(torch.isfinite(ref[[0, 2, 3]]).all())
    assert torch.allclose(ref[0], w["h"][0, :3].double().mean(0), atol=1e-15) and torch.allclose(ref[3], w["h"][3].double().mean(0), atol=1e-15)


def test_gpu_case_list_covers_what_it_promises():
    """(CPU: the case list of tests/test_gpu_attn_envelope.py is plain data) every kernel form is named; every pipeline instantiation sees nk = 1, 3 tiles, ncu + 1 and 3 ncu + 5 tiles, T = 4 and 64, model and peaked"""
    import test_gpu_attn_envelope as E
    CASES, KERNELS, PIPES = E.CASES, E.KERNELS, E.PIPES
    named = set()
    for d in CASES:
        named.update(KERNELS[d["kernel"]][0])
    assert {"attn_pool_kernel", "attn_pool2_kernel", "attn_pool_fused_kernel"} <= named
    for k in PIPES:
        assert KERNELS[k][0][0] in named
        mine = [d for d in CASES if d["kernel"] == k]
        assert {(0, 1, False), (0, 3, True), (1, 1, True), (3, 5, True)} <= {d["tiles"] for d in mine} and {4, 64} <= {d["T"] for d in mine}
        assert {"model", "peaked"} <= {d["fam"] for d in mine}
    for k in ("pipe<false,2>", "pipe<false,0>"):
        assert {4, 8, 16, 32, 64} <= {d["T"] for d in CASES if d["kernel"] == k}
    assert set(R.FAMILIES) <= {d["fam"] for d in CASES if d["kernel"] == "pipe<false,2>"}
    assert set(R.FAMILIES) <= {d["fam"] for d in CASES if d["kernel"] == "fused"}
    assert len({d["id"] for d in CASES}) == len(CASES)
