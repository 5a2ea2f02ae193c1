"""CPU: the teeth of the GEMM acceptance criterion (tests/gemm_ref.py).  At the cap of its margin it accepts a faithful emulation of
both split-precision operand formats and rejects the same emulation with any single cross term left out -- so a kernel that loses one
term (everywhere; the GPU cases add the K tail, column tile and epilogue variants) cannot pass tests/test_gpu_gemm_envelope.py."""
import pytest
import torch

import gemm_ref as R

M, N = 256, 192
MUTANTS = {"bf16x3": ("b1b1", "b0b2", "b2b0"), "fp16x2": ("a2w1", "a1w2")}


@pytest.mark.parametrize("fam", ["randn", "positive", "mixed"])
@pytest.mark.parametrize("K", [64, 300, 900, 2048])
@pytest.mark.parametrize("form", ["bf16x3", "fp16x2"])
def test_criterion_accepts_the_full_split_and_rejects_every_single_term_mutant(form, K, fam):
    g = torch.Generator().manual_seed(K * 7 + len(fam))
    a = R.family(fam, g, M, K, "a")
    w = R.family(fam, g, N, K, "w")
    ok, r = R.accept(R.emulate(a, w, form), a, w, form=form, margin=R.MARGIN_CAP)
    print("full %s K=%d %s: e=%.3g e_chain=%.3g bound=%.3g" % (form, K, fam, r["e"], r["e_chain"], r["bound"]))
    assert ok, r
    for drop in MUTANTS[form]:
        ok, r = R.accept(R.emulate(a, w, form, drop=drop), a, w, form=form, margin=R.MARGIN_CAP)
        print("  without %s: e=%.3g = %.2f x bound" % (drop, r["e"], r["e"] / r["bound"]))
        assert not ok, (drop, r)
        assert r["e"] > 1.3 * r["bound"], (drop, r)      # not a near miss: e_chain moves with the BLAS's summation order


def test_margin_is_capped_and_formats_are_ordered():
    assert set(R.MARGIN) == set(R.FMT) and all(1.0 <= m <= R.MARGIN_CAP == 4.0 for m in R.MARGIN.values())
    assert R.FMT["f32"] == 0.0 < R.FMT["bf16x3"] == 2.0 ** -22 < R.FMT["fp16x2"] == 3 * 2.0 ** -22
    with pytest.raises(AssertionError):
        R.accept(torch.zeros(1, 1), torch.ones(1, 1), torch.ones(1, 1), margin=8.0)


def test_split_terms_reconstruct_the_operand():
    g = torch.Generator().manual_seed(3)
    x = R.family("mixed", g, 64, 128, "a").numpy()
    b0, b1, b2 = R.split_terms(x, "bf16x3")
    assert float(abs((b0.astype("f8") + b1 + b2) - x).max() / abs(x).max()) < 2.0 ** -23
    assert (abs(b0) <= abs(x)).all()                       # truncation: never past the value
    e = R.family("edge", g, 64, 128, "a").numpy()
    h1, h2 = R.split_terms(e, "fp16x2")
    assert abs(h1).max() == 32752.0 and abs(h2).max() < 65504.0          # the 2^15 limit: both terms stay finite fp16 values
    assert float((abs((h1.astype("f8") + h2.astype("f8") / 2048.0) - e) / abs(e)).max()) <= 2.0 ** -21
    t = R.family("tiny20", g, 64, 128, "a").numpy()
    h1, h2 = R.split_terms(t, "fp16x2")
    assert float(abs((h1.astype("f8") + h2.astype("f8") / 2048.0) - t).max()) <= 2.0 ** -35   # the subnormal floor of the scaled residual
