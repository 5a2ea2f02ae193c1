"""CPU: the criterion of tests/mt_conv_ref.py has teeth.  The float64 reference is torch's Conv2d and the operation's definition; the in-order
numpy emulation of the kernels (csrc/mt_conv_train.hip, nir_colsum_det_f32) is accepted on every GPU input within 0.8 of the bound at the cap;
the emulation with any single fault of mt_conv_ref.FAULTS is rejected at the cap by more than 1.3 times the bound; the case list covers the
seams it promises; nir_mt_conv3_supported restated in Python agrees with the LDS formulas; the margins follow the committed MI355X log."""
import os
import re

import numpy as np
import pytest
import torch

import mt_conv_ref as R

LOG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "mt_conv_criterion_mi355x.log")


@pytest.mark.parametrize("M,H,W", [(2, 3, 5), (1, 1, 2), (3, 4, 9)])
def test_reference_equals_conv2d_modules(M, H, W):
    x = R.family(R.c(M, H, W))
    ref = R.chain(x, torch.float64)
    convs = [torch.nn.Conv2d(R.C1, R.NF, (3, kw), padding=(1, kw // 2)).double() for kw in R.KW]
    for k, cv in enumerate(convs):
        cv.weight.data, cv.bias.data = x["w%d" % (k + 1)].double(), x["b%d" % (k + 1)].double()
    T = x["T"].double().requires_grad_(True)
    pre = torch.cat([cv(T).permute(0, 2, 3, 1).reshape(M * H * W, R.NF) for cv in convs], 1)
    pre.backward(x["dpre"].double())
    assert float((torch.relu(pre.detach()) - ref["fwd"]).abs().max()) <= 1e-12
    assert float((T.grad - ref["dT"]).abs().max()) <= 1e-12
    for k, cv in enumerate(convs):
        assert float((cv.weight.grad - ref["dw%d" % (k + 1)]).abs().max()) <= 1e-12
        assert float((cv.bias.grad - ref["db%d" % (k + 1)]).abs().max()) <= 1e-12
    # and the definition itself, tap by tap
    Tn, H_, W_ = x["T"].double().numpy(), H, W
    for g in range(3):
        w, b = x["w%d" % (g + 1)].double().numpy(), x["b%d" % (g + 1)].double().numpy()
        want = np.zeros((M, H, W, R.NF)) + b
        for y in range(H):
            for xx in range(W):
                for dy in range(3):
                    for dx in range(R.KW[g]):
                        yy, xs = y + dy - 1, xx + dx - (g + 1)
                        if 0 <= yy < H_ and 0 <= xs < W_:
                            want[:, y, xx] += Tn[:, :, yy, xs] @ w[:, :, dy, dx].T
        assert np.abs(want.reshape(-1, R.NF) - ref["pre"].numpy()[:, g * R.NF:(g + 1) * R.NF]).max() <= 1e-12


@pytest.mark.parametrize("H,W", R.IMPULSE_SHAPES)
def test_impulse_results_are_the_tap_formulas_and_exact_in_fp32(H, W):
    """the reference on the impulse inputs IS the indexing formula of the issue, and rounding it to fp32 loses nothing but one rounding of w + b"""
    x, where = R.impulse_fwd(H, W)
    ref = R.chain(x, torch.float64)["fwd"].reshape(len(where), H, W, R.NCOL)
    for m, ch, y0, x0 in where[::5]:
        for g in range(3):
            w, b = x["w%d" % (g + 1)].double(), x["b%d" % (g + 1)].double()
            for y in range(H):
                for xx in range(W):
                    dy, dx = y0 - y + 1, x0 - xx + g + 1
                    inside = 0 <= dy < 3 and 0 <= dx < R.KW[g]
                    want = torch.relu(w[:, ch, dy, dx] + b if inside else b)
                    assert torch.equal(ref[m, y, xx, g * R.NF:(g + 1) * R.NF], want), (m, g, y, xx)
    x, where = R.impulse_bwd(H, W)
    ref = R.chain(x, torch.float64)
    for k in R.KEYS[1:]:
        assert torch.equal(ref[k].float().double(), ref[k]), k + " is not exactly representable in fp32"
    for m, y0, x0, col in where[::7]:
        g, o = col // R.NF, col % R.NF
        w = x["w%d" % (g + 1)].double()
        want = torch.zeros(R.C1, H, W, dtype=torch.float64)
        for y in range(H):
            for xx in range(W):
                dy, dx = y - y0 + 1, xx - x0 + g + 1
                if 0 <= dy < 3 and 0 <= dx < R.KW[g]:
                    want[:, y, xx] = w[o, :, dy, dx]
        assert torch.equal(ref["dT"][m], want), (m, y0, x0, col)
    counts = torch.zeros(R.NCOL, dtype=torch.float64)
    for m, y0, x0, col in where:
        counts[col] += 1
    assert torch.equal(torch.cat([ref["db%d" % k] for k in (1, 2, 3)]), counts)
    # what the impulses visit
    pos = set(R.impulse_positions(H, W))
    assert {(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (H // 2, W // 2)} <= pos
    if H * W > 256:
        assert {(255 // W, 255 % W), (256 // W, 256 % W)} <= pos
    if W > 1:
        assert {xx for _, xx in pos} >= {R.xchunk(W) - 1, R.xchunk(W)}
    fw = R.impulse_fwd(H, W)[1]
    assert {ch for _, ch, _, _ in fw} == set(R.IMPULSE_CHANNELS) and {(y, xx) for _, _, y, xx in fw} == pos
    assert {(y, xx) for _, y, xx, _ in where} == pos and {col for _, _, _, col in where} == set(range(R.NCOL))


@pytest.mark.parametrize("d", R.CASES, ids=lambda d: d["id"])
def test_honest_emulation_is_accepted_within_the_input_rule(d):
    x, p = R.prepared(d)
    em = R.emulate(x)
    assert set(em) == set(R.KEYS)
    for k in R.KEYS:
        ok, r = R.accept(em[k], k, p)
        print("MTCONVHOST,%s,%s,e=%.3g,e32=%.3g,ratio=%.3f" % (d["id"], k, r["e"], r["e32"], r["ratio"]))
        assert ok, (k, r)
        assert r["ratio"] <= 0.8 * R.MARGIN_CAP, "the input breaks the 0.8 rule on %s: reseed it (SEEDS), do not move the bound" % k
    if d["fam"] == "dead":
        assert float(em["fwd"].abs().max()) == 0.0 and float(p["ref"]["fwd"].abs().max()) == 0.0


def test_reseeded_inputs_are_exactly_those_an_honest_evaluation_fails_on():
    assert set(R.SEEDS) <= set(R.BY_ID) and all(s > 0 for s in R.SEEDS.values())
    for cid, seed in R.SEEDS.items():
        for s in range(seed):
            x = R.family(R.BY_ID[cid], s)
            ok, worst = R.honest_ok(x, R.prepare(x))
            print("MTCONVHOST,%s,seed %d,worst ratio %.3f" % (cid, s, worst))
            assert not ok, "%s passes at seed %d already" % (cid, s)
    # (that the recorded seed -- 0 where none is recorded -- passes is test_honest_emulation_is_accepted_within_the_input_rule)


FAULT_CASES = {
    "a": ["randn-M2-H5-W8", "randn-M3-H4-W33"], "b": ["randn-M2-H5-W7", "randn-M1-H1-W1"], "c": ["randn-M2-H5-W7", "randn-M3-H4-W33"],
    "d": ["randn-M1-H1-W257", "randn-M1-H1-W255", "randn-M3-H4-W33"], "e": ["randn-M2-H5-W7", "positive-M2-H5-W7"],
    "f": ["randn-M1-H257-W1", "randn-M2-H4-W65"], "g": ["randn-M2-H5-W7", "randn-M2-H4-W65"], "h1": ["randn-M2-H5-W7", "tiny-M2-H5-W7"],
    "h2": ["randn-M2-H5-W7", "mixed-M2-H5-W7"], "l": ["randn-M2-H5-W7", "randn-M3-H2-W4"],
    "i1": ["randn-M3-H4-W33", "randn-M3-H2-W9", "randn-M1-H1-W2"], "i2": ["randn-M3-H4-W33", "randn-M3-H2-W9"],
    "j": ["randn-M2-H5-W7", "randn-M1-H1-W255"], "k1": ["randn-M33-H2-W5", "randn-M97-H2-W5"], "k2": ["randn-M33-H2-W5", "randn-M97-H2-W5"],
}


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_single_fault_is_rejected_at_the_cap(fault):
    assert set(FAULT_CASES) == set(R.FAULTS)
    kernel = R.FAULT_KERNEL[fault]
    for cid in FAULT_CASES[fault]:
        x, p = R.prepared(R.BY_ID[cid])
        em = R.emulate(x, kernels=(kernel,), fault=fault)
        factor = max(r["e"] / r["bound"] for r in (R.accept(v, k, p, R.MARGIN_CAP)[1] for k, v in em.items()))
        print("MTCONVHOST,fault %s,%s,%s,e / bound = %.3g" % (fault, kernel, cid, factor))
        assert factor > 1.3, (fault, cid, factor)


def test_accept_refuses_a_margin_above_the_cap():
    x, p = R.prepared(R.BY_ID["randn-M1-H1-W1"])
    with pytest.raises(AssertionError):
        R.accept(p["ref"]["fwd"], "fwd", p, margin=R.MARGIN_CAP * 1.01)
    assert all(m <= R.MARGIN_CAP for m in R.MARGIN.values()) and R.MARGIN_COL2IM <= R.MARGIN_CAP


def test_case_list_covers_what_it_promises():
    shapes = [(M, H, W) for M, H, W, _ in R.SHAPES]
    hw = {H * W for _, H, W in shapes}
    assert {256, 257, 260, 512, 513} <= hw and max(hw) == 750                            # data gradient: one pass, two, two exactly, three
    tails = {(M * H * W) % 256 for M, H, W in shapes}
    assert {255, 0, 1} <= tails                                                          # forward: last block full, one short, one over
    lds = {R.weight_lds(H, W) for _, H, W in shapes}
    assert max(v for v in lds if v <= 64 * 1024) == 51 * 321 * 4 and min(v for v in lds if v > 64 * 1024) == 51 * 323 * 4
    assert max(lds) == 51 * 751 * 4 and sum(v > 64 * 1024 for v in lds) >= 5
    assert {1, 2, 3} <= {W for _, _, W in shapes} and any(W % 2 and W > 7 for _, _, W in shapes)
    assert {R.colsum_slices(R.MT_XS * M)[1] for M, H, W in shapes if (H, W) == (2, 5)} == {1, 2, 4}
    assert R.colsum_slices(64) == (64, 1) and R.colsum_slices(66) == (64, 2) and R.colsum_slices(194) == (64, 4) and R.colsum_slices(970) == (64, 16)
    assert R.colsum_slices(81920) == (320, 256)                                          # the bias gradient of the benchmark's training step
    assert max(M * H * W for M, H, W in shapes) <= 20000
    assert all(R.supported(6, 51, H, W) for _, H, W in shapes) and not any(R.supported(6, 51, H, W) for _, H, W in R.REFUSED_SHAPES)
    assert {fam for fam in (d["fam"] for d in R.CASES)} == set(R.FAMILIES)


def test_supported_agrees_with_the_lds_formulas():
    """nir_mt_conv3_supported restated: the weight gradient's tile is the condition that binds, the data gradient's never does at C1 = 51"""
    best, first = 0, 1 << 30
    for H in range(1, 41):
        for W in range(1, 801):
            cs = (H * (W + 1)) | 1
            ok = R.supported(6, 51, H, W)
            assert ok == int(R.weight_lds(H, W) <= 150 * 1024) == int(cs <= 752), (H, W)
            if ok:
                assert R.data_lds(H, W) <= 64 * 1024, (H, W)
                best = max(best, cs)
            else:
                first = min(first, cs)
    assert (best, first) == (751, 753)
    shapes = {(H, W) for _, H, W, _ in R.SHAPES}
    assert {(1, 750), (10, 74)} <= shapes and all((H * (W + 1)) | 1 == 751 for H, W in ((1, 750), (10, 74)))
    assert all((H * (W + 1)) | 1 == 753 for _, H, W in R.REFUSED_SHAPES)
    assert (5, 63) in shapes and R.weight_lds(5, 63) <= 64 * 1024 < R.weight_lds(1, 321) and (1, 321) in shapes
    assert not R.supported(5, 51, 4, 64) and not R.supported(6, 50, 4, 64) and not R.supported(6, 52, 4, 64) and not R.supported(6, 51, 0, 4)


def test_margins_follow_the_committed_log():
    """MARGIN is the rule of the module docstring applied to the MTCONVENV lines of the MI355X run"""
    worst = {}
    with open(LOG) as f:
        for ln in f:
            m = re.match(r"MTCONVENV,([^,]+),(\w+),(\w+),e=\S+,e32=\S+,ratio=([0-9.eE+-]+),bound=", ln)
            if m:
                worst[m.group(2)] = max(worst.get(m.group(2), 0.0), float(m.group(4)))
    assert set(worst) == set(R.KERNELS) | {"col2im"}, worst
    for k in R.KERNELS:
        assert abs(worst[k] - R.MEASURED[k]) <= 5e-4 and R.MARGIN[k] == R.margin_rule(R.MEASURED[k]), (k, worst[k], R.MEASURED[k], R.MARGIN[k])
    assert abs(worst["col2im"] - R.MEASURED_COL2IM) <= 5e-4 and R.MARGIN_COL2IM == R.margin_rule(R.MEASURED_COL2IM)
    assert [R.margin_rule(v) for v in (0.3, 0.5, 0.51, 1.0, 1.01, 2.0, 2.01, 3.9)] == [1, 1, 2, 2, 4, 4, 4, 4]


@pytest.mark.parametrize("d", R.IM2COL_CASES[:4], ids=lambda d: d["id"])
def test_patch_row_reference_is_the_definition(d):
    v = R.im2col_family(d)
    rows, din = R.im2col_chain(d, v, torch.float64)
    M, C, H, W, kh, kw = (d[k] for k in ("M", "C", "H", "W", "kh", "kw"))
    xin, dr = v["x"].double(), v["drows"].double().reshape(M, H, W, C, kh, kw)
    want, back = torch.zeros(M, H, W, C, kh, kw, dtype=torch.float64), torch.zeros(M, C, H, W, dtype=torch.float64)
    for y in range(H):
        for xx in range(W):
            for dy in range(kh):
                for dx in range(kw):
                    yy, xs = y + dy - kh // 2, xx + dx - kw // 2
                    if 0 <= yy < H and 0 <= xs < W:
                        want[:, y, xx, :, dy, dx] = xin[:, :, yy, xs]
                        back[:, :, yy, xs] += dr[:, y, xx, :, dy, dx]
    assert torch.equal(rows, want.reshape(M * H * W, -1))
    assert float((din - back).abs().max()) <= 1e-12
