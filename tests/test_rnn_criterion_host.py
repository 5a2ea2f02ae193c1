"""CPU: the teeth of the recurrence acceptance criterion (tests/rnn_ref.py) and the reach of the dispatchers it restates.  At the cap of its
margin the criterion accepts fp32 evaluations of the recurrence in other summation orders and with activation noise of 1e-7, and rejects
every mutant a kernel could plausibly be (precision mutants by at least 1.3 x, on the "randn" and "sat" families) -- so such a kernel cannot
pass tests/test_gpu_rnn_envelope.py.  The enumeration of predict() shows which compiled instantiations no argument set reaches (DESIGN.md
section 11) and that every case of the GPU tables lands on the kernel it names."""
import os
import re

import numpy as np
import pytest

import rnn_ref as R
import test_gpu_rnn_envelope as E

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "context_attentive_ir_amd", "csrc")
PAIRS = [(15, 6), (70, 40), (128, 200), (33, 290)]          # (H, T)
M = 6


def _case(cell, fam, H, T):
    return R.make(fam, H * 1000 + T + len(fam), M, T, H, 2, 0, cell)


def _got(inp, **kw):
    g = R.evaluate(inp, **kw)
    if inp["cell"] == "gru":
        g["cn"] = None
    g["cst"] = None
    return g


@pytest.mark.parametrize("H,T", PAIRS)
@pytest.mark.parametrize("fam", ["randn", "sat"])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_criterion_accepts_fp32_emulations_and_rejects_every_mutant(cell, fam, H, T):
    inp = _case(cell, fam, H, T)
    f = R.figures(inp)
    print("%s %s H=%d T=%d: e32=%.3g e_act=%.3g bound(4)=%.3g" % (cell, fam, H, T, f["e32"], f["e_act"], 4 * max(f["e32"], R.EPS) + f["e_act"]))
    for name, kw in (("sequential", dict(order="seq")), ("quarters", dict(order="quad")), ("noise 1e-7", dict(noise=np.random.default_rng(H + T)))):
        ok, r = R.accept(_got(inp, dt=np.float32, **kw), inp, margin=R.MARGIN_CAP)
        print("  fp32 %-10s e=%.3g = %.2f x bound" % (name, r["e"], r["e"] / r["bound"]))
        assert ok, (name, r)
    for mut in (R.MUTANTS_LSTM if cell == "lstm" else R.MUTANTS_GRU):
        ok, r = R.accept(_got(inp, dt=np.float32, mut=mut), inp, margin=R.MARGIN_CAP)
        print("  mutant %-11s e=%.3g = %.2f x bound" % (mut, r["e"], r["e"] / r["bound"]))
        assert not ok, (mut, r)
        if mut in R.PRECISION_MUTANTS:
            assert r["e"] > 1.3 * r["bound"], (mut, r)      # not a near miss


def test_remember_family_carries_state_but_does_not_judge_precision():
    """forget gate ~ 1 over T = 200: the activation shift accumulates in c, e_act grows by orders of magnitude -- the family is there for state
    carry (every semantic mutant is still rejected), precision is judged elsewhere"""
    inp = R.make("remember", 5, M, 200, 64, 2, 0, "lstm")
    f, g = R.figures(inp), R.figures(_case("lstm", "randn", 64, 200))
    print("remember: e_act=%.3g against %.3g on randn" % (f["e_act"], g["e_act"]))
    assert f["e_act"] > 5 * g["e_act"]
    for mut in ("rev_T", "final_T", "no_h0", "no_c0", "swap_fg", "nbr_len"):
        ok, r = R.accept(_got(inp, dt=np.float32, mut=mut), inp, margin=R.MARGIN_CAP)
        print("  mutant %-8s e=%.3g = %.2f x bound" % (mut, r["e"], r["e"] / r["bound"]))
        assert not ok, (mut, r)


def test_fused_reference_projects_first_and_poison_stays_outside():
    inp = R.make("randn", 11, 5, 9, 20, 2, 24, "lstm")
    assert float(np.abs(inp["x"]).max()) == R.POISON and int(inp["lengths"].min()) == 1
    ref = R.figures(inp)["ref"]
    gin = inp["x"].astype(np.float64) @ inp["w_ih"].astype(np.float64).T + inp["b_ih"].astype(np.float64) + inp["b_hh_in"]
    same = R.lstm_ref(gin, inp["w_hh"], inp["lengths"], inp["h0"], inp["c0"], 2)
    assert np.array_equal(ref["out"], same["out"]) and np.array_equal(ref["cn"], same["cn"]) and float(np.abs(ref["out"]).max()) <= 1.0
    clean = dict(inp, x=np.where(np.abs(inp["x"]) == R.POISON, 0, inp["x"]).astype(np.float32), _fig=None)
    assert np.array_equal(R.figures(clean)["ref"]["out"], ref["out"])
    ok, r = R.accept(_got(inp, dt=np.float32), inp, margin=1.0)                  # e32 is this very evaluation
    assert ok and r["e"] == r["e32"]


def test_padded_tail_must_be_exactly_zero_and_forgotten_elements_show():
    inp = _case("lstm", "randn", 15, 6)
    g = _got(inp)
    assert R.accept(g, inp, margin=R.MARGIN_CAP)[0]
    t = dict(g, out=g["out"].copy())
    t["out"][-1, -1, 0] = 1e-30                               # the last sequence has length 1
    ok, r = R.accept(t, inp, margin=R.MARGIN_CAP)
    assert not ok and r["tail"] == 1 and r["e"] <= r["bound"]
    n = dict(g, hn=g["hn"].copy())
    n["hn"][1, 2, 3] = np.nan
    assert not R.accept(n, inp, margin=R.MARGIN_CAP)[0]


def test_length_clamp_of_the_reference():
    inp = R.make("randn", 3, 4, 5, 8, 2, 0, "lstm", lengths=[0, 5 + 5, 3, -2])
    ref = R.figures(inp)["ref"]
    assert not ref["out"][0].any() and not ref["out"][3].any() and ref["out"][1].all()
    assert np.array_equal(ref["hn"][:, 0], inp["h0"][:, 0].astype(np.float64)) and np.array_equal(ref["cn"][:, 3], inp["c0"][:, 3].astype(np.float64))
    full = R.figures(dict(inp, lengths=np.array([0, 5, 3, 0]), _fig=None))["ref"]
    assert np.array_equal(full["out"], ref["out"]) and np.array_equal(full["hn"], ref["hn"])


def test_margin_is_capped():
    assert set(R.MARGIN) == {R.family_of(d["kernel"]) for d in E.ALL_CASES} and all(1.0 <= m <= R.MARGIN_CAP == 4.0 for m in R.MARGIN.values())
    inp = _case("lstm", "randn", 15, 6)
    with pytest.raises(AssertionError):
        R.accept(_got(inp), inp, margin=8.0)


# ------------------------------------------------------------------ the dispatchers
def test_restatement_matches_the_tables_in_the_source():
    mfma = open(os.path.join(CSRC, "lstm_mfma.hip")).read()
    lstm = open(os.path.join(CSRC, "lstm.hip")).read()
    assert [(int(a), int(b)) for a, b in re.findall(r"NIR_MFMA_CASE\((\d+), (\d+)\)", mfma)] == R.MFMA_TABLE
    assert [int(a) for a in re.findall(r"NIR_M16_CASE\((\d+)\)", mfma)] == list(range(1, 11))
    assert sorted({int(a) for a in re.findall(r"launch_s<(\d+), IP>", lstm)}) == list(R.REC_KP)
    assert sorted({int(a) for a in re.findall(r"launch_one<KP, (\d+), ", lstm)}) == [1, 2, 3, 4, 8]
    assert sorted(re.findall(r"launch_mfma_gin<(\d+, \d+, \d+)>", mfma)) == ["3, 24, 2", "4, 16, 1", "4, 32, 2"]
    assert sorted(re.findall(r"return launch_mfma16_gin<(\d+, \d+)>", mfma)) == ["3, 1", "4, 1", "5, 2", "6, 2", "7, 2", "8, 2"]
    assert "0.85 + 0.29 * S" in lstm and "< 128)" in mfma and "< 160)" in mfma


def _reach():
    got = set()
    Ms = (1, 5, 260, 390, 520, 770, 1008, 1009, 1264, 1265, 1540, 2033, 2600)
    for H in range(1, 129):
        for ndir in (1, 2):
            for M_ in Ms:
                for T in (8, 130, 300):
                    got.add(R.predict("fwd", M_, T, H, 0, ndir))
                    for I in range(1, 65):
                        for bif in (1, 4):
                            try:
                                got.add(R.predict("fused", M_, T, H, I, ndir, None, bif))
                            except ValueError:
                                pass
    return got


def test_enumeration_of_the_dispatchers():
    """H = 1..128, I = 0 (unfused) and 1..64, ndir 1 and 2, M from 1 to well past both 16-sequence thresholds, T = 8 / 130 / 300 (the fused VALU
    kernel halves S once S T IP floats outgrow 96 KB), 1 and 4 batches in flight; no tunables."""
    reached, comp = _reach(), R.compiled()
    assert reached <= comp, sorted(reached - comp)
    unreached = comp - reached
    rec = lambda kp, s: R.Pred("lstm_rec_kernel<%d>" % kp, s, 0)
    # pick_s: S = 2 costs rounds x 1.43 where S = 1 covers the same sequences in the same number of rounds (twice the slots) at 1.14
    assert all(rec(kp, 2) in unreached for kp in R.REC_KP)
    # H = 17 .. 48, 65 .. 112 go to the 4x4x1-MFMA kernel at any M (its own 32-bit offset limit is half the entry's: no fall-back left)
    assert all(rec(kp, s) in unreached for kp in (32, 48, 80, 96, 112) for s in (1, 2, 3, 4, 8))
    assert all(rec(kp, s) in reached for kp in (16, 64, 128) for s in (1, 3, 4, 8))
    assert all(R.Pred("lstm_rec_kernel[fused]<%d>" % kp, s, 48) in reached for kp in R.REC_KP for s in (1, 2, 3, 4))
    assert all(R.Pred("lstm_rec_kernel[fused]<%d>" % kp, s, 64) in (reached if kp >= 96 else unreached) for kp in R.REC_KP for s in (1, 2, 3, 4))
    for ng, kq in R.MFMA_TABLE:                              # NG <= 4 means 4H <= 256: only the one-task form; NG = 5: the other two
        forms = {(s, t) for s, t in ((4, 1), (3, 1), (4, 2)) if R.Pred("lstm_mfma_kernel<%d,%d,%d,%d>" % (ng, kq, s, t), s, 0) in reached}
        assert forms == ({(4, 1)} if ng <= 4 else {(3, 1), (4, 2)}), (ng, kq, forms)
    m16 = {(g, nt) for g in range(1, 11) for nt in (1, 2) if R.Pred("lstm_mfma16_kernel<%d,%d>" % (g, nt), 16, 0) in reached}
    assert m16 == {(g, 1) for g in range(1, 9)} | {(g, 2) for g in range(5, 11)}, m16     # two tiles need H > 64, one tile H + I <= 128
    assert all(p in reached for p in comp if p.kernel.startswith(("lstm_mfma_gin", "lstm_mfma16_gin")))
    names = sorted("%s S=%d%s" % (p.kernel, p.S, " IP=%d" % p.IP if p.IP else "") for p in unreached)
    print("%d of %d compiled instantiations are reached by no argument set:" % (len(unreached), len(comp)))
    for n in names:
        print("  " + n)
    assert (len(unreached), len(comp)) == (86, 189)          # DESIGN.md section 11 lists them: a change here is a change there
    covered = {(d["kernel"], d["S"]) for d in E.ALL_CASES if d["entry"] in ("fwd", "fused")}
    missing = sorted({(p.kernel, p.S) for p in reached} - covered)
    print("reached but not in the GPU tables: %s" % missing)
    assert not missing


def test_every_gpu_case_lands_on_the_kernel_it_names():
    assert len({d["id"] for d in E.ALL_CASES}) == len(E.ALL_CASES)
    for d in E.ALL_CASES:
        if d["entry"] in ("fwd", "fused"):
            p = R.predict(d["entry"], d["M"], d["T"], d["H"], d["I"], d["ndir"], d["tun"], d["bif"] or 1)
            assert (p.kernel, p.S) == (d["kernel"], d["S"]), (d["id"], p)
        else:
            cell = "gru" if d["entry"] == "birnn_gru" else "lstm"
            want = R.predict_steps(cell, d["M"], d["T"], d["H"], d["ndir"], d["h0"])
            assert (d["kernel"], d["T"] * d["ndir"]) in want and all(n in R.FP32_GEMMS for n, _ in want if "gemm" in n), (d["id"], want)
        assert d["T"] <= 40 or d["fam"] == "remember" or d["S"] == 2, d["id"]      # small: no call runs longer than a fraction of a second
        assert d["M"] * d["T"] * d["H"] <= 7e6, d["id"]
    for d in E.DISPATCH:                                    # the natural cases are ragged: mixed lengths, no tunables
        assert d["lens"] == "mixed" and not d["tun"], d["id"]
        assert d["S"] == 1 or d["M"] % d["S"] != 0 or d["M"] in (384, 1008, 2032, 2544), d["id"]     # (the exact edge of a threshold)
    for name, r in E.REPS.items():
        assert {d["lens"] for d in E.VARIANTS if d["id"].endswith(name)} >= {None, "mixed", "ones", "wg1", "zero", "over"}, name
