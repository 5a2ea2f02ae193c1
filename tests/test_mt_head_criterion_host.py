"""CPU: the teeth of the MatchTensor head criterion (tests/mt_head_ref.py), on the very case list tests/test_gpu_mt_head_envelope.py runs.
  * every planted case meets the coverage condition, from the float64 reference alone: the arg-max cells visit both document ends, both
    sides of every chunk seam, the first and the last query row and the rows at every pass seam;
  * at the margin of its form (mt_head_ref.MARGIN, the one the GPU test uses) the criterion accepts the numpy emulation of each kernel form,
    fp32 accumulators included, on every case of that form;
  * it rejects the same emulation with any single fault a .. m of mt_head_ref.emulate, on the cases REJECTS names -- so a kernel with one
    of these faults cannot pass the GPU test.  Every fault prints by how many times it exceeds the bound (pytest -s);
  * the weights of every family stay within what rankers.mtensor.interaction_bounded assumes, `large` sits just under the 2^15 of the
    fp16 split and its companion just over."""
import numpy as np
import pytest

import mt_head_ref as R

PLANTED = "%s-%s-planted-B2N3-Q17-D65-C50-K30.140"
MATCH = "%s-%s-match-B2N3-Q17-D130-C50-K30.140"
SEL = {"f32": "unbounded", "x2": "nofrag", "x2p": "frag"}
# fault -> the cases that reject it (a, b: the split forms; i: the fused projection).  The planted case has two passes and two chunks; h and
# j need padded positions, which the planted family does not have
REJECTS = {f: [(MATCH if f in "hj" else PLANTED) % (form, SEL[form]) for form in R.FORMS if not (form == "f32" and f in "abi") and not (form == "x2" and f == "i")]
           for f in R.FAULTS}


@pytest.mark.parametrize("d", [d for d in R.CASES if d["fam"] == "planted"], ids=lambda d: d["id"])
def test_planted_cases_meet_the_coverage_condition(d):
    x, p = R.prepared(d)
    assert R.coverage(d, p["arg"].numpy()) == [], d["id"]


@pytest.mark.parametrize("d", R.CASES, ids=lambda d: d["id"])
def test_criterion_accepts_the_honest_form(d):
    x, p = R.prepared(d)
    ok, r = R.accept(R.emulate(d, x), d, x, p)
    print("honest %s: e=%.3g e32=%.3g fmt=%.3g floor=%.3g bound=%.3g e/fmt=%.2f" % (d["id"], r["e"], r["e32"], r["fmt"], r["floor"], r["bound"],
                                                                                  r["e"] / r["fmt"] if r["fmt"] else 0.0))
    assert ok, r
    if d["fam"] == "dead":
        want, tol = R.dead_score(x)
        assert float((p["ref"] - want).abs().max()) <= tol


@pytest.mark.parametrize("fault", R.FAULTS)
def test_criterion_rejects_every_single_fault(fault):
    assert REJECTS[fault]
    for cid in REJECTS[fault]:
        d = R.BY_ID[cid]
        x, p = R.prepared(d)
        ok, r = R.accept(R.emulate(d, x, fault), d, x, p, margin=R.MARGIN_CAP)
        f = r["e"] / r["bound"]
        print("fault %s on %s: e=%.3g = %.3g x bound (%.0f x max(e32, 2^-23))" % (fault, cid, r["e"], f, r["e"] / max(r["e32"], R.EPS)))
        assert not ok, (fault, cid, r)
        assert f > 1.3, (fault, cid, r)                  # not a near miss: e32 moves with the BLAS's summation order


@pytest.mark.parametrize("d", R.CASES, ids=lambda d: d["id"])
def test_weights_stay_within_interaction_bounded(d):
    """the reference's real max|Pq|, max|Pd|, max|U| against the reaches interaction_bounded derives from the weights"""
    x, p = R.prepared(d)
    pq, pd, u, bounded = R.reach(x)
    assert bounded and max(pq, pd, u) < 32768.0
    umax = max(float(np.abs(t).max()) for t in R.fold(p["Pq"].numpy(), x))
    assert float(p["Pq"].abs().max()) <= pq and float(p["Pd"].abs().max()) <= pd and umax <= u
    if d["fam"] == "large":
        assert 2.0 ** 13 <= umax < 2.0 ** 15, umax


@pytest.mark.parametrize("d", [d for d in R.CASES if d["fam"] == "large"], ids=lambda d: d["id"])
def test_large_has_a_companion_just_over_the_bound(d):
    over = dict(d, fam="large_over")
    assert R.reach(R.family(over))[3] is False
    assert R.reach(R.family(d))[3] is True


def test_margin_is_capped_and_the_case_list_covers_what_it_promises():
    assert set(R.MARGIN) == set(R.FORMS) and all(1.0 <= m <= R.MARGIN_CAP == 4.0 for m in R.MARGIN.values())
    d = R.CASES[0]
    x, p = R.prepared(d)
    with pytest.raises(AssertionError):
        R.accept(p["ref"], d, x, p, margin=8.0)
    for d in R.CASES:
        if d["jt"]:
            assert R.chunk_width(d["form"], d["QL"], d["DL"]) == d["jt"], d["id"]
        # the LDS figure the GPU test reads tells the fp32 kernel from the fp16-term one, and one chunk width from the other, at every shape
        jts = {32: 5, 64: 6}[R.chunk_width(d["form"], d["QL"], d["DL"])]
        mine = R.lds_bytes(d["form"], d["QL"], d["DL"], jts)
        other = "x2" if d["form"] == "f32" else "f32"
        assert mine not in (R.lds_bytes(other, d["QL"], d["DL"], 5), R.lds_bytes(other, d["QL"], d["DL"], 6), R.lds_bytes(d["form"], d["QL"], d["DL"], 11 - jts)), d["id"]
    have = lambda form, key: {d[key] for d in R.CASES if d["form"] == form}
    for form in R.FORMS:
        assert {1, 2, 5, 6, 11, 16, 17, 33} <= have(form, "QL") and {1, 3, 31, 32, 33, 64, 65, 129} <= have(form, "DL")
        assert {50, 2, 8} <= have(form, "C") and {30, 2, 14} <= have(form, "Kq") and {(1, 1), (7, 1), (8, 3), (9, 3)} <= {(d["B"], d["N"]) for d in R.CASES if d["form"] == form}
        assert set(R.FAMILIES) <= have(form, "fam")
        for fam in ("match", "edge", "tiny", "large", "dead"):
            assert {R.passes(d["QL"])[0] > 1 for d in R.CASES if d["form"] == form and d["fam"] == fam} == {False, True}
    assert {40, 41, 321} <= have("f32", "DL") and 49 in have("f32", "C") and {"unbounded", "exact", "oddC"} <= have("f32", "sel")
    assert {81, 82, 257} <= have("x2", "DL") and {"nofrag", "decline"} <= have("x2", "sel") and 10 in have("x2", "Kd")
    assert {140, 8, 12, 32, 36, 64, 256} <= have("x2p", "Kd") and 257 in have("x2p", "DL")
    assert {(d["form"], d["jt"]) for d in R.CASES if d["jt"]} == {("f32", 32), ("x2", 32), ("x2", 64), ("x2p", 32), ("x2p", 64)}
