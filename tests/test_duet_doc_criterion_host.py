"""CPU: the teeth of the DUET document-branch criterion (tests/duet_doc_ref.py), on the very case list tests/test_gpu_duet_doc_envelope.py runs.
  * every case lands in the form, tile height and tile count it names under the restated dispatch and tiling, and the restatement is
    self-consistent: each pooled row of each document is counted by exactly one (tile, slot), the finish walk adds exactly the (tile, slot)
    partials that count rows of its pair, and the three-document cases really touch three documents;
  * every seam case meets the coverage condition, from the tiling restatement and the float64 reference alone;
  * at MARGIN_CAP the criterion accepts the numpy emulation of every form on every case;
  * it rejects the same emulation with each single fault of duet_doc_ref.emulate on the cases REJECTS names, one per applicable form, by more
    than 1.3 x the bound (the ratio is printed, pytest -s) -- so a kernel with one of these faults cannot pass the GPU test.  Fault 12 (a third
    document's token rows read at the second document's offset) is the exception and is pinned as such: the rows of a third document lie past
    a tile's own rows and feed only pooled rows of weight 0 (duet_doc_ref's docstring has the argument), so no check of m1 can see it;
  * the weights of every family stay within what `bounded` assumes; `large` sits just under the 2^15 of the fp16 split, its companion just
    over; `trained` reaches |z| >= 2, `negative` keeps every pooled value below 0."""
import numpy as np
import pytest
import torch

import duet_doc_ref as R

SEL = {"f96": "planes", "p64": "planes", "t64": "noplanes", "hp": "presplit", "ch": "unfused", "ex": "exact", "un": "unbounded"}
CHAIN = ("hp", "ch", "ex", "un")


def _cid(form, fam):
    if form in R.FUSED:
        return "%s-%s-%s-B2N3-D%d-E20-F20-P5" % (form, SEL[form], fam, 95 if form == "f96" else 63)
    return "%s-%s-%s-B2N3-D40-E20-F20-P5" % (form, SEL[form], fam)


def _rejects():
    out = {}
    for f in R.FAULTS:
        fam = "negative" if f == 6 else "seam"
        forms = R.FORMS
        if f in (1, 2, 3):
            forms = R.SPLIT
        elif f in (7, 8, 9, 10, 11, 17):
            forms = R.FUSED
        elif f == 12:
            forms = ()
        out[f] = [_cid(form, fam) for form in forms]
    return out


REJECTS = _rejects()
THREE_DOC = [d for d in R.CASES if d["rows"] and (d["DL"], d["P"], d["rows"]) in ((63, 5, 64), (95, 5, 96), (64, 4, 64), (96, 4, 96)) and d["B"] * d["N"] >= 3]


@pytest.mark.parametrize("d", R.CASES, ids=lambda d: d["id"])
def test_case_lands_where_it_says_and_the_tiling_is_consistent(d):
    form, rows = R.predicted_form(d)
    assert (form, rows) == (d["form"], d["rows"]), d["id"]
    if not rows:
        return
    M, PL = d["B"] * d["N"], d["DL"] - 1 - d["P"]
    tl = R.case_tiling(d)
    assert tl["n"] == d["tiles"], (tl["n"], d["id"])
    own = R.owners(tl, M)
    assert sorted(own) == [(m, t) for m in range(M) for t in range(PL)] and all(len(v) == 1 for v in own.values()), d["id"]
    for pair in range(M):
        counted = {v[0] for (m, t), v in own.items() if m == pair}
        walk = [(b, s) for b, s in tl["finish"][pair] if b < tl["n"]]
        assert counted <= set(walk) and len(set(walk)) == len(walk), (pair, d["id"])
        for b, s in walk:                                   # a partial the walk adds belongs to this pair (or is empty)
            T = tl["tiles"][b]
            assert T["doc0"] + s == pair or not (T["ok"] & (T["slot"] == s)).any(), (pair, b, s, d["id"])
    # the kernel's plane mode holds rows + 6 token rows per tile: row pr of document offset dd reads token rows pr + 2 dd + (0, 1, 2)
    for T in tl["tiles"]:
        assert len(T["touches"]) <= 3 and int((T["doc"] - T["doc0"]).max()) <= 2


@pytest.mark.parametrize("d", THREE_DOC, ids=lambda d: d["id"])
def test_three_document_cases_touch_three_documents(d):
    tl = R.case_tiling(d)
    three = [T for T in tl["tiles"] if len(T["touches"]) == 3]
    assert three, d["id"]
    for T in three:                                         # the third document's rows are never a tile's own
        assert not T["ok"][T["doc"] == T["doc0"] + 2].any()


def test_three_document_lengths_are_the_derived_ones():
    for rows in (64, 96):
        for P in (1, 2, 3, 4, 5):
            cap = rows - (P - 1)
            for Tc in range(cap - 2, cap + 8):
                has = any(len(T["touches"]) == 3 for T in R.tiling(7, Tc + 2, P, rows)["tiles"])
                assert not has or cap + 1 <= Tc <= cap + P - 3, (rows, P, Tc)          # necessary: a tile start t00 with t00 + rows > 2 Tc
                assert has or Tc != cap + 1 or P < 4, (rows, P, Tc)                    # Tc == cap + 1: tile 1 starts at Tc - 1
    assert {(d["DL"], d["P"], d["rows"]) for d in THREE_DOC} == {(63, 5, 64), (95, 5, 96), (64, 4, 64), (96, 4, 96)}


@pytest.mark.parametrize("d", [d for d in R.CASES if d["fam"] == "seam"], ids=lambda d: d["id"])
def test_seam_cases_meet_the_coverage_condition(d):
    x, p = R.prepared(d)
    assert R.coverage(d, p) == [], d["id"]


@pytest.mark.parametrize("d", R.CASES, ids=lambda d: d["id"])
def test_criterion_accepts_the_honest_form(d):
    x, p = R.prepared(d)
    ok, r = R.accept(R.emulate(d, x), d, x, p, margin=R.MARGIN_CAP)
    print("honest %s: e=%.3g e32=%.3g fmt=%.3g floor=%.3g bound=%.3g ratio=%.2f" % (d["id"], r["e"], r["e32"], r["fmt"], r["floor"], r["bound"], r["ratio"]))
    assert ok, r


@pytest.mark.parametrize("fault", [f for f in R.FAULTS if f != 12])
def test_criterion_rejects_every_single_fault(fault):
    assert REJECTS[fault]
    for cid in REJECTS[fault]:
        d = R.BY_ID[cid]
        x, p = R.prepared(d)
        ok, r = R.accept(R.emulate(d, x, fault), d, x, p, margin=R.MARGIN_CAP)
        f = r["e"] / r["bound"]
        print("fault %d on %s: e=%.3g = %.3g x bound (%.0f x max(e32, 2^-23))" % (fault, cid, r["e"], f, r["r"]))
        assert not ok, (fault, cid, r)
        assert f > 1.3, (fault, cid, r)                  # not a near miss: e32 moves with the BLAS's summation order


@pytest.mark.parametrize("d", [d for d in THREE_DOC if d["form"] in R.PLANE], ids=lambda d: d["id"])
def test_fault_12_cannot_reach_m1(d):
    """what a three-document tile reads for its third document only feeds pooled rows of weight 0: the emulation with fault 12 equals the honest
    one bit for bit, while the conv rows it computes there do differ"""
    x, p = R.prepared(d)
    assert torch.equal(R.emulate(d, x, 12), R.emulate(d, x))
    T = next(T for T in R.case_tiling(d)["tiles"] if len(T["touches"]) == 3)
    third = np.nonzero(T["doc"] == T["doc0"] + 2)[0]
    assert not np.array_equal(R._rows_of(x, T["doc"][third], T["t"][third], shift=-2), R._rows_of(x, T["doc"][third], T["t"][third]))


@pytest.mark.parametrize("d", R.CASES, ids=lambda d: d["id"])
def test_weights_stay_within_bounded(d):
    x, p = R.prepared(d)
    assert R.bounded(x) is True
    assert bool(torch.isfinite(p["ref"]).all())
    if d["fam"] == "large":
        top = max(float(x[k].abs().max()) for k in ("table", "w1", "w2"))
        assert 2.0 ** 14.9 <= top < 2.0 ** 15, top
        assert all(float(x[k].abs().max()) >= 2.0 ** 14.9 for k in ("table", "w1", "w2"))
        assert R.bounded(R.family(dict(d, fam="large_over"))) is False
    if d["fam"] in ("trained", "seam") and d["DL"] >= 20:          # (a handful of conv rows at DL = 7)
        assert float(p["z1"].abs().max()) >= 2.0, float(p["z1"].abs().max())
    if d["fam"] == "negative":
        assert float(p["p"].max()) < 0.0, float(p["p"].max())
    ids = x["d_ids"]
    assert bool((ids == R.PAD).any()) and bool((ids == d["V"] - 1).any()) and int(ids.min()) >= 0 and int(ids.max()) < d["V"]


def test_margin_is_capped_and_the_case_list_covers_what_it_promises():
    assert set(R.MARGIN) == set(R.FORMS) == set(R.MEASURED) and all(1.0 <= m <= R.MARGIN_CAP == 4.0 for m in R.MARGIN.values())
    assert all(R.MEASURED[f][1] <= R.MARGIN[f] for f in R.FORMS)
    d = R.CASES[0]
    x, p = R.prepared(d)
    with pytest.raises(AssertionError):
        R.accept(p["ref"], d, x, p, margin=8.0)
    have = lambda form, key, **kw: {d[key] for d in R.CASES if d["form"] == form and all(d[k] == v for k, v in kw.items())}
    assert {7, 61, 62, 63, 64, 93} <= have("p64", "DL", P=5) and {94, 95, 97, 200} <= have("f96", "DL", P=5) and {7, 62, 63, 64} <= have("t64", "DL", P=5)
    assert any(d["form"] == "f96" and d["DL"] == 95 and d["B"] * d["N"] == 1 for d in R.CASES)
    for form in ("p64", "t64"):
        assert {1, 2, 3, 4, 5} <= have(form, "P")
        for P in (1, 2, 3, 4):
            assert {R.case_tiling(d)["flat"] for d in R.CASES if d["form"] == form and d["P"] == P} == {False, True}
    assert {1, 2, 3, 4, 5} <= have("f96", "P")
    for form in R.FUSED:
        assert {4, 20, 52, 300} <= have(form, "E") and {4, 60, 300, 320} <= have(form, "NF") and (300, 300, 5) in {(d["E"], d["NF"], d["P"]) for d in R.CASES if d["form"] == form}
        assert set(R.FAMILIES) <= have(form, "fam")
    assert 448 in have("p64", "E") and 640 in have("t64", "E") and "rows64" in have("p64", "sel") and {"noplanes", "planes"} <= have("t64", "sel")
    assert {(1, 1), (1, 3), (2, 3)} <= {(d["B"], d["N"]) for d in R.CASES}
    for form in CHAIN:
        assert {"model", "trained", "negative", "seam"} <= have(form, "fam") and {20, 300} <= have(form, "E")
    for f, cids in REJECTS.items():
        assert all(c in R.BY_ID for c in cids), f
