"""CPU: the criterion of the CARS session tail (tests/cars_session_ref.py) accepts an honest fp32 evaluation on every input the GPU
envelope uses, in two summation orders, and rejects every planted mistake on a named case of that same list."""
import itertools
import os
import re

import pytest
import torch

import cars_session_ref as R
import gemm_ref
from conftest import ROOT

CAP = gemm_ref.MARGIN_CAP
# the planted mistake -> the GPU-file case on which the criterion at the cap rejects it, and the output that shows it
REJECTED_ON = {
    "clicked_only": ("labels_none", "clicks"),                    # m = 0: nothing is clicked, the mistake masks every candidate (NaN pattern)
    "m_own_rows": ("rows_all65_n3", "clicks"),
    "ties_reversed": ("labels_graded", "clicks"),
    "cross_no_zero_state": ("switch_q1d1r1", "scores"),
    "doc_attn_keyed_by_click": ("switch_q0d1r1", "scores"),
    "inner_with_zero_state": ("switch_q1d1r0", "inner_q"),
    "dec_session_major": ("step16_b17_h160", "dec_h"),
    "no_priv1": ("switch_q1d0r1", "scores"),
    "doc_chain_first_candidate": ("switch_q0d1r0", "inner_d"),
    "split_drop_cross": ("step16_b33_h512", "inner_q"),
}


def _fp32(d, **kw):
    return R.restate(d["sd"], d["pooled_q"], d["pooled_docs"], d["labels"], dtype=torch.float32, **dict(d["kw"], **kw))


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_restatement_is_the_oracle_and_honest_fp32_is_accepted(name):
    d = R.build(name)
    c = d["case"]
    for k in R.OUTPUTS:
        ref, mine = d["ref"][k], d["restated"][k]
        assert (ref is None) == (mine is None), k
        if ref is None:
            continue
        nan = torch.isnan(ref)
        assert torch.equal(nan, torch.isnan(mine)), k
        # outside the planted cases no input has a NaN in its reference (a row without a click while m = N)
        assert c["nan"] or not bool(nan.any()), (name, k)
        assert float((ref - mine)[~nan].abs().max()) <= 1e-12 * float(ref[~nan].abs().max()), k
    if c["nan"]:
        assert bool(torch.isnan(d["ref"]["clicks"][1]).any()) and not bool(torch.isnan(d["ref"]["clicks"][[0] + list(range(2, c["B"]))]).any())
        assert bool(torch.isnan(d["ref"]["scores"][1, 1:]).all()) and not bool(torch.isnan(d["ref"]["inner_q"]).any())
    ok, figs = R.accept_all(d["chain"], d, CAP)
    assert ok, figs
    ok, figs = R.accept_all(_fp32(d, order="chunk"), d, CAP)
    print(name, {k: "%.2f" % v["ratio"] for k, v in figs.items()})
    assert ok, figs


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_is_rejected_on_a_named_case(fault):
    name, output = REJECTED_ON[fault]
    d = R.build(name)
    if fault == "split_drop_cross":
        assert R.steps_are_f16(d["case"])
    ok, figs = R.accept_all(_fp32(d, fault=fault), d, CAP)
    f = figs[output]
    print(fault, name, output, "nan pattern equal: %s, e / bound = %.3g" % (f["nan_equal"], f["e"] / f["bound"]))
    assert not ok
    assert not f["nan_equal"] or f["e"] > 4 * f["bound"], f              # not a near miss
    # and the same evaluation without the mistake passes
    assert R.accept_all(_fp32(d), d, CAP)[0]


def test_the_fault_table_is_complete():
    assert set(REJECTED_ON) == set(R.FAULTS) and len(R.FAULTS) == 10
    assert all(name in R.CASES for name, _ in REJECTED_ON.values())


def _enumerate_products(c):
    """flags -> products, written out without cars_session_ref's helpers: (product, outputs whose path holds it, times) for each split product"""
    B, S, N, D, HS = c["B"], c["S"], c["N"], c["D"], c["HS"]
    NR = c["cols"][1] if c["cols"] else N
    big = lambda M, N_, K: not c["exact"] and N_ >= 96 and K >= 32 and ((M + 127) // 128) * ((N_ + 127) // 128) >= 96
    nch = c["q_on"] + c["d_on"]
    chain_outs = ("scores", "dec_h", "dec_c", "inner_q", "inner_d")
    out = []
    if c["d_on"] and c["bits"] & 4 and big(B * S * N, D, D):
        out.append(("click0", ("clicks", "scores", "dec_h", "dec_c", "inner_d"), 1))
    if nch and c["bits"] & 8 and big(B * S, 4 * HS, D):
        out.append(("wih", chain_outs, 1))
    frags = (not c["q_on"] or c["frag_q"]) and (not c["d_on"] or c["frag_d"])
    if nch and frags and HS % 32 == 0 and not c["exact"]:
        out.append(("rec", ("scores", "dec_h", "dec_c"), max(S - 2, 0)))
        out.append(("rec", ("inner_q", "inner_d"), S - 1))
    if c["rank_on"] and c["bits"] & 1 and big(B * S * NR, 512, 4 * D):
        out.append(("mo0", ("scores",), 1))
    if c["rank_on"] and c["bits"] & 2 and big(B * S * NR, 256, 256):
        out.append(("mo1", ("scores",), 1))
    return out


def test_n_split_against_a_plain_enumeration():
    base = R.CASES["opf_all_bits"]
    variants = list(R.CASES.values())
    for bits, fq, fd, ex in itertools.product(range(16), (False, True), (False, True), (False, True)):
        variants.append(dict(base, bits=bits, frag_q=fq, frag_d=fd, exact=ex))
    for q, d_, r in itertools.product((False, True), repeat=3):
        variants.append(dict(base, q_on=q, d_on=d_, rank_on=r))
    for c in variants:
        want = dict.fromkeys(R.OUTPUTS, 0)
        for _, outs, times in _enumerate_products(c):
            for o in outs:
                want[o] += times
        assert R.n_split(c) == want, (c, R.n_split(c), want)
    # the figures the docstring promises for the product shape with everything on: S = 4
    assert R.n_split(base) == dict(clicks=1, scores=6, dec_h=4, dec_c=4, inner_q=4, inner_d=5)
    assert R.n_split(R.CASES["opf_bit0_clear_big"])["scores"] == 4 and R.n_split(R.CASES["opf_bit1_clear_big"])["scores"] == 5 and R.n_split(R.CASES["opf_bit2_clear_big"])["clicks"] == 0
    assert set(R.n_split(R.CASES["step32_mixed_b16_h64"]).values()) == {0}          # the f16 decision is an AND over the chains


def test_every_step_instantiation_and_both_pool_kernels_have_a_case():
    kernels = {R.step_kernel(c) for c in R.CASES.values()}
    assert kernels == {"lstm_step16_kernel<1,1,8>", "lstm_step16_kernel<2,1,8>", "lstm_step16_kernel<4,1,4>", "lstm_step16_kernel<4,4,2>",
                       "lstm_step_kernel<1>", "lstm_step_kernel<2>", "lstm_step_kernel<4>", "lstm_step_kernel<4,2>"}
    # a second chunk round of the k-loop in every instantiation: KB = HS / 32 > 4 CK (fp16), HS / 16 > 4 CH (fp32)
    rounds = {"lstm_step16_kernel<1,1,8>": 32, "lstm_step16_kernel<2,1,8>": 32, "lstm_step16_kernel<4,1,4>": 16, "lstm_step16_kernel<4,4,2>": 8,
              "lstm_step_kernel<1>": 48, "lstm_step_kernel<2>": 32, "lstm_step_kernel<4>": 24, "lstm_step_kernel<4,2>": 16}
    for k, first in rounds.items():
        per = 32 if "16_kernel" in k else 16
        assert any(R.step_kernel(c) == k and c["HS"] // per > first for c in R.CASES.values()), k
    Ns = {c["N"] for c in R.CASES.values() if c["d_on"]}
    assert {1, 2, 63, 64, 65, 128, 129, 2048} <= Ns
    assert {1, 63, 64, 65, 129} <= {c["rows_all"] for c in R.CASES.values()}
    assert {c["B"] for c in R.CASES.values() if c["name"].startswith("step")} >= {1, 16, 17, 32, 33, 65, 255, 256, 257}


def test_struct_field_order_matches_the_header():
    from context_attentive_ir_amd import lib
    hdr = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} nir_cars_session_weights;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [n.strip().lstrip("*") for n in re.sub(r"^(const\s+)?(float|void|int)\s+", "", decl).split(",")]
    assert names == [f for f, _ in lib.CarsSessionWeights._fields_]
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} nir_cars_session_outputs;", hdr, re.S).group(1)
    assert re.findall(r"float\*\s*(\w+);", body) == [f for f, _ in lib.CarsSessionOutputs._fields_]
    assert set(R._FIELDS) | {"wrank", "attn_ut"} == {f for f, t in lib.CarsSessionWeights._fields_ if t is lib.c_fp} - {"sq_whh_frag", "sd_whh_frag"}
    src = open(os.path.join(ROOT, "context_attentive_ir_amd", "csrc", "cars_session.hip")).read()
    assert "B % sessions_per_group == 0" in src and "B % sessions_per_group" in hdr
