"""CPU: the sampling decode's criterion and host side (tests/sample_ref.py; include/neuroir_sample.h; Seq2seq.decode_sample,
Recommender.predict_samples).  The Philox known answers; the header, lib.SAMPLE_SIGNATURES and the exported symbols agree; argument errors and
refusals without a GPU; every planted fault is rejected by the model-level or the statistical criterion at its stated threshold; and the
conditions the GPU tests rely on hold for the seeds they use -- the gaps of the model fixtures, the near-tie budget of the generator-level
cases, the chi-square of the float32 restatement."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import beam_ref
import sample_ref as R
import seq2seq_ref as S

SRC, LENS, MAXLEN = beam_ref.inputs()


# ---- the noise ------------------------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    z = np.zeros(4, dtype=np.uint64)
    assert [hex(int(v)) for v in R.philox4x32_10(z, z[:2])] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    f = np.full(4, 0xFFFFFFFF, dtype=np.uint64)
    assert [hex(int(v)) for v in R.philox4x32_10(f, f[:2])] == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]


def test_the_noise_is_keyed_by_source_row_sample_step_and_id_alone():
    a = R.words(7, 3, 3, 6, 37)                                                   # rows r = n 3 + b
    b = R.words(7, 3, 5, 10, 37)                                                  # the same (b, n) in a larger batch: rows n 5 + b
    for n in range(2):
        for s in range(3):
            assert np.array_equal(a[n * 3 + s], b[n * 5 + s])
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], a[3])
    assert not np.array_equal(a, R.words(7, 4, 3, 6, 37)) and not np.array_equal(a, R.words(8, 3, 3, 6, 37))
    assert not np.array_equal(a, R.words(7 + (1 << 32), 3, 3, 6, 37))             # the high half of the seed is part of the key
    ids = np.array([[36, 0, 5]] * 6)
    assert np.array_equal(R.words(7, 3, 3, 6, 37, ids), a[:, [36, 0, 5]])         # the top-k form reads the same function
    u = R.uniform(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert u[0] == 2.0 ** -24 and u[1] == 1 - 2.0 ** -24
    assert np.float32(u[1]) == u[1] and np.float32(1 - u[1]) == 1 - u[1]          # u and 1 - u are exact in fp32
    g = R.gumbel(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert -2.82 < g[0] < -2.8 and 16.6 < g[1] < 16.7


def test_the_noise_bound_is_derived_and_rejects_a_fast_log():
    assert R.E_G <= R.E_G_CAP == 4 * 2.0 ** -19                                   # four ulps of an fp32 in [16, 32)
    wd = np.concatenate([np.arange(0xFFFFFFFF - (1 << 20), 0xFFFFFFFF, 512, dtype=np.uint64),
                         np.random.default_rng(0).integers(0, 1 << 32, 1 << 16, dtype=np.uint64)]).astype(np.uint32)
    g64 = R.gumbel(wd)
    assert float(np.abs(g64.astype(np.float32).astype(np.float64) - g64).max()) <= 2.0 ** -20         # the rounding of g alone: half an ulp
    assert float(np.abs(R.gumbel_fast32(wd) - g64).max()) > R.E_G_CAP             # -log u from a log of absolute accuracy: far outside


# ---- symbols and arguments --------------------------------------------------------------------------------------------------------------------
NAMES = {"nir_sample_noise", "nir_sample_gen_workspace_bytes", "nir_sample_gen", "nir_sample_topk_select", "nir_sample_seq2seq_decode_workspace_bytes",
         "nir_sample_seq2seq_decode", "nir_sample_seq2seq_gru_decode_workspace_bytes", "nir_sample_seq2seq_gru_decode"}


def test_new_symbols_exist_with_their_prototypes():
    from conftest import ROOT
    from context_attentive_ir_amd import lib
    main = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    assert '#include "neuroir_sample.h"' in main
    assert not re.findall(r"\bnir_sample_\w*\s*\(", main)                       # no prototypes of its own, comments included
    hdr = open(os.path.join(ROOT, "include", "neuroir_sample.h")).read()
    declared = set(re.findall(r"\b(nir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert NAMES == declared == set(lib.SAMPLE_SIGNATURES)
    assert all(n.startswith("nir_sample_") for n in NAMES)
    others = (set(lib.SIGNATURES) | set(lib.GRU_DECODE_SIGNATURES) | set(lib.BEAM_SIGNATURES) | set(lib.SESSION_BEAM_SIGNATURES) | set(lib.ACG_BEAM_SIGNATURES)
              | set(lib.HREDQS_BEAM_SIGNATURES) | set(lib.SCORE_SIGNATURES) | set(lib.TEACHER_SIGNATURES))
    assert not NAMES & others
    L = lib.load()
    for n in NAMES:
        assert hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, hdr, re.S)
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert nargs == len(lib.SAMPLE_SIGNATURES[n][1]), n
        assert getattr(L, n).argtypes == lib.SAMPLE_SIGNATURES[n][1]            # registered by lib.load
    assert "Philox4x32-10" in hdr[:hdr.index("int nir_sample_noise")]            # the contract stands at the head of the header


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    from context_attentive_ir_amd import lib
    L = lib.load()
    p = 4096                                                                     # a non-null pointer that is never dereferenced: every call fails its checks
    assert L.nir_sample_noise(0, 0, 1, 4, 5, None, None, None) < 0
    assert L.nir_sample_noise(0, -1, 1, 4, 5, p, None, None) < 0 and L.nir_sample_noise(0, 1 << 32, 1, 4, 5, p, None, None) < 0
    assert L.nir_sample_noise(0, 0, 0, 4, 5, p, None, None) < 0 and L.nir_sample_noise(0, 0, 1, -1, 5, p, None, None) < 0
    assert L.nir_sample_noise(0, 0, 1, 4, 0, p, None, None) < 0
    assert L.nir_sample_noise(0, 0, 1, 0, 5, p, None, None) == 0                 # no rows: nothing enqueued
    order = ("x", "rows", "nsrc", "K", "gen_w", "gen_b", "gen_frag", "VT", "inv", "seed", "step", "ws", "nb", "token", "logp", "lse", "st")
    good = dict(x=p, rows=4, nsrc=1, K=32, gen_w=p, gen_b=None, gen_frag=None, VT=5, inv=1.0, seed=0, step=0, ws=p, nb=1 << 20, token=p, logp=p, lse=None,
                st=None)

    def gen(**kw):
        a = dict(good, **kw)
        return L.nir_sample_gen(*[a[k] for k in order])
    for bad in (dict(x=None), dict(token=None), dict(logp=None), dict(gen_w=None), dict(rows=-1), dict(nsrc=0), dict(K=30), dict(K=0), dict(VT=0),
                dict(inv=0.0), dict(inv=-1.0), dict(inv=float("inf")), dict(inv=float("nan")), dict(step=-1)):
        assert gen(**bad) == -1, bad
    assert gen(nb=8) == -3 and gen(ws=None) == -3                                # NIR_ERR_WORKSPACE
    assert gen(rows=0) == 0
    assert L.nir_sample_gen_workspace_bytes(4, 32, 5, 0) >= 4 * 5 * 4 and L.nir_sample_gen_workspace_bytes(4, 32, 5, 1) > 0
    assert L.nir_sample_gen_workspace_bytes(0, 32, 5, 0) == 0 and L.nir_sample_gen_workspace_bytes(4, 30, 5, 0) == 0
    sel = lambda W=3, inv=1.0, tv=p, rows=4: L.nir_sample_topk_select(tv, p, p, rows, 1, W, inv, 0, 0, p, p, None)      # noqa: E731
    assert sel(W=0) == -1 and sel(W=9) == -1 and sel(inv=0.0) == -1 and sel(tv=None) == -1 and sel(rows=0) == 0
    for entry in ("nir_sample_seq2seq_decode", "nir_sample_seq2seq_gru_decode"):
        assert getattr(L, entry + "_workspace_bytes")(4, 7, 2, 0, 6, None) == 0  # no weights
    w = lib.Seq2seqDecoderWeights()
    for f in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "attn_out_w", "gen_w", "gen_b"):
        setattr(w, f, p)
    w.H, w.VT, w.attn_type = 64, 10, lib.S2S_ATTN["dot"]
    ref = lib.C.byref(w)
    assert L.nir_sample_seq2seq_decode_workspace_bytes(4, 7, 2, 0, 6, ref) > 0
    dec = lambda B=0, N=2, top_k=0, inv=1.0, ws=None, nb=0: L.nir_sample_seq2seq_decode(p, p, p, p, B, 7, N, top_k, inv, 0, p, 100, 32, None, 2, 6, ref,   # noqa: E731
                                                                                       ws, nb, p, p, p, p, p, None)
    assert dec() == 0                                                            # B == 0: nothing enqueued, no workspace needed
    assert dec(N=0) == -1 and dec(top_k=9) == -1 and dec(top_k=11) == -1 and dec(inv=0.0) == -1       # ... once the arguments pass
    assert dec(B=4) == -3 and dec(B=4, ws=p, nb=64) == -3                        # rows and a null or short workspace


def _net(kind="s2s", tag="general"):
    return (S.case(tag) if kind == "s2s" else beam_ref.GR.case("s2s", tag))[0]


def test_decode_sample_argument_errors_without_a_gpu():
    net = _net()
    VT = net.generator.weight.shape[0]
    kw = dict(source_rep=SRC, source_len=LENS, max_len=MAXLEN)
    for bad in (dict(num_samples=0), dict(num_samples=-2), dict(num_samples=2, temperature=0.0), dict(num_samples=2, temperature=-1.0),
                dict(num_samples=2, temperature=float("inf")), dict(num_samples=2, temperature=float("nan")), dict(num_samples=2, temperature=1e-60),
                dict(num_samples=2, top_k=-1), dict(num_samples=2, top_k=9), dict(num_samples=2, seed=-1), dict(num_samples=2, seed=1 << 64)):
        with pytest.raises(ValueError):
            net.decode_sample(**kw, **bad)
    small = S.case_args("general", tgt_vocab_size=5)
    from context_attentive_ir_amd.recommender import Seq2seq
    tiny = Seq2seq(small).eval()
    with pytest.raises(ValueError):
        tiny.decode_sample(**kw, num_samples=2, top_k=6)                          # above the target vocabulary
    assert VT > 8
    with pytest.raises(RuntimeError, match="ROCm device"):                        # valid arguments reach the device check: there is no CPU path
        net.decode_sample(**kw, num_samples=2, top_k=8, temperature=0.5, seed=(1 << 64) - 1)


def test_refusals():
    net = _net()
    net.train()
    with pytest.raises(NotImplementedError, match="eval mode"):
        net.decode_sample(SRC, LENS, MAXLEN, 2)
    from context_attentive_ir_amd.recommender import ACG, ACGGRU, Seq2seqGRU
    for cls in (ACG, ACGGRU):
        with pytest.raises(NotImplementedError, match="collapsed extended distribution"):
            cls.decode_sample(SimpleNamespace(), SRC, LENS, MAXLEN, 2)
    assert Seq2seqGRU.decode_sample is type(net).decode_sample and Seq2seqGRU._ENTRY_CELL == "_gru"
    from context_attentive_ir_amd.wrappers import CopyRecommender, SessionRecommender
    for cls in (CopyRecommender, SessionRecommender):
        with pytest.raises(NotImplementedError, match="DESIGN.md section 28"):
            cls.predict_samples(SimpleNamespace(), {}, 2)


# ---- the criterion's teeth ------------------------------------------------------------------------------------------------------------------------
def _decodes(kind, tag, tau, top_k, fault=None):
    net, c, cell, lut = R.case(kind, tag)
    sd = net.state_dict()
    seed = R.SEEDS["%s_%s" % (kind, tag)]
    ref = R.decode(sd, c, cell, SRC, LENS, MAXLEN, R.N, seed, tau, top_k, lut)
    chain = R.decode(sd, c, cell, SRC, LENS, MAXLEN, R.N, seed, tau, top_k, lut, dtype=torch.float32, force=ref["tokens"])
    bad = R.decode(sd, c, cell, SRC, LENS, MAXLEN, R.N, seed, tau, top_k, lut, fault=fault) if fault else None
    return ref, chain, bad


def _chi2(fault, tau, dtype=torch.float32, rows=16384, seed=21, pooled=False):
    x, w, b = R.stat_problem(rows)
    l64 = x[:1].double() @ w.double().t() + b.double()
    c = R.choose((x @ w.t() + b) if dtype == torch.float32 else l64.expand(rows, -1), seed, 0, 128, 1.0 / tau, 0, fault, dtype)
    probs = torch.softmax(l64[0] / tau, 0).numpy()
    return R.chi_square_pooled(c["token"].numpy(), probs) if pooled else R.chi_square(c["token"].numpy(), probs)


def test_the_chi_square_threshold_is_the_stated_quantile():
    assert abs(R.wilson_hilferty(36, R.Z_1E6) - R.CHI2_THRESHOLD) < 0.5           # z of 1 - 1e-6
    x, w, b = R.stat_problem()
    l64 = x[:1].double() @ w.double().t() + b.double()
    assert x.shape == (16384, 32) and w.shape == (37, 32) and 1.2 < float(l64.std()) < 1.9
    low = {tau: 16384 * float(torch.softmax(l64[0] / tau, 0).min()) for tau in (0.5, 1.0, 2.0)}
    print("smallest expected counts: %s" % low)
    # at tau >= 1 every cell expects at least five draws; at tau = 0.5 the rarest tokens expect less than one, where the statistic over all 37
    # cells is badly approximated by its nominal distribution: there the pooled statistic (cells below five expected draws taken as one, its
    # own degrees of freedom and quantile) is asserted NEXT TO the unpooled one against 92
    assert low[1.0] >= 5 and low[2.0] >= 5 and low[0.5] < 1
    probs = torch.softmax(l64[0] / 0.5, 0).numpy()
    stat, df, thr = R.chi_square_pooled(np.arange(37).repeat(400), probs)
    nrare = int((37 * 400 * probs < 5).sum())
    assert nrare > 1 and df == 36 - nrare + 1                                     # the rare cells count as one
    assert abs(thr - R.wilson_hilferty(df, R.Z_1E6)) < 1e-9 and thr < R.CHI2_THRESHOLD
    same = R.chi_square_pooled(np.arange(37).repeat(400), np.full(37, 1 / 37))
    assert same[1] == 36 and abs(same[2] - R.CHI2_THRESHOLD) < 0.5 and same[0] == 0.0      # nothing to pool: the plain statistic


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_the_float32_restatement_passes_the_statistical_criterion(tau):
    for seed in (21, 22):
        v = _chi2(None, tau, seed=seed)
        pv, df, thr = _chi2(None, tau, seed=seed, pooled=True)
        print("chi-square tau=%g seed=%d: %.1f (92); pooled %.1f at %d degrees of freedom (%.1f)" % (tau, seed, v, pv, df, thr))
        assert v < R.CHI2_THRESHOLD and pv < thr
        assert (df == 36) == (tau >= 1)                                           # only tau = 0.5 has cells to pool


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_is_rejected(fault):
    if fault in ("no_noise", "row_shared_noise", "tau_ignored"):
        for tau in ((0.5, 2.0) if fault == "tau_ignored" else (0.5, 1.0, 2.0)):
            pv, df, thr = _chi2(fault, tau, pooled=True)
            assert _chi2(fault, tau) > R.CHI2_THRESHOLD and pv > thr
    tau, top_k = (0.7, 3) if fault == "noise_on_topk_rank" else (0.7, 0)
    kind, tag = "s2s", "general"
    ref, chain, bad = _decodes(kind, tag, tau, top_k, fault)
    ok, fig = R.accept_decode(chain, ref, chain, 2 * MAXLEN)
    assert ok, fig                                                                # the float32 chain itself passes
    ok, fig = R.accept_decode(bad, ref, chain, 2 * MAXLEN)
    assert not ok, (fault, fig)
    if fault == "raw_logit_logp":
        assert fig["same"] and fig["scores"]["e"] > fig["scores"]["bound"]        # the tokens are right, the scores are not
    else:
        assert not fig["same"]


# ---- the conditions the GPU tests rely on ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", R.CASES)
def test_fixture_gaps_and_conditions(kind, tag):
    net, c, cell, lut = R.case(kind, tag)
    sd = net.state_dict()
    seed = R.SEEDS["%s_%s" % (kind, tag)]
    eos_early = False
    for tau, top_k in R.SETTINGS:
        ref, chain, _ = _decodes(kind, tag, tau, top_k)
        free32 = R.decode(sd, c, cell, SRC, LENS, MAXLEN, R.N, seed, tau, top_k, lut, dtype=torch.float32)
        bound = R.model_token_bound(ref, chain, 2 * MAXLEN, tau)
        gap = float(ref["gaps"].min())
        print("%s %s tau=%g top_k=%d: min gap %.3g, token bound %.3g" % (kind, tag, tau, top_k, gap, bound))
        assert gap >= 10 * bound and gap >= R.MIN_GAP
        assert torch.equal(free32["predictions"], ref["predictions"]) and torch.equal(free32["lengths"], ref["lengths"])
        eos_early = eos_early or (bool((ref["lengths"] < MAXLEN).any()) and bool((ref["lengths"] == MAXLEN).any()))
        other = R.decode(sd, c, cell, SRC, LENS, MAXLEN, R.N, seed + R.OTHER_SEED, tau, top_k, lut)
        assert not torch.equal(other["predictions"], ref["predictions"])          # another seed: another draw
        if top_k:
            full = _decodes(kind, tag, tau, 0)[0]
            assert not torch.equal(full["predictions"], ref["predictions"])       # the restriction shows
    assert eos_early                                                              # frozen and live rows side by side
    one = R.decode(sd, c, cell, SRC, LENS, MAXLEN, R.N, seed, 0.3, 1, lut)
    greedy = beam_ref.decode(sd, c, cell, SRC, LENS, MAXLEN, 1, lut)
    assert torch.equal(one["predictions"], greedy["predictions"].expand(-1, R.N, -1))      # top_k = 1 is the greedy decode (frozen at EOS alike)


def test_a_source_rows_samples_do_not_depend_on_the_batch():
    """the (b, n) keying on the restatement, with the batch the GPU test uses: one row appended whose length keeps the sorted-order pairing"""
    net, c, cell, lut = R.case("s2s", "general")
    sd = net.state_dict()
    keep, more = R.appended_batch(LENS)
    a = R.decode(sd, c, cell, SRC[keep], LENS[keep], MAXLEN, R.N, 5, 1.0, 0, lut)
    b = R.decode(sd, c, cell, SRC[more], LENS[more], MAXLEN, R.N, 5, 1.0, 0, lut)
    assert torch.equal(b["predictions"][:keep.numel()], a["predictions"]) and torch.equal(b["scores"][:keep.numel()], a["scores"])
    assert not torch.equal(b["predictions"][-1], a["predictions"][-1])


@pytest.mark.parametrize("ci", range(len(R.GEN_CASES)))
def test_generator_level_cases_stay_within_the_near_tie_budget(ci):
    rows, K, VT, tau, bias, nsrc = R.GEN_CASES[ci]
    for n_split in ((1, 0) if K % 32 == 0 else (0,)):
        d = R.gen_reference(ci, n_split)
        f32 = R.choose(d["logits32"], R.GEN_SEEDS[ci], R.GEN_STEPS[ci], nsrc, 1.0 / tau, dtype=torch.float32)
        ok, near = R.accept_tokens(f32["token"], d["ref"], d["e_p"])
        print("case %d n_split %d: e_y %.3g e_p %.3g near-tie rows %d of %d" % (ci, n_split, d["e_y"], d["e_p"], near, rows))
        assert ok and near <= rows // 100
        if d["dom"] is not None:
            assert bool((d["ref"]["token"] == d["dom"]).all()) and float(d["ref"]["gap"].min()) > 0.3


@pytest.mark.parametrize("kind,tag", R.CASES)
def test_the_score_round_trip_seeds_draw_no_pad_and_keep_their_gaps(kind, tag):
    net, c, cell, lut = R.case(kind, tag)
    sd = net.state_dict()
    seed = R.SCORE_SEEDS["%s_%s" % (kind, tag)]
    ref = R.decode(sd, c, cell, SRC, LENS, MAXLEN, R.N, seed, 0.7, 0, lut)
    chain = R.decode(sd, c, cell, SRC, LENS, MAXLEN, R.N, seed, 0.7, 0, lut, dtype=torch.float32, force=ref["tokens"])
    free32 = R.decode(sd, c, cell, SRC, LENS, MAXLEN, R.N, seed, 0.7, 0, lut, dtype=torch.float32)
    assert bool((ref["predictions"] != 0).all())                                  # no PAD among the samples score_candidates is given
    gap = float(ref["gaps"].min())
    assert gap >= 10 * R.model_token_bound(ref, chain, 2 * MAXLEN, 0.7) and gap >= R.MIN_GAP
    assert torch.equal(free32["predictions"], ref["predictions"])
    assert bool((ref["lengths"] < MAXLEN).any())                                  # an EOS in front of the end: lengths are not all max_len


def test_the_pad_case_holds_pad_in_front_of_an_eos():
    kind, tag, seed = R.PAD_CASE
    net, c, cell, lut = R.case(kind, tag)
    ref = R.decode(net.state_dict(), c, cell, SRC, LENS, MAXLEN, R.N, seed, 0.7, 0, lut)
    pred = ref["predictions"]
    live = torch.arange(MAXLEN).view(1, 1, -1) < ref["lengths"].unsqueeze(2)
    assert bool(((pred == 0) & live).any()) and seed == R.SEEDS["%s_%s" % (kind, tag)]      # (its gaps are test_fixture_gaps_and_conditions')
