"""CPU: ACG's sampling decode (include/neuroir_acg_sample.h; ACG.sample_extended) without a device -- the symbols and their prototypes, the
refusals, and the acceptance criterion of tests/acg_sample_ref.py itself: the restatement against an enumeration, top_k = 1 against the recorded
greedy tokens, the (b, n) keying, every planted fault rejected, and the stored seeds of the GPU fixtures reproduced by their search."""
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import acg_ref as AR
import acg_sample_ref as R
import gemm_ref
import gru_dec_ref as GR
import sample_ref as SR
from conftest import T

D = R.batch()
SRC, LENS = D["src"], D["lens"]
VT = len(D["tgt_dict"])
MAPS = (D["idx"], D["e2t"], D["e2s"])

# ---- symbols and arguments ----------------------------------------------------------------------------------------------------------------------------
NAMES = {"nir_acg_sample_gen_select_workspace_bytes", "nir_acg_sample_gen_select", "nir_acg_sample_decode_workspace_bytes", "nir_acg_sample_decode",
         "nir_acg_sample_gru_decode_workspace_bytes", "nir_acg_sample_gru_decode"}


def test_new_symbols_exist_with_their_prototypes():
    from conftest import ROOT
    from context_attentive_ir_amd import lib
    main = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    assert '#include "neuroir_acg_sample.h"' in main
    assert not re.findall(r"\bnir_(acg_)?sample\w*\s*\(", main)                 # no prototypes of its own, comments included
    hdr = open(os.path.join(ROOT, "include", "neuroir_acg_sample.h")).read()
    declared = set(re.findall(r"\b(nir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert NAMES == declared == set(lib.ACG_SAMPLE_SIGNATURES) and all(n.startswith("nir_acg_sample_") for n in NAMES)
    others = (set(lib.SIGNATURES) | set(lib.GRU_DECODE_SIGNATURES) | set(lib.BEAM_SIGNATURES) | set(lib.SESSION_BEAM_SIGNATURES) | set(lib.ACG_BEAM_SIGNATURES)
              | set(lib.HREDQS_BEAM_SIGNATURES) | set(lib.SCORE_SIGNATURES) | set(lib.TEACHER_SIGNATURES) | set(lib.SAMPLE_SIGNATURES)
              | set(lib.SESSION_SAMPLE_SIGNATURES) | set(lib.ACG_SCORE_SIGNATURES))
    assert not NAMES & others
    L = lib.load()
    for n in NAMES:
        assert hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, hdr, re.S)
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert nargs == len(lib.ACG_SAMPLE_SIGNATURES[n][1]), n
        assert getattr(L, n).argtypes == lib.ACG_SAMPLE_SIGNATURES[n][1]        # registered by lib.load


def test_the_entries_refuse_bad_arguments_before_any_launch():
    """over fake pointers: nothing may be enqueued (no device needed)"""
    from context_attentive_ir_amd import lib
    C = lib.C
    L = lib.load()
    err = lambda: L.nir_last_error_string()                                    # noqa: E731
    p, big = C.c_void_p(16), 1 << 40
    size = L.nir_acg_sample_gen_select_workspace_bytes

    def gen(rows=6, nsrc=2, K=64, VT=40, top_k=0, inv=1.0, step=0, QL=7, CV=9, stride=7, ws=big, o=p, w=p, frag=None, cw=p, cb=p, at=p, ln=p, mp=p,
            et=p, es=p, tok=p, lp=p, gm=None, gl=None, wsp=p):
        return L.nir_acg_sample_gen_select(o, rows, nsrc, K, w, p, frag, VT, top_k, inv, 5, step, cw, cb, at, stride, ln, QL, mp, et, es, CV, wsp, ws, tok,
                                           lp, gm, gl, None)
    for kw in (dict(o=None), dict(w=None), dict(cw=None), dict(cb=None), dict(at=None), dict(ln=None), dict(mp=None), dict(et=None), dict(es=None),
               dict(tok=None), dict(lp=None)):
        assert gen(**kw) == -1 and b"null" in err(), kw
    for kw in (dict(rows=-1), dict(rows=1 << 31), dict(nsrc=0), dict(nsrc=7), dict(step=-1), dict(step=1 << 32)):
        assert gen(**kw) == -1 and b"step outside" in err(), kw
    for K in (0, -4, 2, 30, 8196):
        assert gen(K=K) == -1 and b"K outside" in err(), K
        assert size(6, K, 40, 0, 0) == 0 and size(6, K, 40, 3, 1) == 0
    assert gen(stride=6) == -1 and b"attn_stride" in err()
    for kw in (dict(QL=0), dict(QL=4097, stride=4097), dict(CV=1), dict(CV=1025), dict(VT=0), dict(VT=(1 << 31) - 16 - 9)):
        assert gen(**kw) == -1 and b"QL outside" in err(), kw
    for top_k in (-1, 9, 41):                                                   # outside 0 .. 8, or above VT
        assert gen(top_k=top_k) == -1 and b"top_k" in err(), top_k
        assert size(6, 64, 40, top_k, 0) == 0
    for inv in (0.0, -1.0, float("inf"), float("nan")):
        assert gen(inv=inv) == -1 and b"inv_temperature" in err(), inv
    assert gen(top_k=3, gm=p) == -1 and gen(top_k=3, gl=p) == -1 and b"whole-distribution" in err()
    for top_k in (0, 3):                                                        # both forms: a short or a null workspace
        assert gen(ws=16, top_k=top_k) == -3 and b"workspace" in err()
        assert gen(wsp=None, top_k=top_k) == -3 and b"workspace" in err()
    assert gen(rows=0, wsp=None, ws=0) == 0                                     # no rows: nothing to enqueue, whatever the workspace
    assert size(6, 64, 40, 0, 1) > 0 and size(6, 64, 40, 3, 0) > size(6, 64, 40, 0, 1) and size(0, 64, 40, 0, 0) == 0
    for cell in ("", "_gru"):
        dec = getattr(L, "nir_acg_sample%s_decode" % cell)
        assert getattr(L, "nir_acg_sample%s_decode_workspace_bytes" % cell)(2, 7, 9, 4, 0, 6, None, None) == 0
        args = ([p, p] if cell == "" else [p]) + [p, p, 2, 7, p, 50, 16, None, 2, 6, None, None, p, p, p, 9, 4, 0, 1.0, 5, p, big, p, p, p, p, p, None]
        assert dec(*args) == -1 and b"null copy weights" in err()


def test_the_old_names_still_refuse_and_name_the_new_ones():
    from context_attentive_ir_amd.recommender import ACG, ACGGRU
    from context_attentive_ir_amd.wrappers import CopyRecommender
    for cls in (ACG, ACGGRU):
        with pytest.raises(NotImplementedError, match="collapsed extended distribution") as e:
            cls.decode_sample(SimpleNamespace(), SRC, LENS, R.MAXLEN, 2)
        assert "sample_extended" in str(e.value)
        assert cls.sample_extended is ACG.sample_extended                       # ACGGRU inherits it
    with pytest.raises(NotImplementedError, match="DESIGN.md section 28") as e:
        CopyRecommender.predict_samples(SimpleNamespace(), {}, 2)
    assert "sample_extended" in str(e.value)
    net, _, _ = R.case("lstm", "general")
    kw = dict(source_rep=SRC, source_len=LENS, max_len=R.MAXLEN, src_map_idx=D["idx"], ext2tgt=D["e2t"], ext2src=D["e2s"])
    for bad in (dict(num_samples=0), dict(num_samples=2, temperature=0.0), dict(num_samples=2, top_k=9), dict(num_samples=2, seed=-1),
                dict(num_samples=2, seed=1 << 64)):
        with pytest.raises(ValueError):
            net.sample_extended(**kw, **bad)
    with pytest.raises(RuntimeError, match="ROCm device"):                      # valid arguments reach the device check: there is no CPU path
        net.sample_extended(**kw, num_samples=2, top_k=8, temperature=0.5, seed=(1 << 64) - 1)
    net.train()
    with pytest.raises(NotImplementedError, match="eval mode"):
        net.sample_extended(**kw, num_samples=2)


# ---- identities ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_restatement_equals_an_enumeration_at_vt_4_cv_3():
    """VT 4, CV 3, slot 2 collapsed onto word 1: five candidates, every one written out by hand"""
    g = torch.Generator().manual_seed(3)
    K, QL = 4, 3
    d = dict(o=torch.randn(2, K, generator=g).double(), gen_w=torch.randn(4, K, generator=g).double(), gen_b=torch.randn(4, generator=g).double(),
             copy_w=torch.randn(K, generator=g).double(), copy_b=torch.tensor([0.3]).double(),
             attn=torch.softmax(torch.randn(2, QL, generator=g), 1).double(), lens=torch.tensor([3]), smap=torch.tensor([[2, 0, 1]]),
             e2t=torch.tensor([[-1, -1, 1]]))
    logp, live, _, _ = R.gen_rows(d, 1)
    assert live.tolist() == [[True] * 6 + [False]] * 2
    drawn = set()
    for seed in range(60):
        for tau in (0.5, 1.0, 3.0):
            c = R.choose(logp, live, seed, 4, 1, 1.0 / tau, 4)
            for r in range(2):
                l = (d["gen_w"] @ d["o"][r] + d["gen_b"]).tolist()
                l[0] = -1e-20
                Z = sum(np.exp(v) for v in l)
                z = 1 / (1 + np.exp(-float(d["copy_w"] @ d["o"][r] + d["copy_b"][0])))
                a = d["attn"][r].tolist()
                P = [(1 - z) * np.exp(l[0]) / Z, (1 - z) * np.exp(l[1]) / Z + z * a[0], (1 - z) * np.exp(l[2]) / Z, (1 - z) * np.exp(l[3]) / Z,
                     z * a[1], z * a[2]]                                        # ids 0 .. 3, VT + 0, VT + 1; VT + 2 is no candidate
                gn = SR.gumbel(SR.words(seed, 4, 1, 2, 7, np.arange(6)[None, :].repeat(2, 0)))[r]       # row r is sample n = r of source row 0
                p = [np.log(P[e]) / tau + gn[e] for e in range(6)]
                e = int(np.argmax(p))
                assert int(c["token"][r]) == e and abs(float(c["logp"][r]) - np.log(P[e])) < 1e-12
                drawn.add(e)
    assert drawn == set(range(6))                                               # every candidate is drawn, the collapsed slot never


CASES6 = [("lstm", t) for t in AR.CASES] + [("gru", t) for t in GR.ACG_CASES]


@pytest.mark.parametrize("kind,tag", CASES6)
def test_top_k_one_reproduces_the_recorded_greedy_tokens(kind, tag):
    net, c, g = AR.case(tag) if kind == "lstm" else GR.case("acg", tag)          # the unmodified greedy fixture
    max_len = int(AR.golden()["max_len"])
    greedy = T(g["predictions"])
    for seed, tau in ((0, 1.0), (77, 0.25)):
        out = R.decode(net.state_dict(), c, "GRU" if kind == "gru" else "LSTM", SRC, LENS, max_len, 2, seed, *MAPS, tau=tau, top_k=1)
        for b in range(SRC.shape[0]):
            for n in range(2):
                L = int(out["lengths"][b, n])
                assert out["predictions"][b, n, :L].tolist() == greedy[b, :L].tolist()


def _dec(kind="lstm", tag="general", N=R.N, seed=None, tau=1.0, top_k=0, src=SRC, lens=LENS, maps=MAPS, **kw):
    net, c, cell = R.case(kind, tag)
    seed = R.SEEDS["%s_%s" % (kind, tag)][R.SETTINGS.index((tau, top_k))] if seed is None else seed
    return R.decode(net.state_dict(), c, cell, src, lens, R.MAXLEN, N, seed, *maps, tau=tau, top_k=top_k, **kw)


def test_two_samples_are_the_first_two_of_four_and_appended_rows_move_nothing():
    four, two = _dec(N=4, seed=5), _dec(N=2, seed=5)
    assert torch.equal(two["predictions"], four["predictions"][:, :2]) and torch.equal(two["scores"], four["scores"][:, :2])
    keep, more = SR.appended_batch(LENS)
    a = _dec(seed=5, src=SRC[keep], lens=LENS[keep], maps=tuple(m[keep] for m in MAPS))
    b = _dec(seed=5, src=SRC[more], lens=LENS[more], maps=tuple(m[more] for m in MAPS))
    assert torch.equal(b["predictions"][:keep.numel()], a["predictions"]) and torch.equal(b["scores"][:keep.numel()], a["scores"])


# ---- the criterion's teeth ------------------------------------------------------------------------------------------------------------------------
def _chi2(fault, tau, rows=16384, seed=21):
    """Pearson's statistic (and its pooled form) of `rows` draws of the restatement, under `fault`, against the true P^(1/tau)"""
    d = R.stat_problem(1)
    logp, live, _, mass = R.gen_rows(d, 1)
    q = torch.where(live[0], logp[0] / tau, torch.full_like(logp[0], float("-inf")))
    probs = torch.softmax(q, 0).numpy()
    flogp, flive, _, _ = R.gen_rows(d, 1, fault=fault if fault == "target_offered_twice" else None)
    if fault in ("collapsed_slot_drawn", "copy_mass_ignored"):
        flogp, flive = R.faulty_rows(flogp, flive, mass, d["e2t"], R.STAT_VT, fault)
    c = R.choose(flogp.expand(rows, -1), flive.expand(rows, -1), seed, 2, 1, 1.0 / tau, R.STAT_VT, 0, fault, torch.float32)
    tok = c["token"].numpy()
    keep = probs > 0
    stray = int((~keep[tok]).sum())                                             # draws of entries the true distribution never offers
    cells = np.searchsorted(np.nonzero(keep)[0], tok[keep[tok]])
    df = int(keep.sum()) - 1
    stat = SR.chi_square(cells, probs[keep]) if stray == 0 else float("inf")
    pooled = SR.chi_square_pooled(cells, probs[keep]) if stray == 0 else (float("inf"), df, 0.0)
    return stat, SR.wilson_hilferty(df, SR.Z_1E6), pooled, stray


@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_the_float32_restatement_passes_the_statistical_criterion(tau):
    for seed in (21, 22):
        stat, thr, (pv, pdf, pthr), stray = _chi2(None, tau, seed=seed)
        print("acg chi-square tau=%g seed=%d: %.1f (%.1f); pooled %.1f at %d degrees of freedom (%.1f)" % (tau, seed, stat, thr, pv, pdf, pthr))
        assert stray == 0 and stat < thr and pv < pthr


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_is_rejected_at_the_margin_cap(fault):
    if fault in R.STAT_FAULTS:
        for tau in (0.5, 1.0, 2.0):
            stat, thr, (pv, pdf, pthr), stray = _chi2(fault, tau)
            assert stat > thr and pv > pthr, (fault, tau, stat, thr)
    # eos_grows shows on a fixture whose samples hold an EOS in front of the end; the others on the first fixture at tau 0.7
    kw = dict(kind="lstm", tag="dot", tau=1.0, top_k=0) if fault == "eos_grows" else dict(tau=0.7, top_k=0)
    ref = _dec(**kw)
    assert fault != "eos_grows" or bool((ref["lengths"] < R.MAXLEN).any())
    chain = _dec(**kw, dtype=torch.float32, force=ref["tokens"])
    ok, fig = R.accept_decode(chain, ref, chain, R.N_SPLIT * R.MAXLEN, gemm_ref.MARGIN_CAP)
    assert ok, fig                                                              # the float32 chain itself passes
    bad = _dec(**kw, fault=fault)
    ok, fig = R.accept_decode(bad, ref, chain, R.N_SPLIT * R.MAXLEN, gemm_ref.MARGIN_CAP)
    assert not ok, (fault, fig)
    if fault == "logp_at_tau":
        assert fig["same"] and fig["scores"]["e"] > fig["scores"]["bound"]      # the tokens are right, the scores are not


# ---- the stored seeds are the search's ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,tag", R.CASES)
def test_the_stored_seeds_are_the_searchs_and_the_draws_hold_every_kind(kind, tag):
    net = R.case(kind, tag)
    key = "%s_%s" % (kind, tag)
    slot = fed = word = False
    for i, (tau, top_k) in enumerate(R.SETTINGS):
        assert R.search_seed(kind, tag, tau, top_k, D=D, net=net) == R.SEEDS[key][i], (tau, top_k)      # within SEARCH_LIMIT at MAXLEN = 6
        cond, ref = R.seed_conditions(kind, tag, tau, top_k, R.SEEDS[key][i], D, net)
        print("%s tau=%g top_k=%d seed %d: min gap %.3g, token bound %.3g" % (key, tau, top_k, R.SEEDS[key][i], cond["gap"], cond["bound"]))
        assert cond["gap"] > max(10 * cond["bound"], R.MIN_GAP) and cond["f32"]
        k = R.drawn_kinds(ref, VT, D["e2t"])
        slot, fed, word = slot or k[0], fed or k[1], word or k[2]
    assert slot and fed and word          # a drawn un-collapsed slot, a drawn target with nonzero copy mass, a drawn word with none
    assert R.search_seed(kind, tag, 0.7, 0, extra=R.pad_free, D=D, net=net) == R.SCORE_SEEDS[key]


def test_some_fixtures_freeze_rows_behind_an_early_eos_and_draw_pad():
    early = pad = 0
    for kind, tag in R.CASES:
        ref = R.seed_conditions(kind, tag, 1.0, 0, R.SEEDS["%s_%s" % (kind, tag)][0], D)[1]
        early += bool((ref["lengths"] < R.MAXLEN).any()) and bool((ref["lengths"] == R.MAXLEN).any())
        pad += bool((ref["predictions"] == 0).any())
    assert early >= 3 and pad >= 1                                              # frozen and live rows side by side; PAD has real mass under ACG
