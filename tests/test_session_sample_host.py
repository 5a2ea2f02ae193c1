"""CPU: the criterion and the host side of the sampling decode of HredQS and the session models (tests/session_sample_ref.py;
include/neuroir_session_sample.h; CARS / M_MATCH_TENSOR / MNSRF / HredQS .decode_sample; SessionRecommender.predict_session_samples,
Multitask.predict_samples).  The header, lib.SESSION_SAMPLE_SIGNATURES and the exported symbols agree; every C entry refuses bad arguments without
a GPU; the Python argument errors and refusals; the conditions the GPU tests rely on hold for the stored seeds; the float32 restatement passes
the model-level criterion on every case and every planted fault is rejected by it; the (decode row, sample) keying of the noise."""
import os
import re
from types import SimpleNamespace

import gemm_ref
import pytest
import torch

import sample_ref as SR
import session_sample_ref as R

NAMES = {"nir_sample_hredqs_gen_workspace_bytes", "nir_sample_hredqs_gen", "nir_sample_hredqs_decode_workspace_bytes", "nir_sample_hredqs_decode",
         "nir_sample_plain_decode_workspace_bytes", "nir_sample_plain_decode", "nir_sample_cars_decode_workspace_bytes", "nir_sample_cars_decode"}


# ---- symbols and arguments --------------------------------------------------------------------------------------------------------------------
def test_new_symbols_exist_with_their_prototypes():
    from conftest import ROOT
    from context_attentive_ir_amd import lib
    main = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    assert '#include "neuroir_session_sample.h"' in main
    assert not re.findall(r"\bnir_sample_\w*\s*\(", main)                       # no prototypes of its own, comments included
    hdr = open(os.path.join(ROOT, "include", "neuroir_session_sample.h")).read()
    declared = set(re.findall(r"\b(nir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert NAMES == declared == set(lib.SESSION_SAMPLE_SIGNATURES)
    others = (set(lib.SIGNATURES) | set(lib.GRU_DECODE_SIGNATURES) | set(lib.BEAM_SIGNATURES) | set(lib.SESSION_BEAM_SIGNATURES) | set(lib.ACG_BEAM_SIGNATURES)
              | set(lib.HREDQS_BEAM_SIGNATURES) | set(lib.SCORE_SIGNATURES) | set(lib.TEACHER_SIGNATURES) | set(lib.SAMPLE_SIGNATURES))
    assert not NAMES & others
    L = lib.load()
    for n in NAMES:
        assert hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, hdr, re.S)
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert nargs == len(lib.SESSION_SAMPLE_SIGNATURES[n][1]), n
        assert getattr(L, n).argtypes == lib.SESSION_SAMPLE_SIGNATURES[n][1]    # registered by lib.load
    head = hdr[:hdr.index("size_t nir_sample_hredqs_gen_workspace_bytes")]
    assert "neuroir_sample.h" in head and "Philox" not in head                   # the semantics by reference: nothing restated that could drift


def _hq_weights(H=8, VT=10, packs=False):
    from context_attentive_ir_amd import lib
    w = lib.HredqsDecoderWeights()
    for f in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "gen_w", "gen_b") + (("rnn_gate_fold", "rnn_whh_frag", "gen_frag") if packs else ()):
        setattr(w, f, 16)
    w.H, w.VT = H, VT
    return w


def test_the_split_state_entry_refuses_bad_arguments_without_a_gpu():
    from context_attentive_ir_amd import lib
    L = lib.load()
    err = lambda: L.nir_last_error_string()                                  # noqa: E731
    p, big = lib.C.c_void_p(16), 1 << 30

    def gen(h16=p, rows=5, nsrc=1, K=64, frag=p, VT=40, inv=1.0, step=0, ws=p, nb=big, token=p, logp=p):
        return L.nir_sample_hredqs_gen(h16, rows, nsrc, K, p, frag, VT, inv, 0, step, ws, nb, token, logp, None, None)
    for bad in (dict(h16=None), dict(frag=None), dict(token=None), dict(logp=None)):
        assert gen(**bad) == -1 and b"null" in err(), bad
    for bad in (dict(rows=-1), dict(nsrc=0), dict(step=-1), dict(step=1 << 32)):
        assert gen(**bad) == -1, bad
    for K in (0, 16, 48, 1056):                                                 # fast form only: K a multiple of 32 in [32, 1024]
        assert gen(K=K) == -1 and b"multiple of 32" in err()
        assert L.nir_sample_hredqs_gen_workspace_bytes(5, K, 40) == 0
    assert gen(VT=0) == -1 and gen(VT=(1 << 31) - 16) == -1
    for inv in (0.0, -1.0, float("inf"), float("nan")):
        assert gen(inv=inv) == -1 and b"inv_temperature" in err()
    assert gen(nb=64) == -3 and gen(ws=None) == -3 and b"workspace" in err()     # NIR_ERR_WORKSPACE
    assert gen(rows=0) == 0 and gen(rows=0, ws=None, nb=0) == 0                  # no rows: nothing enqueued
    assert L.nir_sample_hredqs_gen_workspace_bytes(0, 64, 40) == 0
    assert L.nir_sample_hredqs_gen_workspace_bytes(65, 64, 4099) > L.nir_sample_hredqs_gen_workspace_bytes(5, 64, 40) > 0


def test_the_decode_entries_refuse_bad_arguments_without_a_gpu():
    """over fake pointers: nothing may be enqueued"""
    from context_attentive_ir_amd import lib
    C = lib.C
    L = lib.load()
    err = lambda: L.nir_last_error_string()                                  # noqa: E731
    p, big = C.c_void_p(16), 1 << 30
    # --- the decoders without attention
    def plain(Bd=2, N=2, top_k=0, inv=1.0, VT=10, ws=p, nb=big, pred=p, tlp=p, H=8, dec_h=p, fold=None, frag=None):
        return L.nir_sample_plain_decode(dec_h, p, Bd, H, p, 20, 4, p, p, p, p, p, p, VT, None, 2, 6, fold, fold, frag, N, top_k, inv, 0, ws, nb, pred, tlp, p, p,
                                         None)
    assert plain(N=0) == -1 and plain(top_k=9) == -1 and plain(top_k=-1) == -1 and b"top_k" in err()
    assert plain(top_k=6, VT=5) == -1 and b"top_k" in err()                     # above the target vocabulary
    assert plain(inv=0.0) == -1 and plain(inv=float("nan")) == -1 and b"inv_temperature" in err()
    assert plain(pred=None) == -1 and plain(tlp=None) == -1 and plain(dec_h=None) == -1 and b"null" in err()
    assert plain(H=6) == -1 and b"bad dims" in err()
    assert plain(nb=16) == -3 and plain(ws=None, nb=0) == -3 and b"workspace" in err()
    assert plain(Bd=0, ws=None, nb=0) == 0 and plain(Bd=0, ws=None, nb=0, H=32, VT=100, fold=p, frag=p) == 0     # in both forms
    assert plain(Bd=0, N=0, ws=None, nb=0) == -1                                # ... once the arguments pass
    q = L.nir_sample_plain_decode_workspace_bytes
    assert q(2, 8, 10, 2, 0, 6, 0, 0) > q(0, 8, 10, 2, 0, 6, 0, 0) and q(2, 8, 10, 4, 0, 6, 0, 0) > q(2, 8, 10, 2, 0, 6, 0, 0)
    assert q(2, 8, 10, 0, 0, 6, 0, 0) == 0 and q(2, 8, 10, 2, 9, 6, 0, 0) == 0 and q(2, 8, 5, 2, 6, 6, 0, 0) == 0 and q(2, 6, 10, 2, 0, 6, 0, 0) == 0
    assert q(40, 32, 5000, 4, 0, 6, 0, 0) > 160 * 5000 * 4 > q(40, 32, 5000, 4, 0, 6, 1, 1) > 0      # the fused form holds no [R, VT] logits
    # --- HredQS
    w = _hq_weights()
    def hq(B=2, S=3, N=2, top_k=0, inv=1.0, wt=w, ws=p, nb=big, pred=p, tlp=p, E=4, max_len=6):
        return L.nir_sample_hredqs_decode(p, p, B, S, p, 20, E, None, 2, max_len, C.byref(wt) if wt is not None else None, N, top_k, inv, 0, ws, nb, pred, tlp,
                                          p, p, None)
    assert hq(N=0) == -1 and hq(top_k=9) == -1 and b"top_k" in err()
    assert hq(top_k=6, wt=_hq_weights(VT=5)) == -1 and b"top_k" in err()
    assert hq(inv=0.0) == -1 and b"inv_temperature" in err()
    assert hq(pred=None) == -1 and hq(tlp=None) == -1 and hq(wt=None) == -1 and b"null" in err()
    assert hq(wt=_hq_weights(H=6)) == -1 and b"weights" in err()
    assert hq(E=6) == -1 and hq(max_len=0) == -1 and hq(B=-1) == -1 and b"bad dims" in err()
    half = _hq_weights()
    half.rnn_gate_fold = 16
    assert hq(wt=half) == -1 and b"come together" in err()
    assert hq(B=1 << 20, S=1 << 20) == -1 and b"too many" in err()
    assert hq(nb=16) == -3 and hq(ws=None, nb=0) == -3 and b"workspace" in err()
    for wt in (w, _hq_weights(H=32, VT=100, packs=True)):
        assert hq(B=0, wt=wt, ws=None, nb=0) == 0 and hq(S=0, wt=wt, ws=None, nb=0) == 0
    qh = lambda B, S, N, K, wt: L.nir_sample_hredqs_decode_workspace_bytes(B, S, N, K, 6, C.byref(wt))        # noqa: E731
    assert qh(2, 3, 2, 0, w) > qh(0, 3, 2, 0, w) and qh(2, 3, 4, 0, w) > qh(2, 3, 2, 0, w) and qh(2, 3, 2, 9, w) == 0 and qh(2, 3, 0, 0, w) == 0
    plain_w, fast_w = _hq_weights(H=32, VT=5000), _hq_weights(H=32, VT=5000, packs=True)
    assert qh(4, 4, 8, 0, plain_w) > 128 * 5000 * 4 > qh(4, 4, 8, 0, fast_w) > 0
    # --- CARS
    cw = lib.CarsDecoderWeights()
    for f in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "attn_in_w", "attn_out_w", "dec_attn_w", "pred1_w", "pred2_w", "sess_w"):
        setattr(cw, f, 16)
    cw.HD, cw.DQ, cw.P, cw.KS, cw.VT = 8, 8, 8, 4, 10
    ref = C.byref(cw)
    def cars(Bd=2, N=2, top_k=0, inv=1.0, ws=p, nb=big, pred=p, tlp=p, frag=None, sess=p):
        return L.nir_sample_cars_decode(p, p, p, p, 3, 5, p, Bd, sess, p, 20, 4, None, 2, 6, ref, frag, N, top_k, inv, 0, ws, nb, pred, tlp, p, p, None)
    assert cars(N=0) == -1 and cars(top_k=9) == -1 and cars(top_k=11) == -1 and b"top_k" in err()
    assert cars(inv=0.0) == -1 and b"inv_temperature" in err()
    assert cars(pred=None) == -1 and cars(tlp=None) == -1 and b"null" in err()
    assert cars(sess=None) == -1 and b"session" in err()
    assert cars(nb=16) == -3 and cars(ws=None, nb=0) == -3 and b"workspace" in err()
    assert cars(Bd=0, ws=None, nb=0) == 0 and cars(Bd=0, ws=None, nb=0, frag=p) == 0
    qc = L.nir_sample_cars_decode_workspace_bytes
    assert qc(3, 2, 5, 2, 0, 6, ref, 0) > qc(3, 0, 5, 2, 0, 6, ref, 0) > 0 and qc(3, 2, 5, 2, 9, 6, ref, 0) == 0 and qc(3, 2, 5, 0, 0, 6, ref, 0) == 0
    cw.VT = 5
    assert cars(top_k=6) == -1 and b"top_k" in err()                            # above the target vocabulary
    cw.VT, cw.P = 10, 6
    assert cars() == -1 and b"bad dims" in err()


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------------------
BAD_ARGS = (dict(num_samples=0), dict(num_samples=-2), dict(num_samples=2, temperature=0.0), dict(num_samples=2, temperature=-1.0),
            dict(num_samples=2, temperature=float("inf")), dict(num_samples=2, temperature=float("nan")), dict(num_samples=2, temperature=1e-60),
            dict(num_samples=2, top_k=-1), dict(num_samples=2, top_k=9), dict(num_samples=2, seed=-1), dict(num_samples=2, seed=1 << 64))


def _session_net(key):
    from helpers import build_model
    c = R.load(key)
    cs = c["cs"]
    kind = cs["kind"]
    m = build_model({"cars": "CARS", "mmt": "M_MATCH_TENSOR", "mnsrf": "MNSRF"}[kind], tgt_vocab_size=cs["lut"].shape[0], **cs.get("cfg", {}))
    kw = dict(states=(cs["dec_h"].unsqueeze(0), cs["dec_c"].unsqueeze(0)), max_len=cs["max_len"], src_dict=None, tgt_dict=None, batch_size=cs["B"],
              session_len=cs["SD"])
    if kind == "cars":
        kw.update(encoded_source=cs["enc"], source_len=cs["lens"], session_attns=cs["attns"])
    return m.eval(), kw


@pytest.mark.parametrize("key", ["cars_full", "mmt", "mnsrf", "hq_h64"])
def test_decode_sample_argument_errors_and_the_device_check_without_a_gpu(key):
    if key.startswith("hq_"):
        import hredqs_ref as H
        cs = R.load(key)["cs"]
        net = H.case(key[3:])[0].eval()
        kw = dict(source_rep=cs["src"], source_len=cs["lens"], max_len=cs["max_len"])
    else:
        net, kw = _session_net(key)
    for bad in BAD_ARGS:
        with pytest.raises(ValueError, match="decode_sample"):
            net.decode_sample(**kw, **bad)
    with pytest.raises(RuntimeError, match="ROCm device"):                        # valid arguments reach the device check: there is no CPU path
        net.decode_sample(**kw, num_samples=2, top_k=8, temperature=0.5, seed=(1 << 64) - 1)
    net.train()
    with pytest.raises(NotImplementedError, match="eval mode"):
        net.decode_sample(**kw, num_samples=2)


def test_the_argument_checks_are_one_helper_with_seq2seqs_texts():
    import seq2seq_ref as S
    from context_attentive_ir_amd.multitask import suggest
    import beam_ref
    SRC, LENS, MAXLEN = beam_ref.inputs()
    net = S.case("general")[0]
    VT = net.generator.weight.shape[0]
    for bad in BAD_ARGS:
        with pytest.raises(ValueError) as a:
            net.decode_sample(SRC, LENS, MAXLEN, **bad)
        with pytest.raises(ValueError) as b:
            suggest.check_sample_args(net, bad["num_samples"], bad.get("temperature", 1.0), bad.get("top_k", 0), bad.get("seed", 0), VT)
        assert str(a.value) == str(b.value)
    assert suggest.check_sample_args(net, 3, 0.5, 2, 7, VT) == (3, 2, 0.5, 7)
    assert suggest.sample_fused(SimpleNamespace(), suggest.FUSE_SAMPLE_MAX_ROWS, 0) and not suggest.sample_fused(SimpleNamespace(), suggest.FUSE_SAMPLE_MAX_ROWS + 1, 0)
    assert suggest.sample_fused(SimpleNamespace(), suggest.FUSE_SAMPLE_MAX_ROWS, 3) and not suggest.sample_fused(SimpleNamespace(fuse_generator_topk=False), 4, 3)
    assert not suggest.sample_fused(SimpleNamespace(), suggest.FUSE_SAMPLE_MAX_ROWS + 1, 3)      # the cap holds with and without top_k (measured)
    assert suggest.sample_fused(SimpleNamespace(fuse_sample_max_rows=None), 1 << 20, 0) and suggest.sample_fused(SimpleNamespace(fuse_sample_max_rows=None), 1 << 20, 3)
    from context_attentive_ir_amd.multitask import CARS, MNSRF
    assert CARS.fuse_sample_max_rows is None and not hasattr(MNSRF, "fuse_sample_max_rows")       # DESIGN.md section 29's table
    assert not suggest.sample_fused(SimpleNamespace(fuse_generator_argmax=False), 4, 0) and suggest.sample_fused(SimpleNamespace(fuse_sample_max_rows=8), 8, 0)


def test_refusals_and_the_wrappers_surface():
    from context_attentive_ir_amd.recommender import ACG, ACGGRU
    from context_attentive_ir_amd.wrappers import CopyRecommender, Multitask, SessionRecommender
    for cls in (ACG, ACGGRU):
        with pytest.raises(NotImplementedError, match="collapsed extended distribution"):
            cls.decode_sample(SimpleNamespace(), None, None, 5, 2)
    with pytest.raises(NotImplementedError, match="DESIGN.md section 28"):
        CopyRecommender.predict_samples(SimpleNamespace(), {}, 2)
    with pytest.raises(NotImplementedError, match="predict_session_samples.*DESIGN.md\\s+section 28"):
        SessionRecommender.predict_samples(SimpleNamespace(), {}, 2)
    assert callable(SessionRecommender.predict_session_samples) and callable(Multitask.predict_samples)
    from context_attentive_ir_amd.config import default_args
    off = Multitask(default_args("CARS", src_vocab_size=200, tgt_vocab_size=200, turn_recommender_off=True))
    assert off.network.no_recommender


# ---- the conditions the GPU tests rely on ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decodes():
    """per (case, setting): (fp64 decode, fp32 decode forced along the fp64 tokens) at the stored seed -- once"""
    out = {}
    for key in R.KEYS:
        for si, (tau, top_k) in enumerate(R.SETTINGS):
            ref = R.decode(key, R.SEEDS[key][si], tau, top_k)
            out[key, si] = (ref, R.decode(key, R.SEEDS[key][si], tau, top_k, dtype=torch.float32, force=ref["tokens"]))
    return out


@pytest.mark.parametrize("key", R.KEYS)
def test_the_stored_seeds_keep_their_gaps_in_every_setting(decodes, key):
    c = R.load(key)
    for si, (tau, top_k) in enumerate(R.SETTINGS):
        seed = R.SEEDS[key][si]
        ref, chain = decodes[key, si]
        bound = R.token_bound(ref, chain, R.n_split(c, True, True), tau)
        gap = float(ref["gaps"].min())
        print("%s tau=%g top_k=%d seed %d: min gap %.3g, token bound %.3g" % (key, tau, top_k, seed, gap, bound))
        assert ref["gaps"].shape == (c["max_len"], c["Bd"] * R.N)                # no step and no row is left out
        assert gap >= max(10 * bound, SR.MIN_GAP)
        free = R.decode(key, seed, tau, top_k, dtype=torch.float32)
        assert torch.equal(free["predictions"], ref["predictions"]) and torch.equal(free["lengths"], ref["lengths"])
        other = R.decode(key, seed + R.OTHER_SEED, tau, top_k)
        assert not torch.equal(other["predictions"], ref["predictions"])          # another seed: another draw
        ok, fig = R.accept_decode(dict(chain), ref, chain, 0)                     # the float32 restatement passes the model-level criterion
        assert ok, fig


@pytest.mark.parametrize("key", R.KEYS)
def test_the_score_round_trip_seeds_draw_no_pad_and_keep_their_gaps(key):
    d = R.seed_conditions(key, R.SCORE_SEEDS[key], *R.SCORE_SETTING, score=True)
    assert d["gap_ok"] and d["f32"] and d["pad_ok"], d
    assert R.gapped_seed(key, *R.SCORE_SETTING, score=True) == R.SCORE_SEEDS[key]     # the first such seed: the stored value is the search's


def test_the_stored_seeds_are_the_searchs():
    for key in ("cars_full", "mmt", "hq_h64"):
        assert [R.gapped_seed(key, tau, top_k) for tau, top_k in R.SETTINGS] == R.SEEDS[key]


@pytest.mark.parametrize("key", R.KEYS)
def test_top_k_one_is_the_recorded_greedy_decode(key):
    c = R.load(key)
    cs = c["cs"]
    want = cs["greedy"].reshape(c["Bd"], -1)
    for seed in (1, 2):
        one = R.decode(key, seed, 0.3, 1)
        for i in range(c["Bd"]):
            for n in range(R.N):                                                # up to each row's first EOS
                ln = int(one["lengths"][i, n])
                assert torch.equal(one["predictions"][i, n, :ln], want[i, :ln]), (key, i, n)


# ---- the criterion's teeth ------------------------------------------------------------------------------------------------------------------------
def _rejected(key, fault, tau, top_k, seeds=range(1, 13)):
    """whether some seed's float64 decode with `fault` planted is rejected at the margin's cap while the float32 chain passes"""
    c = R.load(key)
    ns = R.n_split(c, True, True)
    for seed in seeds:
        ref = R.decode(key, seed, tau, top_k)
        chain = R.decode(key, seed, tau, top_k, dtype=torch.float32, force=ref["tokens"])
        ok, fig = R.accept_decode(dict(chain), ref, chain, ns, margin=gemm_ref.MARGIN_CAP)
        assert ok, (key, seed, fig)
        bad = R.decode(key, seed, tau, top_k, fault=fault)
        if not R.accept_decode(bad, ref, chain, ns, margin=gemm_ref.MARGIN_CAP)[0]:
            return True
    return False


@pytest.mark.parametrize("fault", SR.FAULTS)
def test_every_planted_fault_is_rejected_on_a_session_case_and_an_hredqs_case(fault):
    tau, top_k = (0.7, 3) if fault == "noise_on_topk_rank" else (0.7, 0)
    for key in ("mnsrf", "hq_h64"):                                             # (small target vocabularies: an EOS is drawn within a few seeds)
        assert _rejected(key, fault, tau, top_k), (key, fault)


@pytest.mark.parametrize("key,fault", [("cars_full", "wrong_source_row"), ("cars_full", "sess_dropped"), ("cars_qoff", "sess_dropped"),
                                       ("cars_doff", "sess_dropped"), ("hq_h64", "natural_pairing"), ("hq_h1024", "natural_pairing")])
def test_the_layout_faults_are_rejected_where_they_apply(key, fault):
    assert _rejected(key, fault, 1.0, 0, seeds=(R.SEEDS[key][0],))


# ---- the keying of the noise --------------------------------------------------------------------------------------------------------------------
def _first_rows(cs, n):
    return dict(cs, dec_h=cs["dec_h"][:n], dec_c=cs["dec_c"][:n])


def test_a_decode_rows_samples_do_not_change_when_rows_are_appended_behind_it():
    """the (decode row, sample) keying on the restatement: the plain decoder's first rows alone and with the others behind them"""
    c = R.load("mnsrf")
    keep = c["Bd"] - 2
    a = R.decode("mnsrf", 5, 1.0, 0, cs=_first_rows(c["cs"], keep))
    b = R.decode("mnsrf", 5, 1.0, 0)
    assert a["predictions"].shape[0] == keep
    assert torch.equal(b["predictions"][:keep], a["predictions"]) and torch.equal(b["lengths"][:keep], a["lengths"])
    assert float((b["scores"][:keep] - a["scores"]).abs().max()) <= 1e-12       # (the host's GEMM blocks a larger batch differently: last bits)
    bad = R.decode("mnsrf", 5, 1.0, 0, fault="row_shared_noise")
    assert not torch.equal(bad["predictions"], b["predictions"])


@pytest.mark.parametrize("key", ["cars_full", "hq_h96"])
def test_two_samples_are_the_first_two_of_four(key):
    for tau, top_k in ((1.0, 0), (0.7, 3)):
        four, two = R.decode(key, 3, tau, top_k, n=4), R.decode(key, 3, tau, top_k, n=2)
        for k in ("predictions", "token_logprobs", "scores", "lengths"):
            assert torch.equal(four[k][:, :2], two[k]), k


# ---- the generator-level cases of the split-state entry ----------------------------------------------------------------------------------------------
def test_the_split_state_cases_hit_every_edge():
    rows, Ks, VTs, taus, nsrcs, steps = (set(c[i] for c in R.SPLIT_GEN_CASES) for i in range(6))
    assert rows == {1, 17, 33, 65} and Ks == {32, 96, 512, 544, 1024} and VTs == {5, 37, 4099} and taus == {0.25, 1.0, 4.0}
    assert {1, 3} <= nsrcs and any(c[4] == c[0] > 3 for c in R.SPLIT_GEN_CASES) and {0, 1, 1 << 20} <= steps
    assert any(c[2] in (5, 37) and c[1] <= 96 for c in R.SPLIT_GEN_CASES)         # one vocabulary range: the grid's `nvr % 8 != 0` branch
    assert len(R.SPLIT_GEN_CASES) == len(R.SPLIT_GEN_SEEDS) <= 14


@pytest.mark.parametrize("ci", range(len(R.SPLIT_GEN_CASES)))
def test_the_split_state_cases_stay_within_the_near_tie_budget(ci):
    rows, K, VT, tau, nsrc, step = R.SPLIT_GEN_CASES[ci]
    d = R.split_gen_reference(ci)
    x = R.split_gen_problem(ci)[0]
    assert float(x.abs().max()) < 1 and float(((x - x.half().float()) != 0).float().mean()) > 0.5     # the low term plane carries data
    f32 = SR.choose(d["l32"], R.SPLIT_GEN_SEEDS[ci], step, nsrc, 1.0 / tau, dtype=torch.float32)
    ok, near = SR.accept_tokens(f32["token"], d["ref"], d["e_p"])
    print("split case %d: e_y %.3g e_p %.3g near-tie rows %d of %d, min gap %.3g" % (ci, d["e_y"], d["e_p"], near, rows, float(d["ref"]["gap"].min())))
    assert ok and near <= rows // 100
    assert R.split_gen_seed(ci) == R.SPLIT_GEN_SEEDS[ci]
