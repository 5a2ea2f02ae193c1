"""Host-side (no GPU) checks of teacher-forced candidate scoring: the teeth of the acceptance criterion (score_ref's seven faults), the
restatement against the loss restatements at N = 1, nir_score_sequences' rule against brute force, the registration of the new symbols, their
argument checks over fake pointers, and the Python surface."""
import os
import re

import pytest
import torch

import gemm_ref
import gru_dec_ref as GR
import hredqs_ref as HQ
import score_ref as R
import seq2seq_ref as S
from conftest import T, load_golden

N_CAND = 4


def _case(kind):
    """(kind, state dict, cfg, src, lens, gold target_seq, gold target_words, tgt2src) of one fixture network per model"""
    if kind == "hredqs":
        net, c, a = HQ.case("h64")
        return kind, net.state_dict(), c, a["source_words"], a["source_lens"], a["target_seq"], a["target_words"], T(a["tgt2src"])
    net, c, a = S.case("general") if kind == "s2s" else GR.case("s2s", "general")
    g = load_golden("seq2seq")
    return kind, net.state_dict(), c, T(g["source_words"]), T(g["source_lens"]), T(g["target_seq"]), T(g["target_words"]), T(g["tgt2src"])


@pytest.fixture(scope="module")
def scored():
    """per model: (case, candidates, fp64 scores, fp32 chain, the fused form's n_split per token) -- once"""
    out = {}
    for kind in ("s2s", "gru", "hredqs"):
        cs = _case(kind)
        _, sd, cfg, src, lens, tseq, _, lut = cs
        cand = R.candidates(tseq, N_CAND)
        ref = R.score(kind, sd, cfg, src, lens, cand, tgt2src=lut)
        chain = R.score(kind, sd, cfg, src, lens, cand, tgt2src=lut, dtype=torch.float32)
        ns = R.n_path(kind, src.shape[-1], cand.shape[-1] - 1, src.shape[1] if kind == "hredqs" else 0) + 2
        out[kind] = (cs, cand, ref, chain, ns)
    return out


# ---- the criterion ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["s2s", "gru", "hredqs"])
def test_the_unfaulted_float32_chain_is_accepted(scored, kind):
    cs, cand, ref, chain, ns = scored[kind]
    ok, fig = R.accept(chain, ref, chain, 0)
    assert ok, fig
    assert ref["s"] > 1e-3 and int(ref["lengths"].min()) >= 1 and int(ref["lengths"].max()) == cand.shape[-1] - 1
    assert len({int(v) for v in ref["lengths"].reshape(-1)}) >= 3              # candidates of unequal lengths


@pytest.mark.parametrize("kind", ["s2s", "gru", "hredqs"])
@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_criterion_rejects_every_fault_at_the_margins_cap(scored, kind, fault):
    (_, sd, cfg, src, lens, _, _, lut), cand, ref, chain, ns = scored[kind]
    bad = R.score(kind, sd, cfg, src, lens, cand, tgt2src=lut, dtype=torch.float32, fault=fault)
    ok, fig = R.accept(bad, ref, chain, ns, margin=gemm_ref.MARGIN_CAP)
    assert not ok, (kind, fault, fig)


@pytest.mark.parametrize("fault", R.GEN_FAULTS)
def test_the_generator_level_criterion_rejects_its_faults(fault):
    g = torch.Generator().manual_seed(3)
    nseq, Tn, K, VT = 6, 5, 64, 250
    x, w = gemm_ref.family("randn", g, nseq * Tn, K, "a"), gemm_ref.family("randn", g, VT, K, "w")
    b = torch.randn(VT, generator=g)
    cand = R.candidates(torch.randint(4, VT, (nseq, Tn + 1), generator=g), 1, VT).view(nseq, Tn + 1)
    cand[1, 3:] = R.PAD
    cand[2, 2] = R.EOS
    ref = R.score_rows(x.view(nseq, Tn, K), w, b, cand)
    chain = R.score_rows(x.view(nseq, Tn, K), w, b, cand, dtype=torch.float32)
    assert R.accept(chain, ref, chain, 0)[0]
    bad = R.score_rows(x.view(nseq, Tn, K), w, b, cand, dtype=torch.float32, fault=fault)
    ok, fig = R.accept(bad, ref, chain, 2, margin=gemm_ref.MARGIN_CAP)
    assert not ok, (fault, fig)


def test_the_margin_may_not_pass_the_cap():
    assert R.MARGIN <= gemm_ref.MARGIN_CAP
    g = dict(token_logprobs=torch.zeros(1, 2), scores=torch.zeros(1), lengths=torch.zeros(1), s=1.0)
    with pytest.raises(AssertionError):
        R.accept(g, g, g, 0, margin=2 * gemm_ref.MARGIN_CAP)
    with pytest.raises(AssertionError):
        R.accept_rows(g["scores"], (g["scores"], None, torch.ones(1, 1)), (g["scores"],), 0, margin=2 * gemm_ref.MARGIN_CAP)


# ---- the restatement against the loss restatements ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["s2s", "gru", "hredqs"])
def test_one_gold_candidate_gives_the_loss_restatement(kind):
    _, sd, cfg, src, lens, tseq, twords, lut = _case(kind)
    sd64 = S._cast(sd, torch.float64)
    out = R.score(kind, sd, cfg, src, lens, tseq.unsqueeze(-2), rep=twords.unsqueeze(-2))
    if kind == "hredqs":
        want = HQ.loss(sd64, src, lens, twords, tseq)
    else:
        want = (S.loss if kind == "s2s" else GR.loss)(sd64, cfg, src, lens, twords, tseq)
    assert EOS_FREE(tseq)                                                       # the gold rows hold no EOS id: nothing is frozen
    assert abs(float(-out["scores"].mean()) - float(want)) <= 1e-12 * abs(float(want))
    assert torch.equal(out["lengths"].reshape(-1), (tseq.reshape(-1, tseq.shape[-1])[:, 1:] != R.PAD).sum(1))


def EOS_FREE(tseq):
    return not bool((tseq[..., 1:-1] == R.EOS).any())


def test_the_default_inputs_are_what_the_decodes_feed_back():
    lut = torch.tensor([5, 7, 99, 2, -1])
    cand = torch.tensor([[0, 1, 2, 3, 4, 9, -3]])
    assert R.default_rep(cand, lut, 50).tolist() == [[0, 7, R.UNK, 2, R.UNK, R.UNK, 5]]           # the first token is fed as it is
    assert R.default_rep(cand.clamp(0, 4), None, 3).tolist() == [[0, 1, 2, R.UNK, R.UNK, R.UNK, 0]]


# ---- nir_score_sequences' rule ------------------------------------------------------------------------------------------------------------------------
TABLE = [[5, 6, 3, 3, 3, 3],          # a beam row: EOS repeated behind the first EOS
         [3, 0, 0, 0, 0, 0],          # EOS at once
         [5, 0, 6, 7, 0, 0],          # a PAD in the middle does not end the sequence
         [5, 6, 7, 8, 9, 4],          # no EOS
         [0, 0, 0, 0, 0, 0],          # nothing counts
         [5, -1, 6, 3, 7, 3],         # a negative id is skipped
         [9, 9, 3, 5, 0, 3]]          # tokens and PAD behind the EOS


@pytest.mark.parametrize("pad,eos", [(0, 3), (9, 3), (0, -1), (0, 5)])
def test_sequences_rule_against_brute_force(pad, eos):
    tg = torch.tensor(TABLE)
    lp = -torch.arange(1, tg.numel() + 1, dtype=torch.float64).view_as(tg) / 7
    a, b = R.sequences(lp, tg, pad, eos), R.sequences_brute(lp, tg, pad, eos)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    if (pad, eos) == (0, 3):
        assert a[2].tolist() == [3, 1, 3, 6, 0, 3, 3]
        assert a[0][0].tolist() == lp[0, :3].tolist() + [0.0] * 3


# ---- symbols and arguments ----------------------------------------------------------------------------------------------------------------------------
NAMES = {"nir_score_gen_target_workspace_bytes", "nir_score_gen_target", "nir_score_sequences"}


def test_new_symbols_exist_with_their_prototypes():
    from conftest import ROOT
    from context_attentive_ir_amd import lib
    main = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    assert '#include "neuroir_score.h"' in main
    assert not re.findall(r"\bnir_score\w*\s*\(", main)                         # no prototypes of its own, comments included
    hdr = open(os.path.join(ROOT, "include", "neuroir_score.h")).read()
    declared = set(re.findall(r"\b(nir_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert NAMES == declared == set(lib.SCORE_SIGNATURES)
    others = (set(lib.SIGNATURES) | set(lib.GRU_DECODE_SIGNATURES) | set(lib.BEAM_SIGNATURES) | set(lib.SESSION_BEAM_SIGNATURES) | set(lib.ACG_BEAM_SIGNATURES)
              | set(lib.HREDQS_BEAM_SIGNATURES))
    assert not NAMES & others
    L = lib.load()
    for n in NAMES:
        assert hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, hdr, re.S)
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert nargs == len(lib.SCORE_SIGNATURES[n][1]), n
        assert getattr(L, n).argtypes == lib.SCORE_SIGNATURES[n][1]             # registered by lib.load


def test_gen_target_entry_refuses_bad_arguments_before_any_launch():
    """over fake pointers: nothing may be enqueued (no device needed)"""
    from context_attentive_ir_amd import lib
    C = lib.C
    L = lib.load()
    err = lambda: L.nir_last_error_string()                                    # noqa: E731
    p, big = C.c_void_p(16), 1 << 40
    size = L.nir_score_gen_target_workspace_bytes

    def gen(rows=5, K=64, VT=40, ws=big, x=p, w=p, frag=p, tg=p, out=p, wsp=p, lse=None):
        return L.nir_score_gen_target(x, rows, K, w, p, frag, VT, tg, 0, wsp, ws, out, lse, None, None)
    for kw in (dict(x=None), dict(w=None), dict(tg=None), dict(out=None)):
        assert gen(**kw) == -1 and b"null" in err(), kw
    assert gen(rows=-1) == -1 and b"rows" in err()
    assert gen(rows=1 << 31) == -1 and b"rows" in err()
    for K in (0, -4, 2, 30, 8196):                                              # K a multiple of 4 in [4, 8192], either form
        assert gen(K=K) == -1 and b"K outside" in err(), K
        assert size(5, K, 40, 0) == 0 and size(5, K, 40, 1) == 0
    for VT in (0, -1, (1 << 31) - 16):
        assert gen(VT=VT) == -1 and b"VT" in err(), VT
        assert size(5, 64, VT, 1) == 0
    for frag in (p, None):                                                      # both forms: a short or a null workspace
        assert gen(ws=16, frag=frag) == -3 and b"workspace" in err()
        assert gen(wsp=None, frag=frag) == -3 and b"workspace" in err()
        assert gen(rows=0, frag=frag) == 0 and gen(rows=0, frag=frag, wsp=None, ws=0) == 0
    assert size(0, 64, 40, 1) == 0
    # the fused form holds partials, the plain form logits: bounded by 256 MiB however many rows
    assert 0 < size(24320, 512, 30000, 1) < 64 << 20
    assert size(100, 512, 30000, 0) == 100 * 30000 * 4 + 256
    assert size(24320, 512, 30000, 0) <= (256 << 20) + 256 and size(1 << 30, 512, 30000, 0) == size(24320, 512, 30000, 0)
    assert size(5, 48, 40, 1) == size(5, 48, 40, 0) > 0                         # a K without a fragment form: the plain form's size
    assert size((1 << 18) + 5, 64, 40, 1) == size(1 << 18, 64, 40, 1)           # rows beyond a chunk reuse the chunk's partials
    assert size(1 << 30, 64, 40, 1) == size(1 << 18, 64, 40, 1)


def test_sequences_entry_refuses_bad_arguments_before_any_launch():
    from context_attentive_ir_amd import lib
    C = lib.C
    L = lib.load()
    err = lambda: L.nir_last_error_string()                                    # noqa: E731
    p = C.c_void_p(16)

    def seq(nseq=4, Tn=5, lp=p, tg=p, sc=p, ln=p):
        return L.nir_score_sequences(lp, tg, nseq, Tn, 0, 3, sc, ln, None)
    for kw in (dict(lp=None), dict(tg=None), dict(sc=None), dict(ln=None)):
        assert seq(**kw) == -1 and b"null" in err(), kw
    assert seq(nseq=-1) == -1 and b"bad dims" in err()
    assert seq(Tn=0) == -1 and seq(Tn=(1 << 20) + 1) == -1
    assert seq(nseq=0) == 0


# ---- the Python surface -------------------------------------------------------------------------------------------------------------------------------
def test_score_candidates_and_the_wrappers_on_the_cpu():
    import context_attentive_ir_amd.wrappers as Wr
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.recommender import HredQS, Seq2seq, Seq2seqGRU
    for cls in (Seq2seq, Seq2seqGRU, HredQS):
        assert callable(getattr(cls, "score_candidates"))
    for cls in (Wr.Recommender, Wr.SessionRecommender, Wr.CopyRecommender):
        assert callable(getattr(cls, "score"))
    _, _, _, src, lens, tseq, _, _ = _case("s2s")
    cand = R.candidates(tseq, 3)
    for net in (S.case("general")[0], GR.case("s2s", "general")[0]):
        with pytest.raises(RuntimeError, match="ROCm device only"):            # no CPU fallback
            net.score_candidates(src, lens, cand)
        with pytest.raises(ValueError, match="candidate_seq"):
            net.score_candidates(src, lens, cand[:, :, :1])
        with pytest.raises(ValueError, match="candidate_seq"):
            net.score_candidates(src, lens, cand[:2])
        net.train()
        with pytest.raises(NotImplementedError, match="eval mode"):
            net.score_candidates(src, lens, cand)
    _, _, _, hsrc, hlens, htseq, _, _ = _case("hredqs")
    hnet, hcand = HQ.case("h64")[0], R.candidates(htseq, 3)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        hnet.score_candidates(hsrc, hlens, hcand)
    with pytest.raises(ValueError, match="candidate_seq"):
        hnet.score_candidates(hsrc, hlens, hcand[:, 0])
    hnet.train()
    with pytest.raises(NotImplementedError, match="eval mode"):
        hnet.score_candidates(hsrc, hlens, hcand)
    kw = dict(src_vocab_size=50, tgt_vocab_size=50, nhid=32)
    with pytest.raises(IndexError, match="tuple index out of range"):          # the same refusals as decode()
        HredQS(default_args("HREDQS", bidirection=False, nlayers=2, nhid_session=32, **kw)).eval().score_candidates(hsrc, hlens, hcand)
    c = Wr.CopyRecommender(default_args("ACG", nlayers=1, **kw))
    with pytest.raises(NotImplementedError, match="extended distribution"):
        c.score({})
    with pytest.raises(NotImplementedError, match="extended distribution"):    # ACG does not inherit Seq2seq's scorer: another distribution
        c.network.eval().score_candidates(src % 50, lens, cand % 50)
    r = Wr.Recommender(default_args("SEQ2SEQ", nlayers=1, **kw))
    ex = dict(source_words=src.unsqueeze(1) % 50, source_lens=lens.unsqueeze(1), target_seq=tseq.unsqueeze(1) % 50, target_words=tseq.unsqueeze(1) % 50)
    with pytest.raises(RuntimeError, match="ROCm device only"):                # loud without a device, with and without candidates
        r.score(ex)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        r.score(ex, cand % 50)
