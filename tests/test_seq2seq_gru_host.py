"""Host-side (no GPU) checks of the GRU decoders: the fp64 restatement (tests/gru_dec_ref.py) against the reference's recorded decode and loss
with rnn_type = 'GRU' (tests/golden/seq2seq_gru.npz, written by generate_seq2seq_gru.py), the teeth of the acceptance criterion, the state-dict
layout, the wrappers' dispatch, the nlayers = 2 failure and the registration of the new symbols."""
import json
import os
import re

import pytest
import torch

import acg_ref as AR
import gemm_ref
import gru_dec_ref as R
from conftest import ROOT, T
from context_attentive_ir_amd.config import default_args

GS, GA = R.golden("s2s"), R.golden("acg")
SRC, LENS = T(GS["source_words"]), T(GS["source_lens"])
QL, MAXLEN = SRC.shape[1], int(GS["max_len"])


@pytest.fixture(scope="module")
def chains():
    """per Seq2seq case: (network, cfg, golden arrays, fp64 decode, fp32 decode) -- computed once"""
    out = {}
    for tag in R.S2S_CASES:
        net, c, g = R.case("s2s", tag)
        sd, lut = net.state_dict(), T(g["tgt2src"])
        out[tag] = (net, c, g, R.decode(sd, c, SRC, LENS, MAXLEN, lut), R.decode(sd, c, SRC, LENS, MAXLEN, lut, torch.float32))
    return out


@pytest.fixture(scope="module")
def acg_chains():
    out = {}
    d = R.acg_batch()
    e2t, e2s = AR.index_tensors(d)
    for tag in R.ACG_CASES:
        net, c, g = R.case("acg", tag)
        out[tag] = (net, c, g, d, R.acg_decode(net.state_dict(), c, d["src"], d["lens"], int(GA["max_len"]), d["idx"], e2t, e2s))
    return out


def test_fixture_keeps_every_step_in_the_token_comparison():
    for tag in R.S2S_CASES:
        assert float(GS["gaps_" + tag].min()) >= float(GS["min_gap"]) == 1e-3
        assert len(set(GS["predictions_" + tag].reshape(-1).tolist())) >= 4
        assert json.loads(str(GS["cfg_" + tag]))["seed"] >= 1
    for tag in R.ACG_CASES:
        assert float(GA["gaps_" + tag].min()) >= 1e-3 and min(GA["classes_" + tag][:3]) >= 1


@pytest.mark.parametrize("tag", R.S2S_CASES)
def test_restatement_equals_the_reference_decode_and_loss(chains, tag):
    net, c, g, ref, chain = chains[tag]
    want = R.pad_attn(g["attentions"], QL)
    assert torch.equal(ref["predictions"], T(g["predictions"])) and torch.equal(chain["predictions"], T(g["predictions"]))
    assert float((ref["attentions"] - want.double()).abs().max()) <= 1e-6
    sd = {k: v.double() for k, v in net.state_dict().items()}
    got = R.loss(sd, c, SRC, LENS, T(GS["target_words"]), T(GS["target_seq"]))
    assert abs(float(got) - float(g["loss"])) <= 1e-5


@pytest.mark.parametrize("tag", R.ACG_CASES)
def test_acg_restatement_equals_the_reference_decode_and_loss(acg_chains, tag):
    net, c, g, d, ref = acg_chains[tag]
    assert torch.equal(ref["predictions"], T(g["predictions"])) and torch.equal(ref["gen_top"], T(g["gen_top"]))
    assert float((ref["attentions"] - R.pad_attn(g["attentions"], d["src"].shape[1]).double()).abs().max()) <= 1e-6
    sd = {k: v.double() for k, v in net.state_dict().items()}
    got = R.acg_loss(sd, c, d["src"], d["lens"], d["tw"], d["ts"], d["idx"], d["al"])
    assert abs(float(got) - float(g["loss"])) <= 1e-5
    if tag == "general":
        got = R.acg_loss(sd, c, d["src"], d["lens"], d["tw"], d["ts"], d["idx"], d["al"], force_copy=True)
        assert abs(float(got) - float(GA["loss_force_copy"])) <= 1e-5


@pytest.mark.parametrize("tag", R.S2S_CASES)
def test_the_criterion_accepts_the_fp32_chain(chains, tag):
    _, _, _, ref, chain = chains[tag]
    ok, fig = R.accept_decode(chain, ref, chain, 0)
    assert ok, fig


@pytest.mark.parametrize("tag", R.S2S_CASES)
@pytest.mark.parametrize("fault", R.FAULTS)
def test_the_criterion_has_teeth_at_the_margins_cap(chains, tag, fault):
    net, c, g, ref, chain = chains[tag]
    bad = R.decode(net.state_dict(), c, SRC, LENS, MAXLEN, T(g["tgt2src"]), fault=fault)
    ok, fig = R.accept_decode(bad, ref, chain, MAXLEN, margin=gemm_ref.MARGIN_CAP)
    assert not ok, (tag, fault, fig)
    assert fig["e"] > 100 * fig["bound"], (tag, fault, fig)                  # the attentions alone refuse it


@pytest.mark.parametrize("fault", ["bhn_outside", "gate_order", "blend_swap"])          # (the other two are faults of the loop, not of a step)
def test_one_step_criterion_has_teeth(fault):
    """the bound of tests/test_gpu_gru_step_envelope.py at its cap rejects every fault of the cell on that test's own input family"""
    x = R.step_inputs(64, 17, 20)
    ref, chain = R.step(*x), R.step(*x, dtype=torch.float32)
    bad = R.step(*x, fault=fault)
    ok, fig = R.accept(bad, ref, chain, 1, margin=gemm_ref.MARGIN_CAP)
    assert not ok and fig["e"] > 100 * fig["bound"], fig


@pytest.mark.parametrize("kind,tag", [("s2s", t) for t in ("general", "dot", "mlp")] + [("acg", t) for t in R.ACG_CASES])
def test_state_dict_keys_and_shapes_are_the_references(kind, tag):
    net = R.case(kind, tag)[0]
    g = R.golden(kind)
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in g["sd_keys_" + tag]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(g["sd_shapes_" + tag]))
    H = net.nhid
    assert tuple(sd["decoder.decoder.rnn.weight_hh_l0"].shape) == (3 * H, H)
    assert isinstance(net.decoder.decoder.rnn, torch.nn.GRU) and isinstance(net.encoder.encoder.rnns[0], torch.nn.GRU)


def test_wrappers_dispatch_on_rnn_type_and_the_old_constructors_still_refuse():
    import context_attentive_ir_amd.wrappers as W
    from context_attentive_ir_amd.recommender import ACG, ACGGRU, HredQS, Seq2seq, Seq2seqGRU
    kw = dict(src_vocab_size=50, tgt_vocab_size=50, nhid=32, nlayers=1)
    r = W.Recommender(default_args("SEQ2SEQ", rnn_type="GRU", **kw))
    assert type(r.network) is Seq2seqGRU
    assert type(W.Recommender(default_args("SEQ2SEQ", **kw)).network) is Seq2seq
    c = W.CopyRecommender(default_args("ACG", rnn_type="GRU", copy_attn=True, **kw), list(range(50)), list(range(50)))
    assert type(c.network) is ACGGRU and isinstance(c.network, ACG)
    assert type(W.CopyRecommender(default_args("ACG", copy_attn=True, **kw), list(range(50)), list(range(50))).network) is ACG
    for cls, name in ((Seq2seq, "SEQ2SEQ"), (ACG, "ACG")):
        with pytest.raises(NotImplementedError, match="GRU") as e:
            cls(default_args(name, rnn_type="GRU", copy_attn=cls is ACG, **kw))
        assert "Seq2seqGRU" in str(e.value) and "ACGGRU" in str(e.value)
    with pytest.raises(NotImplementedError, match="LSTM"):
        Seq2seqGRU(default_args("SEQ2SEQ", **kw))
    with pytest.raises(NotImplementedError):
        HredQS(default_args("HREDQS", rnn_type="GRU", bidirection=False, **kw))
    # a checkpoint written by the GRU wrapper loads back into the GRU class
    sd = dict(r.network.state_dict(), fixed_embedding=torch.zeros(3))
    r2 = W.Recommender(default_args("SEQ2SEQ", rnn_type="GRU", **kw), None, None, sd)
    assert torch.equal(r2.network.decoder.decoder.rnn.weight_hh_l0, r.network.decoder.decoder.rnn.weight_hh_l0)


@pytest.mark.parametrize("kind", ["s2s", "acg"])
def test_nlayers_2_fails_with_the_gru_text_before_any_launch(kind):
    from context_attentive_ir_amd.recommender import ACGGRU, Seq2seqGRU
    want = str(GS["nlayers2_error"])
    B = SRC.shape[0]
    if kind == "s2s":
        net = Seq2seqGRU(default_args("SEQ2SEQ", src_vocab_size=200, tgt_vocab_size=200, nhid=64, rnn_type="GRU")).eval()
    else:
        net = ACGGRU(default_args("ACG", src_vocab_size=200, tgt_vocab_size=200, nhid=64, rnn_type="GRU", copy_attn=True, nlayers=2)).eval()
    assert net.nlayers == 2 and "decoder.decoder.rnn.weight_ih_l1" in net.state_dict()
    # CPU tensors: anything but the layer check would hit the no-fallback error first
    with pytest.raises(RuntimeError) as e1:
        net(SRC, LENS, T(GS["target_words"]), T(GS["target_lens"]), T(GS["target_seq"]), SRC, T(GS["target_seq"]))
    with pytest.raises(RuntimeError) as e2:
        net.decode(SRC, LENS, MAXLEN, None, None, src_map_idx=SRC, ext2tgt=SRC, ext2src=SRC) if kind == "acg" else net.decode(SRC, LENS, MAXLEN, None, None)
    for e in (e1, e2):
        assert str(e.value) == "Expected hidden size (2, %d, 64), got [1, %d, 64]" % (B, B)
        assert want.startswith(str(e.value))


def test_no_cpu_fallback():
    net = R.case("s2s", "general")[0]
    with pytest.raises(RuntimeError, match="ROCm device only"):
        net.decode(SRC, LENS, MAXLEN, None, None)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        net(SRC, LENS, T(GS["target_words"]), T(GS["target_lens"]), T(GS["target_seq"]))


def test_new_symbols_exist_with_their_prototypes():
    from context_attentive_ir_amd import lib
    names = {"nir_gru_step_whh_frag_bytes", "nir_gru_step_pack_whh_frag", "nir_gru_step_workspace_bytes", "nir_gru_step",
             "nir_seq2seq_gru_decode_workspace_bytes", "nir_seq2seq_gru_decode_greedy", "nir_acg_gru_decode_workspace_bytes",
             "nir_acg_gru_decode_greedy"}
    assert '#include "neuroir_gru_decode.h"' in open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    hdr = open(os.path.join(ROOT, "include", "neuroir_gru_decode.h")).read()
    declared = set(re.findall(r"\b(nir_(?:gru_step|seq2seq_gru|acg_gru)[a-z0-9_]*)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert names == declared == set(lib.GRU_DECODE_SIGNATURES) and not names & set(lib.SIGNATURES)
    L = lib.load()
    for n in names:
        assert hasattr(L, n), n
    # the ctypes prototypes have the arity of the declarations
    for n in names:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, hdr, re.S)
        nargs = len([a for a in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if a.strip()])
        assert nargs == len(lib.GRU_DECODE_SIGNATURES[n][1]), n
    assert "decoder.py:175-177" in hdr and "rnn_decoder.py:46-47" in hdr          # the reference lines the entries replace
    assert L.nir_gru_step_whh_frag_bytes(64) == 3 * 64 * 64 * 4 and L.nir_gru_step_whh_frag_bytes(48) == 0
    assert L.nir_gru_step_workspace_bytes(5, 64) > 0 and L.nir_gru_step_workspace_bytes(5, 6) == 0
    # bad arguments are refused before anything is enqueued (no device needed)
    err = lambda: L.nir_last_error_string()                                # noqa: E731
    p = lib.C.c_void_p(16)
    assert L.nir_gru_step(None, 2, p, 50, 4, p, p, None, p, p, None, 8, p, None, p, None, p, 1 << 20, None) == -1 and b"null" in err()
    assert L.nir_gru_step(p, 2, p, 50, 4, p, p, None, p, p, None, 6, p, None, p, None, p, 1 << 20, None) == -1 and b"bad dims" in err()
    assert L.nir_gru_step(p, 2, None, 50, 4, p, p, None, p, p, None, 8, p, None, p, None, p, 1 << 20, None) == -1 and b"gate_fold" in err()
    assert L.nir_gru_step(p, 2, p, 50, 4, p, p, None, p, p, None, 8, p, None, p, None, p, 16, None) != 0 and b"workspace" in err()
    assert L.nir_gru_step(p, 0, p, 50, 4, p, p, None, p, p, None, 8, p, None, p, None, p, 1 << 20, None) == 0
    assert L.nir_gru_step_pack_whh_frag(p, 48, p, None, None) == -1
