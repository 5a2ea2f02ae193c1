"""Host-side (no GPU) checks of the Seq2seq mirror: the fp64 / fp32 restatement (tests/seq2seq_ref.py) against the reference's recorded
decode and loss (tests/golden/seq2seq.npz, written by generate_seq2seq.py), the state-dict layout of the three attention types, the config
table and its nlayers = 2 failure, the construction errors, registration of the new symbols, the loud failure without a device, and the teeth
of the acceptance criterion."""
import json
import os
import re

import numpy as np
import pytest
import torch

import gemm_ref
import seq2seq_ref as R
from conftest import ROOT, T, load_golden
from context_attentive_ir_amd.config import MODEL_ARCHITECTURE, default_args

G = load_golden("seq2seq")
SRC, LENS = T(G["source_words"]), T(G["source_lens"])
QL, MAXLEN = SRC.shape[1], int(G["max_len"])


@pytest.fixture(scope="module")
def chains():
    """per case: (network, cfg, golden arrays, fp64 decode, fp32 decode) -- computed once"""
    out = {}
    for tag in R.CASES:
        net, c, g = R.case(tag)
        sd, lut = net.state_dict(), T(g["tgt2src"])
        out[tag] = (net, c, g, R.decode(sd, c, SRC, LENS, MAXLEN, lut), R.decode(sd, c, SRC, LENS, MAXLEN, lut, torch.float32))
    return out


def test_fixture_shape_is_the_one_the_hazards_need():
    lens = LENS.tolist()
    assert len(set(lens)) == len(lens) and lens != sorted(lens, reverse=True)          # pairwise distinct, unsorted: the sorted-order pairing shows
    assert not np.array_equal(G["tgt2src"], np.arange(len(G["tgt2src"])))               # a permuted src_dict
    for tag in R.CASES:
        assert float(G["gaps_" + tag].min()) >= float(G["min_gap"]) == 1e-3              # no step is left out of the token comparison
        assert len(set(G["predictions_" + tag].reshape(-1).tolist())) >= 4


@pytest.mark.parametrize("tag", R.CASES)
def test_restatement_equals_the_reference_decode_and_loss(chains, tag):
    net, c, g, ref, chain = chains[tag]
    want = R.pad_attn(g["attentions"], QL)
    for d in (ref, chain):
        assert torch.equal(d["predictions"], T(g["predictions"]))
        assert float((d["attentions"].double() - want.double()).abs().max()) <= 8 * 2.0 ** -23          # the recorded values are an fp32 chain
        masked = (torch.arange(QL).view(1, 1, QL) >= LENS.view(-1, 1, 1)).expand_as(d["attentions"])
        assert bool((d["attentions"][masked] == 0).all())
    assert float((ref["gaps"] - T(g["gaps"]).double()).abs().max()) <= 1e-5
    sd = {k: v.double() for k, v in net.state_dict().items()}
    got = R.loss(sd, c, SRC, LENS, T(G["target_words"]), T(G["target_seq"]))
    assert abs(float(got) - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))


@pytest.mark.parametrize("tag", ["general", "dot", "mlp"])
def test_state_dict_keys_and_shapes_are_the_references(tag):
    net = R.case(tag)[0]
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in G["sd_keys_" + tag]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(G["sd_shapes_" + tag]))
    assert net.generator.bias is not None
    att = net.decoder.decoder.attn
    assert hasattr(att, "linear_in") == (tag == "general") and hasattr(att, "linear_context") == (tag == "mlp")
    assert (att.linear_out.bias is not None) == (tag == "mlp")


def test_config_table_is_the_references_and_its_nlayers_fails_like_the_reference():
    from context_attentive_ir_amd.recommender import Seq2seq
    assert MODEL_ARCHITECTURE["SEQ2SEQ"]["arch"] == json.loads(str(G["arch"]))
    assert MODEL_ARCHITECTURE["SEQ2SEQ"]["data"] == json.loads(str(G["data"]))
    a = default_args("SEQ2SEQ", src_vocab_size=200, tgt_vocab_size=200, nhid=64)
    assert a.nlayers == 2
    net = Seq2seq(a).eval()                                       # constructs, like the reference (decoder.decoder.rnn.*_l1 included)
    assert "decoder.decoder.rnn.weight_ih_l1" in net.state_dict()
    want = str(G["nlayers2_error"])
    B = SRC.shape[0]
    # raised before any tensor is looked at (CPU tensors would otherwise hit the no-fallback error first)
    with pytest.raises(RuntimeError) as e1:
        net(SRC, LENS, T(G["target_words"]), T(G["target_lens"]), T(G["target_seq"]), None, None)
    with pytest.raises(RuntimeError) as e2:
        net.decode(SRC, LENS, MAXLEN, None, None)
    for e in (e1, e2):
        assert str(e.value) == "Expected hidden[0] size (2, %d, 64), got [1, %d, 64]" % (B, B)
        assert want.startswith(str(e.value))


def test_unsupported_configurations_say_which_follow_up_covers_them():
    from context_attentive_ir_amd.recommender import Seq2seq
    from context_attentive_ir_amd.wrappers import Recommender
    kw = dict(src_vocab_size=50, tgt_vocab_size=50, nhid=32, nlayers=1)
    with pytest.raises(NotImplementedError, match="GRU"):
        Seq2seq(default_args("SEQ2SEQ", rnn_type="GRU", **kw))
    with pytest.raises(NotImplementedError, match="ACG"):
        Seq2seq(default_args("SEQ2SEQ", copy_attn=True, **kw))
    for kind in ("HREDQS", "ACG"):
        a = default_args("SEQ2SEQ", **kw)
        a.model_type = kind
        with pytest.raises(NotImplementedError, match="follow-up"):
            Recommender(a)
    a = default_args("SEQ2SEQ", **kw)
    a.model_type = "nonsense"
    with pytest.raises(RuntimeError, match="Unsupported model"):
        Recommender(a)
    # coverage_attn is never passed by Seq2seq (recommender/layers.py:71-79): ignored, as in the reference
    Seq2seq(default_args("SEQ2SEQ", coverage_attn=True, **kw))


def test_wrapper_construction_and_registration():
    import context_attentive_ir_amd.wrappers as W
    from context_attentive_ir_amd import lib
    assert "Recommender" in W.__all__
    src_dict, tgt_dict = list(range(120)), list(range(70))
    r = W.Recommender(default_args("SEQ2SEQ", nlayers=1, nhid=32), src_dict, tgt_dict)
    assert r.args.src_vocab_size == 120 and r.args.tgt_vocab_size == 70
    assert r.network.generator.weight.shape == (70, 32) and r.network.embedder.word_embeddings.table.shape[0] == 120
    # a reference checkpoint's `fixed_embedding` buffer is dropped on load (models/recommender.py:50-57)
    sd = dict(r.network.state_dict(), fixed_embedding=torch.zeros(3))
    W.Recommender(default_args("SEQ2SEQ", nlayers=1, nhid=32), src_dict, tgt_dict, sd)
    hdr = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    declared = set(re.findall(r"\b(nir_seq2seq_[a-z0-9_]+)\s*\(", hdr))
    assert {"nir_seq2seq_decode_greedy", "nir_seq2seq_decode_workspace_bytes", "nir_seq2seq_attend", "nir_seq2seq_gen_argmax",
            "nir_seq2seq_gen_argmax_workspace_bytes", "nir_seq2seq_pack_gen_frag", "nir_seq2seq_gen_frag_bytes"} == declared
    assert declared <= set(lib.SIGNATURES)
    L = lib.load()
    for name in declared:
        assert hasattr(L, name), name
    # reference lines cited next to the declarations
    assert "seq2seq.py:118-195" in hdr and "global_attention.py" in hdr


def test_no_cpu_fallback():
    net = R.case("general")[0]
    with pytest.raises(RuntimeError, match="ROCm device only"):
        net.decode(SRC, LENS, MAXLEN, None, None)
    with pytest.raises(RuntimeError, match="ROCm device only"):
        net(SRC, LENS, T(G["target_words"]), T(G["target_lens"]), T(G["target_seq"]))


@pytest.mark.parametrize("tag", R.CASES)
def test_the_criterion_accepts_the_fp32_chain(chains, tag):
    _, _, _, ref, chain = chains[tag]
    ok, fig = R.accept_decode(chain, ref, chain, 0)
    assert ok, fig


# a removed tanh leaves the six tokens of the nhid 64 / 96 general and dot cases unchanged (|linear_out| is small there: tanh is close to the
# identity and monotone), and attentions follow the tokens only: the decode criterion sees that fault where it changes a token -- at nhid 512
# ("wide", general) and for mlp
TEETH = [(t, f) for t in R.CASES for f in R.FAULTS if f != "tanh_swap" or t in ("mlp", "wide")]


@pytest.mark.parametrize("tag,fault", TEETH)
def test_the_criterion_has_teeth_at_the_margins_cap(chains, tag, fault):
    net, c, g, ref, chain = chains[tag]
    bad = R.decode(net.state_dict(), c, SRC, LENS, MAXLEN, T(g["tgt2src"]), fault=fault)
    ok, fig = R.accept_decode(bad, ref, chain, MAXLEN, margin=gemm_ref.MARGIN_CAP)
    assert not ok, (tag, fault, fig)
    # the attentions alone refuse it too: the bound is not carried by the token comparison
    assert fig["e"] > 100 * fig["bound"], (tag, fault, fig)
