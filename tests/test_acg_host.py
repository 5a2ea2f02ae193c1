"""Host-side (no GPU) checks of the ACG mirror: the fp64 restatement (tests/acg_ref.py) against the reference's recorded decode and losses
(tests/golden/acg.npz, written by generate_acg.py), the teeth of the fixture against six planted faults, the state-dict layout, the config
table, the pinned construction errors, the conversion of the reference's copy arguments to index tensors, and registration of the new
symbols."""
import json
import os
import re

import numpy as np
import pytest
import torch

import acg_ref as R
from conftest import ROOT, T
from context_attentive_ir_amd.config import MODEL_ARCHITECTURE, default_args

G = R.golden()
D = R.batch_inputs()
SRC, LENS = D["src"], D["lens"]
QL, MAXLEN, VT = SRC.shape[1], int(G["max_len"]), int(G["tgt_vocab"])
E2T, E2S = R.index_tensors(D)
GAP_TOL = 1e-5            # recorded gaps are an fp32 chain's ((top1 - top2) / top1 of entries of O(0.1): a few 1e-7); Seq2seq's figure for its gaps


def ref_decode(tag, fault=None):
    net, c, g = R.case(tag)
    return R.decode(net.state_dict(), c, SRC, LENS, MAXLEN, D["idx"], E2T, E2S, fault=fault), g


@pytest.fixture(scope="module")
def decodes():
    return {tag: ref_decode(tag) for tag in R.CASES}


def test_fixture_shape_is_the_one_the_hazards_need():
    lens = LENS.tolist()
    assert len(set(lens)) == len(lens) and lens != sorted(lens, reverse=True)
    assert int(G["vocab"]) == 260 and VT == 200 and SRC.shape == (5, 7) and MAXLEN == 6
    assert any(len(set(r[:n])) < n and max(r[:n]) >= VT for r, n in zip(SRC.tolist(), lens))      # a repeated out-of-vocabulary word
    for tag in R.CASES:
        assert float(G["gaps_" + tag].min()) >= float(G["min_gap"]) == 1e-3                          # no step is left out of the token comparison
        cop, col, gen, _ = G["classes_" + tag].tolist()
        assert cop >= 1 and col >= 1 and gen >= 1
        p, top = G["predictions_" + tag], G["gen_top_" + tag]
        assert (p >= VT).sum() == cop and ((p < VT) & (p != top)).sum() == col and (p == top).sum() == gen


@pytest.mark.parametrize("tag", R.CASES)
def test_restatement_equals_the_reference_decode_and_loss(decodes, tag):
    ref, g = decodes[tag]
    assert torch.equal(ref["predictions"], T(g["predictions"]))
    assert torch.equal(ref["gen_top"], T(g["gen_top"]))
    assert float((ref["attentions"] - R.pad_attn(g["attentions"], QL).double()).abs().max()) <= 8 * 2.0 ** -23
    assert float((ref["gaps"] - T(g["gaps"]).double()).abs().max()) <= GAP_TOL
    net, c, _ = R.case(tag)
    sd = {k: v.double() for k, v in net.state_dict().items()}
    got = R.loss(sd, c, SRC, LENS, D["tw"], D["ts"], D["idx"], D["al"])
    assert abs(float(got) - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))
    if tag == "general":
        got = R.loss(sd, c, SRC, LENS, D["tw"], D["ts"], D["idx"], D["al"], force_copy=True)
        assert abs(float(got) - float(G["loss_force_copy"])) <= 1e-6 * abs(float(G["loss_force_copy"]))
        assert abs(float(G["loss_force_copy"]) - float(g["loss"])) > 1e-4 * abs(float(g["loss"]))


@pytest.mark.parametrize("fault", R.FAULTS)
def test_fixture_rejects_planted_faults(fault):
    """every fault fails the acceptance of the test above on the general case -- a token moves, or a gap moves beyond GAP_TOL (the PAD
    override only shifts the normaliser: every gap moves by ~6e-5) --; the ones the loss goes through move the loss as well"""
    bad, g = ref_decode("general", fault)
    same_tokens = torch.equal(bad["predictions"], T(g["predictions"]))
    gap_err = float((bad["gaps"] - T(g["gaps"]).double()).abs().max())
    print(fault, "tokens equal:", same_tokens, "largest gap difference: %.3g" % gap_err)
    assert (not same_tokens) or gap_err > GAP_TOL, (fault, same_tokens, gap_err)          # = the acceptance of the test above fails
    if fault in ("no_pad", "no_repeat", "swap_switch"):
        net, c, _ = R.case("general")
        sd = {k: v.double() for k, v in net.state_dict().items()}
        got = R.loss(sd, c, SRC, LENS, D["tw"], D["ts"], D["idx"], D["al"], fault=fault)
        assert abs(float(got) - float(g["loss"])) > 1e-4 * abs(float(g["loss"])), fault


@pytest.mark.parametrize("tag", ["general", "mlp", "own"])
def test_state_dict_keys_round_trip(tag):
    net = R.case(tag)[0]
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in G["sd_keys_" + tag]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(G["sd_shapes_" + tag]))
    assert sd["copy_generator.linear.weight"].data_ptr() == sd["generator.weight"].data_ptr()        # one parameter under two keys
    assert ("decoder.decoder.copy_attn.linear_out.weight" in sd) == (tag == "own")
    from context_attentive_ir_amd.recommender import ACG
    again = ACG(R.case_args(tag))
    again.load_state_dict(sd, strict=True)
    assert all(torch.equal(v, again.state_dict()[k]) for k, v in sd.items())
    assert len(list(net.parameters())) == len(sd) - 2


def test_config_table_is_the_references():
    assert MODEL_ARCHITECTURE["ACG"]["arch"] == json.loads(str(G["arch"]))
    assert MODEL_ARCHITECTURE["ACG"]["data"] == json.loads(str(G["data"]))
    a = default_args("ACG", src_vocab_size=50)
    assert a.nlayers == 1 and a.copy_attn and a.reuse_copy_attn and not a.force_copy and a.tgt_vocab_size == 10000


def test_construction_errors():
    from context_attentive_ir_amd.recommender import ACG, Seq2seq
    from context_attentive_ir_amd.wrappers import CopyRecommender, Recommender
    kw = dict(src_vocab_size=50, tgt_vocab_size=50, nhid=32, nlayers=1)
    # the messages tests/test_seq2seq_host.py pins still match, and now name where ACG lives
    with pytest.raises(NotImplementedError, match="ACG") as e:
        Seq2seq(default_args("SEQ2SEQ", copy_attn=True, **kw))
    assert "recommender.ACG" in str(e.value) and "wrappers.CopyRecommender" in str(e.value)
    a = default_args("ACG", **kw)
    with pytest.raises(NotImplementedError, match="follow-up") as e:
        Recommender(a)
    assert "wrappers.CopyRecommender" in str(e.value)
    with pytest.raises(RuntimeError, match="Unsupported model"):
        CopyRecommender(default_args("SEQ2SEQ", **kw))
    with pytest.raises(NotImplementedError, match="GRU"):
        ACG(default_args("ACG", rnn_type="GRU", **kw))
    with pytest.raises(RuntimeError, match="Attn is turned off, so reuse_copy_attn flag must be false"):
        ACG(default_args("ACG", attn_type="none", **kw))
    with pytest.raises(AssertionError, match="valid attention type"):
        ACG(default_args("ACG", attn_type="none", reuse_copy_attn=False, **kw))
    with pytest.raises(ValueError, match="copy_attn"):
        ACG(default_args("SEQ2SEQ", **kw))
    net = ACG(default_args("ACG", src_vocab_size=50, tgt_vocab_size=50, nhid=32, nlayers=2)).eval()
    with pytest.raises(RuntimeError, match=re.escape("Expected hidden[0] size (2, 3, 32), got [1, 3, 32]")):
        net.decode(torch.ones(3, 4, dtype=torch.long), torch.full((3,), 4), 2, None, None, src_map_idx=torch.zeros(3, 4, dtype=torch.long),
                   ext2tgt=torch.full((3, 6), -1), ext2src=torch.ones(3, 6, dtype=torch.long))


def test_copy_arguments_become_the_index_tensors():
    from context_attentive_ir_amd.recommender import acg as M
    net = R.case("general")[0]
    dense = R.make_src_map(D["maps"])
    blank, fill = R.collapse_copy_scores(D["tgt_dict"], D["vocabs"])
    # the reference's own blank / fill, as recorded
    assert [[x for x in r if x >= 0] for r in G["blank"].tolist()] == blank and [[x for x in r if x >= 0] for r in G["fill"].tolist()] == fill
    want_idx = D["idx"]
    for form in (D["maps"], dense, want_idx):
        idx, e2t, e2s = net.copy_index(QL, form, blank, fill, D["vocabs"], D["src_dict"], D["tgt_dict"])
        assert torch.equal(idx, want_idx) and torch.equal(e2t, E2T) and torch.equal(e2s, E2S)
    idx, e2t, e2s = net.copy_index(QL, D["maps"], None, None, D["vocabs"], D["src_dict"], D["tgt_dict"])          # collapse from the dictionaries
    assert torch.equal(e2t, E2T) and torch.equal(e2s, E2S)
    # the dense one-hot of the index tensor is make_src_map's, position by position
    for b in range(SRC.shape[0]):
        for j in range(int(LENS[b])):
            assert int(dense[b, j].argmax()) == int(want_idx[b, j]) and float(dense[b, j].sum()) == 1.0
    assert bool((E2T[:, :2] == -1).all())                                                                       # PAD and UNK of a row's dictionary never collapse
    ids = T(G["src_vocab_ids"])
    assert torch.equal(torch.where(ids >= 0, ids, torch.ones_like(ids)), E2S)                                   # the reference's src_dict[src_vocab[c]]
    # padding: a wider CV adds slots nothing maps to
    e2t9, e2s9 = M.vocab_index(D["vocabs"], D["src_dict"], D["tgt_dict"], CV=E2T.shape[1] + 3)
    assert torch.equal(e2t9[:, :E2T.shape[1]], E2T) and bool((e2t9[:, E2T.shape[1]:] == -1).all()) and bool((e2s9[:, E2T.shape[1]:] == 1).all())
    with pytest.raises(ValueError):
        M.vocab_index(D["vocabs"], D["src_dict"], D["tgt_dict"], CV=3)
    with pytest.raises(NotImplementedError):
        net.copy_index(QL, D["maps"], blank, fill, None, D["src_dict"], D["tgt_dict"])


def test_new_symbols_are_declared_everywhere():
    from context_attentive_ir_amd import lib
    import context_attentive_ir_amd.wrappers as W
    import context_attentive_ir_amd.recommender as Rm
    hdr = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    for name in ("nir_acg_gen_select_workspace_bytes", "nir_acg_gen_select", "nir_acg_decode_workspace_bytes", "nir_acg_decode_greedy",
                 "nir_acg_copy_loss_fwd", "nir_acg_copy_loss_bwd"):
        assert name in lib.SIGNATURES and re.search(r"\b%s\(" % name, hdr)
    assert "CopyRecommender" in W.__all__ and "ACG" in Rm.__all__
    src = open(os.path.join(ROOT, "context_attentive_ir_amd", "csrc", "acg.hip")).read()
    assert "atomicAdd" not in src                                   # no float atomics: the copy mass is a gather per slot


def test_no_device_is_an_error_not_a_fallback():
    net = R.case("general")[0]
    with pytest.raises(RuntimeError):
        net.decode(SRC, LENS, MAXLEN, None, None, src_map_idx=D["idx"], ext2tgt=E2T, ext2src=E2S)
    with pytest.raises(RuntimeError):
        net(SRC, LENS, D["tw"], D["tlen"], D["ts"], D["idx"], D["al"])
