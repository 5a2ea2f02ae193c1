"""Host-side (no GPU) checks of the HredQS mirror: the fp64 / fp32 restatement (tests/hredqs_ref.py) against the reference's recorded decode,
encode states and loss (tests/golden/hredqs.npz, written by generate_hredqs.py), the state-dict layout, the config table, the configurations
that fail like the reference's, the wrapper's construction, registration of the new symbols, the loud failure without a device, and the teeth
of the acceptance criterion."""
import json
import os
import re

import numpy as np
import pytest
import torch

import gemm_ref
import hredqs_ref as R
from conftest import ROOT, T, load_golden
from context_attentive_ir_amd.config import MODEL_ARCHITECTURE, default_args

G = load_golden("hredqs")
MAXLEN = int(G["max_len"])
KW = dict(src_vocab_size=50, tgt_vocab_size=50, nhid=32, nhid_session=32)


@pytest.fixture(scope="module")
def chains():
    """per case: (network, cfg, golden arrays, fp64 decode, fp32 decode) -- computed once"""
    out = {}
    for tag in R.CASES:
        net, c, g = R.case(tag)
        sd, lut = net.state_dict(), T(g["tgt2src"])
        out[tag] = (net, c, g, R.decode(sd, g["source_words"], g["source_lens"], MAXLEN, lut),
                    R.decode(sd, g["source_words"], g["source_lens"], MAXLEN, lut, torch.float32))
    return out


def test_fixture_shape_is_the_one_the_hazards_need():
    assert [str(t) for t in G["cases"]] == list(R.CASES)
    assert not np.array_equal(G["tgt2src"], np.arange(len(G["tgt2src"])))               # a permuted src_dict
    for tag in R.CASES:
        _, c, g = R.case(tag)
        lens, QL = g["source_lens"], g["source_words"].shape[2]
        assert tuple(lens.shape) == (c["B"], c["S"]) and int(lens.min()) >= 1
        assert bool((lens == QL).any()) and bool((lens < QL).any())                     # the padded positions take part in the max
        assert float(g["gaps"].min()) >= float(G["min_gap"]) == 1e-3                    # no step is left out of the token comparison
        rows = g["predictions"].reshape(-1, MAXLEN)
        assert len(set(map(tuple, rows.tolist()))) >= 4 and len(set(rows.reshape(-1).tolist())) >= 4
    assert R.case_cfg("h1024")["nhid_session"] == 1024 and R.case_cfg("h64")["B"] == 3 and R.case_cfg("h64")["S"] == 4


@pytest.mark.parametrize("tag", R.CASES)
def test_restatement_equals_the_reference_decode_states_and_loss(chains, tag):
    net, c, g, ref, chain = chains[tag]
    for d in (ref, chain):
        assert torch.equal(d["predictions"], T(g["predictions"]))
    for k in ("enc_h", "enc_c"):
        assert tuple(ref[k].shape) == tuple(g[k].shape) == (1, c["S"] * c["B"], c["nhid_session"])
        # against the reference's own classes cast to float64, and against the reference as it runs (an fp32 chain)
        assert T(g[k + "64"]).dtype == torch.float64
        assert float((ref[k] - T(g[k + "64"])).abs().max()) <= 1e-9
        assert float((chain[k].double() - T(g[k]).double()).abs().max()) <= 1e-5
    assert float((ref["gaps"] - T(g["gaps"]).double()).abs().max()) <= 1e-5
    sd = {k: v.double() for k, v in net.state_dict().items()}
    got = R.loss(sd, g["source_words"], g["source_lens"], g["target_words"], g["target_seq"])
    assert abs(float(got) - float(g["loss"])) <= 1e-6 * abs(float(g["loss"]))


def test_the_pairing_moves_ten_of_twelve_rows():
    """B = 3, S = 4: decode row r = b S + s takes the state at step-major index r, i.e. of step r // B of session r % B"""
    B, S = 3, 4
    hs = torch.arange(B * S, dtype=torch.float64).view(B, S, 1)                          # the state of (b, s) is called b S + s
    h, _ = R.paired(hs, hs)
    want = [(r % B) * S + r // B for r in range(B * S)]
    assert h.view(-1).tolist() == want
    assert sum(1 for r, w in enumerate(want) if r != w) == 10
    for b, s in ((1, 4), (3, 1)):
        one = torch.arange(b * s, dtype=torch.float64).view(b, s, 1)
        assert R.paired(one, one)[0].view(-1).tolist() == list(range(b * s))             # B = 1 or S = 1: the natural pairing


@pytest.mark.parametrize("tag", R.CASES)
def test_state_dict_keys_and_shapes_are_the_references(tag):
    net = R.case(tag)[0]
    sd = net.state_dict()
    assert list(sd.keys()) == [str(k) for k in G["sd_keys_" + tag]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(G["sd_shapes_" + tag]))
    assert not hasattr(net.decoder.decoder, "attn") and not any("attn" in k for k in sd)


def test_seq2seq_still_builds_its_attention():
    from context_attentive_ir_amd.recommender import Seq2seq
    net = Seq2seq(default_args("SEQ2SEQ", src_vocab_size=50, tgt_vocab_size=50, nhid=32, nlayers=1))
    assert "decoder.decoder.attn.linear_in.weight" in net.state_dict()


def test_config_table_is_the_references():
    assert MODEL_ARCHITECTURE["HREDQS"]["arch"] == json.loads(str(G["arch"]))
    assert MODEL_ARCHITECTURE["HREDQS"]["data"] == json.loads(str(G["data"]))
    a = default_args("HREDQS", src_vocab_size=200, tgt_vocab_size=200)
    assert a.bidirection is True and a.nlayers == 1 and a.nhid_session == 1024


def _calls(net, g):
    return (lambda: net(g["source_words"], g["source_lens"], g["target_words"], g["target_lens"], g["target_seq"], None, None),
            lambda: net.decode(g["source_words"], g["source_lens"], MAXLEN, None, None))


def test_bidirection_constructs_and_fails_like_the_reference():
    from context_attentive_ir_amd.recommender import HredQS
    g = R.case("h64")[2]
    net = HredQS(default_args("HREDQS", **KW)).eval()                  # hyparam.HREDQS's own bidirection = True
    assert "encoder.encoder.rnns.0.weight_ih_l0_reverse" in net.state_dict()
    assert str(G["bidirection_error_type"]) == str(G["bidirection_decode_error_type"]) == "RuntimeError"
    assert str(G["bidirection_error"]) == str(G["bidirection_decode_error"])
    # raised before any tensor is looked at (CPU tensors would otherwise hit the no-fallback error first)
    for call in _calls(net, g):
        with pytest.raises(RuntimeError) as e:
            call()
        assert str(e.value) == str(G["bidirection_error"])
    assert str(G["bidirection_error"]).startswith("Sizes of tensors must match except in dimension 2. Expected size 1 but got size 0")


def test_gru_and_stacked_layers_are_as_recorded():
    from context_attentive_ir_amd.recommender import HredQS
    # the reference's own encode fails for GRU: refused at construction
    assert str(G["gru_error_type"]) == "RuntimeError" and "ambiguous" in str(G["gru_error"])
    with pytest.raises(NotImplementedError, match="GRU"):
        HredQS(default_args("HREDQS", rnn_type="GRU", bidirection=False, **KW))
    # nlayers = 2: the reference constructs and fails in forward and decode; so does the mirror, with the same type and message
    assert str(G["nlayers2_error_type"]) == str(G["nlayers2_decode_error_type"]) == "IndexError"
    net = HredQS(default_args("HREDQS", nlayers=2, bidirection=False, src_vocab_size=200, tgt_vocab_size=200, nhid=64, nhid_session=64)).eval()
    assert list(net.state_dict().keys()) == [str(k) for k in G["nlayers2_sd_keys"]]
    g = R.case("h64")[2]
    for call, want in zip(_calls(net, g), (str(G["nlayers2_error"]), str(G["nlayers2_decode_error"]))):
        with pytest.raises(IndexError) as e:
            call()
        assert want.startswith(str(e.value)) and str(e.value)


def test_wrappers_construct_and_recommender_still_refuses():
    import context_attentive_ir_amd.wrappers as W
    from context_attentive_ir_amd.recommender import HredQS
    assert "SessionRecommender" in W.__all__ and issubclass(W.SessionRecommender, W.Recommender)
    src_dict, tgt_dict = list(range(120)), list(range(70))
    a = default_args("HREDQS", nhid=32, nhid_session=48, bidirection=False)
    r = W.SessionRecommender(a, src_dict, tgt_dict)
    assert isinstance(r.network, HredQS) and r.args.src_vocab_size == 120 and r.args.tgt_vocab_size == 70
    assert r.network.generator.weight.shape == (70, 48) and r.network.embedder.word_embeddings.table.shape[0] == 120
    sd = dict(r.network.state_dict(), fixed_embedding=torch.zeros(3))
    W.SessionRecommender(default_args("HREDQS", nhid=32, nhid_session=48, bidirection=False), src_dict, tgt_dict, sd)
    with pytest.raises(NotImplementedError, match="follow-up") as e:
        W.Recommender(default_args("HREDQS", **KW))
    assert "SessionRecommender" in str(e.value)
    with pytest.raises(RuntimeError, match="Unsupported model"):
        W.SessionRecommender(default_args("SEQ2SEQ", src_vocab_size=50, tgt_vocab_size=50, nhid=32, nlayers=1))


def test_save_and_load_round_trip(tmp_path):
    import context_attentive_ir_amd.wrappers as W
    r = W.SessionRecommender(default_args("HREDQS", nhid=32, nhid_session=48, bidirection=False), list(range(60)), list(range(40)))
    f = str(tmp_path / "m.mdl")
    r.save(f)
    back = W.SessionRecommender.load(f)
    assert isinstance(back, W.SessionRecommender)
    for (ka, va), (kb, vb) in zip(r.network.state_dict().items(), back.network.state_dict().items()):
        assert ka == kb and torch.equal(va, vb)
    r.init_optimizer(use_gpu=False)
    r.checkpoint(f, 3)
    model, epoch = W.SessionRecommender.load_checkpoint(f, use_gpu=False)
    assert isinstance(model, W.SessionRecommender) and epoch == 3 and model.optimizer is not None


def test_symbols_are_declared_registered_and_exported():
    from context_attentive_ir_amd import lib
    hdr = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    declared = set(re.findall(r"\b(nir_hredqs_[a-z0-9_]+)\s*\(", hdr))
    assert {"nir_hredqs_decode_greedy", "nir_hredqs_decode_workspace_bytes", "nir_hredqs_gen_argmax",
            "nir_hredqs_gen_argmax_workspace_bytes"} == declared
    assert declared <= set(lib.SIGNATURES)
    assert "nir_hredqs_decoder_weights" in hdr and "hredqs.py:169-230" in hdr
    L = lib.load()
    for name in declared:
        assert hasattr(L, name), name
    fields = [f for f, _ in lib.HredqsDecoderWeights._fields_]
    assert fields == ["rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "gen_w", "gen_b", "H", "VT", "rnn_gate_fold", "rnn_whh_frag", "gen_frag"]
    # every kernel and launcher of the new file is named for it; it edits nothing of its siblings
    src = open(os.path.join(ROOT, "context_attentive_ir_amd", "csrc", "hredqs.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (nir_\w+)\(', src)) == declared


def test_no_cpu_fallback():
    net, _, g = R.case("h64")
    for call in _calls(net, g):
        with pytest.raises(RuntimeError, match="ROCm device only"):
            call()
    with pytest.raises(RuntimeError, match="ROCm device only"):
        net.encode(g["source_words"].reshape(12, -1), g["source_lens"].reshape(-1), 3, 4)


@pytest.mark.parametrize("tag", R.CASES)
def test_the_criterion_accepts_the_fp32_chain(chains, tag):
    _, _, _, ref, chain = chains[tag]
    ok, fig = R.accept_decode(chain, ref, chain, 0)
    assert ok, fig


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_is_rejected(chains, fault):
    """at the margin's cap and with every product counted as a split one; the faults that change a state are refused by the states alone"""
    rejected, by_states = [], []
    for tag in R.CASES:
        net, c, g, ref, chain = chains[tag]
        bad = R.decode(net.state_dict(), g["source_words"], g["source_lens"], MAXLEN, T(g["tgt2src"]), fault=fault)
        ok, fig = R.accept_decode(bad, ref, chain, R.n_split(g["source_words"].shape[2], c["S"]), margin=gemm_ref.MARGIN_CAP)
        if not ok:
            rejected.append(tag)
        if fig["e"] > 100 * fig["bound"]:
            by_states.append(tag)
    assert rejected, fault
    if fault in ("pool_valid_only", "no_session_carry", "mean_pool"):
        assert by_states, fault
    if fault == "natural_pairing":
        assert rejected == list(R.CASES), (fault, rejected)                # the fixture's seeds were chosen so that the pairing shows
