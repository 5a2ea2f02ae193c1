"""Host-side (no GPU) checks of the train-mode GRU / stacked encoders: the float64 restatement (tests/rnn_train_ref.py) against torch.nn.GRU under
torch autograd, what fp32 arithmetic costs against the bars at every shape the GPU tests name, the teeth of the bars (planted faults), the new
fixture (tests/golden/match_tensor_rnn_train.npz) against the oracle, registration of the new symbols, argument errors without a device, and the
refusal of the bridge in forward_train."""
import ctypes
import os
import re

import pytest
import torch

import rnn_train_ref as R
from conftest import ROOT, T, load_golden
from helpers import build_model, cpu_state_dict
from oracle import neuroir_cpu as O

CASES = {"gru1": ("GRU", 1), "gru2": ("GRU", 2), "lstm2": ("LSTM", 2)}
SYMBOLS = {"nir_gru_train_fwd", "nir_gru_train_bwd", "nir_gru_train_mfma_supported", "nir_gru_cell_seq_fwd", "nir_gru_cell_seq_bwd"}


@pytest.mark.parametrize("shape", R.SHAPES[:4] + [(24, 8, 9, 9, False)])
@pytest.mark.parametrize("nlayers,use_last", [(1, True), (2, True), (3, False)])
def test_restatement_equals_torch_gru_in_float64(shape, nlayers, use_last):
    case = R.make_case(*shape, nlayers=nlayers, use_last=use_last)
    figs = R.figures(R.gru_stack(*case, shape[4], use_last=use_last), R.torch_stack(*case, shape[4], use_last=use_last))
    assert max(figs) <= 1e-10, figs


def test_restatement_replays_dropout_masks_like_torch():
    shape = (24, 8, 9, 9, True)
    case = R.make_case(*shape, nlayers=2)
    g = torch.Generator().manual_seed(3)
    masks = [None, (torch.rand(9, 9, 48, generator=g) >= 0.2)]
    a = R.gru_stack(*case, True, masks=masks, p_drop=0.2)
    b = R.torch_stack(*case, True, masks=masks, p_drop=0.2)
    assert max(R.figures(a, b)) <= 1e-10
    assert R.rel_err(a[0], R.gru_stack(*case, True)[0]) > 1e-3           # the masks took part


@pytest.mark.parametrize("shape", R.SHAPES + R.SEQ_SHAPES)
def test_the_bars_accept_the_float32_chain(shape):
    """the restatement in float32 against itself in float64: what the arithmetic alone costs (worst figure over these shapes 1.3e-6 of the largest
    entry on the CPU, two orders of magnitude inside the 1e-4 bar)"""
    case = R.make_case(*shape)
    ref = R.gru_stack(*case, shape[4])
    c32 = R.make_case(*shape, dtype=torch.float32)
    ok, figs = R.accept(R.gru_stack(*c32, shape[4]), ref)
    print(shape, "fp32 chain against fp64: bank %.3g dx %.3g parameters %.3g" % figs)
    assert ok, figs


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_is_rejected(fault):
    case = R.make_case(*R.FAULT_SHAPE)
    ref = R.gru_stack(*case, True)
    ok, figs = R.accept(R.gru_stack(*case, True, fault=fault), ref)
    assert not ok, figs
    ok32, _ = R.accept(R.gru_stack(*R.make_case(*R.FAULT_SHAPE, dtype=torch.float32), True, fault=fault), ref)
    assert not ok32


@pytest.mark.parametrize("tag", sorted(CASES))
def test_fixture_scores_equal_the_oracle(tag):
    """pins the new fixture to the oracle (dropouts are 0 in the fixture: the train-mode scores are the eval-mode scores)"""
    g = load_golden("match_tensor_rnn_train")
    assert [str(t) for t in g["cases"]] == ["gru1", "gru2", "lstm2"]
    rnn_type, nlayers = CASES[tag]
    m = build_model("MATCH_TENSOR", vocab=int(g["meta_vocab"]), rnn_type=rnn_type, nlayers=nlayers)
    b = {k: T(g["%s.b0_%s" % (tag, k)]) for k in ("que_rep", "que_len", "doc_rep", "doc_len")}
    s = O.match_tensor_general_scores(cpu_state_dict(m), b["que_rep"], b["que_len"], b["doc_rep"], b["doc_len"], rnn_type, nlayers)[0]
    assert float((s - T(g[tag + ".scores0"])).abs().max()) <= 1e-5
    losses = g[tag + ".losses"]
    assert losses.shape == (5,) and abs(float(losses[0]) - float(g[tag + ".loss0"])) <= 1e-6
    names = {n for n, p in m.named_parameters() if not n.startswith("word_embeddings")}
    recorded = {k.split("_", 1)[1] for k in g if k.startswith(tag + ".grad_") or k.startswith(tag + ".gradsub37_")}
    assert recorded == names                                             # a gradient for every trained parameter


def test_symbols_are_declared_registered_and_exported():
    from context_attentive_ir_amd import lib
    hdr = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    declared = set(re.findall(r"\b(nir_gru_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)))
    assert declared == SYMBOLS
    assert declared <= set(lib.SIGNATURES)
    assert hdr.count("rnn_encoder.py:62-141") >= 3 and "torch.nn.GRU" in hdr
    L = lib.load()
    for name in declared:
        assert hasattr(L, name), name
    src = open(os.path.join(ROOT, "context_attentive_ir_amd", "csrc", "gru_train.hip")).read()
    assert set(re.findall(r'extern "C" \w+ (nir_\w+)\(', src)) == declared
    assert "atomic" not in src.split("namespace nir {", 1)[1]              # the recurrence kernels use no atomics


def test_argument_errors_are_reported_without_a_gpu():
    from context_attentive_ir_amd import lib
    L = lib.load()
    buf = (ctypes.c_float * 4096)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: L.nir_last_error_string()                                # noqa: E731
    assert L.nir_gru_train_fwd(None, None, p, p, p, p, None, 2, 3, 8, 2, None) == -1 and b"null" in err()
    assert L.nir_gru_train_fwd(p, None, p, p, p, p, None, 2, 3, 129, 2, None) == -1 and b"H <= 128" in err()
    assert L.nir_gru_train_fwd(p, None, p, p, p, p, None, 2, 0, 8, 2, None) == -1
    assert L.nir_gru_train_fwd(p, None, p, p, p, p, None, 2, 3, 8, 3, None) == -1
    assert L.nir_gru_train_fwd(p, None, p, p, p, p, None, -1, 3, 8, 1, None) == -1
    assert L.nir_gru_train_fwd(p, None, p, p, p, p, None, 0, 3, 8, 1, None) == 0             # M == 0: nothing to do, no device touched
    assert L.nir_gru_train_bwd(p, None, p, p, None, p, p, None, 2, 3, 8, 2, 0, None) == -1 and b"null" in err()
    assert L.nir_gru_train_bwd(p, None, p, p, None, p, p, p, 2, 3, 129, 2, 0, None) == -1
    assert L.nir_gru_train_bwd(p, None, p, p, None, p, p, p, 2, 3, 8, 2, 3, None) == -1 and b"form" in err()
    assert L.nir_gru_train_bwd(p, None, p, p, None, p, p, p, 2, 3, 15, 2, 2, None) == -1 and b"matrix-core" in err()
    assert L.nir_gru_train_bwd(p, None, p, p, None, p, p, p, 0, 3, 64, 2, 2, None) == 0
    assert [L.nir_gru_train_mfma_supported(h) for h in (1, 15, 16, 29, 32, 64, 65, 70, 96, 100, 128, 129)] == [0, 0, 0, 1, 1, 1, 0, 1, 1, 0, 1, 0]
    assert L.nir_gru_cell_seq_fwd(None, 24, p, p, None, 0, p, 32, p, 8, 2, 8, None) == -1 and b"null" in err()
    assert L.nir_gru_cell_seq_fwd(p, 24, None, None, None, 0, p, 32, p, 8, 2, 8, None) == -1
    assert L.nir_gru_cell_seq_fwd(p, 23, p, p, None, 0, p, 32, p, 8, 2, 8, None) == -1 and b"bad dims" in err()
    assert L.nir_gru_cell_seq_fwd(p, 24, p, p, None, 0, p, 32, p, 8, 0, 8, None) == 0
    assert L.nir_gru_cell_seq_bwd(p, 8, None, None, None, 32, None, 0, p, 24, p, 24, p, 2, 8, None) == -1 and b"null" in err()
    assert L.nir_gru_cell_seq_bwd(p, 8, None, None, p, 31, None, 0, p, 24, p, 24, p, 2, 8, None) == -1 and b"bad dims" in err()
    assert L.nir_gru_cell_seq_bwd(p, 8, None, None, p, 32, None, 0, p, 24, p, 24, p, 2, 0, None) == -1
    assert L.nir_gru_cell_seq_bwd(p, 8, None, None, p, 32, None, 0, p, 24, p, 24, p, 0, 8, None) == 0


def test_forward_train_refuses_the_bridge_and_the_cpu():
    from context_attentive_ir_amd.encoders.rnn_encoder import RNNEncoder
    enc = RNNEncoder("GRU", 8, True, 2, 16, dropout=0.0, use_bridge=True).train()
    with pytest.raises(NotImplementedError, match="use_bridge"):
        enc.forward_train(torch.zeros(2, 3, 8), None)
    with pytest.raises(RuntimeError, match="ROCm device only"):          # no CPU fallback
        RNNEncoder("GRU", 8, True, 2, 16).train().forward_train(torch.zeros(2, 3, 8), None)


def test_birnn_dispatches_on_the_container():
    from context_attentive_ir_amd import autograd as A
    with pytest.raises(NotImplementedError, match="nn.LSTM or nn.GRU"):
        A.birnn(torch.zeros(1, 2, 4), None, torch.nn.RNN(4, 4, batch_first=True))
    with pytest.raises(RuntimeError, match="ROCm device only"):
        A.birnn(torch.zeros(1, 2, 4), None, torch.nn.GRU(4, 4, batch_first=True))
