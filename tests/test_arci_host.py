"""Host-side (no GPU) checks of the ARC-I mirror: the fp64 restatement (tests/arci_ref.py) against the reference's recorded scores
(tests/golden/arci.npz, arci_arch.npz, written by generate_arci.py), the config defaults, the state-dict layout, registration, the
construction errors, the width rule, the head fold, the loud failure without a device, and the teeth of the acceptance bound."""
import json

import numpy as np
import pytest
import torch

import arci_ref
import gemm_ref
from conftest import load_golden
from context_attentive_ir_amd.config import MODEL_ARCHITECTURE, default_args
from context_attentive_ir_amd.detinit import det_state_dict

EMB = arci_ref.EMB


def _net(V=200, **kw):
    from context_attentive_ir_amd.rankers import ARCI
    return ARCI(default_args("ARCI", src_vocab_size=V, **kw))


def _det_sd(net, pad_row_scale=None):
    sd = det_state_dict({k: v.shape for k, v in net.state_dict().items()})
    if pad_row_scale is not None:
        sd[EMB][0] = pad_row_scale * sd[EMB][1]
    return sd


CASES, case = arci_ref.CASES, arci_ref.case


@pytest.mark.parametrize("name,tag,mq,md,arch", CASES)
def test_restatement_equals_the_reference_scores(name, tag, mq, md, arch):
    net, q, d, want, _ = case(name, tag, mq, md, arch)
    got = arci_ref.scores(net.state_dict(), q, d, net.maxpool_size_1d)
    s = np.abs(want).max()
    assert np.abs(got.numpy() - want).max() <= 8 * 2.0 ** -23 * max(s, 1.0)          # the recorded scores are an fp32 chain


def test_config_defaults_state_dict_and_registration():
    from context_attentive_ir_amd.wrappers import Ranker
    from context_attentive_ir_amd.wrappers import ranker as R
    g = load_golden("arci")
    assert MODEL_ARCHITECTURE["ARCI"]["arch"] == json.loads(str(g["arch"]))
    assert MODEL_ARCHITECTURE["ARCI"]["data"] == json.loads(str(g["data"]))
    r = Ranker(default_args("ARCI", src_vocab_size=200, max_query_len=int(g["max_query_len"]), max_doc_len=int(g["max_doc_len"])))
    sd = r.network.state_dict()
    assert len(sd) == 13
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(g["sd_shapes"]))
    assert sum(p.numel() for p in r.network.parameters() if p.requires_grad) == int(g["n_params"])
    assert R.NETWORKS["ARCI"] is type(r.network) and "ARCI" in R.BCE_MODELS and "ARCI" not in R.NLL_MODELS
    # the defaults of scripts/ranker.sh: inp = 128 * (2 + 50), a 6656 x 3328 first Linear
    big = _net()
    assert big.mlp[0].weight.shape == (3328, 6656) and (big.query_feats, big.doc_feats) == (2, 50)


def test_construction_errors():
    with pytest.raises(AssertionError):
        _net(kernel_size_1d=[3])
    with pytest.raises(AssertionError):
        _net(maxpool_size_1d=[2, 2, 2])
    with pytest.raises(AssertionError):
        _net(max_query_len=3)                                  # 3 // 2 // 2 == 0 features
    with pytest.raises(ValueError, match="odd kernel sizes 1 .. 7 only"):
        _net(kernel_size_1d=[3, 4])
    _net(kernel_size_1d=[7, 1])


@pytest.mark.parametrize("bad,limit", [
    (dict(emsize=1025), "emsize 1025 unsupported .*<= 1024"), (dict(emsize=0), "emsize 0 unsupported"),
    (dict(filters_1d=[1025, 8]), "filters_1d 1025 unsupported .*<= 1024"), (dict(filters_1d=[8, 0]), "filters_1d 0 unsupported"),
    (dict(kernel_size_1d=[9, 3]), "kernel_size_1d 9 unsupported"), (dict(kernel_size_1d=[3, 0]), "kernel_size_1d 0 unsupported"),
    (dict(maxpool_size_1d=[65, 1], max_query_len=70), "maxpool_size_1d 65 unsupported .*<= 64"),
    (dict(maxpool_size_1d=[0, 1]), "maxpool_size_1d 0 unsupported"),
    (dict(filters_1d=[4] * 9, kernel_size_1d=[1] * 9, maxpool_size_1d=[1] * 9), "9 conv layers unsupported .*<= 8"),
])
def test_sizes_outside_the_envelope_are_refused_at_construction(bad, limit):
    from context_attentive_ir_amd.wrappers import Ranker
    with pytest.raises(ValueError, match=limit):
        _net(V=20, **bad)
    with pytest.raises(ValueError, match=limit):
        Ranker(default_args("ARCI", src_vocab_size=20, **bad))


def test_largest_sizes_construct():
    _net(V=4, emsize=1024, filters_1d=[1024, 4], kernel_size_1d=[7, 7], maxpool_size_1d=[64, 1], max_query_len=64, max_doc_len=64)
    _net(V=4, emsize=4, filters_1d=[4] * 8, kernel_size_1d=[1] * 8, maxpool_size_1d=[1] * 8)


@pytest.mark.parametrize("ql,dl,ok", [(10, 200, True), (11, 201, True), (10, 203, True), (8, 200, True), (12, 200, False), (10, 204, False),
                                      (10, 199, False), (7, 200, False), (3, 200, False)])
def test_width_rule(ql, dl, ok):
    """any width that pools to the feature counts of construction is accepted, any other is a RuntimeError raised on the host (here without
    a device: an accepted width gets as far as the device check)"""
    net = _net(V=20, emsize=8, filters_1d=[6, 4])
    q, d = torch.ones(2, ql, dtype=torch.long), torch.ones(2, 3, dl, dtype=torch.long)
    with pytest.raises(RuntimeError, match="ROCm device" if ok else "shapes cannot be multiplied"):
        net(q, None, d, None)
    net.train()
    with pytest.raises(RuntimeError, match="ROCm device" if ok else "shapes cannot be multiplied"):
        net(q, None, d, None)


def test_recorded_width_expectations():
    g = load_golden("arci")
    net, q, d, _, _ = case("arci", "", 9, 23, None)
    assert str(g["refused_error"]) == "RuntimeError"
    wq, wd = (int(v) for v in g["refused_widths"])
    with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
        net(torch.ones(2, wq, dtype=torch.long), None, torch.ones(2, 3, wd, dtype=torch.long), None)


def test_fold_head_against_the_unfolded_fp64_head():
    from context_attentive_ir_amd.rankers.arci import fold_head
    net = _net(V=20)                                                            # the 6656 -> 3328 -> 1 head of the defaults
    net.load_state_dict(_det_sd(net))
    w_eff, b_eff = fold_head(net.mlp)
    assert w_eff.dtype == torch.float32 and w_eff.shape == (6656,) and b_eff.shape == (1,)
    x = torch.rand(5, 6656, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    w1, b1, w2, b2 = (t.detach().double() for t in (net.mlp[0].weight, net.mlp[0].bias, net.mlp[1].weight, net.mlp[1].bias))
    ref = ((x @ w1.t() + b1) @ w2.t() + b2).reshape(-1)
    got = x @ w_eff.double() + b_eff.double()
    # one rounding of every folded weight: |x| <= 1, so the dot is off by at most 2^-24 sum |w_eff|
    assert float((got - ref).abs().max()) <= 2.0 ** -24 * float(w_eff.double().abs().sum() + b_eff.double().abs().sum())
    # and the fold is the float64 product rounded once
    assert torch.equal(w_eff, (w2 @ w1).reshape(-1).float())


def test_model_needs_the_device():
    net = _net(V=50, emsize=8, filters_1d=[6, 4])
    with pytest.raises(RuntimeError, match="ROCm device"):
        net(torch.ones(2, 10, dtype=torch.long), None, torch.ones(2, 3, 200, dtype=torch.long), None)


@pytest.mark.parametrize("fault", ["fp16_layer1", "pad_row", "pool_shift"])
def test_bound_rejects_planted_faults(fault):
    """With MARGIN at its cap the criterion still refuses, on the CPU: one fp16 term in the first layer, the PAD row in place of the conv's
    zero padding (non-zero PAD row), pool windows one position late.  The unfaulted fp64 and fp32 evaluations pass."""
    net, q, d, _, _ = case("arci", "_padrow", 9, 23, None)
    sd, pools = net.state_dict(), net.maxpool_size_1d
    ref, chain = arci_ref.scores(sd, q, d, pools), arci_ref.scores(sd, q, d, pools, torch.float32)
    ok, r = arci_ref.accept(chain, ref, chain, len(pools), margin=gemm_ref.MARGIN_CAP)
    assert ok, r
    ok, r = arci_ref.accept(arci_ref.scores(sd, q, d, pools, fault=fault), ref, chain, len(pools), margin=gemm_ref.MARGIN_CAP)
    assert not ok, r
