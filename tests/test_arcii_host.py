"""Host-side (no GPU) checks of the ARC-II mirror: the fp64 restatement (tests/arcii_ref.py) against the reference's recorded scores
(tests/golden/arcii.npz, arcii_arch.npz, written by generate_arcii.py), the separable first pool, the config defaults, the state-dict
layout, registration, the construction errors, the product width rule, the head fold, the loud failure without a device, and the teeth of
the acceptance bound."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import arcii_ref
import gemm_ref
from conftest import load_golden
from context_attentive_ir_amd.config import MODEL_ARCHITECTURE, default_args
from context_attentive_ir_amd.detinit import det_state_dict

EMB = arcii_ref.EMB
CASES, case = arcii_ref.CASES, arcii_ref.case
BY_KEY = {n + t: (n, t, mq, md, a) for n, t, mq, md, a in CASES}


def _net(V=200, **kw):
    from context_attentive_ir_amd.rankers import ARCII
    return ARCII(default_args("ARCII", src_vocab_size=V, **kw))


@pytest.mark.parametrize("name,tag,mq,md,arch", CASES)
def test_restatement_equals_the_reference_scores(name, tag, mq, md, arch):
    net, q, d, want, _ = case(name, tag, mq, md, arch)
    got = arcii_ref.scores(net.state_dict(), q, d, net.maxpool_size_2d)
    s = np.abs(want).max()
    assert np.abs(got.numpy() - want).max() <= 8 * 2.0 ** -23 * max(s, 1.0)          # the recorded scores are an fp32 chain


def test_fixtures_end_in_grids_with_both_sides_above_one():
    """an i / j transposition is invisible on an n x 1 grid (the defaults end in 12 x 1): the wide and the product case do not"""
    from context_attentive_ir_amd.rankers.arcii import pooled_grids
    for key, (wq, wd) in (("arcii_arch_wide", (8, 12)), ("arcii_product", (32, 16))):
        net = case(*BY_KEY[key])[0]
        hd, hq = pooled_grids(wq, wd, net.maxpool_size_2d)[-1]
        assert hd > 1 and hq > 1, (key, hd, hq)
    assert pooled_grids(32, 16, case(*BY_KEY["arcii_product"])[0].maxpool_size_2d)[-1] == (2, 4)      # built for (4, 2)


@pytest.mark.parametrize("key", ["arcii", "arcii_arch_asym"])
def test_first_pool_is_separable_bit_for_bit(key):
    """max_pool2d(Ed + Eq, 2 x 2) == max_pool1d(Ed, 2) + max_pool1d(Eq, 2) in fp32: fp32 addition is monotone in each operand"""
    net, q, d, _, _ = case(*BY_KEY[key])
    eq, ed = arcii_ref.towers(net.state_dict(), q, d)
    assert eq.dtype == torch.float32
    full = F.max_pool2d(ed.unsqueeze(3) + eq.unsqueeze(2), (2, 2))
    sep = F.max_pool1d(ed, 2).unsqueeze(3) + F.max_pool1d(eq, 2).unsqueeze(2)
    assert torch.equal(full, sep)


def test_config_defaults_state_dict_and_registration():
    from context_attentive_ir_amd.wrappers import Ranker
    from context_attentive_ir_amd.wrappers import ranker as R
    g = load_golden("arcii")
    assert MODEL_ARCHITECTURE["ARCII"]["arch"] == json.loads(str(g["arch"]))
    assert MODEL_ARCHITECTURE["ARCII"]["data"] == json.loads(str(g["data"]))
    r = Ranker(default_args("ARCII", src_vocab_size=200, max_query_len=int(g["max_query_len"]), max_doc_len=int(g["max_doc_len"])))
    sd = r.network.state_dict()
    assert len(sd) == 13
    assert list(sd.keys()) == [str(k) for k in g["sd_keys"]]
    assert [list(v.shape) for v in sd.values()] == json.loads(str(g["sd_shapes"]))
    assert sum(p.numel() for p in r.network.parameters() if p.requires_grad) == int(g["n_params"])
    assert R.NETWORKS["ARCII"] is type(r.network) and "ARCII" in R.BCE_MODELS and "ARCII" not in R.NLL_MODELS
    # the defaults of scripts/ranker.sh (max_query_len 10, max_doc_len 100): a final grid of 12 x 1, inp = 128 * 12
    big = _net()
    assert big.mlp[0].weight.shape == (768, 1536) and (big.doc_feats, big.query_feats) == (12, 1)


def test_construction_errors():
    with pytest.raises(AssertionError):
        _net(maxpool_size_2d=[[2, 2]])                         # list lengths (arcii.py:30)
    with pytest.raises(AssertionError):
        _net(max_query_len=7)                                  # 7 // 2 // 2 // 2 == 0 features (arcii.py:48)
    with pytest.raises(ValueError, match="kernel_size_1d 2 unsupported .*odd"):
        _net(kernel_size_1d=2)
    with pytest.raises(ValueError, match="kernel_size_2d \\[3, 2\\] unsupported .*odd"):
        _net(kernel_size_2d=[[3, 3], [3, 2]])
    with pytest.raises(ValueError, match="filters_2d has 1 entries for 2"):
        _net(filters_2d=[8])
    _net(kernel_size_1d=7, kernel_size_2d=[[7, 1], [1, 7]])


@pytest.mark.parametrize("bad,limit", [
    (dict(emsize=1025), "emsize 1025 unsupported .*<= 1024"), (dict(emsize=0), "emsize 0 unsupported"),
    (dict(filters_1d=1025), "filters_1d 1025 unsupported .*<= 1024"), (dict(filters_1d=0), "filters_1d 0 unsupported"),
    (dict(filters_2d=[1025, 8]), "filters_2d 1025 unsupported .*<= 1024"), (dict(filters_2d=[8, 0]), "filters_2d 0 unsupported"),
    (dict(kernel_size_1d=9), "kernel_size_1d 9 unsupported"), (dict(kernel_size_1d=0), "kernel_size_1d 0 unsupported"),
    (dict(kernel_size_2d=[[9, 3], [3, 3]]), "kernel_size_2d \\[9, 3\\] unsupported"),
    (dict(kernel_size_2d=[[3, 3], [3, 0]]), "kernel_size_2d \\[3, 0\\] unsupported"),
    (dict(maxpool_size_2d=[[13, 5], [1, 1]], max_doc_len=200), "maxpool_size_2d \\[13, 5\\] unsupported .*<= 64"),
    (dict(maxpool_size_2d=[[0, 1], [1, 1]]), "maxpool_size_2d \\[0, 1\\] unsupported"),
    (dict(filters_2d=[4] * 9, kernel_size_2d=[[1, 1]] * 9, maxpool_size_2d=[[1, 1]] * 9), "9 conv2d layers unsupported .*<= 8"),
])
def test_sizes_outside_the_envelope_are_refused_at_construction(bad, limit):
    from context_attentive_ir_amd.wrappers import Ranker
    with pytest.raises(ValueError, match=limit):
        _net(V=20, **bad)
    with pytest.raises(ValueError, match=limit):
        Ranker(default_args("ARCII", src_vocab_size=20, **bad))


def test_largest_sizes_construct():
    _net(V=4, emsize=1024, filters_1d=1024, kernel_size_1d=7, filters_2d=[4, 4], kernel_size_2d=[[7, 7], [7, 7]],
         maxpool_size_2d=[[8, 8], [1, 1]], max_query_len=16, max_doc_len=16)
    _net(V=4, emsize=4, filters_1d=4, filters_2d=[1024, 4], kernel_size_2d=[[7, 7], [1, 1]], maxpool_size_2d=[[1, 64], [1, 1]],
         max_query_len=128, max_doc_len=2)
    _net(V=4, emsize=4, filters_1d=4, filters_2d=[4] * 8, kernel_size_2d=[[1, 1]] * 8, maxpool_size_2d=[[1, 1]] * 8)


# the default arch (pools 2 x 2 twice after the first 2 x 2) built for (9, 23): a 2 x 1 final grid, 256 features
DEFAULT_WIDTHS = [(9, 23, True), (8, 22, True), (10, 23, True), (11, 23, True), (15, 23, True), (9, 16, True), (9, 24, False), (9, 15, False),
                  (16, 23, False), (7, 23, False), (9, 7, False), (16, 8, True)]
# a model built for (16, 32) (a 4 x 2 final grid): any grid with the same PRODUCT runs, whichever side carries it
PRODUCT_WIDTHS = [(16, 32, True), (32, 16, True), (8, 64, True), (64, 8, True), (16, 40, False), (24, 32, False), (4, 128, False), (128, 4, False)]


@pytest.mark.parametrize("built,ql,dl,ok", [((9, 23), q, d, ok) for q, d, ok in DEFAULT_WIDTHS] + [((16, 32), q, d, ok) for q, d, ok in PRODUCT_WIDTHS])
def test_width_rule(built, ql, dl, ok):
    """any widths whose final grid has the feature count of construction are accepted, any other -- and any that pool to nothing -- is a
    RuntimeError raised on the host (here without a device: an accepted width gets as far as the device check)"""
    net = _net(V=20, emsize=8, filters_1d=6, filters_2d=[6, 4], max_query_len=built[0], max_doc_len=built[1])
    q, d = torch.ones(2, ql, dtype=torch.long), torch.ones(2, 3, dl, dtype=torch.long)
    with pytest.raises(RuntimeError, match="ROCm device" if ok else "shapes cannot be multiplied"):
        net(q, None, d, None)
    net.train()
    with pytest.raises(RuntimeError, match="ROCm device" if ok else "shapes cannot be multiplied"):
        net(q, None, d, None)


def test_recorded_width_expectations():
    g = load_golden("arcii")
    net = case(*BY_KEY["arcii"])[0]
    assert str(g["refused_error"]) == "RuntimeError"
    wq, wd = (int(v) for v in g["refused_widths"])
    with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
        net(torch.ones(2, wq, dtype=torch.long), None, torch.ones(2, 3, wd, dtype=torch.long), None)
    assert tuple(int(v) for v in g["built_product"]) == (16, 32) and tuple(int(v) for v in g["widths_product"]) == (32, 16)


def test_fold_head_against_the_unfolded_fp64_head():
    from context_attentive_ir_amd.rankers.arci import fold_head
    net = _net(V=20)                                                            # the 1536 -> 768 -> 1 head of the defaults
    net.load_state_dict(det_state_dict({k: v.shape for k, v in net.state_dict().items()}))
    w_eff, b_eff = fold_head(net.mlp)
    assert w_eff.dtype == torch.float32 and w_eff.shape == (1536,) and b_eff.shape == (1,)
    x = torch.rand(5, 1536, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    w1, b1, w2, b2 = (t.detach().double() for t in (net.mlp[0].weight, net.mlp[0].bias, net.mlp[1].weight, net.mlp[1].bias))
    ref = ((x @ w1.t() + b1) @ w2.t() + b2).reshape(-1)
    got = x @ w_eff.double() + b_eff.double()
    # one rounding of every folded weight: |x| <= 1, so the dot is off by at most 2^-24 sum |w_eff|
    assert float((got - ref).abs().max()) <= 2.0 ** -24 * float(w_eff.double().abs().sum() + b_eff.double().abs().sum())
    assert torch.equal(w_eff, (w2 @ w1).reshape(-1).float())


def test_model_needs_the_device():
    net = _net(V=50, emsize=8, filters_1d=6, filters_2d=[6, 4])
    with pytest.raises(RuntimeError, match="ROCm device"):
        net(torch.ones(2, 10, dtype=torch.long), None, torch.ones(2, 3, 100, dtype=torch.long), None)


# each fault on a case where it is visible: the transposition needs a final grid with both sides > 1 (the wide case: 2 x 2)
@pytest.mark.parametrize("fault,key", [("grid_pad", "arcii_padrow"), ("grid_pad", "arcii_arch_wide"), ("hw_swap", "arcii_arch_wide"),
                                       ("hw_swap", "arcii_product"), ("fp16_layer", "arcii_padrow"), ("pool_shift", "arcii_padrow"),
                                       ("pool_shift", "arcii_arch_asym")])
def test_bound_rejects_planted_faults(fault, key):
    """With MARGIN at its cap the criterion still refuses, on the CPU: the one-sided sum where the grid pads zero, the head index
    transposed, one fp16 term in the first 2-D layer, pool windows one position late.  The unfaulted fp64 and fp32 evaluations pass."""
    net, q, d, _, _ = case(*BY_KEY[key])
    sd, pools = net.state_dict(), net.maxpool_size_2d
    n = 1 + len(pools)
    ref, chain = arcii_ref.scores(sd, q, d, pools), arcii_ref.scores(sd, q, d, pools, torch.float32)
    ok, r = arcii_ref.accept(chain, ref, chain, n, margin=gemm_ref.MARGIN_CAP)
    assert ok, r
    ok, r = arcii_ref.accept(arcii_ref.scores(sd, q, d, pools, fault=fault), ref, chain, n, margin=gemm_ref.MARGIN_CAP)
    assert not ok, r


def test_transposition_is_invisible_on_the_default_grid():
    """why the fixtures need the wide case: on an n x 1 final grid the transposed head index is the same index"""
    net, q, d, _, _ = case(*BY_KEY["arcii"])
    sd, pools = net.state_dict(), net.maxpool_size_2d
    assert torch.equal(arcii_ref.scores(sd, q, d, pools), arcii_ref.scores(sd, q, d, pools, fault="hw_swap"))
