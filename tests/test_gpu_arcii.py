"""GPU (-m gpu): the ARC-II mirror (csrc/arcii.hip, rankers/arcii.py) against the reference's recorded outputs (tests/golden/arcii.npz,
arcii_arch.npz, written by generate_arcii.py) and against the fp64 restatement of tests/arcii_ref.py: every fixture case (the product
width rule and a 2 x 2 final grid among them), the width rule before any launch, a non-zero PAD row, N = 1 and B = 0, bitwise
repeatability, and train mode (loss, every gradient, recorded update losses, the bound at the updated weights)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import arcii_ref
from arcii_ref import CASES, case, case_args
from conftest import T, load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda"
EMB = arcii_ref.EMB
FIELDS = ("que_rep", "que_len", "doc_rep", "doc_len")


def _close(a, b, tol):
    np.testing.assert_allclose(np.asarray(a.detach().cpu().double()) if torch.is_tensor(a) else a,
                               np.asarray(b.detach().cpu().double()) if torch.is_tensor(b) else b, rtol=0, atol=tol)


def _wrap(net, args):
    """the Ranker wrapper around a fixture network, on the GPU"""
    from context_attentive_ir_amd.wrappers import Ranker
    r = Ranker(args, state_dict=net.state_dict())
    r.cuda()
    r.network.eval()
    return r


@pytest.fixture(scope="module")
def cases():
    """every fixture case once: (ranker on the GPU, q, d, recorded scores, recorded softmax, fp64 scores, fp32-chain scores)"""
    out = {}
    for name, tag, mq, md, arch in CASES:
        net, q, d, want, soft = case(name, tag, mq, md, arch)
        sd, pools = net.state_dict(), net.maxpool_size_2d
        out[name + tag] = (_wrap(net, case_args(name, tag, mq, md, arch)), q, d, want, soft, arcii_ref.scores(sd, q, d, pools),
                           arcii_ref.scores(sd, q, d, pools, torch.float32))
    return out


KEYS = [n + t for n, t, _, _, _ in CASES]


@pytest.mark.parametrize("key", KEYS)
def test_matches_reference_fixtures(cases, key):
    r, q, d, want, soft, _, _ = cases[key]
    ex = dict(que_rep=q, que_len=torch.ones(q.shape[0], dtype=torch.long), doc_rep=d, doc_len=torch.ones(d.shape[:2], dtype=torch.long))
    _close(r.network(q.to(DEV), None, d.to(DEV), None), want, 1e-5)
    _close(r.predict(ex), soft, 1e-6)
    _close(r.predict(ex), soft, 1e-6)                  # (the second call of a shape replays the captured graph)


@pytest.mark.parametrize("key", KEYS)
def test_meets_the_fp64_bound(cases, key):
    r, q, d, _, _, ref, chain = cases[key]
    got = r.network(q.to(DEV), None, d.to(DEV), None)
    ok, fig = arcii_ref.accept(got, ref, chain, 1 + len(r.network.maxpool_size_2d))
    print("arcii bound %s: %s" % (key, fig))
    assert ok, fig
    w = r.network._weights()
    assert all(l.struct.path == 0 for l in [w.q, w.d] + w.l)          # detinit weights are far inside the split range


def test_width_rule_raises_before_any_launch(cases):
    from context_attentive_ir_amd import lib
    r, q, d, _, _, _, _ = cases["arcii"]
    net = r.network
    with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
        net(q.to(DEV), None, F.pad(d, (0, 1)).to(DEV), None)                 # DL 24: a 3 x 1 grid
    with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
        net(F.pad(q, (0, 7)).to(DEV), None, d.to(DEV), None)                 # QL 16: a 2 x 2 grid
    with pytest.raises(RuntimeError, match="shapes cannot be multiplied"):
        net(q[:, :7].contiguous().to(DEV), None, d.to(DEV), None)            # QL 7 pools to nothing
    # the C entry refuses the same widths with a negative code and enqueues nothing: the scores keep their sentinel
    L, w = lib.load(), net._weights()
    qd, dd = q.to(DEV), F.pad(d, (0, 1)).to(DEV)
    B, N, DL = dd.shape
    table = net.word_embeddings.table
    scores = torch.full((B, N), -7.0, device=DEV)
    ws = torch.empty(1 << 24, dtype=torch.uint8, device=DEV)
    rc = L.nir_arcii_score(lib.ptr(qd), lib.ptr(dd), B, N, qd.shape[1], DL, lib.ptr(table), table.shape[0], table.shape[1], w.ref(), lib.ptr(ws),
                           ws.numel(), lib.ptr(scores), lib.stream())
    torch.cuda.synchronize()
    assert rc < 0 and b"do not pool" in L.nir_last_error_string()
    assert bool((scores == -7.0).all())
    assert L.nir_arcii_workspace_bytes(B, N, 7, DL, w.ref()) == 0            # a width that pools to nothing
    assert L.nir_arcii_workspace_bytes(B, N, qd.shape[1], 23, w.ref()) > 0


def test_single_candidate_and_empty_batch(cases):
    r, q, d, _, _, ref, chain = cases["arcii"]
    got = r.network(q.to(DEV), None, d[:, :1].contiguous().to(DEV), None)
    assert got.shape == (q.shape[0], 1)
    ok, fig = arcii_ref.accept(got, ref[:, :1], chain[:, :1], 3)
    assert ok, fig
    empty = r.network(q[:0].to(DEV), None, d[:0].to(DEV), None)
    assert empty.shape == (0, d.shape[1])


@pytest.mark.parametrize("key", ["arcii", "arcii_long", "arcii_arch_wide"])
def test_two_calls_give_the_same_bits(cases, key):
    r, q, d, _, _, _, _ = cases[key]
    a = r.network(q.to(DEV), None, d.to(DEV), None).clone()
    b = r.network(q.to(DEV), None, d.to(DEV), None)
    assert torch.equal(a, b)


# ---- train mode ---------------------------------------------------------------------------------------------------------------------------
def _train_ranker(fix, **kw):
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import Ranker
    r = Ranker(default_args("ARCII", **dict(dict(src_vocab_size=200, dropout_emb=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0, momentum=0,
                                                grad_clipping=10.0, fix_embeddings=fix, max_query_len=9, max_doc_len=23), **kw)))
    fill_module_(r.network)
    r.cuda()
    return r


def _train_batches():
    g = load_golden("arcii")
    return g, [{k: T(g["train_b%d_%s" % (bi, k)]) for k in FIELDS + ("label",)} for bi in range(2)]


def _first_step_against_fp64(r, ex, tag):
    from context_attentive_ir_amd import autograd as A
    net = r.network
    net.train()
    y = ex["label"].float()
    loss = A.bce_with_logits(net(*[ex[k].to(DEV) for k in FIELDS]), y.to(DEV))
    loss.backward()
    params = {k: v.detach().to(DEV, torch.float64).clone().requires_grad_(True) for k, v in net.state_dict().items()}
    p = dict(params)
    p[EMB] = torch.cat([params[EMB][:1].detach(), params[EMB][1:]], 0)              # nn.Embedding(padding_idx=PAD): no gradient for the PAD row
    s = arcii_ref.forward(p, ex["que_rep"].to(DEV), ex["doc_rep"].to(DEV), net.maxpool_size_2d)
    ref = F.binary_cross_entropy_with_logits(s, y.to(DEV, torch.float64))
    ref.backward()
    assert abs(float(loss) - float(ref)) <= 1e-5 * abs(float(ref))
    for name, prm in net.named_parameters():
        gr = params[name].grad
        err = (prm.grad.double() - gr).abs().max() / max(float(gr.abs().max()), 1e-5)
        print("arcii grad %s %s: %.3g" % (tag, name, float(err)))
        assert float(err) < 1e-4, (name, float(err))


def test_first_step_loss_and_gradients_against_fp64():
    r = _train_ranker(False)
    _, (ex, _) = _train_batches()
    _first_step_against_fp64(r, ex, "default")


def test_first_step_gradients_on_an_asymmetric_arch_with_a_square_final_grid():
    """kernels 5 x 3 / 3 x 1, pools 3 x 1 / 1 x 2 with floor-dropped tails and a 2 x 2 final grid: a transposed window order or flatten in
    the train-mode forward would show here, not at the defaults (final grid 2 x 1)"""
    r = _train_ranker(False, emsize=37, filters_1d=20, kernel_size_1d=5, filters_2d=[24, 12], kernel_size_2d=[[5, 3], [3, 1]],
                      maxpool_size_2d=[[3, 1], [1, 2]], max_query_len=9, max_doc_len=15)
    g = torch.Generator().manual_seed(11)
    B, N = 3, 2
    ex = dict(que_rep=torch.randint(1, 200, (B, 9), generator=g), que_len=torch.full((B,), 9), doc_rep=torch.randint(1, 200, (B, N, 15), generator=g),
              doc_len=torch.full((B, N), 15), label=F.one_hot(torch.randint(0, N, (B,), generator=g), N))
    assert (r.network.doc_feats, r.network.query_feats) == (2, 2)
    _first_step_against_fp64(r, ex, "asym")


@pytest.mark.parametrize("fix", [True, False])
def test_recorded_update_losses(fix):
    g, batches = _train_batches()
    r = _train_ranker(fix)
    r.init_optimizer()
    losses = [float(r.update(batches[step % 2])) for step in range(3)]
    print("arcii update losses (fix_embeddings=%s): %s" % (fix, losses))
    np.testing.assert_allclose(losses, g["train_losses_" + ("fix" if fix else "free")], rtol=1e-4, atol=0)
    assert r.updates == 3
    table = r.network.word_embeddings.table
    assert table.requires_grad == (not fix)
    # predict() at the new weights: a stale pack would miss the bound against the network's own state dict
    r.network.eval()
    sd, ex = r.network.state_dict(), batches[0]
    got = r.network(*[ex[k].to(DEV) for k in FIELDS])
    ok, fig = arcii_ref.accept_scores(got, sd, ex["que_rep"], ex["doc_rep"], r.network.maxpool_size_2d)
    print("arcii bound after 3 updates (fix_embeddings=%s): %s" % (fix, fig))
    assert ok, fig
