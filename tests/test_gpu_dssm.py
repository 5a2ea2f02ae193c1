"""GPU (-m gpu): the DSSM / CDSSM mirrors (csrc/dssm.hip) against the reference's outputs (tests/golden/dssm.npz, cdssm.npz, written by
generate_dssm.py) and against an fp64 torch evaluation of the reference's maths written here: the ranker.sh shape with ragged tails, the
same documents re-padded wider (pins the skip-the-PAD-tail shortcut), a non-zero PAD row, out-of-vocabulary ids, graph replay,
predict_many, the training step (5 Adam steps against fp64) and save / load."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import T, load_golden
from context_attentive_ir_amd.config import default_args
from context_attentive_ir_amd.detinit import det_state_dict, fill_module_

pytestmark = pytest.mark.gpu
DEV = "cuda"
EMB = "word_embeddings.make_embedding.emb_luts.0.weight"
FIELDS = ("que_rep", "que_len", "doc_rep", "doc_len")


def _ranker(kind, V=200, seed=1013, **kw):
    from context_attentive_ir_amd.wrappers import Ranker
    r = Ranker(default_args(kind, src_vocab_size=V, **kw))
    fill_module_(r.network, seed)
    r.cuda()
    r.network.eval()
    return r


def _ref_scores(kind, sd, q, d, reps=False):
    """fp64 evaluation of dssm.py:46-63 / cdssm.py:54-77 (the max over every padded position, ATen cosine); reps: also the tower outputs"""
    sd = {k: v.to(DEV, torch.float64) for k, v in sd.items()}
    q, d = q.to(DEV), d.to(DEV)
    B, N, DL = d.shape
    table = sd[EMB]
    eq, ed = F.embedding(q, table), F.embedding(d.reshape(B * N, DL), table)
    if kind == "dssm":
        def tower(x, pre):
            h = torch.tanh(x.max(1)[0] @ sd[pre + ".0.weight"].t() + sd[pre + ".0.bias"])
            return torch.tanh(h @ sd[pre + ".2.weight"].t() + sd[pre + ".2.bias"])
        rq, rd = tower(eq, "query_mlp"), tower(ed, "doc_mlp")
    else:
        def tower(x, pre):
            L = x.shape[1]
            inter = torch.cat([x[:, i:L - 2 + i] for i in range(3)], -1)
            h = torch.tanh(F.conv1d(inter.transpose(1, 2), sd[pre + "_conv.weight"], sd[pre + "_conv.bias"]).transpose(1, 2))
            return torch.tanh(h @ sd[pre + "_sem.weight"].t() + sd[pre + "_sem.bias"]).max(1)[0]
        rq, rd = tower(eq, "query"), tower(ed, "doc")
    rd = rd.view(B, N, -1)
    s = F.cosine_similarity(rq.unsqueeze(1).expand_as(rd), rd, dim=2)
    return (s, rq, rd) if reps else s


def _batch(rng, B, N, QL, DL, V, qmean, dmean):
    """ragged n-gram lengths around qmean / dmean (at least one row of full width), PAD tails"""
    ql = np.clip(rng.poisson(qmean, size=B), 1, QL)
    dl = np.clip(rng.poisson(dmean, size=(B, N)), 1, DL)
    ql[0], dl[0, 0] = QL, DL
    q = rng.integers(4, V, size=(B, QL))
    d = rng.integers(4, V, size=(B, N, DL))
    q[np.arange(QL)[None] >= ql[:, None]] = 0
    d[np.arange(DL)[None, None] >= dl[..., None]] = 0
    return {"que_rep": T(q), "que_len": T(ql), "doc_rep": T(d), "doc_len": T(dl), "label": torch.zeros(B, N)}


def _close(a, b, tol):
    np.testing.assert_allclose(np.asarray(a.detach().cpu().double()) if torch.is_tensor(a) else a,
                               np.asarray(b.detach().cpu().double()) if torch.is_tensor(b) else b, rtol=0, atol=tol)


@pytest.mark.parametrize("kind", ["dssm", "cdssm"])
def test_matches_reference_fixtures(kind):
    g = load_golden(kind)
    r = _ranker(kind, dropout_emb=0.2, fix_embeddings=False)
    net = r.network
    sfx = [("", "scores", "softmax")] + ([("5", "scores5", "softmax5")])
    for suffix, sk, pk in sfx:
        ex = {k: T(g[k + suffix]) for k in FIELDS}
        s = net(*[ex[k].to(DEV) for k in FIELDS])
        _close(s, g[sk], 1e-5)
        _close(r.predict(ex), g[pk], 1e-6)
    with torch.no_grad():
        net.word_embeddings.table[0] = float(g["pad_row_scale"]) * net.word_embeddings.table[1]
    ex = {k: T(g[k]) for k in FIELDS}
    _close(net(*[ex[k].to(DEV) for k in FIELDS]), g["scores_padrow"], 1e-5)
    _close(r.predict(ex), g["softmax_padrow"], 1e-6)


@pytest.mark.parametrize("kind", ["dssm", "cdssm"])
def test_ranker_shape_against_fp64_and_wider_padding(kind):
    """scripts/ranker.sh: 10 candidates, char-3-gram ids, documents ~5x the word count (about 300 n-grams around a mean, padded to the batch
    maximum of 1000), queries ~30 of 100.  Then the same ids re-padded to a larger width, with a non-zero PAD row: the kernels only evaluate
    up to the last non-PAD id and fold the PAD vector in, so this pins that shortcut."""
    V = 30000
    r = _ranker(kind, V=V)
    rng = np.random.default_rng(7)
    ex = _batch(rng, 16, 10, 100, 1000, V, 30, 300)
    ex["doc_rep"][2, 3, 40:60] = 0                    # interior PAD run
    sd = r.network.state_dict()
    for pad_row in (False, True):
        if pad_row:
            with torch.no_grad():
                r.network.word_embeddings.table[0] = 0.7 * r.network.word_embeddings.table[5]
            sd = r.network.state_dict()
        for extra_q, extra_d in ((0, 0), (9, 77)):
            e = dict(ex, que_rep=F.pad(ex["que_rep"], (0, extra_q)), doc_rep=F.pad(ex["doc_rep"], (0, extra_d)))
            s = r.network(*[e[k].to(DEV) for k in FIELDS])
            _close(s, _ref_scores(kind, sd, e["que_rep"], e["doc_rep"]), 1e-4)


@pytest.mark.parametrize("kind", ["dssm", "cdssm"])
def test_all_pad_rows_and_short_widths(kind):
    r = _ranker(kind)
    rng = np.random.default_rng(3)
    for QL, DL in ((5, 5), (6, 70), (64 + 4, 64 + 5), (1, 3)):
        if kind == "cdssm" and min(QL, DL) < 5:
            continue
        ex = _batch(rng, 3, 4, QL, DL, 200, QL // 2, DL // 2)
        ex["doc_rep"][1, 1] = 0
        ex["que_rep"][2] = 0
        s = r.network(*[ex[k].to(DEV) for k in FIELDS])
        _close(s, _ref_scores(kind, r.network.state_dict(), ex["que_rep"], ex["doc_rep"]), 1e-5)
        s2, rq, rd = r.network(*[ex[k].to(DEV) for k in FIELDS], return_reps=True)
        ref = _ref_scores(kind, r.network.state_dict(), ex["que_rep"], ex["doc_rep"], reps=True)
        for got, want in zip((s2, rq, rd), ref):
            _close(got, want, 1e-5)


@pytest.mark.parametrize("kind", ["dssm", "cdssm"])
def test_out_of_vocabulary_id_raises(kind):
    r = _ranker(kind)
    r.id_check = "blocking"
    ex = _batch(np.random.default_rng(1), 2, 3, 8, 12, 200, 6, 10)
    assert torch.isfinite(r.predict(ex)).all()
    bad = dict(ex, doc_rep=ex["doc_rep"].clone())
    bad["doc_rep"][1, 2, 3] = 205
    with pytest.raises(IndexError):
        r.predict(bad)
    assert torch.isfinite(r.predict(ex)).all()


@pytest.mark.parametrize("kind", ["dssm", "cdssm"])
def test_graph_replay_and_predict_many(kind):
    r = _ranker(kind)
    rng = np.random.default_rng(4)
    exs = [_batch(rng, 4, 5, 20, 90, 200, 10, 50) for _ in range(3)]
    eager = [torch.softmax(r.network(*[e[k].to(DEV) for k in FIELDS]), -1) for e in exs]
    for _ in range(2):                                   # first call captures, later ones replay
        for e, ref in zip(exs, eager):
            _close(r.predict(e), ref, 1e-6)
    many = r.predict_many(exs)
    for i, ref in enumerate(eager):
        _close(many[i], ref, 1e-6)


def _ref_train(kind, sd, batches, steps, lr, clip):
    """fp64 torch: the reference's update (models/ranker.py:192-230) without dropout -> losses, final state dict"""
    params = {k: v.detach().to(DEV, torch.float64).clone().requires_grad_(True) for k, v in sd.items()}
    opt = torch.optim.Adam(list(params.values()), lr)
    losses = []
    for step in range(steps):
        b = batches[step % len(batches)]
        opt.zero_grad()
        p = dict(params)
        # nn.Embedding(padding_idx=PAD): no gradient for the PAD row
        pad_free = torch.cat([params[EMB][:1].detach(), params[EMB][1:]], 0)
        p[EMB] = pad_free
        s = _ref_scores(kind, p, b["que_rep"], b["doc_rep"])
        y = b["label"].to(DEV, torch.float64)
        loss = -(torch.log_softmax(s, -1) * y).sum(1).mean()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(params.values()), clip)
        opt.step()
        losses.append(float(loss))
    return losses, params


@pytest.mark.parametrize("kind", ["dssm", "cdssm"])
def test_update_trajectory_against_fp64(kind):
    """5 Adam steps with a free embedding table, dropout off; then predict() at the new weights (stale packed weights would show)."""
    r = _ranker(kind, dropout_emb=0.0, optimizer="adam", learning_rate=0.001, weight_decay=0, grad_clipping=10.0, fix_embeddings=False)
    rng = np.random.default_rng(9)
    batches = []
    for i in range(2):
        b = _batch(rng, 4, 5, 12, 40, 200, 8, 25)
        lab = np.zeros((4, 5), np.float32)
        lab[np.arange(4), rng.integers(0, 5, size=4)] = 1.0
        lab[1, (np.argmax(lab[1]) + 1) % 5] = 1.0          # two relevant candidates in one row (float labels, sum 2)
        b["label"] = T(lab)
        batches.append(b)
    sd0 = {k: v.detach().clone() for k, v in r.network.state_dict().items()}
    r.init_optimizer()
    losses = [float(r.update(batches[step % 2])) for step in range(5)]
    ref_losses, ref_params = _ref_train(kind, sd0, batches, 5, 0.001, 10.0)
    np.testing.assert_allclose(losses, ref_losses, rtol=1e-4, atol=0)
    # Adam normalises every element's step: an element whose gradient is rounding noise moves by up to lr per step in either implementation,
    # so the final weights are held to a fraction of the total Adam travel (steps x lr) rather than to their own magnitude
    sd = r.network.state_dict()
    for k, v in ref_params.items():
        err = float((sd[k].double() - v.detach()).abs().max())
        assert err < 0.02 * 5 * 0.001, (k, err)
    r.network.eval()
    ex = batches[0]
    _close(r.predict(ex), torch.softmax(_ref_scores(kind, ref_params, ex["que_rep"], ex["doc_rep"]), -1), 1e-4)
    assert r.updates == 5


@pytest.mark.parametrize("kind", ["dssm", "cdssm"])
def test_first_step_gradients_against_fp64(kind):
    r = _ranker(kind, dropout_emb=0.0, fix_embeddings=False)
    ex = _batch(np.random.default_rng(12), 3, 4, 10, 30, 200, 7, 20)
    ex["label"] = T(np.eye(4, dtype=np.float32)[[0, 2, 3]])
    net = r.network
    net.train()
    from context_attentive_ir_amd import autograd as A
    loss = A.softmax_nll(net(*[ex[k].to(DEV) for k in FIELDS]), ex["label"].to(DEV))
    loss.backward()
    params = {k: v.detach().to(DEV, torch.float64).clone().requires_grad_(True) for k, v in net.state_dict().items()}
    p = dict(params)
    p[EMB] = torch.cat([params[EMB][:1].detach(), params[EMB][1:]], 0)
    s = _ref_scores(kind, p, ex["que_rep"], ex["doc_rep"])
    ref = -(torch.log_softmax(s, -1) * ex["label"].to(DEV, torch.float64)).sum(1).mean()
    ref.backward()
    _close(loss, ref, 1e-5)
    for name, prm in net.named_parameters():
        gr = params[name].grad
        err = (prm.grad.double() - gr).abs().max() / max(float(gr.abs().max()), 1e-5)
        assert float(err) < 1e-4, (name, float(err))
    _close(r.loss(ex), ref, 1e-5)                          # the wrapper's criterion (eval-mode forward, no dropout here either)


@pytest.mark.parametrize("kind", ["dssm", "cdssm"])
def test_save_load_round_trip(kind, tmp_path):
    from context_attentive_ir_amd.wrappers import Ranker
    r = _ranker(kind)
    with torch.no_grad():
        r.network.word_embeddings.table[0] = 0.5 * r.network.word_embeddings.table[3]
    ex = _batch(np.random.default_rng(5), 3, 4, 9, 30, 200, 6, 20)
    want = r.predict(ex)
    path = str(tmp_path / "model.mdl")
    r.save(path)
    r2 = Ranker.load(path)
    r2.cuda()
    _close(r2.predict(ex), want, 0)
    assert set(r2.network.state_dict()) == set(det_state_dict({k: v.shape for k, v in r.network.state_dict().items()}))
