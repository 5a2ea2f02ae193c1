"""GPU (-m gpu): corpus retrieval through the models and the wrapper (DSSM / CDSSM encode_queries / encode_documents, retrieval.DocumentIndex,
Ranker.build_index / search): the towers' outputs bit for bit, the reference's scores (tests/golden/dssm.npz, cdssm.npz) found through an index,
graph replay, growth, and save / load of an index."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import retrieve_ref as R
from conftest import T, load_golden
from context_attentive_ir_amd.config import default_args
from context_attentive_ir_amd.detinit import fill_module_

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("que_rep", "que_len", "doc_rep", "doc_len")
KINDS = ["dssm", "cdssm"]


def _ranker(kind, V=200, seed=1013, **kw):
    from context_attentive_ir_amd.wrappers import Ranker
    r = Ranker(default_args(kind, src_vocab_size=V, **kw))
    fill_module_(r.network, seed)
    r.cuda()
    r.network.eval()
    return r


def _batch(rng, B, N, QL, DL, V=200):
    ql = np.clip(rng.poisson(QL // 2, size=B), 1, QL)
    dl = np.clip(rng.poisson(DL // 2, size=(B, N)), 1, DL)
    ql[0], dl[0, 0] = QL, DL
    q = rng.integers(4, V, size=(B, QL))
    d = rng.integers(4, V, size=(B, N, DL))
    q[np.arange(QL)[None] >= ql[:, None]] = 0
    d[np.arange(DL)[None, None] >= dl[..., None]] = 0
    return {"que_rep": T(q), "que_len": T(ql), "doc_rep": T(d), "doc_len": T(dl)}


@pytest.mark.parametrize("kind", KINDS)
def test_encode_is_bit_equal_to_the_return_reps_outputs(kind):
    """a non-zero PAD row, rows with PAD tails, an all-PAD row, and the same rows re-padded wider (the PAD-tail shortcut)"""
    r = _ranker(kind)
    net = r.network
    with torch.no_grad():
        net.word_embeddings.table[0] = 0.7 * net.word_embeddings.table[5]
    ex = _batch(np.random.default_rng(3), 5, 4, 12, 40)
    ex["doc_rep"][1, 2] = 0
    ex["doc_rep"][2, 3, 10:20] = 0
    for extra_q, extra_d in ((0, 0), (9, 77)):
        q, d = F.pad(ex["que_rep"], (0, extra_q)).to(DEV), F.pad(ex["doc_rep"], (0, extra_d)).to(DEV)
        _, rq, rd = net(q, None, d, None, return_reps=True)
        eq, ed = net.encode_queries(q), net.encode_documents(d.reshape(20, -1))
        assert eq.shape == rq.shape and torch.equal(eq, rq)
        assert torch.equal(ed, rd.reshape(20, -1))
        assert torch.equal(net.encode_documents(d.reshape(20, -1)[7:9]), rd.reshape(20, -1)[7:9])       # a row's bits do not depend on its batch
    assert tuple(net.encode_documents(d.reshape(20, -1)[:0]).shape) == (0, rq.shape[1])
    net.train()
    with pytest.raises(NotImplementedError):
        net.encode_queries(q)
    net.eval()


@pytest.mark.parametrize("kind", KINDS)
def test_out_of_vocabulary_ids_go_through_the_shared_check(kind):
    r = _ranker(kind)
    ex = _batch(np.random.default_rng(1), 2, 3, 8, 12)
    d = ex["doc_rep"].reshape(6, -1).clone()
    good = r.network.encode_documents(d.to(DEV))
    r.network.check_ids()
    d[4, 3] = 205
    bad = r.network.encode_documents(d.to(DEV))                                        # read as PAD, like every forward
    with pytest.raises(IndexError):
        r.network.check_ids()
    assert torch.equal(bad[:4], good[:4]) and torch.isfinite(bad).all()


@pytest.mark.parametrize("kind", KINDS)
def test_the_fixture_scores_are_found_through_an_index(kind):
    """the index holds the B N documents of the fixture; with k = B N every document is returned for every query, and the score found for document
    (b, n) under query b is the reference's scores[b, n] -- 1e-5, the tolerance of test_matches_reference_fixtures"""
    g = load_golden(kind)
    r = _ranker(kind, dropout_emb=0.2, fix_embeddings=False)
    for suffix in ("", "5"):
        ex = {k: T(g[k + suffix]) for k in FIELDS}
        B, N, DL = ex["doc_rep"].shape
        index = r.build_index([{"doc_rep": ex["doc_rep"].reshape(B * N, DL)}])
        assert len(index) == B * N and index.dim == r.args.nout
        scores, ids = r.search(ex, index, B * N)
        assert scores.shape == (B, B * N) and ids.dtype == torch.int64 and scores.dtype == torch.float32
        index.check()
        scores, ids = scores.cpu().numpy(), ids.cpu().numpy()
        for b in range(B):
            assert sorted(ids[b].tolist()) == list(range(B * N))
            found = np.zeros(B * N)
            found[ids[b]] = scores[b]
            np.testing.assert_allclose(found[b * N:(b + 1) * N], g["scores" + suffix][b], rtol=0, atol=1e-5)
            assert (np.diff(scores[b]) <= 0).all()
        # ... and the same scores as the ranker's own forward gives for these pairs, to the criterion's bound
        s = r.network(*[ex[k].to(DEV) for k in FIELDS]).cpu().numpy()
        for b in range(B):
            found = np.zeros(B * N)
            found[ids[b]] = scores[b]
            assert np.abs(found[b * N:(b + 1) * N] - s[b]).max() <= 2 * R.E_S(index.dim)


@pytest.mark.parametrize("kind", KINDS)
def test_search_is_the_same_under_graph_replay(kind):
    r = _ranker(kind)
    r.predict_graph_min_calls = 2
    rng = np.random.default_rng(4)
    docs = _batch(rng, 1, 300, 6, 30)["doc_rep"][0]
    index = r.build_index([{"doc_rep": docs[:100]}, {"doc_rep": docs[100:]}])
    exs = [_batch(rng, 4, 1, 20, 30) for _ in range(3)]
    eager = []
    for e in exs:
        reps = r.network.encode_queries(e["que_rep"].to(DEV))
        val, idx = index.search(reps, 10)
        eager.append((val.clone(), idx.clone()))
        ok, why = R.accept(val.cpu().numpy(), idx.cpu().numpy(), reps.cpu().numpy(), r.network.encode_documents(docs.to(DEV)).cpu().numpy(), 10)
        assert ok, why
    for _ in range(3):                                   # the second call of the shape captures, later ones replay
        for e, (val, idx) in zip(exs, eager):
            s, i = r.search(e, index, 10)
            assert torch.equal(s, val) and torch.equal(i, idx)
    assert r._graphs is not None and r._graphs.captures >= 1 and r._graphs.replays >= 3
    first = index.add(r.network.encode_documents(docs[:5].to(DEV)))                    # a changed index is a new graph key, not a stale replay
    assert first == 300 and len(index) == 305
    s, i = r.search(exs[0], index, 10)
    reps = r.network.encode_queries(exs[0]["que_rep"].to(DEV))
    val, idx = index.search(reps, 10)
    assert torch.equal(s, val) and torch.equal(i, idx)


def _search_entries(r):
    return [key for key in r._graphs.entries if isinstance(key[1], tuple) and key[1][:1] == ("search",)]


@pytest.mark.parametrize("kind", KINDS)
def test_a_rebuilt_index_of_equal_size_is_never_served_by_an_old_graph(kind):
    """`for corpus in folds: index = build_index(corpus); search(...)`: every pass drops the previous index, whose id() -- and, built the same
    way, whose version and count -- the next one may well get again.  A graph captured over the dropped buffer must not be replayed: the key
    is the index's process-wide serial.  Graphs of dropped indices and of earlier versions of a growing one leave the cache."""
    import gc
    r = _ranker(kind)
    r.predict_graph_min_calls = 2
    rng = np.random.default_rng(11)
    ex = _batch(rng, 4, 1, 20, 30)
    serials = []
    for fold in range(5):
        docs = _batch(rng, 1, 200, 6, 30)["doc_rep"][0]                                # another corpus of the same size, added in one call
        index = r.build_index([{"doc_rep": docs}])
        serials.append(index.serial)
        assert (index.version, index.count) == (2, 200)                                # the same state numbers in every pass
        val, idx = index.search(r.network.encode_queries(ex["que_rep"].to(DEV)), 10)
        for _ in range(3):                                                             # eager, capture + replay, replay
            s, i = r.search(ex, index, 10)
            assert torch.equal(s, val) and torch.equal(i, idx), fold
        assert len(_search_entries(r)) == 1
        del index
        gc.collect()
    assert len(set(serials)) == 5 and serials == sorted(serials)
    assert r._graphs.captures == 5
    index = r.build_index([{"doc_rep": docs}])                                          # a growing index: one live graph, the superseded ones dropped
    for step in range(3):
        index.add(r.network.encode_documents(docs[:7].to(DEV)))
        val, idx = index.search(r.network.encode_queries(ex["que_rep"].to(DEV)), 10)
        for _ in range(2):
            s, i = r.search(ex, index, 10)
            assert torch.equal(s, val) and torch.equal(i, idx)
        assert len(_search_entries(r)) == 1 and _search_entries(r)[0][1][1:3] == (index.serial, index.version)
    s5, _ = r.search(ex, index, 5)                                                       # another k of the same state is a graph of its own
    s5, _ = r.search(ex, index, 5)
    assert len(_search_entries(r)) == 2 and torch.equal(s5, val[:, :5])


def test_an_index_grows_without_adding_anything_again_and_survives_save_and_load(tmp_path):
    from context_attentive_ir_amd import retrieval as X
    rng = np.random.default_rng(6)
    D = 37
    reps = rng.standard_normal((2500, D)).astype(np.float32)
    q = T(rng.standard_normal((5, D)).astype(np.float32), DEV)
    one = X.DocumentIndex(D, DEV)
    one.add(T(reps, DEV))
    grown, caps = X.DocumentIndex(D, DEV), []
    for lo, hi in ((0, 100), (100, 129), (129, 130), (130, 1100), (1100, 2500)):
        assert grown.add(T(reps[lo:hi], DEV)) == lo
        caps.append(grown.capacity)
    assert caps == [1024, 1024, 1024, 2048, 4096] and one.capacity == 4096 and len(grown) == 2500
    assert torch.equal(grown.rows(), one.rows())
    want = grown.search(q, 64)
    got = one.search(q, 64)
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    ok, why = R.accept(want[0].cpu().numpy(), want[1].cpu().numpy(), q.cpu().numpy(), reps, 64)
    assert ok, why
    for form in ("fused", "plain"):
        v, i = grown.search(q, 64, form=form)
        assert torch.equal(v, want[0]) and torch.equal(i, want[1])
    path = str(tmp_path / "index.pt")
    sd = grown.state_dict()
    assert tuple(sd["rows"].shape) == (2500, D) and sd["rows"].device.type == "cpu"                  # plain [M, D] order, no layout
    assert float((sd["rows"].double() - T(R.unit64(reps))).abs().max()) < 4 * 2.0 ** -24
    torch.save(sd, path)
    back = X.DocumentIndex(D, DEV).load_state_dict(torch.load(path))
    assert len(back) == 2500 and torch.equal(back.rows(), grown.rows())
    got = back.search(q, 64)
    assert torch.equal(want[0], got[0]) and torch.equal(want[1], got[1])
    back.add(T(reps[:3], DEV))                                                                      # a loaded index goes on growing
    assert len(back) == 2503 and int(back.search(q, 64)[1].max()) <= 2502
    bad = X.DocumentIndex(4, DEV)
    bad.add(torch.tensor([[1.0, float("nan"), 0.0, 0.0], [1.0, 0.0, 0.0, 0.0]], device=DEV))
    with pytest.raises(RuntimeError, match="non-finite"):
        bad.check()
    assert torch.equal(bad.rows()[0], torch.zeros(4, device=DEV))
