"""GPU (-m gpu): the DSSM / CDSSM kernels (csrc/dssm.hip) away from the default 300 / 300 / 128 -- every size-dependent path against the
fp64 restatement of test_gpu_dssm.py (_ref_scores): the eval kernels across emsize / nhid / nout (gather column groups, the CDSSM
GEMM-2 second pass, the large-LDS launch), the CDSSM tile and PAD-tail edges and the DSSM gather chunks, the training operators at the
C ABI (ties, -inf, zero rows, > 64 candidates, logits to +-80, an upstream gradient != 1), the embedding lookup at any emsize, first-step
gradients at non-default sizes and at the scripts/ranker.sh batch, and the reference's outputs at one non-default size per model
(tests/golden/dssm_arch.npz, cdssm_arch.npz).  Eval tolerance 1e-5 absolute (scores, tower outputs); gradients 1e-4 relative to the
largest entry (the criterion of test_gpu_dssm.py)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import T, load_golden
from test_gpu_dssm import DEV, EMB, FIELDS, _batch, _ranker, _ref_scores

pytestmark = pytest.mark.gpu


def _close(got, want, tol, what):
    got = got.detach().cpu().double() if torch.is_tensor(got) else torch.as_tensor(np.asarray(got), dtype=torch.float64)
    want = want.detach().cpu().double() if torch.is_tensor(want) else torch.as_tensor(np.asarray(want), dtype=torch.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert torch.isfinite(got).all(), what
    err = float((got - want).abs().max()) if got.numel() else 0.0
    assert err <= tol, "%s: max |diff| %.3g > %.3g" % (what, err, tol)


def _rel(got, want, tol, what, floor=1e-5):
    want = want.detach().cpu().double()
    scale = max(float(want.abs().max()), floor)
    _close(got, want, tol * scale, what)


def _eval_against_fp64(r, kind, ex, what):
    net = r.network
    got = net(*[ex[k].to(DEV) for k in FIELDS], return_reps=True)
    want = _ref_scores(kind, net.state_dict(), ex["que_rep"], ex["doc_rep"], reps=True)
    for name, g, w in zip(("scores", "rep_q", "rep_d"), got, want):
        _close(g, w, 1e-5, "%s %s" % (what, name))
    _close(net(*[ex[k].to(DEV) for k in FIELDS]), want[0], 1e-5, what + " scores without reps")


def _pad_row(r, src=5, scale=0.7):
    with torch.no_grad():
        r.network.word_embeddings.table[0] = scale * r.network.word_embeddings.table[src]


# (emsize, nhid, nout): every value of each list in the issue on both sides of its boundary, without the full grid.
# DSSM: a tower-kernel lane owns the columns lane + 64 j, j < 8 (emsize 449 / 512 need j = 7); rank_finish_kernel j < 4 (nout 256);
# the Linear loops run 8 deep plus a remainder (nhid / emsize off multiples of 8).
DSSM_ARCH = [(7, 1, 1), (64, 9, 63), (65, 257, 64), (449, 256, 65), (512, 320, 256), (512, 9, 161), (449, 1, 200), (65, 320, 160)]
# CDSSM: GEMM 2 runs 2 nout items over 320 threads (a second pass from nout 161); the tile's LDS is 160 emsize bytes, past 64 KiB from
# emsize 410 (the opt-in launch), 1017 the largest the 159 KiB check admits; nhid 320 = one conv column per thread.
CDSSM_ARCH = [(7, 1, 1), (300, 9, 63), (409, 257, 64), (410, 256, 65), (640, 320, 256), (1017, 320, 161), (410, 320, 200), (7, 257, 160)]


@pytest.mark.parametrize("kind,arch", [("dssm", a) for a in DSSM_ARCH] + [("cdssm", a) for a in CDSSM_ARCH],
                         ids=["dssm-%d-%d-%d" % a for a in DSSM_ARCH] + ["cdssm-%d-%d-%d" % a for a in CDSSM_ARCH])
def test_arch_sweep_against_fp64(kind, arch):
    E, NH, NO = arch
    r = _ranker(kind, V=300, emsize=E, nhid=NH, nout=NO)
    rng = np.random.default_rng(E * 7 + NH * 3 + NO)
    # queries of 2 CDSSM tiles, documents of 3; DSSM documents past one 256-position round of the four waves
    QL, DL = (40, 90) if kind == "cdssm" else (40, 300)
    ex = _batch(rng, 3, 4, QL, DL, 300, QL // 2, DL // 2)
    ex["doc_rep"][1, 2] = 0
    if (DSSM_ARCH if kind == "dssm" else CDSSM_ARCH).index(arch) % 2 == 0:
        _pad_row(r)
    _eval_against_fp64(r, kind, ex, "%s %s" % (kind, arch))


def _rows_with_last(rng, lasts, L, V, interior):
    """one id row per entry of `lasts`: random non-PAD ids up to that position (-1: an all-PAD row), PAD after it; with `interior` the
    rows that are long enough get a second copy with an interior run of 6 PAD ids (two all-PAD windows evaluated in place, so that
    copy's fold is redundant and the first copy's is not)"""
    rows = [(last, False) for last in lasts] + ([(last, True) for last in lasts if last >= 16] if interior else [])
    ids = rng.integers(4, V, size=(len(rows), L))
    for i, (last, run) in enumerate(rows):
        ids[i, last + 1:] = 0
        if run:
            ids[i, last - 12:last - 6] = 0
    return ids


def _edge_batch(rng, qlasts, dlasts, QL, DL, V, interior=True):
    q = _rows_with_last(rng, qlasts, QL, V, interior)
    d = _rows_with_last(rng, dlasts, DL, V, interior)
    B = q.shape[0]
    N = -(-d.shape[0] // B)
    d = d[np.arange(B * N) % d.shape[0]].reshape(B, N, DL)
    lens = lambda ids: (np.asarray(ids) != 0).sum(-1)          # (the kernels never read the lengths)
    return {"que_rep": T(q), "que_len": T(lens(q)), "doc_rep": T(d), "doc_len": T(lens(d)), "label": torch.zeros(B, N)}


def _cdssm_lasts(L):
    """last non-PAD positions at the CDSSM edges for width L (P = L - 4 windows): all PAD, position 0, the end of the first window, the
    tile boundaries (windows 31 / 32 and 63 / 64), P - 2 (exactly one all-PAD window), P - 1 and the last 4 positions (no all-PAD window)"""
    P = L - 4
    return sorted({x for x in (-1, 0, 4, 30, 31, 32, 33, 63, 64, P - 3, P - 2, P - 1, L - 4, L - 3, L - 2, L - 1) if -1 <= x < L})


def _cdssm_windows(sd, pre, ids):
    """fp64 per-window outputs tanh(sem(tanh(conv))) [R, P, nout] of one CDSSM tower (cdssm.py:54-63 before the max)"""
    sd = {k: v.to(DEV, torch.float64) for k, v in sd.items()}
    x = F.embedding(ids.to(DEV), sd[EMB])
    L = x.shape[1]
    inter = torch.cat([x[:, i:L - 2 + i] for i in range(3)], -1)
    h = torch.tanh(F.conv1d(inter.transpose(1, 2), sd[pre + "_conv.weight"], sd[pre + "_conv.bias"]).transpose(1, 2))
    return torch.tanh(h @ sd[pre + "_sem.weight"].t() + sd[pre + "_sem.bias"])


# window counts P = L - 4 of 1, 31, 32, 33, 64 and 65 on both sides; a query of 36+ positions spans two tiles
CDSSM_WIDTHS = [(5, 69), (35, 68), (36, 37), (37, 36), (68, 35), (69, 5)]


@pytest.mark.parametrize("QL,DL", CDSSM_WIDTHS)
def test_cdssm_tile_and_pad_tail_edges(QL, DL):
    r = _ranker("cdssm", V=200)
    rng = np.random.default_rng(QL * 100 + DL)
    ex = _edge_batch(rng, _cdssm_lasts(QL), _cdssm_lasts(DL), QL, DL, 200)
    _eval_against_fp64(r, "cdssm", ex, "cdssm %d/%d zero PAD row" % (QL, DL))
    _pad_row(r, src=9, scale=1.5)
    _eval_against_fp64(r, "cdssm", ex, "cdssm %d/%d PAD row" % (QL, DL))


def test_cdssm_folded_pad_window_is_the_max_where_it_is_the_only_one():
    """Rows whose last non-PAD id is at position P - 2 have exactly one all-PAD window (P - 1), which the kernels never evaluate in place:
    its vector is folded in.  With this PAD row that vector is the column max of such rows in some columns (asserted on the fp64 per-window
    outputs, by a margin far above fp32 rounding), so a lost fold changes rep_q / rep_d there."""
    r = _ranker("cdssm", V=200)
    _pad_row(r, src=9, scale=1.5)
    rng = np.random.default_rng(77)
    QL, DL = 37, 69
    qlasts, dlasts = [QL - 6] * 4, [DL - 6, 4, 31, DL - 6, 0, DL - 6]
    ex = _edge_batch(rng, qlasts, dlasts, QL, DL, 200, interior=False)
    sd = r.network.state_dict()
    padwin = torch.zeros(1, 5, dtype=torch.long)
    for side, pre, ids in (("query", "query", ex["que_rep"]), ("doc", "doc", ex["doc_rep"].reshape(-1, DL))):
        L = ids.shape[1]
        rows = [i for i in range(ids.shape[0]) if int((ids[i] != 0).nonzero().max()) == L - 6]
        win = _cdssm_windows(sd, pre, ids[rows])                                 # [rows, P, nout]
        assert bool((ids[rows][:, L - 5:] == 0).all())                           # window P - 1 is all PAD, window P - 2 is not
        pv = _cdssm_windows(sd, pre, padwin)[0, 0]
        assert torch.allclose(win[:, -1], pv.expand_as(win[:, -1]), rtol=0, atol=1e-12)
        gap = pv - win[:, :-1].max(1)[0]                                         # > 0: the folded vector is the max in that column
        assert int((gap > 1e-3).sum()) >= 3, (side, float(gap.max()))
    _eval_against_fp64(r, "cdssm", ex, "cdssm single all-PAD window")


def _dssm_lasts(L):
    """DSSM gather edges: 64-id chunks, four waves striding 256, DS_INFLIGHT = 8 rows per round (counts 7, 63, 65, 257, 258 are not multiples
    of 8); all PAD; the full row"""
    return sorted({x for x in (-1, 0, 6, 62, 63, 64, 255, 256, 257, 300, 511, 512, L - 2, L - 1) if -1 <= x < L})


@pytest.mark.parametrize("QL,DL", [(1, 520), (300, 258), (70, 1)])
def test_dssm_gather_chunk_edges(QL, DL):
    r = _ranker("dssm", V=200)
    rng = np.random.default_rng(QL + DL)
    ex = _edge_batch(rng, _dssm_lasts(QL), _dssm_lasts(DL), QL, DL, 200)
    _eval_against_fp64(r, "dssm", ex, "dssm %d/%d zero PAD row" % (QL, DL))
    _pad_row(r, src=9, scale=1.5)
    _eval_against_fp64(r, "dssm", ex, "dssm %d/%d PAD row" % (QL, DL))


# ---- training operators at the C ABI (autograd.py over csrc/dssm.hip) -----------------------------------------------------------------

@pytest.mark.parametrize("R,T_,D", [(6, 1, 63), (3, 1000, 1), (5, 37, 300), (4, 1000, 63), (9, 3, 1)])
def test_max_pool_routes_ties_to_the_first_arg_max(R, T_, D):
    """A.max_pool against torch.max(dim) in fp64 on the CPU: values from {-2 .. 2} so that most columns tie, -inf columns and a -inf row.
    Max and scatter are exact, so the comparison is exact; ties go to the first arg-max, as torch.max (asserted here too)."""
    from context_attentive_ir_amd import autograd as A
    g = torch.Generator().manual_seed(R * 1000 + T_ + D)
    x = torch.randint(-2, 3, (R, T_, D), generator=g).float()
    x[0, :, : max(1, D // 3)] = float("-inf")
    x[R - 1] = float("-inf")
    dy = torch.randn(R, D, generator=g)
    xr = x.double().requires_grad_(True)
    yr, ir = xr.max(1)
    yr.backward(dy.double())
    assert torch.equal(ir, (x == yr.detach().float().unsqueeze(1)).int().argmax(1))
    xd = x.to(DEV).requires_grad_(True)
    y = A.max_pool(xd)
    y.backward(dy.to(DEV))
    assert torch.equal(y.cpu(), yr.detach().float())
    assert torch.equal(xd.grad.cpu(), xr.grad.float())


def _cosine_inputs(B, N, D, seed):
    g = torch.Generator().manual_seed(seed)
    q, d = torch.randn(B, D, generator=g), torch.randn(B, N, D, generator=g)
    q[1] = 0.0                                     # an all-zero query
    d[2, N - 1] = 0.0                              # an all-zero candidate
    return q, d, torch.randn(B, N, generator=g)


def _cosine_grads_close(dq, dd, q, d, gs, qr, dr, what):
    """the error of a row's gradient is held to 1e-5 of the terms it is made of (|g| / max(|v|, eps) per row), since a gradient can cancel
    exactly (D = 1: the cosine is +-1 wherever it is defined)"""
    eps = 1e-8
    nq, nd = q.double().norm(dim=1).clamp_min(eps), d.double().norm(dim=2).clamp_min(eps)
    gs = gs.double().abs()
    _close(dq.cpu().double() / (gs.sum(1) / nq)[:, None], qr.grad / (gs.sum(1) / nq)[:, None], 1e-5, what + " dq")
    _close(dd.cpu().double() / (gs / nd)[..., None], dr.grad / (gs / nd)[..., None], 1e-5, what + " dd")


@pytest.mark.parametrize("D", [1, 63, 64, 65, 256])
@pytest.mark.parametrize("N", [1, 10, 50])
def test_cosine_forward_backward_against_fp64(N, D):
    """A.cosine against F.cosine_similarity (ATen: x / max(|x|, eps) . y / max(|y|, eps), eps = 1e-8) in fp64.  Clamped-norm convention of
    the backward kernel: a row whose norm is <= eps has the constant norm eps, so ds/dx = y / (eps |y|) at an all-zero row x (s = 0 there);
    that is also ATen's gradient at an exactly zero row.  An all-zero row scores 0, and every gradient is finite."""
    from context_attentive_ir_amd import autograd as A
    B = 5
    q, d, gs = _cosine_inputs(B, N, D, N * 1000 + D)
    qr, dr = q.double().requires_grad_(True), d.double().requires_grad_(True)
    sr = F.cosine_similarity(qr.unsqueeze(1).expand_as(dr), dr, dim=2)
    sr.backward(gs.double())
    qd, dd = q.to(DEV).requires_grad_(True), d.to(DEV).requires_grad_(True)
    s = A.cosine(qd, dd)
    s.backward(gs.to(DEV))
    _close(s, sr, 1e-5, "cosine")
    assert float(s.detach()[1].abs().max()) == 0.0 and float(s.detach()[2, N - 1]) == 0.0
    for v in (qd.grad, dd.grad):
        assert torch.isfinite(v).all()
    zero_q = d[1].double() / (1e-8 * d[1].double().norm(dim=1, keepdim=True).clamp_min(1e-8))
    _close(qr.grad[1], (gs[1].double()[:, None] * zero_q).sum(0), 1e-6 * float(qr.grad[1].abs().max()), "ATen at the zero row")
    _cosine_grads_close(qd.grad, dd.grad, q, d, gs, qr, dr, "cosine N %d D %d" % (N, D))


@pytest.mark.parametrize("D", [257, 449, 512])
def test_cosine_backward_alone_up_to_512(D):
    """nir_cosine_bcast_bwd_f32 accepts D <= 512 (8 columns per lane), the forward only 256: the backward alone, at the C ABI."""
    from context_attentive_ir_amd import lib
    B, N = 6, 10
    q, d, gs = _cosine_inputs(B, N, D, D)
    qr, dr = q.double().requires_grad_(True), d.double().requires_grad_(True)
    F.cosine_similarity(qr.unsqueeze(1).expand_as(dr), dr, dim=2).backward(gs.double())
    qc, dc, gc = q.to(DEV), d.to(DEV), gs.to(DEV)
    dq, dd = torch.full_like(qc, float("nan")), torch.full_like(dc, float("nan"))
    lib.check(lib.load().nir_cosine_bcast_bwd_f32(lib.ptr(qc), lib.ptr(dc), lib.ptr(gc), B, N, D, lib.ptr(dq), lib.ptr(dd), lib.stream()),
              "nir_cosine_bcast_bwd_f32")
    _cosine_grads_close(dq, dd, q, d, gs, qr, dr, "cosine bwd D %d" % D)


@pytest.mark.parametrize("n", [1, 10, 64, 65, 130])
def test_softmax_nll_forward_backward_against_fp64(n):
    """A.softmax_nll against -(log_softmax(s) * y).sum(1).mean() in fp64, logits spread to +-80 (a naive exp overflows fp32 from 88.7),
    labels: one positive, two positives, none, fractional, all ones; upstream gradient 2.5.  The loss is O(100) here, so it is held
    to 1e-6 relative (fp32 carries 6e-8); the gradient to 1e-5 of its largest entry."""
    from context_attentive_ir_amd import autograd as A
    g = torch.Generator().manual_seed(n)
    R = 7
    s = (torch.rand(R, n, generator=g) * 2 - 1) * 80
    s[0, 0], s[1, n - 1] = 80.0, -80.0
    y = torch.zeros(R, n)
    y[0, n // 2] = 1.0
    y[1, 0] = 1.0
    y[1, n - 1] = 1.0
    # row 2: no positive
    y[3] = torch.rand(n, generator=g) * (torch.rand(n, generator=g) < 0.3).float()
    y[3, 0] = 0.25
    y[4] = 1.0
    y[5, n - 1] = 1.0
    y[6, (3 * n) // 4] = 0.5
    sr = s.double().requires_grad_(True)
    ref = -(torch.log_softmax(sr, -1) * y.double()).sum(1).mean()
    (2.5 * ref).backward()
    sd = s.to(DEV).requires_grad_(True)
    loss = A.softmax_nll(sd, y.to(DEV))
    (2.5 * loss).backward()
    _close(loss, ref, 1e-6 * max(abs(float(ref)), 1.0), "softmax_nll loss n %d" % n)
    _rel(sd.grad, sr.grad, 1e-5, "softmax_nll grad n %d" % n)


@pytest.mark.parametrize("E", [1, 37, 411, 300])
def test_embed_lookup_and_scatter_at_any_width(E):
    """A.embed at emsize off a multiple of 4 (the element-wise lookup; 300 takes the 16-byte path): the lookup is a copy, so exact; the
    scatter-add backward skips the PAD row and accumulates repeated ids (fp32 atomics in any order: 1e-6 of the largest entry)."""
    from context_attentive_ir_amd import autograd as A
    g = torch.Generator().manual_seed(E)
    V = 50
    table = torch.randn(V, E, generator=g)
    ids = torch.randint(0, 6, (7, 33), generator=g)
    dout = torch.randn(7, 33, E, generator=g)
    emb = torch.nn.Embedding(V, E, padding_idx=0).double()
    emb.weight.data.copy_(table.double())
    ref = emb(ids)
    ref.backward(dout.double())
    td = table.to(DEV).requires_grad_(True)
    out = A.embed(ids.to(DEV), td)
    out.backward(dout.to(DEV))
    assert torch.equal(out.cpu(), ref.detach().float())
    _rel(td.grad, emb.weight.grad, 1e-6, "embed grad E %d" % E)


# ---- training at non-default sizes -------------------------------------------------------------------------------------------------

def _first_step_grads_against_fp64(kind, r, ex):
    """one training forward + backward of the product against fp64 autograd of _ref_scores (the PAD row has no gradient): the loss at
    1e-5, every parameter gradient at 1e-4 of its largest entry (test_first_step_gradients_against_fp64's criterion)"""
    from context_attentive_ir_amd import autograd as A
    net = r.network
    net.train()
    loss = A.softmax_nll(net(*[ex[k].to(DEV) for k in FIELDS]), ex["label"].to(DEV))
    loss.backward()
    params = {k: v.detach().to(DEV, torch.float64).clone().requires_grad_(True) for k, v in net.state_dict().items()}
    p = dict(params)
    p[EMB] = torch.cat([params[EMB][:1].detach(), params[EMB][1:]], 0)
    s = _ref_scores(kind, p, ex["que_rep"], ex["doc_rep"])
    ref = -(torch.log_softmax(s, -1) * ex["label"].to(DEV, torch.float64)).sum(1).mean()
    ref.backward()
    _close(loss, ref, 1e-5, "loss")
    for name, prm in net.named_parameters():
        _rel(prm.grad, params[name].grad, 1e-4, name)


# one arch with nout > 160 and nhid % 8 != 0, one with an odd emsize (for CDSSM also >= 410: the large-LDS eval launch)
TRAIN_ARCH = [("dssm", (64, 257, 200)), ("dssm", (37, 64, 65)), ("cdssm", (300, 257, 200)), ("cdssm", (411, 9, 63))]


@pytest.mark.parametrize("kind,arch", TRAIN_ARCH, ids=["%s-%d-%d-%d" % ((k,) + a) for k, a in TRAIN_ARCH])
def test_first_step_gradients_at_non_default_sizes(kind, arch):
    E, NH, NO = arch
    r = _ranker(kind, dropout_emb=0.0, fix_embeddings=False, emsize=E, nhid=NH, nout=NO)
    rng = np.random.default_rng(E + NH + NO)
    ex = _batch(rng, 3, 4, 10, 40, 200, 7, 20)
    ex["label"] = T(np.eye(4, dtype=np.float32)[[0, 2, 3]])
    _pad_row(r)
    _first_step_grads_against_fp64(kind, r, ex)
    r.network.eval()
    _eval_against_fp64(r, kind, ex, "%s %s eval after backward" % (kind, arch))


@pytest.mark.parametrize("kind", ["dssm", "cdssm"])
def test_first_step_gradients_at_the_ranker_sh_batch(kind):
    """test_ranker_shape_against_fp64_and_wider_padding's batch (B 16, N 10, QL 100, DL 1000, V 30000), its ids redrawn from a Zipf law as
    char-3-grams are, so that the common ids repeat hundreds of times in a document and their embedding gradients accumulate."""
    V = 30000
    r = _ranker(kind, V=V, dropout_emb=0.0, fix_embeddings=False)
    rng = np.random.default_rng(7)
    ex = _batch(rng, 16, 10, 100, 1000, V, 30, 300)
    for k in ("que_rep", "doc_rep"):
        ids = ex[k].numpy()
        zipf = 4 + (rng.zipf(1.3, size=ids.shape) - 1) % (V - 4)
        ex[k] = T(np.where(ids != 0, zipf, 0))
    top = np.bincount(ex["doc_rep"][0, 0].numpy())[4:].max()
    assert top >= 100, top
    lab = np.zeros((16, 10), np.float32)
    lab[np.arange(16), rng.integers(0, 10, size=16)] = 1.0
    ex["label"] = T(lab)
    _first_step_grads_against_fp64(kind, r, ex)


# ---- the reference's outputs at non-default sizes (tests/golden/generate_dssm.py) ----------------------------------------------------

@pytest.mark.parametrize("kind", ["dssm", "cdssm"])
def test_matches_reference_fixtures_at_non_default_sizes(kind):
    g = load_golden(kind + "_arch")
    r = _ranker(kind, dropout_emb=0.2, fix_embeddings=False, **json.loads(str(g["arch"])))
    ex = {k: T(g[k]) for k in FIELDS}
    _close(r.network(*[ex[k].to(DEV) for k in FIELDS]), g["scores"], 1e-5, "scores")
    _close(r.predict(ex), g["softmax"], 1e-6, "softmax")
    with torch.no_grad():
        r.network.word_embeddings.table[0] = float(g["pad_row_scale"]) * r.network.word_embeddings.table[1]
    _close(r.network(*[ex[k].to(DEV) for k in FIELDS]), g["scores_padrow"], 1e-5, "scores, PAD row")
    _close(r.predict(ex), g["softmax_padrow"], 1e-6, "softmax, PAD row")
