"""GPU (-m gpu): the generator + bias + arg-max kernel of csrc/hredqs.hip (nir_hredqs_gen_argmax) at the C ABI against float64, across its
envelope: K in {32, 96, 512, 544, 1024} (one k-step, a chunk that is not full, both row-tile widths on either side of K = 512, the largest
K) x rows in {1, 16, 17, 33, 65} (a partial row tile, a full one, one row past it, more than one row block at either width) x VT in
{1, 15, 16, 17, 200, 4099} (a single candidate, a partial tile, a full one, one row past it, fewer tiles than waves can share, several
vocabulary ranges with a zero-padded last tile).  The state is handed over as the fp16 term pairs the folded LSTM step writes.

Random weights; the float64 top-1 minus top-2 logit of every row is asserted to be >= 1e-3 on the CPU side (the seed of a case is advanced
until it is), so no row is excluded.  The split product carries each operand to 2^-22: with |h| <= 1 and weight rows of norm 2 the logits
are known to a few 1e-6, far inside that gap.  Planted cases: an exact tie (the first index wins), a winner decided by the bias alone, a
winner in the last, partial vocabulary tile ahead of the padded rows, a tgt2src entry outside [0, V) (<unk>), two calls on one workspace."""
import pytest
import torch

from context_attentive_ir_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG = -1
MIN_GAP = 1e-3


def _h16(x):
    """fp32 [rows, K] -> the fp16 term pairs [rows][K/8][2][8] (h1 rounded to nearest, h2' = fp16(2^11 (x - h1)))"""
    rows, K = x.shape
    hi = x.half()
    lo = ((x - hi.float()) * 2048.0).half()
    return torch.stack([hi.view(rows, K // 8, 8), lo.view(rows, K // 8, 8)], 2).contiguous()


def _pack(W):
    L = lib.load()
    VT, K = W.shape
    nb = L.nir_seq2seq_gen_frag_bytes(VT, K)
    assert nb
    frag = torch.empty(nb, dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    Wd = W.to(DEV).contiguous()
    lib.check(L.nir_seq2seq_pack_gen_frag(lib.ptr(Wd), VT, K, lib.ptr(frag), lib.ptr(flag), lib.stream()), "nir_seq2seq_pack_gen_frag")
    assert int(flag.item()) == 0
    return frag


def _run(x, b, frag, VT, lut=None, V=None, stride=1, ws=None):
    L = lib.load()
    rows, K = x.shape
    V = VT if V is None else V
    hd = _h16(x).to(DEV)
    bd = b.to(DEV).contiguous() if b is not None else None
    ld = lut.to(DEV) if lut is not None else None
    if ws is None:
        ws = torch.empty(L.nir_hredqs_gen_argmax_workspace_bytes(rows), dtype=torch.uint8, device=DEV)
    pred = torch.full((rows, stride), -7, dtype=torch.int64, device=DEV)
    nxt = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    rc = L.nir_hredqs_gen_argmax(lib.ptr(hd), rows, K, lib.ptr(bd), lib.ptr(frag), VT, lib.ptr(ld), V, lib.ptr(ws), ws.numel(), lib.ptr(pred),
                                 stride, lib.ptr(nxt), lib.stream())
    torch.cuda.synchronize()
    return rc, pred.cpu(), nxt.cpu()


def _random_case(seed, rows, K, VT):
    """x [rows, K] in (-1, 1) like an LSTM state, W [VT, K] with rows of norm 2, b [VT]; float64 logits with every row's top-2 gap >= 1e-3"""
    for attempt in range(64):
        g = torch.Generator().manual_seed(seed + 7919 * attempt)
        x = torch.rand(rows, K, generator=g) * 2 - 1
        W = torch.randn(VT, K, generator=g)
        W = 2 * W / W.norm(dim=1, keepdim=True)
        b = torch.randn(VT, generator=g) * 0.2
        logits = x.double() @ W.double().t() + b.double()
        if VT == 1:
            return x, W, b, logits
        top = logits.topk(2, 1).values
        if float((top[:, 0] - top[:, 1]).min()) >= MIN_GAP:
            return x, W, b, logits
    raise AssertionError("no seed gives a top-2 gap >= %g for rows=%d K=%d VT=%d" % (MIN_GAP, rows, K, VT))


@pytest.mark.parametrize("VT", [1, 15, 16, 17, 200, 4099])
@pytest.mark.parametrize("K", [32, 96, 512, 544, 1024])
def test_generator_argmax_against_fp64(K, VT):
    g = torch.Generator().manual_seed(K + VT)
    lut = torch.randperm(VT, generator=g)
    for rows in (1, 16, 17, 33, 65):
        x, W, b, logits = _random_case(100000 * rows + 7 * K + VT, rows, K, VT)
        if VT > 1:
            top = logits.topk(2, 1).values
            assert float((top[:, 0] - top[:, 1]).min()) >= MIN_GAP          # asserted, not skipped
        want = logits.argmax(1)
        frag = _pack(W)
        rc, pred, nxt = _run(x, b, frag, VT, lut, V=max(1, VT - 3), stride=3)
        assert rc == 0
        assert torch.equal(pred[:, 0], want), (rows, K, VT, pred[:, 0], want)
        assert bool((pred[:, 1:] == -7).all())                              # the prediction stride's other columns are not written
        src = lut[want]
        assert torch.equal(nxt, torch.where(src < max(1, VT - 3), src, torch.ones_like(src)))          # no source row: fed back as <unk>
        rc2, pred2, nxt2 = _run(x, b, frag, VT, lut, V=max(1, VT - 3), stride=3)
        assert rc2 == 0 and torch.equal(pred2, pred) and torch.equal(nxt2, nxt)


@pytest.mark.parametrize("K,VT,rows", [(64, 200, 17), (1024, 4099, 33)])
def test_exact_tie_goes_to_the_first_index(K, VT, rows):
    """two identical weight rows with equal bias, far ahead of the rest: in one tile, in different tiles, in different vocabulary ranges"""
    for i, j in ((5, 9), (5, 40), (5, VT - 2)):
        x, W, b, _ = _random_case(K + VT + j, rows, K, VT)
        W[j] = W[i]
        b[i] = b[j] = 50.0
        logits = x.double() @ W.double().t() + b.double()
        logits[:, j] = logits[:, i]                                        # the same numbers in the same order: an exact tie
        rest = logits.clone()
        rest[:, [i, j]] = float("-inf")
        assert float((logits[:, i] - rest.max(1).values).min()) >= MIN_GAP
        rc, pred, _ = _run(x, b, _pack(W), VT)
        assert rc == 0 and bool((pred[:, 0] == i).all()), (i, j, pred[:, 0])


@pytest.mark.parametrize("K,VT,rows", [(96, 200, 16), (544, 4099, 65)])
def test_bias_alone_decides(K, VT, rows):
    """every weight row is the same: the products are one number per decode row, the bias picks the winner"""
    g = torch.Generator().manual_seed(K * VT)
    x = torch.rand(rows, K, generator=g) * 2 - 1
    W = torch.randn(1, K, generator=g).expand(VT, K).contiguous()
    b = torch.rand(VT, generator=g)
    for winner in (0, VT // 2, VT - 1):
        bb = b.clone()
        bb[winner] = 1.0 + 0.01                                             # ahead of every other bias (< 1) by >= 0.01
        rc, pred, _ = _run(x, bb, _pack(W), VT)
        assert rc == 0 and bool((pred[:, 0] == winner).all()), (winner, pred[:, 0])
    # without a bias the tie over the whole vocabulary goes to index 0
    rc, pred, _ = _run(x, None, _pack(W), VT)
    assert rc == 0 and bool((pred[:, 0] == 0).all())


@pytest.mark.parametrize("K,rows", [(32, 17), (1024, 33)])
def test_winner_in_the_last_partial_tile_ahead_of_the_padded_rows(K, rows):
    """VT = 4099: the last tile holds three rows and thirteen zero rows; every real logit is negative, so a padded row (logit 0) would win if
    it took part"""
    VT = 4099
    x, W, b, _ = _random_case(K + rows, rows, K, VT)
    b = b - 50.0
    b[VT - 1] += 20.0
    logits = x.double() @ W.double().t() + b.double()
    top = logits.topk(2, 1).values
    assert bool((logits.argmax(1) == VT - 1).all()) and float(top[:, 0].max()) < 0 and float((top[:, 0] - top[:, 1]).min()) >= MIN_GAP
    rc, pred, _ = _run(x, b, _pack(W), VT)
    assert rc == 0 and bool((pred[:, 0] == VT - 1).all())


def test_a_target_without_a_source_row_is_fed_back_as_unk():
    rows, K, VT, V = 17, 96, 200, 150
    x, W, b, logits = _random_case(11, rows, K, VT)
    want = logits.argmax(1)
    for bad in (V, V + 7, -1, 2 ** 40):
        lut = torch.randint(0, V, (VT,), generator=torch.Generator().manual_seed(3))
        lut[want[0]] = bad
        rc, pred, nxt = _run(x, b, _pack(W), VT, lut, V=V)
        assert rc == 0 and torch.equal(pred[:, 0], want)
        exp = lut[want]
        exp = torch.where((exp >= 0) & (exp < V), exp, torch.ones_like(exp))
        assert int(exp[0]) == 1 and torch.equal(nxt, exp)


def test_two_calls_on_one_workspace_do_not_leak_keys():
    L = lib.load()
    rows, K, VT = 33, 96, 200
    ws = torch.empty(L.nir_hredqs_gen_argmax_workspace_bytes(rows), dtype=torch.uint8, device=DEV)
    x, W, b, logits = _random_case(5, rows, K, VT)
    frag = _pack(W)
    loud = b.clone()
    loud[7] = 1000.0                                                        # first call: keys far above anything the second call produces
    rc, pred, _ = _run(x, loud, frag, VT, ws=ws)
    assert rc == 0 and bool((pred[:, 0] == 7).all())
    rc, pred, _ = _run(x, b, frag, VT, ws=ws)
    assert rc == 0 and torch.equal(pred[:, 0], logits.argmax(1))
    # and fewer rows on the same workspace
    rc, pred, _ = _run(x[:5].contiguous(), b, frag, VT, ws=ws)
    assert rc == 0 and torch.equal(pred[:, 0], logits[:5].argmax(1))


def test_bad_arguments_leave_the_outputs_untouched():
    L = lib.load()
    rows, K, VT = 5, 64, 40
    x, W, b, _ = _random_case(1, rows, K, VT)
    frag = _pack(W)
    hd, bd = _h16(x).to(DEV), b.to(DEV)
    need = L.nir_hredqs_gen_argmax_workspace_bytes(rows)
    assert need > 0 and L.nir_hredqs_gen_argmax_workspace_bytes(0) == 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    for Kx, VTx, Vx, stride, nbytes, want in ((48, VT, VT, 1, need, BAD_ARG), (1056, VT, VT, 1, need, BAD_ARG), (K, 0, VT, 1, need, BAD_ARG),
                                              (K, VT, 0, 1, need, BAD_ARG), (K, VT, VT, 0, need, BAD_ARG), (K, VT, VT, 1, need - 64, -3)):
        pred = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
        nxt = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
        rc = L.nir_hredqs_gen_argmax(lib.ptr(hd), rows, Kx, lib.ptr(bd), lib.ptr(frag), VTx, None, Vx, lib.ptr(ws), nbytes, lib.ptr(pred), stride,
                                     lib.ptr(nxt), lib.stream())
        torch.cuda.synchronize()
        assert rc == want and bool((pred == -7).all()) and bool((nxt == -7).all()), (Kx, VTx, Vx, stride, nbytes)
    pred = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    nxt = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    assert L.nir_hredqs_gen_argmax(lib.ptr(hd), rows, K, lib.ptr(bd), None, VT, None, VT, lib.ptr(ws), need, lib.ptr(pred), 1, lib.ptr(nxt),
                                   lib.stream()) == BAD_ARG
    assert L.nir_hredqs_gen_argmax(lib.ptr(hd), 0, K, lib.ptr(bd), lib.ptr(frag), VT, None, VT, lib.ptr(ws), need, lib.ptr(pred), 1, lib.ptr(nxt),
                                   lib.stream()) == 0
    torch.cuda.synchronize()
    assert bool((pred == -7).all())
