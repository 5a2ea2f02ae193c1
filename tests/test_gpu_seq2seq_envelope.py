"""GPU (-m gpu): the two new kernels of csrc/seq2seq.hip at the C ABI against float64, across their envelope.

Attention (nir_seq2seq_attend): the three score forms x H in {4, 32, 96, 512, 1024} x QL in {1, 7, 33} x B in {1, 5, 70} (one wave per row:
a lane-partial row at H = 4, several float4 trips at H = 1024, more than one block at B = 5 and 70, QL = 33 past a wave's half), a length
above QL in every batch (clamped).  Bound: the house form on both outputs, e <= MARGIN * max(e_chain, 2^-23) with e_chain the same chain in
float32 on the CPU (no split product on this path); masked positions exactly 0.

Generator + arg-max (nir_seq2seq_gen_argmax): K in {32, 96, 512, 1024} x VT in {17, 200, 4099} x rows in {1, 5, 97} (both row-tile
widths, a zero-padded last vocabulary tile, more than one vocabulary range and more than one row block), and K = 544 at VT = 200 (two row
tiles a workgroup with a last chunk of k-steps that is not full), every winner PLANTED with a float64
gap of at least 1e-3 of the row's largest |logit| -- no row is excluded: winners at index 0, at VT - 1 and inside the padded tile, a winner
decided by the bias alone, an exact tie (first index wins); and every condition that sends the call to the fp32 GEMM + arg-max path, once.
Bad arguments return NIR_ERR_BAD_ARG and leave a sentinel output untouched."""
import numpy as np
import pytest
import torch

import gemm_ref
from context_attentive_ir_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
ATTN = {"general": 0, "dot": 1, "mlp": 2}
MARGIN = 4.0          # the house rule (gemm_ref.py): the largest ratio measured on the MI355X is 1.958 (mlp, H = 32), doubled, up to a power of two
BAD_ARG = -1


# ---- attention -----------------------------------------------------------------------------------------------------------------------------
def _attend_ref(q, h, mem, sb, v, lens, mlp, dt):
    q, h, mem, sb = (t.to(dt) for t in (q, h, mem, sb))
    QL = mem.shape[1]
    if mlp:
        align = (torch.tanh(q.unsqueeze(1) + sb) * v.to(dt).view(1, 1, -1)).sum(2)
    else:
        align = (q.unsqueeze(1) * sb).sum(2)
    mask = torch.arange(QL).unsqueeze(0) < lens.clamp(0, QL).unsqueeze(1)
    a = torch.softmax(align.masked_fill(~mask, float("-inf")), 1)
    return a, torch.cat([(a.unsqueeze(2) * mem).sum(1), h], 1)


def _attend(q, h, mem, sb, v, lens, kind, stride=None):
    L = lib.load()
    B, QL, H = mem.shape
    stride = QL if stride is None else stride
    d = [t.to(DEV).contiguous() for t in (q, h, mem, sb)]
    vd = v.to(DEV).contiguous() if v is not None else None
    ld = lens.to(DEV)
    cat = torch.full((B, 2 * H), -7.0, device=DEV)
    attn = torch.full((B, stride), -7.0, device=DEV)
    rc = L.nir_seq2seq_attend(lib.ptr(d[0]), lib.ptr(d[1]), lib.ptr(d[2]), lib.ptr(d[3]), lib.ptr(vd), lib.ptr(ld), B, QL, H, ATTN[kind], lib.ptr(cat),
                              lib.ptr(attn), stride, lib.stream())
    torch.cuda.synchronize()
    return rc, cat.cpu(), attn.cpu()


def _figure(got, ref, chain):
    s = float(ref.abs().max())
    e = float((got.double() - ref).abs().max()) / s
    e_chain = float((chain.double() - ref).abs().max()) / s
    return e, e_chain, e / max(e_chain, gemm_ref.EPS)


@pytest.mark.parametrize("H", [4, 32, 96, 512, 1024])
@pytest.mark.parametrize("kind", ["general", "dot", "mlp"])
def test_attention_kernel_against_fp64(kind, H):
    assert MARGIN <= gemm_ref.MARGIN_CAP
    g = torch.Generator().manual_seed(1000 * ATTN[kind] + H)
    worst = 0.0
    for QL in (1, 7, 33):
        for B in (1, 5, 70):
            # scores of order 1 (queries scaled by 1 / sqrt(H)), as behind a trained linear_in: softmax rows with several live entries
            h = torch.randn(B, H, generator=g)
            mem = torch.randn(B, QL, H, generator=g)
            mlp = kind == "mlp"
            q = torch.randn(B, H, generator=g) if mlp else h / H ** 0.5
            sb = mem if kind == "dot" else torch.randn(B, QL, H, generator=g)
            v = torch.randn(H, generator=g) / H ** 0.5 if mlp else None
            lens = torch.randint(1, QL + 1, (B,), generator=g)
            lens[B // 2] = QL + 3                                      # above QL: clamped
            rc, cat, attn = _attend(q, h, mem, sb, v, lens, kind, stride=QL + 5)
            assert rc == 0
            ra, rcat = _attend_ref(q, h, mem, sb, v, lens, mlp, torch.float64)
            ca, ccat = _attend_ref(q, h, mem, sb, v, lens, mlp, torch.float32)
            assert bool((attn[:, QL:] == -7.0).all())                  # the row stride's tail is not written
            attn = attn[:, :QL]
            masked = torch.arange(QL).unsqueeze(0) >= lens.clamp(0, QL).unsqueeze(1)
            assert bool((attn[masked] == 0).all())
            assert torch.equal(cat[:, H:], h)
            for name, got, ref, chain in (("attn", attn, ra, ca), ("cat", cat, rcat, ccat)):
                e, e_chain, ratio = _figure(got, ref, chain)
                worst = max(worst, ratio)
                assert e <= MARGIN * max(e_chain, gemm_ref.EPS), (kind, H, QL, B, name, e, e_chain)
    print("seq2seq attend %s H=%d: worst ratio %.3f" % (kind, H, worst))


# ---- generator + arg-max ---------------------------------------------------------------------------------------------------------------------
def _pack(W):
    """(fragments or None, flag): None when the library has no fused form for this shape or the weights are outside the split's range"""
    L = lib.load()
    VT, K = W.shape
    nb = L.nir_seq2seq_gen_frag_bytes(VT, K)
    if not nb:
        return None, 0
    frag = torch.empty(nb, dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.check(L.nir_seq2seq_pack_gen_frag(lib.ptr(W), VT, K, lib.ptr(frag), lib.ptr(flag), lib.stream()), "nir_seq2seq_pack_gen_frag")
    f = int(flag.item())
    return (frag if f == 0 else None), f


def _gen_argmax(x, W, b, frag, lut=None, V=None, stride=1):
    L = lib.load()
    rows, K = x.shape
    VT = W.shape[0]
    V = VT if V is None else V
    xd, Wd = x.to(DEV).contiguous(), W.to(DEV).contiguous()
    bd = b.to(DEV).contiguous() if b is not None else None
    ld = lut.to(DEV) if lut is not None else None
    ws = torch.empty(max(1, L.nir_seq2seq_gen_argmax_workspace_bytes(rows, K, VT, 1 if frag is not None else 0)), dtype=torch.uint8, device=DEV)
    pred = torch.full((rows, stride), -7, dtype=torch.int64, device=DEV)
    nxt = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    rc = L.nir_seq2seq_gen_argmax(lib.ptr(xd), rows, K, lib.ptr(Wd), lib.ptr(bd), lib.ptr(frag), VT, lib.ptr(ld), V, lib.ptr(ws), ws.numel(),
                                  lib.ptr(pred), stride, lib.ptr(nxt), lib.stream())
    torch.cuda.synchronize()
    return rc, pred.cpu(), nxt.cpu()


def _planted(g, rows, K, VT, winners, twin=None, bias_delta=0.0):
    """x [rows, K], W [VT, K], b [VT] (float32) whose float64 logits have row r's maximum at winners[r], ahead of every other index by at least
    1e-3 of the row's largest |logit|.  twin = (i, j, rows_): W[j] = W[i] and b[j] = b[i] + bias_delta; the rows in rows_ are planted on i."""
    W = torch.randn(VT, K, generator=g)
    W = W / W.norm(dim=1, keepdim=True)                                    # unit rows: a row's logit along another row's direction is their cosine
    b = torch.randn(VT, generator=g) * 0.1
    if twin is not None:
        i, j, _ = twin
        W[j] = W[i]
        b[j] = b[i] + bias_delta
    # 8 along the winner's weight row (the others get 8 cos) on top of a random part of order 0.3 per logit
    x = (0.3 * torch.randn(rows, K, generator=g).double() + 8.0 * W[winners].double()).float()
    dots = x.double() @ W.double().t()
    if twin is not None:
        # the twins' weight rows are the same numbers, so their products are the same number; a blocked float64 GEMM may still sum column j in
        # another order than column i and differ in the last bit, which would turn the reference's exact tie into a 1e-16 preference
        dots[:, twin[1]] = dots[:, twin[0]]
    logits = dots + b.double()
    return x, W, b, logits


def _check_planted(logits, winners, pred, allow_equal=None):
    top = logits.max(1).values
    others = logits.clone()
    others[torch.arange(logits.shape[0]), winners] = float("-inf")
    if allow_equal is not None:
        others[:, allow_equal] = float("-inf")
    gap = top - others.max(1).values
    scale = logits.abs().max(1).values
    assert bool((logits.argmax(1) == winners).all() or allow_equal is not None)
    assert bool((gap >= 1e-3 * scale).all()), (gap / scale).min()          # the planted gap: no row is excluded
    assert torch.equal(pred, winners), (pred, winners)


# (544, 200): the fp32 staging at two row tiles a workgroup with a last chunk of k-steps that is not full
@pytest.mark.parametrize("K,VT", [(K, VT) for VT in (17, 200, 4099) for K in (32, 96, 512, 1024)] + [(544, 200)])
def test_generator_argmax_planted_winners(K, VT):
    g = torch.Generator().manual_seed(7 * K + VT)
    lut = torch.randperm(VT, generator=g)
    for rows in (1, 5, 97):
        # winners at index 0, at VT - 1, inside the last (zero-padded) vocabulary tile, anywhere
        winners = torch.randint(0, VT, (rows,), generator=g)
        winners[0] = 0 if rows == 1 else VT - 1
        if rows > 1:
            winners[1] = 0
            winners[2] = (VT - 1) // 16 * 16
            winners[3] = max(0, VT - 2)
        x, W, b, logits = _planted(g, rows, K, VT, winners)
        frag, flag = _pack(W.to(DEV))
        assert frag is not None and flag == 0
        rc, pred, nxt = _gen_argmax(x, W, b, frag, lut, V=VT - 3, stride=3)
        assert rc == 0
        _check_planted(logits, winners, pred[:, 0])
        assert bool((pred[:, 1:] == -7).all())                            # the prediction stride's other columns are not written
        want = lut[winners]
        assert torch.equal(nxt, torch.where(want < VT - 3, want, torch.ones_like(want)))          # a token without a source row is fed back as <unk>
        rc2, pred2, _ = _gen_argmax(x, W, b, frag, lut, V=VT - 3, stride=3)
        assert rc2 == 0 and torch.equal(pred2, pred)


@pytest.mark.parametrize("K,VT", [(64, 200), (512, 4099)])
def test_generator_argmax_bias_decides_and_ties_go_to_the_first_index(K, VT):
    g = torch.Generator().manual_seed(K + VT)
    rows = 5
    i, j = 5, VT - 2                                                       # two identical weight rows, in different tiles (and ranges)
    for delta, winner in ((0.05, j), (-0.05, i), (0.0, i)):
        winners = torch.full((rows,), i, dtype=torch.long)
        x, W, b, logits = _planted(g, rows, K, VT, winners, twin=(i, j, None), bias_delta=delta)
        frag, _ = _pack(W.to(DEV))
        assert frag is not None
        want = torch.full((rows,), winner, dtype=torch.long)
        if delta == 0.0:
            assert bool((logits[:, i] == logits[:, j]).all())              # an exact tie: the first index wins, like torch.max
        rc, pred, _ = _gen_argmax(x, W, b, frag)
        assert rc == 0
        # every other index is behind by the planted gap; between the twins the bias alone decides (|delta| = 0.05 is >= 1e-3 of the logits here)
        _check_planted(logits, want, pred[:, 0], allow_equal=[i, j])
        if delta != 0.0:
            assert bool(((logits[:, i] - logits[:, j]).abs() >= 1e-3 * logits.abs().max(1).values).all())
        # the unfused path gives the same answer
        rc, pred_g, _ = _gen_argmax(x, W, b, None)
        assert rc == 0 and torch.equal(pred_g[:, 0], want)


def test_every_fallback_condition_takes_the_gemm_path():
    L = lib.load()
    g = torch.Generator().manual_seed(5)
    rows, VT = 5, 200
    # (a) K % 32 != 0: no fused form
    winners = torch.randint(0, VT, (rows,), generator=g)
    x, W, b, logits = _planted(g, rows, 48, VT, winners)
    assert L.nir_seq2seq_gen_frag_bytes(VT, 48) == 0 and L.nir_seq2seq_gen_frag_bytes(VT, 1056) == 0
    assert _pack(W.to(DEV)) == (None, 0)
    rc, pred, _ = _gen_argmax(x, W, b, None)
    assert rc == 0
    _check_planted(logits, winners, pred[:, 0])
    # (b) |w| >= 2^15: the pack raises bit 1 of its flag, the caller leaves the fragments out
    x, W, b, logits = _planted(g, rows, 64, VT, winners)
    W[7, 3] = 40000.0
    x[:, 3] = 1.0
    logits = x.double() @ W.double().t() + b.double()
    w7 = logits.argmax(1)
    frag, flag = _pack(W.to(DEV))
    assert frag is None and flag == 2
    rc, pred, _ = _gen_argmax(x, W, b, None)
    assert rc == 0
    _check_planted(logits, w7, pred[:, 0])
    # (c) the switch: fragments given, exact_f32 on -> the same call takes the fp32 path (its workspace is the larger one)
    x, W, b, logits = _planted(g, rows, 64, VT, winners)
    frag, _ = _pack(W.to(DEV))
    with lib.tunable("exact_f32", 1, 0):
        small = torch.empty(L.nir_seq2seq_gen_argmax_workspace_bytes(rows, 64, VT, 0) - 256, dtype=torch.uint8, device=DEV)
        pred = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
        nxt = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
        xd, Wd, bd = x.to(DEV), W.to(DEV), b.to(DEV)
        rc = L.nir_seq2seq_gen_argmax(lib.ptr(xd), rows, 64, lib.ptr(Wd), lib.ptr(bd), lib.ptr(frag), VT, None, VT, lib.ptr(small), small.numel(),
                                      lib.ptr(pred), 1, lib.ptr(nxt), lib.stream())
        torch.cuda.synchronize()
        assert rc == -3 and bool((pred == -7).all())                       # NIR_ERR_WORKSPACE: the GEMM path's logits do not fit
        rc, pred, _ = _gen_argmax(x, W, b, None)
        assert rc == 0
        _check_planted(logits, winners, pred[:, 0])
    rc, pred, _ = _gen_argmax(x, W, b, frag)
    assert rc == 0
    _check_planted(logits, winners, pred[:, 0])


# ---- argument checks -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_untouched():
    import seq2seq_ref as R
    L = lib.load()
    g = torch.Generator().manual_seed(3)
    B, QL, H = 3, 5, 8
    q, h, mem = torch.randn(B, H, generator=g), torch.randn(B, H, generator=g), torch.randn(B, QL, H, generator=g)
    lens = torch.tensor([5, 2, 1])
    d = [t.to(DEV) for t in (q, h, mem, lens)]
    for QLx, Hx, kind, stride, v in ((QL, 6, 1, QL, None), (0, H, 1, QL, None), (QL, H, 3, QL, None), (QL, H, 2, QL, None), (QL, H, 1, QL - 1, None)):
        cat = torch.full((B, 2 * H), -7.0, device=DEV)
        attn = torch.full((B, QL), -7.0, device=DEV)
        rc = L.nir_seq2seq_attend(lib.ptr(d[0]), lib.ptr(d[1]), lib.ptr(d[2]), lib.ptr(d[2]), v, lib.ptr(d[3]), B, QLx, Hx, kind, lib.ptr(cat), lib.ptr(attn),
                                  stride, lib.stream())
        torch.cuda.synchronize()
        assert rc == BAD_ARG and bool((cat == -7.0).all()) and bool((attn == -7.0).all()), (QLx, Hx, kind, stride)
    # generator: K not a multiple of 4, no vocabulary, a zero prediction stride
    x, W = torch.randn(B, 8, generator=g).to(DEV), torch.randn(10, 8, generator=g).to(DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    for K, VT, stride in ((6, 10, 1), (8, 0, 1), (8, 10, 0)):
        pred = torch.full((B,), -7, dtype=torch.int64, device=DEV)
        nxt = torch.full((B,), -7, dtype=torch.int64, device=DEV)
        rc = L.nir_seq2seq_gen_argmax(lib.ptr(x), B, K, lib.ptr(W), None, None, VT, None, 10, lib.ptr(ws), ws.numel(), lib.ptr(pred), stride, lib.ptr(nxt),
                                      lib.stream())
        torch.cuda.synchronize()
        assert rc == BAD_ARG and bool((pred == -7).all()) and bool((nxt == -7).all()), (K, VT, stride)
    assert L.nir_seq2seq_pack_gen_frag(lib.ptr(W), 10, 8, lib.ptr(ws), None, lib.stream()) == BAD_ARG          # K = 8 has no fragment form
    # the whole decode: BOS outside the vocabulary, max_len 0, an odd embedding width, one fold pointer without the other, a short workspace
    net, c, arrs = R.case("general")
    net = net.to(DEV)
    w = net._decoder_weights()
    Bq, QLq = 5, 7
    table = net.embedder.word_embeddings.table.detach()
    Hn = net.nhid
    dh, dc, bank = torch.zeros(Bq, Hn, device=DEV), torch.zeros(Bq, Hn, device=DEV), torch.zeros(Bq, QLq, Hn, device=DEV)
    sl = torch.full((Bq,), 3, dtype=torch.int64, device=DEV)
    need = L.nir_seq2seq_decode_workspace_bytes(Bq, QLq, w.ref())
    assert need > 0 and L.nir_seq2seq_decode_workspace_bytes(Bq, 0, w.ref()) == 0
    wsd = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(V=table.shape[0], E=table.shape[1], bos=2, max_len=4, ws_bytes=need, ref=None):
        pred = torch.full((Bq, 4), -7, dtype=torch.int64, device=DEV)
        att = torch.full((Bq, 4, QLq), -7.0, device=DEV)
        rc = L.nir_seq2seq_decode_greedy(lib.ptr(dh), lib.ptr(dc), lib.ptr(bank), lib.ptr(sl), Bq, QLq, lib.ptr(table), V, E, None, bos, max_len,
                                         ref if ref is not None else w.ref(), lib.ptr(wsd), ws_bytes, lib.ptr(pred), lib.ptr(att), lib.stream())
        torch.cuda.synchronize()
        return rc, bool((pred == -7).all()) and bool((att == -7.0).all())
    assert call(bos=table.shape[0]) == (BAD_ARG, True)
    assert call(max_len=0) == (BAD_ARG, True)
    assert call(E=table.shape[1] - 2) == (BAD_ARG, True)
    assert call(ws_bytes=need - 256) == (-3, True)
    half = type(w.struct).from_buffer_copy(w.struct)                       # (copy.copy refuses a ctypes structure that holds pointers)
    half.rnn_gate_fold = None
    assert call(ref=lib.C.byref(half)) == (BAD_ARG, True)
    bad = type(w.struct).from_buffer_copy(w.struct)
    bad.attn_type = 2                                                      # mlp without its weights
    assert call(ref=lib.C.byref(bad)) == (BAD_ARG, True)
    rc, untouched = call()
    assert rc == 0 and not untouched
