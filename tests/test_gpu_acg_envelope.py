"""GPU (-m gpu): the kernels of csrc/acg.hip at the C ABI against float64, across their envelope.

Statistics (the STATS form of s2s_gen_argmax_kernel, and the plain GEMM + acg_row_stats_kernel), read through nir_acg_gen_select's optional
outputs: K in {32, 96, 512, 1024} x VT in {17, 200, 4099} x rows in {1, 5, 97} (both row-tile widths, a padded last tile, more than one
vocabulary range, more than one row block), and K = 544 at VT = 200 (two row tiles a workgroup with a last chunk of k-steps that is not
full).  The arg-max is planted with a float64 gap of at least 1e-3 of the row's largest |logit|; from 5
rows on a batch holds a row whose logits ascend along v (every tile moves the running maximum), one that descends, one with a spread above 60,
and one whose other logits are all negative so that PAD (-1e-20) wins; the RAW PAD logit is the largest of every row through its bias and must
neither win nor count.  lse = max + log(sum): with e = |lse - lse64| relative to the row's largest |logit| and e_chain the same chain in
float32 on the CPU,   e <= MARGIN * max(e_chain, 2^-23) + FMT   (FMT: gemm_ref's fp16x2 for the fused form, f32 for the plain one).

Select (acg_select_kernel): every winner class planted in float64 with a relative gap of at least 1e-3, none excluded -- generator winner,
out-of-vocabulary slot, a collapsed winner neither of whose parts wins alone, a repeated source word, two slots sharing one target id, slots
0 / 1 never collapsed, saturated switch both ways, an exact tie (the lower id wins) -- with garbage map indices and attention values at
j >= len in every row, the next token through tgt2src, through ext2src, and out of range (-> 1); QL in {1, 7, 33} x CV in {3, QL + 2} x
rows in {1, 5, 70}.

Loss rows (nir_acg_copy_loss_fwd / _bwd): forward and the three gradients for VT in {17, 4099} x R in {1, 37}, every combination of
al = UNK / other and t in {PAD, UNK, other}, both force_copy values, a row with out = 1e-20.

Bad arguments return NIR_ERR_BAD_ARG and leave a sentinel untouched."""
import pytest
import torch

import gemm_ref
from context_attentive_ir_amd import lib
from test_gpu_seq2seq_envelope import _pack

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG = -1
EPS = gemm_ref.EPS
# the house rule (gemm_ref.py): the largest ratio (e - FMT) / max(e_chain, 2^-23) measured on the MI355X, doubled, up to a power of two, never
# above MARGIN_CAP.  Measured: statistics fused -0.25 (inside the format term), plain 2.08 (K = 1024, VT = 4099, 97 rows: the fp32
# GEMM's summation order); loss rows: loss 1.38, dlogits 3.10 (the rounding of the saved fp32 lse), d switch 0.77, d mass 1.22.  The largest, doubled,
# asks for more than the cap: the margin is the cap and DESIGN.md explains the two figures above 2.
MARGIN = 4.0
PAD_LOGIT = -1e-20


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _gen_select(o, W, b, frag, copy_w, copy_b, attn, lens, smap, e2t, e2s, lut=None, V=None, stride=1, stats=True):
    """one nir_acg_gen_select call -> (rc, pred [rows], next [rows], max [rows], lse [rows], idx [rows]) on the CPU"""
    L = lib.load()
    rows, K = o.shape
    VT, QL, CV = W.shape[0], attn.shape[1], e2t.shape[1]
    V = VT if V is None else V
    d = [_dev(t) for t in (o, W, b, copy_w, copy_b, attn, lens, smap, e2t, e2s, lut)]
    ws = torch.empty(max(1, L.nir_acg_gen_select_workspace_bytes(rows, K, VT, 1 if frag is not None else 0)), dtype=torch.uint8, device=DEV)
    pred = torch.full((rows, stride), -7, dtype=torch.int64, device=DEV)
    nxt = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    smax, slse = torch.full((rows,), -7.0, device=DEV), torch.full((rows,), -7.0, device=DEV)
    sidx = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    rc = L.nir_acg_gen_select(lib.ptr(d[0]), rows, K, lib.ptr(d[1]), lib.ptr(d[2]), lib.ptr(frag), VT, lib.ptr(d[3]), lib.ptr(d[4]), lib.ptr(d[5]),
                              attn.shape[1], lib.ptr(d[6]), QL, lib.ptr(d[7]), lib.ptr(d[8]), lib.ptr(d[9]), CV, lib.ptr(d[10]), V, lib.ptr(ws),
                              ws.numel(), lib.ptr(pred), stride, lib.ptr(nxt), lib.ptr(smax) if stats else None, lib.ptr(slse) if stats else None,
                              lib.ptr(sidx) if stats else None, lib.stream())
    torch.cuda.synchronize()
    return rc, pred.cpu(), nxt.cpu(), smax.cpu(), slse.cpu(), sidx.cpu()


# ---- statistics ------------------------------------------------------------------------------------------------------------------------------
def _stat_inputs(g, rows, K, VT):
    """x [rows, K], W [VT, K], b [VT] (float32) and the planted arg-max of every row.  Feature 0 of W is a ramp v / (VT - 1), feature 1 is 1
    for every v, the rest of a weight row has unit length: x = 8 W[winner] + noise puts the winner 8 (1 - cos) ahead; a row's entry at
    feature 0 tilts its logits along v, its entry at feature 1 shifts them all."""
    W = torch.randn(VT, K, generator=g)
    W[:, :2] = 0
    W = W / W.norm(dim=1, keepdim=True)
    W[:, 0] = torch.arange(VT) / max(VT - 1, 1)
    W[:, 1] = 1.0
    b = torch.randn(VT, generator=g) * 0.1
    b[0] = 50.0                                                             # the raw PAD logit is the largest of every row
    winners = torch.randint(1, VT, (rows,), generator=g)
    tilt, shift = torch.zeros(rows), torch.zeros(rows)
    winners[0] = VT - 1
    if rows >= 5:
        winners[1], tilt[1] = VT - 1, 30.0                                  # ascending along v
        winners[2], tilt[2] = 1, -30.0                                      # descending
        winners[3], tilt[3] = VT - 1, 70.0                                  # spread >= 60
        winners[4], shift[4] = 0, -60.0                                     # every other logit negative: PAD wins
        if rows > 6:
            winners[5] = (VT - 1) // 16 * 16                                # first row of the padded last tile
            winners[6] = max(1, VT - 2)
    x = 0.3 * torch.randn(rows, K, generator=g).double()
    x[:, :2] = 0
    plant = 8.0 * W[winners].double()
    plant[:, :2] = 0
    plant[winners == 0] = 0                                                 # (PAD is not planted through the weights)
    x = x + plant
    x[:, 0], x[:, 1] = tilt.double(), shift.double()
    return x.float(), W, b, winners


def _stat_ref(x, W, b, dt):
    l = x.to(dt) @ W.to(dt).t() + b.to(dt)
    l[:, 0] = PAD_LOGIT
    return l, torch.logsumexp(l, 1)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "plain"])
# (544, 200): the fp32 staging at two row tiles a workgroup with a last chunk of k-steps that is not full
@pytest.mark.parametrize("K,VT", [(K, VT) for VT in (17, 200, 4099) for K in (32, 96, 512, 1024)] + [(544, 200)])
def test_statistics_against_fp64(K, VT, fused):
    assert MARGIN <= gemm_ref.MARGIN_CAP
    g = torch.Generator().manual_seed(11 * K + VT)
    fmt = gemm_ref.FMT["fp16x2" if fused else "f32"]
    worst = 0.0
    for rows in (1, 5, 97):
        x, W, b, winners = _stat_inputs(g, rows, K, VT)
        frag = None
        if fused:
            frag, flag = _pack(W.to(DEV))
            assert frag is not None and flag == 0
        l64, lse64 = _stat_ref(x, W, b, torch.float64)
        lse32 = _stat_ref(x, W, b, torch.float32)[1]
        scale = l64.abs().max(1).values
        top = l64.max(1).values
        others = l64.clone()
        others[torch.arange(rows), winners] = float("-inf")
        assert torch.equal(l64.argmax(1), winners)
        assert bool(((top - others.max(1).values) >= 1e-3 * scale).all())   # the planted gap: no row is excluded
        if rows >= 5:
            assert float(l64[3].max() - l64[3].min()) >= 60 and float(l64[4, 1:].max()) < 0 and bool((l64[1, -1] > l64[1, 1]) and (l64[2, 1] > l64[2, -1]))
        # the switch is shut (z ~ 1e-13) and nothing is collapsed: the prediction is the generator's own arg-max
        one = torch.ones(rows, 1)
        rc, pred, nxt, smax, slse, sidx = _gen_select(x, W, b, frag, torch.zeros(K), torch.tensor([-30.0]), one, one.long().view(-1), 0 * one.long(),
                                                      torch.full((rows, 2), -1), torch.ones(rows, 2).long())
        assert rc == 0
        assert torch.equal(sidx, winners) and torch.equal(pred[:, 0], winners) and torch.equal(nxt, winners)
        l32, _ = _stat_ref(x, W, b, torch.float32)
        assert float(((smax.double() - top).abs() / scale).max()) <= MARGIN * max(float(((l32.max(1).values.double() - top).abs() / scale).max()), EPS) + fmt
        e = float(((slse.double() - lse64).abs() / scale).max())
        e_chain = float(((lse32.double() - lse64).abs() / scale).max())
        ratio = (e - fmt) / max(e_chain, EPS)
        worst = max(worst, ratio)
        print("acg stats %s K=%d VT=%d rows=%d: e %.3g e_chain %.3g ratio %.3f" % ("fused" if fused else "plain", K, VT, rows, e, e_chain, ratio))
        assert e <= MARGIN * max(e_chain, EPS) + fmt, (K, VT, rows, e, e_chain)
    print("acg stats %s K=%d VT=%d: worst ratio %.3f" % ("fused" if fused else "plain", K, VT, worst))


def test_statistics_fall_back_to_the_plain_form():
    """K not a multiple of 32, K above 1024 and the tunable exact_f32 run the GEMM form (frag given or not): same winners"""
    L = lib.load()
    g = torch.Generator().manual_seed(5)
    for K, VT in ((36, 200), (1056, 17)):
        x, W, b, winners = _stat_inputs(g, 5, K, VT)
        assert L.nir_seq2seq_gen_frag_bytes(VT, K) == 0
        one = torch.ones(5, 1)
        rc, pred, _, _, slse, sidx = _gen_select(x, W, b, None, torch.zeros(K), torch.tensor([-30.0]), one, one.long().view(-1), 0 * one.long(),
                                                 torch.full((5, 2), -1), torch.ones(5, 2).long())
        assert rc == 0 and torch.equal(sidx, winners) and torch.equal(pred[:, 0], winners)
    x, W, b, winners = _stat_inputs(g, 5, 64, 200)
    frag, _ = _pack(W.to(DEV))
    one = torch.ones(5, 1)
    args = (x, W, b, frag, torch.zeros(64), torch.tensor([-30.0]), one, one.long().view(-1), 0 * one.long(), torch.full((5, 2), -1), torch.ones(5, 2).long())
    fast = _gen_select(*args)
    assert L.nir_debug_set_tunable(b"exact_f32", 1) == 0
    try:
        exact = _gen_select(*args)
    finally:
        L.nir_debug_set_tunable(b"exact_f32", 0)
    assert fast[0] == 0 and exact[0] == 0 and torch.equal(fast[5], winners) and torch.equal(exact[5], winners)
    _, lse64 = _stat_ref(x, W, b, torch.float64)
    _, lse32 = _stat_ref(x, W, b, torch.float32)
    assert float((exact[4].double() - lse64).abs().max()) <= MARGIN * max(float((lse32.double() - lse64).abs().max()), EPS * float(lse64.abs().max()))


# ---- select ----------------------------------------------------------------------------------------------------------------------------------
SEL_K, SEL_VT = 64, 40            # generator rows are unit vectors of the first 40 features: logit v of a row is o[v] + b[v] (+ small noise)
CLASSES = ("generator", "oov", "collapsed", "repeated", "shared", "slot01", "sat_copy", "sat_gen", "tie")


def _feasible(cls, QL, CV):
    need = {"generator": (1, 3), "oov": (1, 3), "collapsed": (2, 3), "repeated": (3, 3), "shared": (3, 4), "slot01": (1, 3), "sat_copy": (1, 3),
            "sat_gen": (1, 3), "tie": (2, 3)}[cls]
    return QL >= need[0] and CV >= need[1]


def _select_inputs(g, rows, QL, CV):
    """per row one class of CLASSES (cycled; a class that does not fit QL / CV gives way to "oov"): logits [rows, VT], switch logit [rows],
    attention [rows, QL], lengths, the three index tensors, the class names"""
    VT = SEL_VT
    logit = -4.0 + 0.2 * torch.randn(rows, VT, generator=g).double()
    zl = torch.zeros(rows).double()
    attn = torch.zeros(rows, QL).double()
    lens = torch.zeros(rows, dtype=torch.long)
    smap = torch.zeros(rows, QL, dtype=torch.long)
    e2t = torch.full((rows, CV), -1, dtype=torch.long)
    e2s = torch.randint(4, 300, (rows, CV), generator=g)
    names = []
    for r in range(rows):
        cls = CLASSES[r % len(CLASSES)]
        if not _feasible(cls, QL, CV):
            cls = "oov"
        names.append(cls)
        n = int(torch.randint(max(1, min(QL, 3)), QL + 1, (1,), generator=g))
        lens[r] = n
        gw, t = 5 + r % 7, 20 + r % 9                                        # the generator's own winner; a target a slot collapses onto
        logit[r, gw] = 2.0
        rest = torch.rand(n, generator=g).double() * 0.01                   # a little attention everywhere, on slot 0
        a = rest.clone()
        if cls in ("generator", "sat_gen"):
            zl[r] = -6.0 if cls == "generator" else -40.0
            a[0] += 1.0
            smap[r, 0] = 2 if CV > 2 else 1
        elif cls in ("oov", "sat_copy"):
            zl[r] = 4.0 if cls == "oov" else 40.0
            a[n - 1] += 1.0
            smap[r, n - 1] = CV - 1                                          # the last slot, not collapsed
        elif cls == "collapsed":                                            # P[gw] = .25, slot 1 = .275, P[t] = .20 + .225: neither part alone
            zl[r] = 0.0
            logit[r, t] = 2.0 + float(torch.log(torch.tensor(0.8)))
            a[0] += 0.55
            a[1] += 0.45
            smap[r, 0], smap[r, 1] = 1, 2
            e2t[r, 2] = t
        elif cls == "repeated":                                             # slot 2 at two positions: .3 + .3 beats slot 1's .4 only as a sum
            zl[r] = 4.0
            a[0] += 0.3
            a[1] += 0.4
            a[2] += 0.3
            smap[r, 0], smap[r, 1], smap[r, 2] = 2, 1, 2
        elif cls == "shared":                                               # slots 2 and 3 collapse onto one t: .3 + .3 beats slot 1's .4 only accumulated
            zl[r] = 4.0
            a[0] += 0.3
            a[1] += 0.4
            a[2] += 0.3
            smap[r, 0], smap[r, 1], smap[r, 2] = 2, 1, 3
            e2t[r, 2] = e2t[r, 3] = t
        elif cls == "slot01":                                               # the mass sits on slot 1, whose ext2tgt entry must be ignored
            zl[r] = 4.0
            a[0] += 1.0
            smap[r, 0] = r % 2
            e2t[r, 0] = e2t[r, 1] = t
        elif cls == "tie":                                                  # slots 1 and 2 hold the same mass exactly: the lower id wins
            zl[r] = 4.0
            a[:] = 0
            a[0] = a[1] = 0.5
            smap[r, 0], smap[r, 1] = 2, 1
        attn[r, :n] = a / a.sum()
        if cls == "tie":
            attn[r, :n] = a
        # garbage behind the length: never read
        attn[r, n:] = 0.77
        smap[r, n:] = torch.tensor([10 ** 9, -5, 2, CV - 1] * QL)[:QL - n]
    return logit, zl, attn.float(), lens, smap, e2t, e2s, names


def _select_ref(l, zl, attn, lens, smap, e2t):
    """float64: the whole extended distribution, collapsed -> P [rows, VT + CV]"""
    rows, VT = l.shape
    CV = e2t.shape[1]
    l = l.clone()
    l[:, 0] = PAD_LOGIT
    s = torch.softmax(l, 1)
    z = torch.sigmoid(zl).unsqueeze(1)
    omz = torch.sigmoid(-zl).unsqueeze(1)
    copy = torch.zeros(rows, CV, dtype=torch.float64)
    for r in range(rows):
        for j in range(int(lens[r])):
            copy[r, int(smap[r, j])] += z[r, 0] * attn[r, j].double()
    P = torch.cat([omz * s, copy], 1)
    for r in range(rows):
        for c in range(2, CV):
            if int(e2t[r, c]) >= 0:
                P[r, int(e2t[r, c])] += P[r, VT + c]
                P[r, VT + c] = 1e-10
    return P


@pytest.mark.parametrize("rows", [1, 5, 70])
@pytest.mark.parametrize("QL", [1, 7, 33])
def test_select_planted_winner_classes(QL, rows):
    K, VT = SEL_K, SEL_VT
    W = torch.zeros(VT, K)
    W[torch.arange(VT), torch.arange(VT)] = 1.0
    frag, flag = _pack(W.to(DEV))
    assert frag is not None and flag == 0
    copy_w = torch.zeros(K)
    copy_w[K - 1] = 8.0                                                     # the switch reads feature K - 1 alone
    seen = set()
    for CV in sorted({3, QL + 2}):
        g = torch.Generator().manual_seed(1000 * QL + 10 * rows + CV)
        b = torch.randn(VT, generator=g) * 0.1
        V = 200
        lut = torch.randint(0, 260, (VT,), generator=g)                     # some target words have no source row: fed back as <unk>
        for start in range(len(CLASSES) if rows < len(CLASSES) else 1):     # fewer rows than classes: rotate so that every class is run
            logit, zl, attn, lens, smap, e2t, e2s, names = _select_inputs(g, rows + start, QL, CV)
            logit, zl, attn, lens, smap, e2t, e2s, names = (t[start:] for t in (logit, zl, attn, lens, smap, e2t, e2s, names))
            e2s[::3] = 250                                                   # out of [0, V): <unk>
            o = torch.zeros(rows, K)
            o[:, :VT] = (logit - b.double()).float()
            o[:, K - 1] = (zl / 8.0).float()
            # the inputs as the kernel sees them, in float64
            l64 = o[:, :VT].double() + b.double()
            zl64 = o[:, K - 1].double() * 8.0
            P = _select_ref(l64, zl64, attn, lens, smap, e2t)
            top2 = P.topk(2, 1)
            want = P.argmax(1)
            gap = (top2.values[:, 0] - top2.values[:, 1]) / top2.values[:, 0]
            for r, cls in enumerate(names):
                seen.add(cls)
                if cls == "tie":
                    assert gap[r] == 0 and sorted(top2.indices[r].tolist()) == [VT + 1, VT + 2]
                    want[r] = VT + 1
                    third = P[r].topk(3).values[2]
                    assert float((P[r, VT + 1] - third) / P[r, VT + 1]) >= 1e-3
                else:
                    assert float(gap[r]) >= 1e-3, (cls, float(gap[r]))       # planted: no row is excluded
                gw, t = 5 + (r + start) % 7, 20 + (r + start) % 9
                expect = {"generator": gw, "sat_gen": gw, "oov": VT + CV - 1, "sat_copy": VT + CV - 1, "collapsed": t, "repeated": VT + 2, "shared": t,
                          "slot01": VT + (r + start) % 2, "tie": VT + 1}[cls]
                assert int(want[r]) == expect, (cls, int(want[r]), expect)
            rc, pred, nxt, _, _, sidx = _gen_select(o, W, b, frag, copy_w, torch.zeros(1), attn, lens, smap, e2t, e2s, lut, V, stride=2)
            assert rc == 0
            assert torch.equal(pred[:, 0], want), (names, pred[:, 0], want)
            assert bool((pred[:, 1] == -7).all())
            tok = torch.where(want < VT, lut[want.clamp(max=VT - 1)], e2s[torch.arange(rows), (want - VT).clamp(min=0)])
            tok = torch.where((tok >= 0) & (tok < V), tok, torch.ones_like(tok))
            assert torch.equal(nxt, tok)
            rc, pred2, nxt2, _, _, _ = _gen_select(o, W, b, None, copy_w, torch.zeros(1), attn, lens, smap, e2t, e2s, None, V, stride=2, stats=False)
            assert rc == 0 and torch.equal(pred2[:, 0], want)                # the plain statistics, identity tgt2src
            tok = torch.where(want < VT, want, e2s[torch.arange(rows), (want - VT).clamp(min=0)])
            assert torch.equal(nxt2, torch.where((tok >= 0) & (tok < V), tok, torch.ones_like(tok)))
    if QL >= 3:
        assert seen == set(CLASSES), seen


# ---- loss rows -----------------------------------------------------------------------------------------------------------------------------
def _loss_ref(z, sw, ms, t, al, force, g, dt):
    """(loss, dlogits, dswitch, dmass) and, for the float64 call, the scale every element's error is measured against"""
    z, sw, ms = (x.detach().to(dt).requires_grad_(True) for x in (z, sw, ms))
    l = torch.cat([torch.full_like(z[:, :1], PAD_LOGIT), z[:, 1:]], 1)
    st = torch.softmax(l, 1).gather(1, t.unsqueeze(1)).squeeze(1)
    zz, omz = torch.sigmoid(sw), torch.sigmoid(-sw)
    anu, au = (al != 1).to(dt), (al == 1).to(dt)
    w = au if force else (t != 1).to(dt) + au * (t == 1).to(dt)
    out = anu * zz * ms + 1e-20 + w * omz * st
    loss = -out.log()
    loss.backward(g.to(dt))
    with torch.no_grad():
        # loss: absolute below 1; dlogits: a row's largest entry; dswitch: the sum of the magnitudes of its two cancelling terms; dmass: itself
        scales = (loss.abs().clamp(min=1.0), z.grad.abs().max(1, keepdim=True).values.expand_as(z.grad),
                  g.to(dt) * (anu * ms + w * st) * zz * omz / out, ms.grad.abs())
    return (loss.detach(), z.grad, sw.grad, ms.grad), scales


def _err(got, ref, scale):
    """max_i |got_i - ref_i| / scale_i; where the scale is 0 the value has to be exactly the reference's"""
    got, ref, scale = got.double(), ref.double(), scale.double()
    d = (got - ref).abs()
    live = scale > 0
    assert bool((d[~live] == 0).all())
    return float((d[live] / scale[live]).max()) if bool(live.any()) else 0.0


@pytest.mark.parametrize("force", [False, True])
@pytest.mark.parametrize("R", [1, 37])
@pytest.mark.parametrize("VT", [17, 4099])
def test_copy_loss_rows_against_fp64(VT, R, force):
    L = lib.load()
    g = torch.Generator().manual_seed(VT + R)
    z = 3.0 * torch.randn(R, VT, generator=g)
    sw = 2.0 * torch.randn(R, generator=g)
    ms = torch.rand(R, generator=g)
    r = torch.arange(R)
    t = torch.tensor([0, 1, 7])[(r + 2) % 3]                                # PAD, UNK, other   (R = 1: other)
    al = torch.tensor([1, 5])[(r // 3 + 1) % 2]                             # UNK, other        (R = 1: other)
    if R > 1:
        t[R - 1], al[R - 1], ms[R - 1] = 1, 5, 0.0                          # nothing can be copied, nothing generated: out = 1e-20
        assert {(int(a == 1), int(x)) for a, x in zip(al.tolist(), t.tolist())} == {(a, x) for a in (0, 1) for x in (0, 1, 7)}
    gl = torch.rand(R, generator=g) + 0.5
    zd, swd, msd, td, ald, gd = (_dev(x) for x in (z, sw, ms, t, al, gl))
    loss, lse = torch.full((R,), -7.0, device=DEV), torch.full((R,), -7.0, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    assert L.nir_acg_copy_loss_fwd(lib.ptr(zd), VT, lib.ptr(swd), lib.ptr(msd), lib.ptr(td), lib.ptr(ald), int(force), R, VT, lib.ptr(loss), lib.ptr(lse),
                                   lib.ptr(flag), lib.stream()) == 0
    dz, dsw, dms = torch.full((R, VT), -7.0, device=DEV), torch.full((R,), -7.0, device=DEV), torch.full((R,), -7.0, device=DEV)
    assert L.nir_acg_copy_loss_bwd(lib.ptr(zd), VT, lib.ptr(swd), lib.ptr(msd), lib.ptr(td), lib.ptr(ald), int(force), lib.ptr(lse), lib.ptr(gd), R, VT,
                                   lib.ptr(dz), lib.ptr(dsw), lib.ptr(dms), lib.stream()) == 0
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    ref, scales = _loss_ref(z, sw, ms, t, al, force, gl, torch.float64)
    chain, _ = _loss_ref(z, sw, ms, t, al, force, gl, torch.float32)
    if R > 1:
        assert abs(float(ref[0][R - 1]) - 46.0517) < 1e-3 and abs(float(loss[R - 1]) - 46.0517) < 1e-3
    assert bool((dz[:, 0] == 0).all())                                      # the PAD logit is a constant
    assert bool(torch.isfinite(dz).all() and torch.isfinite(dsw).all() and torch.isfinite(dms).all())
    for name, got, k in (("loss", loss, 0), ("dlogits", dz, 1), ("dswitch", dsw, 2), ("dmass", dms, 3)):
        e, e_chain = _err(got.cpu(), ref[k], scales[k]), _err(chain[k], ref[k], scales[k])
        print("acg loss rows VT=%d R=%d force=%s %s: e %.3g e_chain %.3g ratio %.3f" % (VT, R, force, name, e, e_chain, e / max(e_chain, EPS)))
        assert e <= MARGIN * max(e_chain, EPS), (name, e, e_chain)


# ---- bad arguments -------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_the_outputs_untouched():
    L = lib.load()
    rows, K, VT, QL, CV = 3, 32, 17, 4, 6
    W = torch.randn(VT, K)
    args = dict(o=torch.randn(rows, K), W=W, b=torch.zeros(VT), frag=None, copy_w=torch.zeros(K), copy_b=torch.zeros(1), attn=torch.rand(rows, QL),
                lens=torch.full((rows,), QL), smap=torch.zeros(rows, QL, dtype=torch.long), e2t=torch.full((rows, CV), -1), e2s=torch.ones(rows, CV).long())
    ok = _gen_select(**args)
    assert ok[0] == 0 and bool((ok[1] >= 0).all())
    for bad in (dict(e2t=torch.full((rows, 1), -1), e2s=torch.ones(rows, 1).long()),                   # CV < 2
                dict(e2t=torch.full((rows, 1025), -1), e2s=torch.ones(rows, 1025).long()),              # CV above the kernel's LDS budget
                dict(o=torch.randn(rows, 30), W=torch.randn(VT, 30), copy_w=torch.zeros(30)),           # K % 4 != 0
                dict(V=0)):
        rc, pred, nxt, smax, slse, sidx = _gen_select(**dict(args, **bad))
        assert rc == BAD_ARG
        assert bool((pred == -7).all() and (nxt == -7).all() and (smax == -7).all() and (slse == -7).all() and (sidx == -7).all())
    # a workspace that is too small
    d = [_dev(args[k]) for k in ("o", "W", "b", "copy_w", "copy_b", "attn", "lens", "smap", "e2t", "e2s")]
    pred = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    nxt = torch.full((rows,), -7, dtype=torch.int64, device=DEV)
    ws = torch.empty(64, dtype=torch.uint8, device=DEV)
    rc = L.nir_acg_gen_select(lib.ptr(d[0]), rows, K, lib.ptr(d[1]), lib.ptr(d[2]), None, VT, lib.ptr(d[3]), lib.ptr(d[4]), lib.ptr(d[5]), QL, lib.ptr(d[6]),
                              QL, lib.ptr(d[7]), lib.ptr(d[8]), lib.ptr(d[9]), CV, None, VT, lib.ptr(ws), ws.numel(), lib.ptr(pred), 1, lib.ptr(nxt), None,
                              None, None, lib.stream())
    torch.cuda.synchronize()
    assert rc != 0 and bool((pred == -7).all() and (nxt == -7).all())
    # the decode: CV out of range, a null index tensor, null copy weights
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.recommender import ACG
    net = ACG(default_args("ACG", src_vocab_size=50, tgt_vocab_size=VT, nhid=32, emsize=32)).to(DEV).eval()
    w, cw = net._decoder_weights(), net._copy_weights()
    B, H = rows, 32
    h0, bank = torch.zeros(B, H, device=DEV), torch.zeros(B, QL, H, device=DEV)
    lens = torch.full((B,), QL, device=DEV)
    table = net.embedder.word_embeddings.table.detach().float().contiguous()
    idx, e2t, e2s = (_dev(args[k]) for k in ("smap", "e2t", "e2s"))
    ws = torch.empty(max(1, L.nir_acg_decode_workspace_bytes(B, QL, CV, w.ref(), cw.ref())), dtype=torch.uint8, device=DEV)
    assert L.nir_acg_decode_workspace_bytes(B, QL, 1, w.ref(), cw.ref()) == 0
    for cv, cwref, e2tp in ((1, cw.ref(), lib.ptr(e2t)), (CV, None, lib.ptr(e2t)), (CV, cw.ref(), None)):
        preds = torch.full((B, 2), -7, dtype=torch.int64, device=DEV)
        attns = torch.full((B, 2, QL), -7.0, device=DEV)
        rc = L.nir_acg_decode_greedy(lib.ptr(h0), lib.ptr(h0), lib.ptr(bank), lib.ptr(lens), B, QL, lib.ptr(table), table.shape[0], table.shape[1], None, 2, 2,
                                     w.ref(), cwref, lib.ptr(idx), e2tp, lib.ptr(e2s), cv, lib.ptr(ws), ws.numel(), lib.ptr(preds), lib.ptr(attns),
                                     lib.stream())
        torch.cuda.synchronize()
        assert rc == BAD_ARG and bool((preds == -7).all() and (attns == -7).all())
    # the loss rows: a row stride below V, too many rows for one backward launch
    loss = torch.full((rows,), -7.0, device=DEV)
    z = torch.zeros(rows, VT, device=DEV)
    v = torch.zeros(rows, device=DEV)
    ti = torch.zeros(rows, dtype=torch.int64, device=DEV)
    assert L.nir_acg_copy_loss_fwd(lib.ptr(z), VT - 1, lib.ptr(v), lib.ptr(v), lib.ptr(ti), lib.ptr(ti), 0, rows, VT, lib.ptr(loss), lib.ptr(loss), None,
                                   lib.stream()) == BAD_ARG
    assert L.nir_acg_copy_loss_bwd(lib.ptr(z), VT, lib.ptr(v), lib.ptr(v), lib.ptr(ti), lib.ptr(ti), 0, lib.ptr(v), lib.ptr(v), 65536, VT, lib.ptr(z), lib.ptr(loss),
                                   lib.ptr(loss), lib.stream()) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((loss == -7).all())
