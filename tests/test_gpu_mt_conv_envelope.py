"""GPU (-m gpu): the train-mode MatchTensor convolutions (csrc/mt_conv_train.hip) called through the C ABI -- nir_mt_conv3_supported, _fwd,
_wt_floats, _partial_floats, _bwd -- and the fixed-order column sum that reduces their gradients (nir_colsum_det_f32, as
autograd._MTConv3.backward calls it), against float64 on the case list of tests/mt_conv_ref.py.  Each case asserts:
  * every output tensor (forward rows, dT, dw1..3, db1..3) meets the criterion of mt_conv_ref (fp32-yardstick error times a margin <= 4);
    the `impulse` inputs and the forward of `dead` are bit-exact;
  * the profile report shows mt_conv3_fwd_kernel x 1 for the forward, mt_conv3_bwd_data_kernel x 1 only with dT, mt_conv3_bwd_weight_kernel
    x 1 only with partial, nothing when both are NULL or M = 0;
  * outputs are prefilled with NaN between guard rows holding a sentinel, wt and partial (and the slice buffer of the column sum) have exactly
    the sizes the _floats entries return with a patterned region behind them: no NaN is left, guards and patterns stay intact;
  * a second call gives the same bits on every output, the reduced gradients included.
Every case prints one "MTCONVENV" line per tensor before it asserts.  The eight-call bit check runs at the C ABI and through A.mt_conv3 (the
production call site of the reduction); nir_colsum_det_f32 also runs by itself at the row counts and strides the convolutions do not reach.  The fall-back of the same head, nir_im2col_rows_f32 (copies: bit-equal)
and nir_col2im_rows_f32 (criterion), is held to the same at the end."""
import ctypes as C
import re
import types

import pytest
import torch

import mt_conv_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0
TAIL = 1024
NAN = float("nan")
C1, NF, NCOL, NW = R.C1, R.NF, R.NCOL, R.NW


def _profiled(L, fn):
    buf = C.create_string_buffer(1 << 16)
    L.nir_profile_report(buf, len(buf))                     # drop what earlier tests left
    L.nir_profile_enable(1)
    try:
        rc = fn()
        torch.cuda.synchronize()
    finally:
        L.nir_profile_enable(0)
    L.nir_profile_report(buf, len(buf))
    out = {}
    for ln in buf.value.decode().strip().splitlines():
        name, launches, _ = ln.rsplit(",", 2)
        name = re.sub(r"\[M=[^\]]*\]$", "", name)
        out[name] = out.get(name, 0) + int(launches)
    return rc, out


def _bits(t):
    return t.contiguous().view(torch.int32)


def _same(a, b):
    return all(torch.equal(_bits(a[k]), _bits(b[k])) for k in a) and set(a) == set(b)


class _Buf(object):
    """n floats prefilled with NaN between a sentinel float in front (`lead` of them: 4 keeps torch's alignment, 5 moves the payload 4 bytes
    off it) and TAIL sentinel floats behind"""

    def __init__(self, n, lead=4, fill=NAN):
        self.n, self.lead = n, lead
        self.buf = torch.full((lead + n + TAIL,), SENT, device=DEV)
        self.t = self.buf[lead:lead + n]
        self.t.fill_(fill)

    def load(self, src):
        self.t.copy_(src.reshape(-1))
        return self

    def intact(self):
        return bool((self.buf[:self.lead] == SENT).all()) and bool((self.buf[self.lead + self.n:] == SENT).all())

    def untouched(self):
        return bool(torch.isnan(self.t).all())

    def nans(self):
        return int(torch.isnan(self.t).sum())


class _Call(object):
    """the C entries on one input: device copies, guarded outputs, wt / partial / slice buffers of exactly the sizes the library names"""

    def __init__(self, x, off=0):
        from context_attentive_ir_amd import lib
        self.lib, self.L = lib, lib.load()
        self.M, _, self.H, self.W = x["T"].shape
        M, H, W = self.M, self.H, self.W
        lead = 4 + off
        self.T = _Buf(x["T"].numel(), lead).load(x["T"].to(DEV))
        self.dpre = _Buf(x["dpre"].numel(), lead).load(x["dpre"].to(DEV))
        self.w = [x["w%d" % k].to(DEV) for k in (1, 2, 3)]
        self.b = [x["b%d" % k].to(DEV) for k in (1, 2, 3)]
        self.out = _Buf(M * H * W * NCOL, lead)
        self.dT = _Buf(M * C1 * H * W, lead)
        self.nwt, self.npart = int(self.L.nir_mt_conv3_wt_floats(C1, NF)), int(self.L.nir_mt_conv3_partial_floats(M, C1, NF))
        assert self.nwt == 45 * NF * 52 and self.npart == M * R.MT_XS * NW
        self.wt, self.part = _Buf(self.nwt), _Buf(self.npart)
        self.dw, self.db = _Buf(NW), _Buf(NCOL)
        self.ws_w = _Buf(int(self.L.nir_colsum_det_floats(R.MT_XS * M, NW)))
        self.ws_b = _Buf(int(self.L.nir_colsum_det_floats(M * H * W, NCOL)))
        self.bufs = dict(T=self.T, dpre=self.dpre, out=self.out, dT=self.dT, wt=self.wt, partial=self.part, dw=self.dw, db=self.db, ws_w=self.ws_w, ws_b=self.ws_b)

    def fwd(self, M=None, c1=C1, H=None, W=None, nf=NF, T=True, w1=True, dpre=True):
        p, L = self.lib.ptr, self.L
        args = [p(self.w[0]) if w1 else None, p(self.b[0]), p(self.w[1]), p(self.b[1]), p(self.w[2]), p(self.b[2])]
        return _profiled(L, lambda: L.nir_mt_conv3_fwd(p(self.T.t) if T else None, *args, self.M if M is None else M, c1, H or self.H, W or self.W, nf,
                                                       p(self.out.t), self.lib.stream()))

    def bwd(self, dT=True, partial=True, wt=True, M=None, c1=C1, H=None, W=None, nf=NF, T=True, w1=True, dpre=True):
        p, L = self.lib.ptr, self.L
        return _profiled(L, lambda: L.nir_mt_conv3_bwd(p(self.dpre.t) if dpre else None, p(self.T.t) if T else None, p(self.w[0]) if w1 else None, p(self.w[1]), p(self.w[2]),
                                                       self.M if M is None else M, c1, H or self.H, W or self.W, nf, p(self.dT.t) if dT else None,
                                                       p(self.wt.t) if wt else None, p(self.part.t) if partial else None, self.lib.stream()))

    def reduce(self):
        """dw [NW] and db [3 NF] as autograd._MTConv3.backward forms them"""
        p, L, st = self.lib.ptr, self.L, self.lib.stream()
        M, H, W = self.M, self.H, self.W
        self.lib.check(L.nir_colsum_det_f32(p(self.part.t), NW, R.MT_XS * M, NW, p(self.dw.t), p(self.ws_w.t) if self.ws_w.n else None, st), "nir_colsum_det_f32")
        self.lib.check(L.nir_colsum_det_f32(p(self.dpre.t), NCOL, M * H * W, NCOL, p(self.db.t), p(self.ws_b.t) if self.ws_b.n else None, st), "nir_colsum_det_f32")
        torch.cuda.synchronize()

    def results(self, fwd=True, bwd=True):
        M, H, W = self.M, self.H, self.W
        out = {}
        if fwd:
            out["fwd"] = self.out.t.cpu().reshape(M * H * W, NCOL).clone()
        if bwd:
            out["dT"] = self.dT.t.cpu().reshape(M, C1, H, W).clone()
            out.update({k: v.clone() for k, v in R.split_grads(self.dw.t.cpu(), self.db.t.cpu()).items()})
        return out

    def violations(self):
        return [k for k, b in self.bufs.items() if not b.intact()]

    def run_all(self):
        """forward, backward and reduction once: (launches of the forward, of the backward, results)"""
        rc, ran_f = self.fwd()
        self.lib.check(rc, "nir_mt_conv3_fwd")
        rc, ran_b = self.bwd()
        self.lib.check(rc, "nir_mt_conv3_bwd")
        self.reduce()
        return ran_f, ran_b, self.results()


FWD_ONLY = {"mt_conv3_fwd_kernel": 1}
BWD_BOTH = {"mt_conv3_bwd_data_kernel": 1, "mt_conv3_bwd_weight_kernel": 1}


def _judge(cid, got, p, exact=()):
    """prints one MTCONVENV line per tensor; returns the lines of the tensors that miss the criterion (or bit-exactness for keys of `exact`)"""
    bad = []
    for k in R.KEYS:
        if k not in got:
            continue
        ok, r = R.accept(got[k], k, p)
        line = "MTCONVENV,%s,%s,%s,e=%.3g,e32=%.3g,ratio=%.3f,bound=%.3g" % (cid, R.KERNEL_OF[k], k, r["e"], r["e32"], r["ratio"], r["bound"])
        print(line)
        if k in exact and not torch.equal(_bits(got[k]), _bits(p["ref"][k].float())):
            bad.append(line + " not bit-exact")
        if not ok:
            bad.append(line)
    return bad


@pytest.mark.parametrize("d", R.CASES, ids=lambda d: d["id"])
def test_mt_conv(d):
    x, p = R.prepared(d)
    call = _Call(x)
    assert call.L.nir_mt_conv3_supported(NF, C1, d["H"], d["W"]) == 1
    ran_f, ran_b, got = call.run_all()
    nans = {k: b.nans() for k, b in call.bufs.items() if b.nans()}
    ran_f2, ran_b2, again = call.run_all()
    bad = _judge(d["id"], got, p, exact=("fwd",) if d["fam"] == "dead" else ())
    assert call.violations() == [], "wrote outside: %s" % call.violations()
    assert nans == {}, "NaN left: %s" % nans
    assert ran_f == FWD_ONLY and ran_f2 == FWD_ONLY, (ran_f, ran_f2)
    assert ran_b == BWD_BOTH and ran_b2 == BWD_BOTH, (ran_b, ran_b2)
    assert _same(got, again), "results differ between two calls"
    assert bad == [], "\n".join(bad)
    if d["fam"] == "dead":
        assert float(got["fwd"].abs().max()) == 0.0


@pytest.mark.parametrize("H,W", R.IMPULSE_SHAPES)
def test_impulse_forward_is_bit_exact(H, W):
    x, where = R.impulse_fwd(H, W)
    p = R.prepare(x)
    call = _Call(x)
    rc, ran = call.fwd()
    call.lib.check(rc, "nir_mt_conv3_fwd")
    got = call.results(bwd=False)
    bad = _judge("impulse-fwd-M%d-H%d-W%d" % (len(where), H, W), got, p, exact=("fwd",))
    assert ran == FWD_ONLY and call.violations() == [] and call.out.nans() == 0
    assert bad == [], "\n".join(bad)


@pytest.mark.parametrize("H,W", R.IMPULSE_SHAPES)
def test_impulse_backward_is_bit_exact(H, W):
    x, where = R.impulse_bwd(H, W)
    p = R.prepare(x)
    call = _Call(x)
    rc, ran = call.bwd()
    call.lib.check(rc, "nir_mt_conv3_bwd")
    call.reduce()
    got = call.results(fwd=False)
    bad = _judge("impulse-bwd-M%d-H%d-W%d" % (len(where), H, W), got, p, exact=[k for k in R.KEYS if k != "fwd"])
    # the partial rows themselves: the row of (m, range of x0) holds the tile around the impulse, the other range zeros
    part = call.part.t.cpu().reshape(len(where), R.MT_XS, NW)
    T = x["T"]
    for m, y0, x0, col in where:
        j, g, o = x0 // R.xchunk(W), col // NF, col % NF
        want = torch.zeros(NW)
        base = sum(NF * C1 * 3 * R.KW[k] for k in range(g))
        blk = want[base:base + NF * C1 * 3 * R.KW[g]].view(NF, C1, 3, R.KW[g])
        for dy in range(3):
            for dx in range(R.KW[g]):
                yy, xx = y0 + dy - 1, x0 + dx - (g + 1)
                if 0 <= yy < H and 0 <= xx < W:
                    blk[o, :, dy, dx] = T[m, :, yy, xx]
        assert torch.equal(_bits(part[m, j]), _bits(want)), (m, y0, x0, col)
        assert not bool(part[m, 1 - j].any()), (m, y0, x0, col)
    assert ran == BWD_BOTH and call.violations() == [] and call.dT.nans() == 0 and call.part.nans() == 0
    assert bad == [], "\n".join(bad)


def test_gradient_bits_do_not_change_over_eight_calls():
    """M = 97 at (2, 5): the filter gradient sums 194 partial rows in 4 slices, the bias gradient 970 rows in 16 -- with atomics between the
    slices the order of arrival would show in the last bits.  Necessary, not sufficient: nir_colsum_det_f32 has no atomics by construction."""
    d = R.BY_ID["randn-M97-H2-W5"]
    x, p = R.prepared(d)
    assert R.colsum_slices(R.MT_XS * d["M"])[1] == 4 and R.colsum_slices(d["M"] * d["H"] * d["W"])[1] == 16
    call = _Call(x)
    first = call.run_all()[2]
    for n in range(7):
        assert _same(first, call.run_all()[2]), "call %d gives other bits" % (n + 2)
    assert call.violations() == []


def test_gradient_bits_do_not_change_over_eight_backward_passes_of_autograd():
    """the same through the production call site, A.mt_conv3 and autograd._MTConv3.backward, at M = 97, (2, 5): with nir_colsum_set_f32 there the
    four slices of the filter gradient and the sixteen of the bias gradient meet in atomics and these bits move; the results are also those of
    the C entries called directly"""
    from context_attentive_ir_amd import autograd as A
    d = R.BY_ID["randn-M97-H2-W5"]
    x, p = R.prepared(d)
    names = ("T", "w1", "b1", "w2", "b2", "w3", "b3")

    def run():
        t = {k: x[k].to(DEV).requires_grad_(True) for k in names}
        convs = [types.SimpleNamespace(weight=t["w%d" % k], bias=t["b%d" % k]) for k in (1, 2, 3)]
        out = A.mt_conv3(t["T"], *convs)
        out.backward(x["dpre"].to(DEV))
        torch.cuda.synchronize()
        got = {"dT": t["T"].grad.cpu()}
        for k in (1, 2, 3):
            got["dw%d" % k], got["db%d" % k] = t["w%d" % k].grad.cpu(), t["b%d" % k].grad.cpu()
        return out.detach().cpu(), got

    fwd, first = run()
    for n in range(7):
        assert _same(first, run()[1]), "backward pass %d gives other bits" % (n + 2)
    # the C entries on the same masked gradient give these bits too
    xm = dict(x)
    xm["dpre"] = x["dpre"] * (fwd > 0)
    call = _Call(xm)
    direct = call.run_all()[2]
    assert all(torch.equal(_bits(first[k]), _bits(direct[k])) for k in first)


@pytest.mark.parametrize("cid", ["randn-M3-H4-W33", "randn-M2-H4-W65"])
def test_pointers_four_bytes_off_alignment_give_the_same_bits(cid):
    x, p = R.prepared(R.BY_ID[cid])
    a, b = _Call(x), _Call(x, off=1)
    assert a.T.t.data_ptr() % 16 == 0 and b.T.t.data_ptr() % 16 == 4 and b.out.t.data_ptr() % 16 == 4 and b.dT.t.data_ptr() % 16 == 4 and b.dpre.t.data_ptr() % 16 == 4
    ra, rb = a.run_all()[2], b.run_all()[2]
    assert b.violations() == [] and _same(ra, rb)


def test_optional_outputs_and_empty_batch():
    d = R.BY_ID["randn-M3-H4-W33"]
    x, p = R.prepared(d)
    full = _Call(x)
    want = full.run_all()[2]
    call = _Call(x)
    rc, ran = call.bwd(dT=False)                                         # filters only (wt_workspace is then not needed either)
    assert rc == 0 and ran == {"mt_conv3_bwd_weight_kernel": 1} and call.dT.untouched() and call.wt.untouched() and call.part.nans() == 0
    assert torch.equal(_bits(call.part.t), _bits(full.part.t))
    call = _Call(x)
    rc, ran = call.bwd(dT=False, wt=False)
    assert rc == 0 and ran == {"mt_conv3_bwd_weight_kernel": 1} and torch.equal(_bits(call.part.t), _bits(full.part.t))
    call = _Call(x)
    rc, ran = call.bwd(partial=False)                                    # data gradient only
    assert rc == 0 and ran == {"mt_conv3_bwd_data_kernel": 1} and call.part.untouched() and call.dT.nans() == 0
    assert torch.equal(_bits(call.dT.t.cpu().reshape(want["dT"].shape)), _bits(want["dT"]))
    call = _Call(x)
    for kw in (dict(dT=False, partial=False), dict(M=0)):               # nothing to do: nothing launched, nothing written, rc 0
        rc, ran = call.bwd(**kw)
        assert rc == 0 and ran == {}, (kw, rc, ran)
        assert call.dT.untouched() and call.part.untouched() and call.wt.untouched() and call.violations() == []
    rc, ran = call.fwd(M=0)
    assert rc == 0 and ran == {} and call.out.untouched()
    # the column sum of no rows is zero
    call.lib.check(call.L.nir_colsum_det_f32(call.lib.ptr(call.dpre.t), NCOL, 0, NCOL, call.lib.ptr(call.db.t), None, call.lib.stream()), "nir_colsum_det_f32")
    torch.cuda.synchronize()
    assert not bool(call.db.t.any()) and call.db.intact() and int(call.L.nir_colsum_det_floats(0, NCOL)) == 0


def test_supported_at_the_boundary_shapes():
    """the C entry on the boundary shapes the CPU test picks by enumeration (tests/test_mt_conv_criterion_host.py)"""
    from context_attentive_ir_amd import lib
    L = lib.load()
    for M, H, W, _ in R.SHAPES:
        assert L.nir_mt_conv3_supported(NF, C1, H, W) == 1, (H, W)
    for _, H, W in R.REFUSED_SHAPES:
        assert L.nir_mt_conv3_supported(NF, C1, H, W) == 0, (H, W)
    for nf, c1 in ((5, 51), (6, 50), (6, 52), (7, 51)):
        assert L.nir_mt_conv3_supported(nf, c1, 4, 64) == 0, (nf, c1)
    for H, W in ((0, 5), (5, 0), (-1, 5)):
        assert L.nir_mt_conv3_supported(NF, C1, H, W) == 0, (H, W)


def test_refused_arguments_launch_nothing():
    """each refused call returns non-zero, launches nothing and leaves every output as it was; a good call afterwards succeeds.  The calls are
    turned away by argument checks: no kernel runs on them."""
    d = R.BY_ID["randn-M2-H5-W7"]
    x, p = R.prepared(d)
    call = _Call(x)
    refused = [("%dx%d" % (H, W), dict(M=1, H=H, W=W)) for _, H, W in R.REFUSED_SHAPES]
    refused += [("C1=50", dict(c1=50)), ("C1=52", dict(c1=52)), ("NF=5", dict(nf=5)), ("NULL T", dict(T=False)), ("NULL w1", dict(w1=False)),
                ("NULL dpre", dict(dpre=False))]                          # (the forward takes no dpre: there the last one is a good call, skipped below)
    for name, kw in refused:
        for which, fn in (("fwd", call.fwd), ("bwd", call.bwd)):
            if (name, which) == ("NULL dpre", "fwd"):
                continue
            rc, ran = fn(**kw)
            assert rc != 0 and ran == {}, (name, which, rc, ran)
            assert call.L.nir_last_error_string(), (name, which)
    rc, ran = call.bwd(wt=False)
    assert rc != 0 and ran == {} and call.L.nir_last_error_string()
    assert call.violations() == []
    assert all(b.untouched() for b in (call.out, call.dT, call.wt, call.part)), "a refused call wrote to an output"
    ran_f, ran_b, got = call.run_all()
    assert ran_f == FWD_ONLY and ran_b == BWD_BOTH and call.violations() == []
    assert _judge(d["id"] + "-after-refusals", got, p) == []


# ------------------------------------------------------------------ through autograd
def _mask_ok(dev_fwd, p):
    """the device's ReLU mask may differ from the float64 one only where |pre64| is within the forward bound"""
    pre, s = p["ref"]["pre"], float(p["ref"]["fwd"].abs().max()) or 1.0
    bound = R.MARGIN["fwd"] * max(p["e32"]["fwd"], R.EPS) * s
    differ = (dev_fwd > 0) != (pre > 0)
    return bool((pre[differ].abs() <= bound).all())


@pytest.mark.parametrize("cid", ["randn-M3-H4-W33", "randn-M2-H10-W74"])
def test_through_autograd(cid):
    from context_attentive_ir_amd import autograd as A
    d = R.BY_ID[cid]
    x, p = R.prepared(d)
    M, H, W = d["M"], d["H"], d["W"]
    names = ("T", "w1", "b1", "w2", "b2", "w3", "b3")

    def run(need_T, need_w, views=False):
        t = {k: x[k].to(DEV) for k in names}
        dout = x["dpre"].to(DEV)
        if views:                                                        # a non-contiguous T and a dout that is a transposed view
            t["T"] = t["T"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
            dout = dout.t().contiguous().t()
            assert not t["T"].is_contiguous() and not dout.is_contiguous()
        t["T"].requires_grad_(need_T)
        for k in names[1:]:
            t[k].requires_grad_(need_w)
        convs = [types.SimpleNamespace(weight=t["w%d" % k], bias=t["b%d" % k]) for k in (1, 2, 3)]
        out = A.mt_conv3(t["T"], *convs)
        out.backward(dout)
        torch.cuda.synchronize()
        got = {"fwd": out.detach().cpu()}
        if need_T:
            got["dT"] = t["T"].grad.cpu()
        else:
            assert t["T"].grad is None
        for k in (1, 2, 3):
            if need_w:
                got["dw%d" % k], got["db%d" % k] = t["w%d" % k].grad.cpu(), t["b%d" % k].grad.cpu()
            else:
                assert t["w%d" % k].grad is None and t["b%d" % k].grad is None
        return got

    both = run(True, True)
    assert _mask_ok(both["fwd"], p), "the device's ReLU mask differs from float64 outside the forward bound"
    xm = dict(x)
    xm["dpre"] = x["dpre"] * (both["fwd"] > 0)                          # the gradient reference under the device's own mask
    pm = R.prepare(xm)
    bad = _judge(cid + "-autograd", both, pm)
    for need_T, need_w, views in ((True, False, False), (False, True, False), (True, True, True)):
        got = run(need_T, need_w, views)
        assert all(torch.equal(_bits(v), _bits(both[k])) for k, v in got.items()), (need_T, need_w, views)
    assert bad == [], "\n".join(bad)


# ------------------------------------------------------------------ the fall-back: patch rows and their backward
def _im2col_call(d, v, which, buf):
    from context_attentive_ir_amd import lib
    L = lib.load()
    fn = L.nir_im2col_rows_f32 if which == "im2col" else L.nir_col2im_rows_f32
    src = v["x"] if which == "im2col" else v["drows"]
    rc, ran = _profiled(L, lambda: fn(lib.ptr(src), d["M"], d["C"], d["H"], d["W"], d["kh"], d["kw"], d["kh"] // 2, d["kw"] // 2, lib.ptr(buf.t), lib.stream()))
    return rc, ran


@pytest.mark.parametrize("d", R.IM2COL_CASES, ids=lambda d: d["id"])
def test_im2col_rows_and_col2im_rows(d):
    v = R.im2col_family(d)
    rows64, din64 = R.im2col_chain(d, v, torch.float64)
    rows32, din32 = R.im2col_chain(d, v, torch.float32)
    dv = {k: t.to(DEV) for k, t in v.items()}
    rows, din = _Buf(rows64.numel()), _Buf(din64.numel())
    res = []
    for _ in range(2):
        rc, ran = _im2col_call(d, dv, "im2col", rows)
        assert rc == 0 and ran == {"im2col_rows_kernel": 1}, (rc, ran)
        rc, ran = _im2col_call(d, dv, "col2im", din)
        assert rc == 0 and ran == {"col2im_rows_kernel": 1}, (rc, ran)
        res.append((rows.t.cpu().clone(), din.t.cpu().clone()))
    p = dict(ref={"col2im": din64.reshape(-1)}, e32={"col2im": R.err(din32.reshape(-1), din64.reshape(-1))})
    e = R.err(res[0][1], p["ref"]["col2im"])
    ratio, bound = e / max(p["e32"]["col2im"], R.EPS), R.MARGIN_COL2IM * max(p["e32"]["col2im"], R.EPS)
    print("MTCONVENV,%s,col2im,din,e=%.3g,e32=%.3g,ratio=%.3f,bound=%.3g" % (d["id"], e, p["e32"]["col2im"], ratio, bound))
    assert rows.intact() and din.intact() and rows.nans() == 0 and din.nans() == 0
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1])), "results differ between two calls"
    assert torch.equal(_bits(res[0][0]), _bits(rows64.float().reshape(-1))), "patch rows are copies: they must be bit-equal"
    assert e <= bound, (e, bound)


@pytest.mark.parametrize("d", R.IM2COL_REFUSED, ids=lambda d: d["id"])
def test_col2im_rows_refusals(d):
    from context_attentive_ir_amd import lib
    v = {k: t.to(DEV) for k, t in R.im2col_family(R.IM2COL_CASES[0]).items()}       # never read: the call is turned away by its argument checks
    din = _Buf(64)
    rc, ran = _im2col_call(d, v, "col2im", din)
    assert rc != 0 and ran == {} and din.untouched() and din.intact() and lib.load().nir_last_error_string()


@pytest.mark.parametrize("d", R.IM2COL_REFUSED[1:], ids=lambda d: d["id"])
def test_im2col_rows_refuses_an_even_kernel(d):
    from context_attentive_ir_amd import lib
    v = {k: t.to(DEV) for k, t in R.im2col_family(R.IM2COL_CASES[0]).items()}       # never read: the call is turned away by its argument checks
    rows = _Buf(64)
    rc, ran = _im2col_call(d, v, "im2col", rows)
    assert rc != 0 and ran == {} and rows.untouched() and rows.intact() and lib.load().nir_last_error_string()


def test_im2col_rows_takes_the_row_col2im_refuses():
    """W = 2049 is past col2im's LDS slice only: the patch rows have no such limit and stay bit-equal copies"""
    d = R.IM2COL_REFUSED[0]
    assert d["W"] == 2049
    v = R.im2col_family(d)
    rows64, _ = R.im2col_chain(d, v, torch.float64)
    rows = _Buf(rows64.numel())
    rc, ran = _im2col_call(d, {k: t.to(DEV) for k, t in v.items()}, "im2col", rows)
    assert rc == 0 and ran == {"im2col_rows_kernel": 1} and rows.intact() and rows.nans() == 0
    assert torch.equal(_bits(rows.t.cpu()), _bits(rows64.float().reshape(-1)))


# ------------------------------------------------------------------ the fixed-order column sum by itself
@pytest.mark.parametrize("M,N,ld", R.COLSUM_CASES, ids=lambda v: str(v))
def test_colsum_det(M, N, ld):
    """nir_colsum_det_f32 with ld > N (the columns behind N hold NaN), more than 64 rows a slice, both first-pass kernels: small integers sum
    exactly in any order, so they must equal the float64 sum bit for bit (a row dropped or counted twice shows); a randn matrix meets the a
    priori bound of its addition chains and gives the same bits on eight calls"""
    from context_attentive_ir_amd import lib
    L = lib.load()
    ms, S = R.colsum_slices(M)
    nws = int(L.nir_colsum_det_floats(M, N))
    assert nws == (S * N if S > 1 else 0)
    g = torch.Generator().manual_seed(M + N)
    for kind in ("integers", "randn"):
        x = torch.full((M, ld), NAN)
        x[:, :N] = torch.randint(-8, 9, (M, N), generator=g).float() if kind == "integers" else torch.randn(M, N, generator=g)
        xd, out, ws = x.to(DEV), _Buf(N), _Buf(nws)
        res = []
        for _ in range(8 if kind == "randn" else 2):
            lib.check(L.nir_colsum_det_f32(lib.ptr(xd), ld, M, N, lib.ptr(out.t), lib.ptr(ws.t) if nws else None, lib.stream()), "nir_colsum_det_f32")
            torch.cuda.synchronize()
            res.append(out.t.cpu().clone())
        assert out.intact() and ws.intact() and out.nans() == 0 and ws.nans() == 0
        assert all(torch.equal(_bits(r), _bits(res[0])) for r in res[1:]), "bits differ between calls"
        ref = x[:, :N].double().sum(0)
        if kind == "integers":
            assert torch.equal(res[0].double(), ref)
        else:
            du = R.colsum_chain_depth(M, N) * 2.0 ** -24
            bound = du / (1.0 - du) * x[:, :N].double().abs().sum(0)
            worst = float(((res[0].double() - ref).abs() / bound).max())
            print("MTCONVENV-COLSUM,M%d-N%d-ld%d,|err| / bound = %.3f" % (M, N, ld, worst))
            assert worst <= 1.0
    rc = L.nir_colsum_det_f32(lib.ptr(xd), ld, M, N, lib.ptr(out.t), None, lib.stream())
    assert (rc != 0) == (S > 1)                                          # more than one slice without the slice buffer is refused
    rc = L.nir_colsum_det_f32(lib.ptr(xd), N - 1, M, N, lib.ptr(out.t), lib.ptr(ws.t) if nws else None, lib.stream())
    assert rc != 0                                                       # ld < N
    torch.cuda.synchronize()
