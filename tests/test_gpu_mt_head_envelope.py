"""GPU (-m gpu): the MatchTensor interaction head (csrc/mtensor.hip: mt_fold_kernel<H2>, mt_head_kernel<H2>) in its three forms, called
through the C ABI (nir_matchtensor_score_encoded: the caller supplies the encoder states, so no recurrence runs and the head with its two
projections is isolated), against float64 on the case list of tests/mt_head_ref.py.  Each case asserts:
  * the profile report shows mt_fold_kernel x 1, mt_head_kernel x 1 and the projection GEMMs the form leaves (two; one when the document
    projection is fused into the head and proj_d is not asked for);
  * scores meet the criterion of mt_head_ref (fp32-chain error times a margin <= 4, plus what the fp16 term pairs cost); proj_q and proj_d
    meet the GEMM criterion of gemm_ref; the `dead` family gives ow . cb + ob to 4 ulp of the score;
  * scores are bit-identical run to run, and in the fused form with and without proj_d;
  * scores, proj_q and proj_d sit between guard rows holding a sentinel, the workspace has exactly nir_matchtensor_workspace_bytes with a
    patterned region behind it, and all of these stay untouched;
  * the dynamic LDS the library reports under tunable `debug` is the figure of the kernel form the case is judged as (fp32 or fp16-term)
    at the chunk width the case names or the shape implies (a shape that lands in the other width is moved, not the assertion).
Every case prints one "MTHEADENV" line before it asserts."""
import ctypes as C
import re

import pytest
import torch

import gemm_ref as G
import mt_head_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0
PATTERN = 0xA5
GUARD = 4096
WEIGHTS = ("qproj_w", "qproj_b", "dproj_w", "dproj_b", "alpha", "conv1_w", "conv1_b", "conv2_w", "conv2_b", "conv3_w", "conv3_b", "conv_w", "conv_b",
           "out_w", "out_b")


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


def _guarded(rows, cols):
    buf = torch.full((rows + 2, cols), SENT, device=DEV)
    return buf, buf[1:rows + 1]


def _intact(buf, rows):
    g = buf.cpu()
    return bool((g[0] == SENT).all()) and bool((g[rows + 1:] == SENT).all())


class _Call(object):
    """nir_matchtensor_score_encoded on one case: device copies, the packed weights, guarded outputs, a workspace of the exact size"""

    def __init__(self, d, x):
        from context_attentive_ir_amd import lib
        from context_attentive_ir_amd.rankers.mtensor import attach_projection_fragments
        self.lib, self.L, self.d = lib, lib.load(), d
        B, N, QL, DL, C_ = d["B"], d["N"], d["QL"], d["DL"], d["C"]
        self.dims = (B, N, QL, DL)
        self.pk = lib.Packed(lib.MatchTensorWeights, {k: x[k].to(DEV) for k in WEIGHTS},
                             dict(F=1, Hq=d["Kq"] // 2, Hd=d["Kd"] // 2, C=C_, NF=R.NF, MF=R.MF, bounded=int(d["sel"] != "unbounded")))
        if d["sel"] in ("frag", "decline"):
            attach_projection_fragments(self.pk)
            assert ("dproj_frag" in self.pk.keep) == (d["sel"] == "frag")
        self.tun = {"exact_f32": 1} if d["sel"] == "exact" else {}
        self.dev = {k: x[k].to(DEV) for k in ("hq", "hd", "q_ids", "d_ids")}
        self.nbytes = int(self.L.nir_matchtensor_workspace_bytes(B, N, QL, DL, self.pk.ref()))
        assert self.nbytes > 0
        self.ws = torch.full((self.nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.sbuf, self.scores = _guarded(B * N, 1)
        self.qbuf, self.pq = _guarded(B * QL, C_)
        self.dbuf, self.pd = _guarded(B * N * DL, C_)

    def raw(self, proj_d=True, nbytes=None, dims=None, hq="hq", struct=None):
        """(rc, launches by scope name); nothing is raised"""
        lib, L, v = self.lib, self.L, self.dev
        B, N, QL, DL = dims or self.dims
        ctx = [lib.tunable(k, val, 0) for k, val in self.tun.items()]
        for t in ctx:
            t.__enter__()
        try:
            return _profiled(L, lambda: L.nir_matchtensor_score_encoded(
                lib.ptr(v["q_ids"]), lib.ptr(v["d_ids"]), lib.ptr(v[hq]) if hq else None, lib.ptr(v["hd"]), B, N, QL, DL,
                C.byref(struct) if struct is not None else self.pk.ref(), lib.ptr(self.ws), self.nbytes if nbytes is None else nbytes,
                lib.ptr(self.scores), lib.ptr(self.pq), lib.ptr(self.pd) if proj_d else None, lib.stream()))
        finally:
            for t in reversed(ctx):
                t.__exit__(None, None, None)

    def run(self, proj_d=True):
        """(launches, scores [B N] on the CPU); the caller checks violations()"""
        rc, ran = self.raw(proj_d)
        self.lib.check(rc, "nir_matchtensor_score_encoded")
        return ran, self.scores.cpu().reshape(-1).clone()

    def violations(self):
        """what was written outside the outputs and the workspace"""
        B, N, QL, DL = self.dims
        bad = [name for name, buf, rows in (("scores", self.sbuf, B * N), ("proj_q", self.qbuf, B * QL), ("proj_d", self.dbuf, B * N * DL)) if not _intact(buf, rows)]
        return bad + ["behind the workspace"] * (not bool((self.ws[self.nbytes:] == PATTERN).all()))


def _launches(ran):
    return ran.get("mt_fold_kernel", 0), ran.get("mt_head_kernel", 0), sum(n for k, n in ran.items() if not k.startswith("mt_"))


@pytest.mark.parametrize("d", R.CASES, ids=lambda d: d["id"])
def test_mt_head(d, capfd):
    from context_attentive_ir_amd import lib
    x, p = R.prepared(d)
    call = _Call(d, x)
    fused = d["form"] == "x2p"
    capfd.readouterr()
    with lib.tunable("debug", 1, 0):
        ran, got = call.run()
    lds = re.search(r"mt_head_kernel: lds dyn=(\d+)", capfd.readouterr().err)
    pq, pd = call.pq.cpu().clone(), call.pd.cpu().clone()
    ran2, again = call.run()
    bad = call.violations()
    if fused:
        call.dbuf.fill_(SENT)
        ran3, lean = call.run(proj_d=False)
        untouched = bool((call.dbuf == SENT).all())
        bad += call.violations()
    ok, r = R.accept(got, d, x, p)
    okq, rq = G.accept(pq, x["hq"].reshape(-1, d["Kq"]), x["qproj_w"], bias=x["qproj_b"], form="f32")
    okd, rd = G.accept(pd, x["hd"].reshape(-1, d["Kd"]), x["dproj_w"], bias=x["dproj_b"], form="f32")
    line = "MTHEADENV,%s,%s,e=%.3g,e32=%.3g,fmt=%.3g,floor=%.3g,ratio=%.3f,bound=%.3g" % (d["id"], d["form"], r["e"], r["e32"], r["fmt"], r["floor"], r["ratio"], r["bound"])
    print(line + ",pq_ratio=%.3f,pd_ratio=%.3f,lds=%s" % (rq["ratio"], rd["ratio"], lds.group(1) if lds else None))
    # the kernel form the case is judged as is the one that ran: the LDS figure of the fp32 and of the fp16-term kernel differ at every shape
    # (tests/test_mt_head_criterion_host.py), and so do those of the two chunk widths
    assert bad == [], "wrote outside: %s" % bad
    assert lds, "no LDS figure under tunable debug"
    jts = {32: 5, 64: 6}[d["jt"] or R.chunk_width(d["form"], d["QL"], d["DL"])]
    assert int(lds.group(1)) == R.lds_bytes(d["form"], d["QL"], d["DL"], jts), (lds.group(0), d["id"])
    assert _launches(ran) == (1, 1, 2), ran
    assert _launches(ran2) == (1, 1, 2), ran2
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "scores differ run to run"
    if fused:
        assert _launches(ran3) == (1, 1, 1), ran3
        assert untouched, "proj_d written though not asked for"
        assert torch.equal(got.view(torch.int32), lean.view(torch.int32)), "scores differ with and without proj_d"
    assert ok, line
    assert okq and okd, (rq, rd)
    if d["fam"] == "dead":
        want, tol = R.dead_score(x)
        assert float((got.double() - want).abs().max()) <= tol, (got, want, tol)


def test_refused_arguments_launch_nothing():
    """each refused call returns non-zero, launches nothing, leaves every sentinel in place, and a good call afterwards succeeds"""
    from context_attentive_ir_amd import lib
    d = R.BY_ID["x2p-frag-model-B2N3-Q17-D65-C50-K30.140"]
    x, p = R.prepared(d)
    call = _Call(d, x)

    def patched(**kw):
        s = lib.MatchTensorWeights()
        C.memmove(C.byref(s), C.byref(call.pk.struct), C.sizeof(s))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    refused = [("C=51", dict(struct=patched(C=51)), None), ("NF=5", dict(struct=patched(NF=5)), None), ("MF=19", dict(struct=patched(MF=19)), None),
               ("QL=257", dict(dims=(d["B"], d["N"], 257, d["DL"])), None), ("NULL states", dict(hq=None), None),
               ("workspace one byte short", dict(nbytes=call.nbytes - 1), -3)]                              # NIR_ERR_WORKSPACE
    for name, kw, code in refused:
        rc, ran = call.raw(**kw)
        assert rc != 0 and (code is None or rc == code), (name, rc)
        assert ran == {}, (name, ran)
        assert call.violations() == [], name
        assert bool((call.sbuf == SENT).all()) and bool((call.qbuf == SENT).all()) and bool((call.dbuf == SENT).all()), name
        assert call.L.nir_last_error_string(), name
    ran, got = call.run()
    assert _launches(ran) == (1, 1, 2) and call.violations() == []
    ok, r = R.accept(got, d, x, p)
    assert ok, r
