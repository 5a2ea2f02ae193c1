"""GPU (-m gpu): the DUET document branch (csrc/duet_fused.hip: duet_doc_kernel<RT, POOL, PL>, duet_doc_finish_kernel; csrc/duet.hip: the
GEMM-per-layer chain) in its seven forms, called through the C ABI (nir_duet_document_branch: the caller supplies the query vector, so the
branch is isolated and its real output m1 [M, NF] is compared, not a score behind fc3 / fc4), against float64 on the case list of
tests/duet_doc_ref.py.  The weights are packed by the shipped rankers.duet.attach_document_fragments.  Each case asserts:
  * the profile report shows the launches the form implies: duet_doc_kernel x 1 and duet_doc_finish_kernel x 1 and nothing else for the fused
    forms, with the [M=...] suffix equal to tiles x tile height of the tiling restatement (96 against 64 rows, flattened against per-document
    tiling); the two GEMMs, the pool and the Hadamard kernel and no duet_doc_kernel for the chain forms (a shape that lands in another form is
    moved to that form, not the assertion);
  * m1 meets the criterion of duet_doc_ref at MARGIN[form] (fp32-chain error times a margin <= 4, plus what the fp16 term pairs and the
    hardware tanh cost);
  * m1 is bit-identical run to run;
  * m1 sits between guard rows holding a sentinel, the workspace has exactly nir_duet_document_workspace_bytes with a patterned region behind
    it, and all of these stay untouched;
  * d_ids sits between guards of valid ids that name a table row of large values, so an over-read that reaches the result shows as a wrong value.
Every case prints one "DUETDOCENV" line before it asserts.  Further: one document stacked twice in a batch at different pair indices gives the
same m1 row within the bound; refused arguments return an error code before anything is enqueued."""
import ctypes as C
import re

import pytest
import torch

import duet_doc_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7777.0
PATTERN = 0xA5
GUARD = 4096
GUARD_VALUE = 1000.0


def _profiled(L, fn):
    """(rc, launches by scope name without the shape suffix, the [M=...] figure of duet_doc_kernel or None)"""
    buf = C.create_string_buffer(1 << 16)
    L.nir_profile_report(buf, len(buf))                     # drop what earlier tests left
    L.nir_profile_enable(1)
    try:
        rc = fn()
        torch.cuda.synchronize()
    finally:
        L.nir_profile_enable(0)
    L.nir_profile_report(buf, len(buf))
    out, rows = {}, None
    for ln in buf.value.decode().strip().splitlines():
        name, launches, _ = ln.rsplit(",", 2)
        m = re.search(r"\[M=(\d+),[^\]]*\]$", name)
        name = re.sub(r"\[M=[^\]]*\]$", "", name)
        if name == "duet_doc_kernel" and m:
            rows = int(m.group(1))
        out[name] = out.get(name, 0) + int(launches)
    return rc, out, rows


class _Call(object):
    """nir_duet_document_branch on one case: device copies, the pack as rankers.duet builds it, guarded ids and m1, a workspace of the exact size"""

    def __init__(self, d, x):
        from context_attentive_ir_amd import lib
        from context_attentive_ir_amd.rankers.duet import attach_document_fragments
        self.lib, self.L, self.d = lib, lib.load(), d
        B, N, DL, E, NF, P, V = (d[k] for k in ("B", "N", "DL", "E", "NF", "P", "V"))
        M = B * N
        self.dims = (B, N, DL)
        # one more table row than the case's ids use: the guard ids around d_ids name it
        self.table = torch.cat([x["table"], torch.full((1, E), GUARD_VALUE)]).to(DEV)
        self.V = V + 1
        t = dict(convd1_w=x["w1"], convd1_b=x["b1"], convd2_w=x["w2"], convd2_b=x["b2"], fc2_w=x["fc2w"].reshape(1, -1), fc2_b=x["fc2b"])
        self.pk = lib.Packed(lib.DuetWeights, {k: v.to(DEV) for k, v in t.items()}, dict(NF=NF, pool=P, bounded=int(R.bounded(x))))
        sel = d["sel"]
        attach_document_fragments(self.pk, self.table, fuse=sel != "presplit", table_planes=sel != "noplanes", presplit=sel == "presplit")
        s = self.pk.struct
        if d["form"] in R.FUSED or sel in ("unfused", "exact", "unbounded"):
            assert (bool(s.fw1) and bool(s.fw2)) == (P <= 5), "fragments not attached"
        assert bool(s.ftable) == (sel != "noplanes" and sel != "presplit" and P <= 5) and bool(s.table_h1) == (sel == "presplit")
        if sel == "unbounded":
            s.bounded = 0
        self.tun = {"rows64": {"duet_rows64": 1}, "unfused": {"duet_unfused": 1}, "exact": {"exact_f32": 1}}.get(sel, {})
        self.idbuf = torch.full((M * DL + 2 * GUARD,), V, dtype=torch.int64, device=DEV)
        self.ids = self.idbuf[GUARD:GUARD + M * DL]
        self.ids.copy_(x["d_ids"].reshape(-1))
        self.qv = x["qv"].to(DEV)
        with self._tunables():
            self.nbytes = int(self.L.nir_duet_document_workspace_bytes(B, N, DL, E, self.pk.ref()))
        assert self.nbytes > 0
        self.ws = torch.full((self.nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=DEV)
        self.mbuf = torch.full((M + 2, NF), SENT, device=DEV)
        self.m1 = self.mbuf[1:M + 1]

    def _tunables(self):
        lib, tun = self.lib, self.tun

        class _Ctx(object):
            def __enter__(s):
                s.ctx = [lib.tunable(k, v, 0) for k, v in tun.items()]
                for t in s.ctx:
                    t.__enter__()

            def __exit__(s, *exc):
                for t in reversed(s.ctx):
                    t.__exit__(None, None, None)
                return False
        return _Ctx()

    def raw(self, nbytes=None, dims=None, struct=None):
        """(rc, launches by scope name, rows of the duet_doc_kernel launch); nothing is raised"""
        lib, L = self.lib, self.L
        B, N, DL = dims or self.dims
        with self._tunables():
            return _profiled(L, lambda: L.nir_duet_document_branch(
                lib.ptr(self.ids), B, N, DL, lib.ptr(self.table), self.V, self.d["E"], C.byref(struct) if struct is not None else self.pk.ref(),
                lib.ptr(self.qv), lib.ptr(self.ws), self.nbytes if nbytes is None else nbytes, lib.ptr(self.m1), lib.stream()))

    def run(self):
        """(launches, rows, m1 [M, NF] on the CPU); the caller checks violations()"""
        rc, ran, rows = self.raw()
        self.lib.check(rc, "nir_duet_document_branch")
        return ran, rows, self.m1.cpu().clone()

    def violations(self):
        """what was written outside m1 and the workspace"""
        g, M = self.mbuf.cpu(), self.dims[0] * self.dims[1]
        bad = ["m1 guard rows"] * (not (bool((g[0] == SENT).all()) and bool((g[M + 1:] == SENT).all())))
        bad += ["behind the workspace"] * (not bool((self.ws[self.nbytes:] == PATTERN).all()))
        ib = self.idbuf.cpu()
        return bad + ["id guards"] * (not (bool((ib[:GUARD] == self.V - 1).all()) and bool((ib[-GUARD:] == self.V - 1).all())))


def _expected_launches(d):
    if d["form"] in R.FUSED:
        return {"duet_doc_kernel": 1, "duet_doc_finish_kernel": 1}
    if d["form"] == "hp":
        return {"gemm_h2p_kernel[gather]": 1, "gemm_h2p_kernel": 1, "maxpool_t_planes_kernel": 1, "duet_hadamard_kernel": 1}
    return {"maxpool_t_kernel": 1, "duet_hadamard_kernel": 1}


def _check_launches(d, ran, rows):
    want = _expected_launches(d)
    if d["form"] in R.FUSED:
        assert ran == want, ran
        assert rows == d["tiles"] * d["rows"] == R.case_tiling(d)["n"] * d["rows"], (rows, d["tiles"], d["rows"])
        return
    assert "duet_doc_kernel" not in ran and "duet_doc_finish_kernel" not in ran, ran
    if d["form"] == "hp":
        assert ran == want, ran
        return
    assert {k: v for k, v in ran.items() if not k.startswith("gemm")} == want, ran
    gemms = {k: v for k, v in ran.items() if k.startswith("gemm")}
    assert sum(gemms.values()) == 2 and sum(v for k, v in gemms.items() if k.endswith("[gather]")) == 1, ran
    assert not any(k.startswith("gemm_h2p") for k in gemms), ran
    if d["form"] in ("ex", "un"):                            # no fp16-term GEMM: exact_f32 forces the fp32 MFMA kernels, bounded = 0 forbids the split
        assert not any(k.startswith("gemm3h") for k in gemms), ran
    if d["form"] == "ex":
        assert not any(k.startswith("gemm3") for k in gemms), ran


def _line(d, r):
    return "DUETDOCENV,%s,%s,e=%.3g,e32=%.3g,fmt=%.3g,floor=%.3g,r=%.3f,ratio=%.3f,bound=%.3g" % (
        d["id"], d["form"], r["e"], r["e32"], r["fmt"], r["floor"], r["r"], r["ratio"], r["bound"])


@pytest.mark.parametrize("d", R.CASES, ids=lambda d: d["id"])
def test_duet_document_branch(d):
    x, p = R.prepared(d)
    call = _Call(d, x)
    ran, rows, got = call.run()
    ran2, rows2, again = call.run()
    bad = call.violations()
    ok, r = R.accept(got, d, x, p)
    line = _line(d, r)
    print(line + ",launches=%s,rows=%s" % ("+".join("%s x %d" % kv for kv in sorted(ran.items())), rows))
    assert bad == [], "wrote outside: %s" % bad
    _check_launches(d, ran, rows)
    _check_launches(d, ran2, rows2)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32)), "m1 differs run to run"
    assert ok, line


STACKED = ["f96-planes-seam-B2N3-D95-E20-F20-P5", "p64-planes-seam-B2N3-D63-E20-F20-P5", "t64-noplanes-seam-B2N3-D63-E20-F20-P5",
           "f96-planes-trained-B2N3-D95-E20-F20-P5", "p64-planes-negative-B2N3-D64-E20-F20-P4", "hp-presplit-trained-B2N3-D40-E20-F20-P5",
           "ch-unfused-trained-B2N3-D40-E20-F20-P5", "ex-exact-trained-B2N3-D40-E20-F20-P5", "un-unbounded-trained-B2N3-D40-E20-F20-P5"]


@pytest.mark.parametrize("cid", STACKED)
def test_one_document_twice_in_a_batch(cid):
    """document 0 copied to pair 2 (the same query, N = 3): it starts 2 Tc rows further down the flattened axis, so it falls differently against
    the tile seams; both rows meet the criterion and agree with each other within the bound"""
    d = R.BY_ID[cid]
    assert d["N"] >= 3
    x = dict(R.prepared(d)[0])
    x["d_ids"] = x["d_ids"].clone()
    x["d_ids"][2] = x["d_ids"][0]
    p = R.reference(d, x)
    assert torch.equal(p["ref"][0], p["ref"][2])
    call = _Call(d, x)
    ran, rows, got = call.run()
    ok, r = R.accept(got, d, x, p)
    gap = float((got[0].double() - got[2].double()).abs().max())
    print(_line(d, r) + ",stacked_gap=%.3g" % gap)
    assert call.violations() == []
    _check_launches(d, ran, rows)
    assert ok, r
    assert gap <= r["bound"], (gap, r["bound"])


def test_refused_arguments_launch_nothing():
    """each refused call returns non-zero, launches nothing, leaves every sentinel in place, and a good call afterwards succeeds"""
    from context_attentive_ir_amd import lib
    d = R.BY_ID["p64-planes-seam-B2N3-D63-E20-F20-P5"]
    x, p = R.prepared(d)
    call = _Call(d, x)

    def patched(**kw):
        s = lib.DuetWeights()
        C.memmove(C.byref(s), C.byref(call.pk.struct), C.sizeof(s))
        for k, v in kw.items():
            setattr(s, k, v)
        return s

    refused = [("DL < P + 2", dict(dims=(d["B"], d["N"], d["P"] + 1)), None), ("NF % 4 != 0", dict(struct=patched(NF=d["NF"] + 2)), None),
               ("workspace one byte short", dict(nbytes=call.nbytes - 1), -3)]                              # NIR_ERR_WORKSPACE
    for name, kw, code in refused:
        rc, ran, rows = call.raw(**kw)
        assert rc != 0 and (code is None or rc == code), (name, rc)
        assert ran == {}, (name, ran)
        assert call.violations() == [], name
        assert bool((call.mbuf == SENT).all()) and bool((call.ws == PATTERN).all()), name
        assert call.L.nir_last_error_string(), name
    ran, rows, got = call.run()
    _check_launches(d, ran, rows)
    assert call.violations() == []
    ok, r = R.accept(got, d, x, p)
    assert ok, r
