"""GPU (-m gpu): the CARS session tail (csrc/cars_session.hip) at the C ABI against float64 across its dispatch paths -- the eight
instantiations launch_lstm_step picks from (both sides of every batch boundary, a second chunk round of every k-loop, the three ways
into the fp32 forms, a mixed pair of chains), every rank_bounded bit set and clear with a weight at +-40000, both click-pooling kernels
from N = 1 to the documented N = 2048, labels_all wider than the call, m_groups, both forms of nir_cars_click_max, the label patterns
up to the planted all-masked row, the q_on x d_on x rank_on switches, every optional output, the entry-point identities and the argument
errors.  The cases, their float64 reference and the bound come from tests/cars_session_ref.py (tests/test_cars_session_host.py shows on
the CPU that the bound accepts honest fp32 on these very inputs and rejects ten planted mistakes).

Every output buffer and the workspace carry a guard region on either side, filled with a sentinel that must survive the call; an output
the call does not produce must keep the sentinel too.  The ratio (e - fmt - act_term) / max(e_chain, 2^-23) is printed per case and output:
cars_session_ref.MARGIN is chosen from these figures."""
import ctypes as C

import numpy as np
import pytest
import torch

import cars_session_ref as R
from context_attentive_ir_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG, ERR_WORKSPACE = -1, -3
GUARD = 1024                     # floats on either side of every output
WS_GUARD = 4096                  # bytes on either side of the workspace
SENT = -7.0e33
EXTRA = ("inner_q", "inner_d", "dec_h", "dec_c")


class Buf(object):
    """a float32 device buffer of `shape` between two guard regions, all of it the sentinel"""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.flat = torch.full((self.n + 2 * GUARD,), SENT, device=DEV)
        self.view = self.flat[GUARD:GUARD + self.n].view(*shape)

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def guards_intact(self):
        return bool((self.flat[:GUARD] == SENT).all()) and bool((self.flat[GUARD + self.n:] == SENT).all())

    def untouched(self):
        return bool((self.flat == SENT).all())

    def cpu(self):
        return self.view.cpu()


_WEIGHTS = {}


def _weights(name, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _WEIGHTS:
        d = R.build(name)
        _WEIGHTS[key] = R.device_weights(d["sd"], d["case"], DEV, **kw)
    return _WEIGHTS[key]


def _call(name, w=None, entry="rows", extra=EXTRA, clicks_out=True, ws_short=0, over=None, null=(), pre=None, full=False):
    """one call of the case `name` -> (rc, {output: Buf}, workspace guards intact).  entry: plain / shard / rows / pre; extra: the members of
    nir_cars_session_outputs that are given (None: no struct at all); over: arguments replaced for an argument-error call; null: inputs
    passed as NULL; pre: (U, gq) device tensors for entry "pre"; full: a slice case without its slice (all N candidates ranked)."""
    L = lib.load()
    d = R.build(name)
    c = d["case"]
    over = dict(over or {})
    w = _weights(name)[0] if w is None else w
    B, S, N, D, HS, HDEC = c["B"], c["S"], c["N"], c["D"], c["HS"], c["HDEC"]
    cols = None if full else c["cols"]
    NR = cols[1] if cols else N
    pq, docs, lab = (d[k].to(DEV).contiguous() for k in ("pooled_q", "pooled_docs", "labels"))
    rdocs = docs[:, :, cols[0]:cols[0] + NR].contiguous() if cols else None
    lab_all = d["labels_all"].to(DEV).contiguous() if d["labels_all"] is not None else None
    mg = torch.tensor(c["m_groups"], dtype=torch.int32, device=DEV) if c["m_groups"] else None
    bufs = dict(scores=Buf(B, S, NR), clicks=Buf(B, S, D), inner_q=Buf(B, S, HS), inner_d=Buf(B, S, HS),
                dec_h=Buf(max((S - 1) * B, 1), HDEC), dec_c=Buf(max((S - 1) * B, 1), HDEC))
    ex = None
    if extra is not None:
        ex = lib.CarsSessionOutputs()
        for k in extra:
            setattr(ex, k, bufs[k].view.data_ptr())
    Bc, Sc, Nc = over.get("B", B), over.get("S", S), over.get("N", N)
    need = L.nir_cars_session_workspace_bytes(B, S, N, C.byref(w))
    assert need > 0 and need % 256 == 0
    ws = torch.full((need + 2 * WS_GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    wsp = C.c_void_p(ws.data_ptr() + WS_GUARD)
    assert (ws.data_ptr() + WS_GUARD) % 256 == 0
    a = dict(pq=None if "pooled_q" in null else lib.ptr(pq), docs=None if "pooled_docs" in null else lib.ptr(docs),
             lab=None if "labels" in null else lib.ptr(lab), scores=None if "scores" in null else bufs["scores"].ptr(),
             clicks=bufs["clicks"].ptr() if clicks_out else None, ex=C.byref(ex) if ex is not None else None,
             rdocs=lib.ptr(rdocs), NR=NR if rdocs is not None else 0, lab_all=lib.ptr(lab_all), rows_all=c["rows_all"], mg=lib.ptr(mg), spg=c["spg"])
    a.update({k: v for k, v in over.items() if k in a})
    head = (a["pq"], a["docs"], a["lab"], Bc, Sc, Nc, C.byref(w), wsp, need - ws_short, a["scores"], a["clicks"], a["ex"])
    st = lib.stream()
    if entry == "plain":
        rc = L.nir_cars_rank_session(*head, st)
    elif entry == "shard":
        rc = L.nir_cars_rank_session_shard(*head, a["rdocs"], a["NR"], st)
    elif entry == "rows":
        rc = L.nir_cars_rank_session_rows(*head, a["rdocs"], a["NR"], a["lab_all"], a["rows_all"], a["mg"], a["spg"], st)
    else:
        U, gq = pre if pre is not None else (None, None)
        rc = L.nir_cars_rank_session_pre(*head, a["rdocs"], a["NR"], a["lab_all"], a["rows_all"], a["mg"], a["spg"], lib.ptr(U), lib.ptr(gq), st)
    torch.cuda.synchronize()
    ws_ok = bool((ws[:WS_GUARD] == 0xA5).all()) and bool((ws[WS_GUARD + need:] == 0xA5).all())
    return rc, bufs, ws_ok


def _produced(c, w, extra, clicks_out):
    """the outputs a call has to write"""
    q, d_, r = w.q_on != 0, w.d_on != 0, w.rank_on != 0
    out = set()
    if r:
        out.add("scores")
    if d_ and clicks_out:
        out.add("clicks")
    for k in extra or ():
        if (k == "inner_q" and q) or (k == "inner_d" and d_) or (k in ("dec_h", "dec_c") and c["S"] > 1):
            out.add(k)
    return out


def _check(name, rc, bufs, ws_ok, w=None, extra=EXTRA, clicks_out=True, tag=""):
    """rc, guards, untouched outputs, NaN pattern and the bound of every produced output -> {output: figures}"""
    d = R.build(name)
    c = d["case"]
    w = _weights(name)[0] if w is None else w
    assert rc == 0, lib.load().nir_last_error_string()
    assert ws_ok, "the call wrote outside its workspace"
    made = _produced(c, w, extra, clicks_out)
    figs = {}
    for k, b in bufs.items():
        assert b.guards_intact(), "%s: guard region overwritten" % k
        if k not in made:
            assert b.untouched(), "%s was written although the call does not produce it" % k
            continue
        got = b.cpu()
        assert not bool((got == SENT).any()), "%s: entries left unwritten" % k
        ok, f = R.accept(got, d["ref"][k], d["chain"][k], d["n_split"][k], d["act"][k])
        if not f["nan_equal"]:
            print("%s %s NaN rows: got %s, reference %s" % (name, k, torch.isnan(got).reshape(-1, got.shape[-1]).any(1).nonzero().flatten().tolist()[:40],
                                                          torch.isnan(d["ref"][k]).reshape(-1, got.shape[-1]).any(1).nonzero().flatten().tolist()[:40]))
        print("%s%s %-8s e=%.3e e_chain=%.3e extra=%.3e ratio=%.3f bound=%.3e nan_equal=%s" % (name, tag, k, f["e"], f["e_chain"], f["extra"],
                                                                                               f["ratio"], f["bound"], f["nan_equal"]))
        figs[k] = (ok, f)
    bad = {k: f for k, (ok, f) in figs.items() if not ok}
    assert not bad, (name, bad)
    return figs


def _profiled(fn):
    """fn() with the library profiler on -> (result, {kernel name: launches})"""
    L = lib.load()
    buf = C.create_string_buffer(1 << 16)
    L.nir_profile_report(buf, len(buf))             # drain what earlier calls left
    L.nir_profile_enable(1)
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        L.nir_profile_enable(0)
    L.nir_profile_report(buf, len(buf))
    names = {}
    for ln in buf.value.decode().strip().splitlines():
        nm, launches, _ = ln.rsplit(",", 2)
        names[nm.split("[")[0]] = names.get(nm.split("[")[0], 0) + int(launches)
    return res, names


STEP_CASES = [n for n in R.CASES if n.startswith("step")]


@pytest.mark.parametrize("name", STEP_CASES)
def test_step_dispatch(name):
    """one case per instantiation of launch_lstm_step and per side of every batch boundary, every output requested"""
    c = R.CASES[name]
    if c["exact"]:
        with lib.tunable("exact_f32", 1, 0):
            (rc, bufs, ws_ok), names = _profiled(lambda: _call(name))
    else:
        (rc, bufs, ws_ok), names = _profiled(lambda: _call(name))
    want, other = ("lstm_step16_kernel", "lstm_step_kernel") if R.steps_are_f16(c) else ("lstm_step_kernel", "lstm_step16_kernel")
    print(name, R.step_kernel(c), names)
    assert names.get(want) == c["S"] and other not in names, names
    assert names.get("click_pool2_kernel") == 1 and names.get("session_attend2_kernel") == 1
    _check(name, rc, bufs, ws_ok)


@pytest.mark.parametrize("name", ["opf_all_bits"] + ["opf_bit%d_clear_big" % b for b in range(4)])
def test_operand_formats(name):
    """every rank_bounded bit set (the split products are counted), then each bit clear with one weight of its GEMM at +-40000 (that product
    counted as fp32): the shape is the smallest at which all four GEMMs reach the split kernels"""
    c = R.CASES[name]
    p = R.products(c)
    if c["big"] is None:
        assert p == dict(click0=1, wih=1, rec=1, mo0=1, mo1=1)
    else:
        gone = {0: ("mo0", "mo1"), 1: ("mo1",), 2: ("click0",), 3: ("wih",)}[c["big"]]        # (bit 1 rests on bit 0: cars_session_ref._build_cases)
        assert all(p[k] == 0 for k in gone) and sum(p.values()) == 5 - len(gone)
        assert all(float(R.build(name)["sd"][k].abs().max()) == R.BIG for k in R.BIT_WEIGHTS[c["big"]])
    (rc, bufs, ws_ok), names = _profiled(lambda: _call(name))
    print(name, names)
    split = sum(v for k, v in names.items() if k.startswith("gemm3h_kernel"))
    assert split == (5 if c["big"] is None else 3 if c["big"] in (0, 3) else 4), names       # wih: one GEMM per chain
    _check(name, rc, bufs, ws_ok)


def test_whh_outside_the_split_range_raises_the_flag_and_fp32_steps_hold():
    name = "whh_out_of_range"
    d = R.build(name)
    c = d["case"]
    whh = d["sd"][R.SQ + ".weight_hh_l0"].to(DEV).contiguous()
    assert float(whh.abs().max()) == 32768.0
    _, flag = R.pack_whh_frag(whh, c["HS"])
    assert flag & 2
    _, flag = R.pack_whh_frag(d["sd"][R.SD + ".weight_hh_l0"].to(DEV).contiguous(), c["HS"])
    assert flag == 0
    (rc, bufs, ws_ok), names = _profiled(lambda: _call(name))
    assert names.get("lstm_step_kernel") == c["S"] and "lstm_step16_kernel" not in names, names
    _check(name, rc, bufs, ws_ok)


POOL_CASES = [n for n in R.CASES if n.startswith(("pool_", "rows_all", "labels_"))]


@pytest.mark.parametrize("name", POOL_CASES)
def test_click_pooling(name):
    """N from 1 to 2048 through both pooling kernels, labels_all wider than the call (the batch-wide m in its last row), the label patterns;
    in the planted NaN cases the NaN pattern of every output equals the reference's and everything else stays inside the bound"""
    c = R.CASES[name]
    rc, bufs, ws_ok = _call(name)
    _check(name, rc, bufs, ws_ok)
    if c["nan"]:
        got = bufs["clicks"].cpu()
        assert bool(torch.isnan(got[1, 0]).all()) and not bool(torch.isnan(got[0]).any())
        assert bool(torch.isnan(bufs["scores"].cpu()[1, 1:]).all())


@pytest.mark.parametrize("name", ["mgroups3", "mgroups1", "mgroups2_n70"])
def test_m_groups_equal_the_separate_calls_bit_for_bit(name):
    d = R.build(name)
    c = d["case"]
    rc, bufs, ws_ok = _call(name)
    _check(name, rc, bufs, ws_ok)
    L = lib.load()
    w = _weights(name)[0]
    B, S, N, D, spg = c["B"], c["S"], c["N"], c["D"], c["spg"]
    for g, m in enumerate(c["m_groups"]):
        sl = slice(g * spg, (g + 1) * spg)
        pq, docs, lab = (d[k][sl].to(DEV).contiguous() for k in ("pooled_q", "pooled_docs", "labels"))
        one = torch.zeros(spg * S, N, device=DEV)                 # a label matrix of the block's batch: its click count m in one row
        one[-1, :m] = 1.0
        one[: spg * S - 1] = lab.reshape(spg * S, N)[: spg * S - 1]
        assert int((one != 0).sum(1).max()) == m
        sc, ck = Buf(spg, S, N), Buf(spg, S, D)
        need = L.nir_cars_session_workspace_bytes(spg, S, N, C.byref(w))
        ws = torch.empty(need, dtype=torch.uint8, device=DEV)
        rc = L.nir_cars_rank_session_rows(lib.ptr(pq), lib.ptr(docs), lib.ptr(lab), spg, S, N, C.byref(w), lib.ptr(ws), need, sc.ptr(), ck.ptr(), None,
                                          None, 0, lib.ptr(one), spg * S, None, 0, lib.stream())
        torch.cuda.synchronize()
        assert rc == 0 and sc.guards_intact() and ck.guards_intact()
        assert torch.equal(ck.cpu(), bufs["clicks"].cpu()[sl]), g
        if name != "mgroups2_n70":
            # (at N = 70 the merged call's first ranknet GEMM has 560 rows and takes another GEMM kernel than a block's 280: its scores are the
            # separate calls' inside the bound, checked above, not bit for bit)
            assert torch.equal(sc.cpu(), bufs["scores"].cpu()[sl]), g


@pytest.mark.parametrize("N", [3, 64, 65, 130])
@pytest.mark.parametrize("rows", [1, 256, 257])
def test_click_max_against_numpy(rows, N):
    """both forms of nir_cars_click_max (a thread per row in rounds of 256 rows for N <= 64, a wave per row above), three groups; the largest
    count sits in the last row of a group"""
    L = lib.load()
    groups = 3
    g = torch.Generator().manual_seed(rows * 1000 + N)
    lab = (torch.rand(groups, rows, N, generator=g) < 0.3).float() * torch.randint(1, 4, (groups, rows, N), generator=g).float()
    lab[1, rows - 1] = 1.0
    lab[2] = 0.0
    want = np.count_nonzero(lab.numpy(), axis=2).max(axis=1)
    assert want[1] == N and want[2] == 0
    out = torch.full((groups + 2 * 8,), -9, dtype=torch.int32, device=DEV)
    rc = L.nir_cars_click_max(lib.ptr(lab.to(DEV)), groups, rows, N, C.c_void_p(out.data_ptr() + 32), lib.stream())
    torch.cuda.synchronize()
    assert rc == 0
    got = out.cpu().numpy()
    assert (got[8:8 + groups] == want).all(), (got, want)
    assert (got[:8] == -9).all() and (got[8 + groups:] == -9).all()
    assert L.nir_cars_click_max(lib.ptr(lab.to(DEV)), 0, rows, N, C.c_void_p(out.data_ptr() + 32), lib.stream()) == BAD_ARG


SWITCH_CASES = [n for n in R.CASES if n.startswith("switch_")]


@pytest.mark.parametrize("name", SWITCH_CASES)
def test_switches(name):
    c = R.CASES[name]
    extra = EXTRA if (c["q_on"] or c["d_on"]) else None
    rc, bufs, ws_ok = _call(name, extra=extra)
    _check(name, rc, bufs, ws_ok, extra=extra)
    if extra is None:
        # both encoders off with `extra` given is an argument error
        rc, bufs, ws_ok = _call(name, extra=EXTRA)
        assert rc == BAD_ARG and ws_ok and all(b.untouched() for b in bufs.values())
        assert lib.load().nir_last_error_string()


def test_everything_off_writes_nothing():
    name = "switch_q0d0r1"
    w, _ = _weights(name, rank_on=False, pack=False)
    rc, bufs, ws_ok = _call(name, w=w, extra=None)
    assert rc == 0 and ws_ok and all(b.untouched() for b in bufs.values())


def test_optional_outputs():
    """each member of `extra` NULL in turn, no struct at all, clicks_out NULL: what is asked for is written and meets the bound, bit-identical to
    the call that asks for everything; nothing else is touched"""
    name = "switch_q1d1r1"
    rc, full, ws_ok = _call(name)
    _check(name, rc, full, ws_ok)
    for extra, clicks_out in [(tuple(k for k in EXTRA if k != gone), True) for gone in EXTRA] + [(None, True), (EXTRA, False), ((), False)]:
        rc, bufs, ws_ok = _call(name, extra=extra, clicks_out=clicks_out)
        _check(name, rc, bufs, ws_ok, extra=extra, clicks_out=clicks_out, tag=" extra=%s clicks_out=%s" % (extra, clicks_out))
        for k in _produced(R.CASES[name], _weights(name)[0], extra, clicks_out):
            assert torch.equal(bufs[k].cpu(), full[k].cpu()), k


def test_a_single_step_session_and_an_empty_batch():
    rc, bufs, ws_ok = _call("s1")
    _check("s1", rc, bufs, ws_ok)                    # S = 1: dec_h / dec_c have no rows and stay untouched
    rc, bufs, ws_ok = _call("s1", over=dict(B=0))
    assert rc == 0 and ws_ok and all(b.untouched() for b in bufs.values())


def test_entry_point_identities():
    """bitwise: plain == rows with neutral arguments; shard with a slice == the matching columns of the full call (NR = 1, NR = N); query_side
    followed by _pre == rows, for each encoder combination"""
    rc, rows, ws_ok = _call("labels_graded")
    assert rc == 0 and ws_ok
    rc, plain, ws_ok = _call("labels_graded", entry="plain")
    assert rc == 0 and ws_ok
    for k in rows:
        assert torch.equal(rows[k].cpu(), plain[k].cpu()), k
    for sl in ("slice_nr1", "slice_nr5"):
        n0, NR = R.CASES[sl]["cols"]
        rc, full, ws_ok = _call(sl, full=True)
        assert rc == 0 and ws_ok and all(b.guards_intact() for b in full.values())
        rc, part, ws_ok = _call(sl, entry="shard")
        _check(sl, rc, part, ws_ok)
        assert torch.equal(part["scores"].cpu(), full["scores"].cpu()[:, :, n0:n0 + NR])
        for k in ("clicks",) + EXTRA:
            assert torch.equal(part[k].cpu(), full[k].cpu()), k
    L = lib.load()
    for sw in ("switch_q1d1r1", "switch_q1d0r1", "switch_q0d1r1", "switch_q1d1r0", "switch_q0d0r1"):
        c = R.CASES[sw]
        w = _weights(sw)[0]
        extra = EXTRA if (c["q_on"] or c["d_on"]) else None
        rc, rows, ws_ok = _call(sw, extra=extra)
        assert rc == 0 and ws_ok
        nch = int(c["q_on"]) + int(c["d_on"])
        BS = c["B"] * c["S"]
        U, gq = Buf(BS, max(nch * c["HS"] + nch, 1)), Buf(BS, 4 * c["HS"])
        pq = R.build(sw)["pooled_q"].to(DEV).contiguous()
        assert L.nir_cars_session_query_side(lib.ptr(pq), c["B"], c["S"], C.byref(w), U.ptr(), gq.ptr(), lib.stream()) == 0
        torch.cuda.synchronize()
        assert U.guards_intact() and gq.guards_intact()
        assert U.untouched() == (not (nch and c["rank_on"])) and gq.untouched() == (not c["q_on"])
        rc, pre, ws_ok = _call(sw, entry="pre", extra=extra, pre=(U.view, gq.view))
        _check(sw, rc, pre, ws_ok, extra=extra, tag=" pre")
        for k in rows:
            assert torch.equal(rows[k].cpu(), pre[k].cpu()), (sw, k)


def test_argument_errors_are_rejected_before_any_launch():
    """negative return code, no output and no workspace byte written, nir_last_error_string non-empty"""
    L = lib.load()
    name = "labels_graded"
    c = R.CASES[name]
    d = R.build(name)
    lab_all = d["labels"].reshape(-1, c["N"]).to(DEV).contiguous()
    mg = torch.tensor([2, 2, 2], dtype=torch.int32, device=DEV)

    def weights(**f):
        w, keep = R.device_weights(d["sd"], c, DEV)
        for k, v in f.items():
            setattr(w, k, v)
        return w, keep

    bad = [("N = 2049", dict(over=dict(N=2049)), BAD_ARG), ("S = 4097", dict(over=dict(S=4097)), BAD_ARG),
           ("D = 96", dict(w=weights(D=96)), BAD_ARG), ("HS = 24", dict(w=weights(HS=24)), BAD_ARG),
           ("NR = 0", dict(over=dict(rdocs=lib.ptr(lab_all), NR=0)), BAD_ARG), ("NR = N + 1", dict(over=dict(rdocs=lib.ptr(lab_all), NR=c["N"] + 1)), BAD_ARG),
           ("rows_all < B S", dict(over=dict(lab_all=lib.ptr(lab_all), rows_all=c["B"] * c["S"] - 1)), BAD_ARG),
           ("m_groups with labels_all", dict(over=dict(lab_all=lib.ptr(lab_all), rows_all=c["B"] * c["S"], mg=lib.ptr(mg), spg=1)), BAD_ARG),
           ("sessions_per_group = 0", dict(over=dict(mg=lib.ptr(mg), spg=0)), BAD_ARG),
           ("B % sessions_per_group != 0", dict(over=dict(mg=lib.ptr(mg), spg=2)), BAD_ARG),
           ("document session on, labels NULL", dict(null=("labels",)), BAD_ARG),
           ("ranker on, nothing packed", dict(w=weights(wrank=None)), BAD_ARG),
           ("ranker on, attention weights not packed", dict(w=weights(attn_ut=None)), BAD_ARG),
           ("ranker on, scores NULL", dict(null=("scores",)), BAD_ARG),
           ("workspace one byte short", dict(ws_short=1), ERR_WORKSPACE)]
    assert c["B"] == 3
    for what, kw, want in bad:
        held = kw.pop("w", None)                     # (struct, the tensors it points into)
        rc, bufs, ws_ok = _call(name, w=held[0] if held else None, **kw)
        msg = L.nir_last_error_string()
        print(what, rc, msg)
        assert rc == want and rc < 0, (what, rc)
        assert ws_ok and all(b.untouched() for b in bufs.values()), what
        assert msg, what
    # and the same call with nothing wrong goes through
    rc, bufs, ws_ok = _call(name)
    _check(name, rc, bufs, ws_ok)


def test_workspace_bytes():
    """sufficient for every case (each call above runs on exactly this many bytes between guards), 0 for dimensions that cannot be"""
    L = lib.load()
    w = _weights("labels_graded")[0]
    assert L.nir_cars_session_workspace_bytes(3, 3, 5, C.byref(w)) > 0
    assert L.nir_cars_session_workspace_bytes(0, 3, 5, C.byref(w)) == 0           # an empty batch is a valid call and needs nothing
    for B, S, N in ((-1, 3, 5), (3, 0, 5), (3, 3, 0), (3, -2, 5)):
        assert L.nir_cars_session_workspace_bytes(B, S, N, C.byref(w)) == 0
    assert L.nir_cars_session_workspace_bytes(3, 3, 5, None) == 0
