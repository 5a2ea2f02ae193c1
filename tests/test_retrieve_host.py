"""CPU: corpus retrieval (include/neuroir_retrieve.h; retrieval.DocumentIndex; Ranker.build_index / search) without a device -- the criterion of
tests/retrieve_ref.py itself (honest float32 arithmetic accepted under several summation orders, every planted fault rejected), the symbols
and their prototypes, the refusals of every entry, the index's host logic and the wrapper's refusal of the other rankers."""
import os
import re

import numpy as np
import pytest
import torch

import retrieve_ref as R

C = R.chunk_docs()
NAMES = {"nir_retrieve_index_bytes", "nir_retrieve_add", "nir_retrieve_export", "nir_retrieve_import", "nir_retrieve_topk_workspace_bytes",
         "nir_retrieve_topk", "nir_retrieve_merge", "nir_retrieve_chunk_docs"}
CASE_NAMES = [c[0] for c in R.case_list(C)]


# ---- the criterion ------------------------------------------------------------------------------------------------------------------------------
def test_the_case_list_covers_every_seam():
    cases = R.case_list(C)
    assert C % 128 == 0 and C >= 256
    Ms, Ds, Bs, ks = ({c[i] for c in cases} for i in (2, 3, 1, 4))
    assert {1, 127, 128, 129, C - 1, C, C + 1, 2 * C + 1} <= Ms and {1, 4, 37, 128, 256} <= Ds and {1, 31, 32, 33, 65} <= Bs
    assert {1, 2, 8, 64, 128} <= ks
    assert any(c[2] == c[4] - 1 for c in cases) and any(c[2] == c[4] for c in cases) and any(c[4] > c[2] + 1 for c in cases)
    assert all(c[3] == 8 for c in cases if c[2] > C)                             # D = 8 at the multi-chunk sizes
    assert {c[5] for c in cases} >= {"one_chunk", "spread", "dups", "zeros", "best_last", "best_first"}
    assert len(R.FAULTS) >= 10 and set(R.FAULT_CASE) == set(R.FAULTS) and set(R.FAULT_CASE.values()) <= set(CASE_NAMES)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_honest_float32_arithmetic_is_accepted_in_every_order(name):
    c = R.make_case(name, C)
    s64 = R.scores64(c["q"], c["d"])
    assert np.isfinite(s64).all()
    for order in R.ORDERS:
        s32 = R.dot32(R.unit32(c["q"]), R.unit32(c["d"]), order)
        err = float(np.abs(s32.astype(np.float64) - s64).max())
        assert err <= R.E_S(c["D"]), (order, err, R.E_S(c["D"]))
        val, idx = R.model_topk(c["q"], c["d"], c["k"], C, order)
        ok, why = R.accept(val, idx, c["q"], c["d"], c["k"])
        assert ok, (order, why)


def test_the_planted_contents_are_what_they_claim():
    z = R.make_case("zeros", C)
    s = R.scores64(z["q"], z["d"])
    assert (s[:, 3] == 0).all() and (s[1] == 0).all() and abs(s[0, 5] - 0.1) < 1e-6          # zero rows score 0; the 1e-9 row is clamped
    val, idx = R.model_topk(z["q"], z["d"], z["k"], C)
    assert idx[1].tolist() == list(range(40))                                        # all-equal scores: ascending document order
    for name in ("one_chunk", "spread", "dups", "best_last", "best_first"):
        c = R.make_case(name, C)
        _, idx = R.topk64(R.scores64(c["q"], c["d"])[0], c["k"])
        assert set(c["planted"]) <= set(idx.tolist()) or name == "dups"
        if name == "dups":
            assert idx[:6].tolist() == c["planted"]                                  # exact duplicates tie; the smaller index first
    one, spread = R.make_case("one_chunk", C), R.make_case("spread", C)
    assert all(C <= j < 2 * C for j in one["planted"]) and sorted(j // C for j in spread["planted"]) == [0, 1, 2]


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_planted_fault_is_rejected(fault):
    c = R.make_case(R.FAULT_CASE[fault], C)
    val, idx = R.model_topk(c["q"], c["d"], c["k"], C)
    assert R.accept(val, idx, c["q"], c["d"], c["k"])[0]
    val, idx = R.model_topk(c["q"], c["d"], c["k"], C, fault=fault)
    ok, why = R.accept(val, idx, c["q"], c["d"], c["k"])
    assert not ok, fault
    print(fault, "->", why)


def test_merge64_is_the_top_k_of_the_union():
    rng = np.random.default_rng(5)
    s = rng.standard_normal(300).round(1)                                            # many equal values
    k = 16
    parts = [R.topk64(s[lo:lo + 64], k) for lo in range(0, 300, 64)]
    vals = np.stack([p[0] for p in parts])
    idx = np.stack([np.where(p[1] >= 0, p[1] + lo, -1) for p, lo in zip(parts, range(0, 300, 64))])
    v, i = R.merge64(vals, idx, k)
    wv, wi = R.topk64(s, k)
    assert np.array_equal(v, wv) and np.array_equal(i, wi)


# ---- symbols and arguments ----------------------------------------------------------------------------------------------------------------------
def _families(lib):
    return [getattr(lib, n) for n in dir(lib) if n.endswith("SIGNATURES") and n != "RETRIEVE_SIGNATURES"]


def test_new_symbols_exist_with_their_prototypes():
    from conftest import ROOT
    from context_attentive_ir_amd import lib
    main = open(os.path.join(ROOT, "include", "neuroir_hip.h")).read()
    assert "neuroir_retrieve.h" not in main and not re.findall(r"\bnir_retrieve\w*", main)       # a header of its own
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuroir_retrieve.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(nir_[a-z0-9_]+)\s*\(", hdr))
    assert NAMES == declared == set(lib.RETRIEVE_SIGNATURES) and all(n.startswith("nir_retrieve_") for n in NAMES)
    fams = _families(lib)
    assert len(fams) >= 12
    for fam in fams:
        assert not NAMES & set(fam)
    L = lib.load()
    for n in NAMES:
        assert hasattr(L, n), n
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, hdr, re.S)
        nargs = len([a for a in m.group(1).split(",") if a.strip() and a.strip() != "void"])
        assert nargs == len(lib.RETRIEVE_SIGNATURES[n][1]), n
        assert getattr(L, n).argtypes == lib.RETRIEVE_SIGNATURES[n][1]               # registered by lib.load
    assert int(re.search(r"#define NIR_RETRIEVE_MAX_K (\d+)", hdr).group(1)) == lib.RETRIEVE_MAX_K == 128
    assert int(re.search(r"#define NIR_RETRIEVE_MAX_D (\d+)", hdr).group(1)) == lib.RETRIEVE_MAX_D == 256


def test_the_entries_refuse_bad_arguments_before_any_launch():
    """over fake pointers: nothing may be enqueued (no device needed)"""
    from context_attentive_ir_amd import lib
    L = lib.load()
    err = lambda: L.nir_last_error_string()                                          # noqa: E731
    p, big = lib.C.c_void_p(256), 1 << 40
    ib = L.nir_retrieve_index_bytes
    assert ib(0, 8) == 0 and ib(1, 8) == 32 * 8 * 4 and ib(33, 37) == 64 * 40 * 4 and ib(100, 256) == 128 * 256 * 4
    assert ib(-1, 8) == 0 and ib(10, 0) == 0 and ib(10, 257) == 0 and ib(1 << 31, 8) == 0

    def add(reps=p, m=4, D=8, index=p, cap=100, off=0):
        return L.nir_retrieve_add(reps, m, D, index, cap, off, None, None)
    for kw in (dict(D=0), dict(D=257), dict(m=-1), dict(off=-1), dict(off=97), dict(m=101), dict(cap=-1), dict(cap=1 << 31)):
        assert add(**kw) == -1 and b"retrieve_add" in err(), kw
    assert add(reps=None) == -1 and b"null" in err() and add(index=None) == -1 and b"null" in err()
    assert add(index=lib.C.c_void_p(260)) == -1 and b"aligned" in err()
    assert add(m=0, reps=None, index=None) == 0                                       # nothing to add: nothing enqueued
    for fn, name in ((lambda **k: L.nir_retrieve_export(k.get("index", p), k.get("cap", 100), k.get("D", 8), k.get("off", 0), k.get("m", 4),
                                                          k.get("rows", p), None), b"retrieve_export"),
                     (lambda **k: L.nir_retrieve_import(k.get("rows", p), k.get("m", 4), k.get("D", 8), k.get("index", p), k.get("cap", 100),
                                                          k.get("off", 0), None), b"retrieve_import")):
        for kw in (dict(D=0), dict(D=257), dict(m=-1), dict(off=-1), dict(off=97), dict(m=101)):
            assert fn(**kw) == -1 and name in err(), kw
        assert fn(rows=None) == -1 and b"null" in err() and fn(index=None) == -1 and b"null" in err()
        assert fn(m=0, rows=None, index=None) == 0

    size = L.nir_retrieve_topk_workspace_bytes

    def topk(q=p, B=3, index=p, M=1000, D=8, k=4, form=0, ws=p, wsb=big, val=p, idx=p):
        return L.nir_retrieve_topk(q, B, index, M, D, k, form, ws, wsb, None, val, idx, None)
    for kw in (dict(B=-1), dict(B=1 << 31), dict(M=-1), dict(M=1 << 31), dict(D=0), dict(D=257), dict(k=0), dict(k=129), dict(form=3), dict(form=-1)):
        assert topk(**kw) == -1 and b"retrieve_topk" in err(), kw
        a = dict(B=3, M=1000, D=8, k=4, form=0)
        a.update(kw)
        assert size(a["B"], a["M"], a["D"], a["k"], a["form"]) == 0
    for kw in (dict(q=None), dict(index=None), dict(val=None), dict(idx=None)):
        assert topk(**kw) == -1 and b"null" in err(), kw
    assert topk(index=lib.C.c_void_p(264)) == -1 and b"aligned" in err()
    for form in (1, 2):                                                               # both forms: a short or a null workspace
        need = size(3, 2 * C + 1, 8, 4, form)
        assert need > 0
        assert topk(M=2 * C + 1, form=form, wsb=need - 1) == -3 and b"workspace" in err()
        assert topk(M=2 * C + 1, form=form, ws=None) == -3 and b"workspace" in err()
    assert size(3, C, 8, 4, 1) == 0                                                   # one chunk, fused: the lists go straight to the outputs
    assert size(3, 1000, 8, 4, 2) >= 3 * 1000 * 4                                     # plain: the score matrix
    fused, plain = size(64, 10 ** 6, 128, 100, 1), size(64, 10 ** 6, 128, 100, 2)
    chunks = -(-10 ** 6 // C)
    assert fused <= 2 * (chunks + -(-chunks // 31) + 2) * 64 * 100 * 4 + 4096 and plain >= fused + 64 * 10 ** 6 * 4      # O(chunks B k) against [B, M]
    assert topk(B=0, q=None, val=None, idx=None, ws=None, wsb=0) == 0                 # no queries: nothing to enqueue

    def merge(vals=p, idx=p, P=3, B=2, k=4, ov=p, oi=p):
        return L.nir_retrieve_merge(vals, idx, P, B, k, ov, oi, None)
    for kw in (dict(P=0), dict(P=1 << 20), dict(B=-1), dict(B=1 << 31), dict(k=0), dict(k=129)):
        assert merge(**kw) == -1 and b"retrieve_merge" in err(), kw
    for kw in (dict(vals=None), dict(idx=None), dict(ov=None), dict(oi=None)):
        assert merge(**kw) == -1 and b"null" in err(), kw
    assert merge(B=0, vals=None, idx=None, ov=None, oi=None) == 0


# ---- the index's host logic and the wrapper ------------------------------------------------------------------------------------------------------
def test_document_index_host_logic():
    from context_attentive_ir_amd import retrieval as X
    assert X.next_capacity(0, 1) == X.MIN_CAPACITY and X.next_capacity(0, X.MIN_CAPACITY + 1) == 2 * X.MIN_CAPACITY
    caps, cap = [], 0
    for need in range(1, 40000, 997):                                                 # geometric: a logarithmic number of distinct capacities
        cap = X.next_capacity(cap, need)
        assert cap >= need
        caps.append(cap)
    assert len(set(caps)) <= 7 and caps == sorted(caps)
    for bad in (0, 257, -3):
        with pytest.raises(ValueError):
            X.DocumentIndex(bad)
    ix = X.DocumentIndex(16)
    assert len(ix) == 0 and ix.count == 0 and ix.capacity == 0
    serials = [ix.serial]
    for _ in range(50):                                                               # a serial is never handed out twice, unlike id()
        serials.append(X.DocumentIndex(16).serial)
    assert serials == sorted(set(serials))
    sd = ix.state_dict()                                                              # an empty index never touches a device
    assert sd["dim"] == 16 and sd["count"] == 0 and tuple(sd["rows"].shape) == (0, 16)
    iy = X.DocumentIndex(16).load_state_dict(sd)
    assert iy.count == 0 and iy.state_dict()["rows"].shape == sd["rows"].shape
    for bad in (dict(sd, dim=8), dict(sd, count=3), dict(sd, rows=torch.zeros(2, 8)), {"dim": 16}):
        with pytest.raises(ValueError):
            X.DocumentIndex(16).load_state_dict(bad)
    with pytest.raises(ValueError):
        ix.search(torch.zeros(2, 16), 0)
    with pytest.raises(ValueError):
        ix.search(torch.zeros(2, 16), 129)
    with pytest.raises(ValueError):
        ix.add(torch.zeros(2, 8))
    with pytest.raises(RuntimeError, match="ROCm device"):                            # valid arguments reach the device check: there is no CPU path
        X.DocumentIndex(16, "cpu").add(torch.zeros(2, 16))


def test_the_wrapper_refuses_the_other_rankers_and_train_mode():
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.wrappers import Ranker
    from context_attentive_ir_amd.wrappers.ranker import NETWORKS
    others = sorted(set(NETWORKS) - {"DSSM", "CDSSM"})
    assert len(others) == 6
    for kind in others:
        r = Ranker.__new__(Ranker)                                                    # the refusal needs no network
        r.kind = kind
        for call in (lambda: r.build_index([]), lambda: r.search({}, None, 3)):
            with pytest.raises(RuntimeError, match="DSSM or CDSSM") as e:
                call()
            assert kind in str(e.value)
    for kind in ("dssm", "cdssm"):
        r = Ranker(default_args(kind, src_vocab_size=50))
        ids = torch.zeros(2, 6, dtype=torch.long)
        r.network.train()
        for fn in (r.network.encode_queries, r.network.encode_documents):
            with pytest.raises(NotImplementedError, match="eval mode"):
                fn(ids)
        r.network.eval()
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            r.network.encode_documents(ids)
