"""GPU (-m gpu): the retrieval entries at the C ABI (include/neuroir_retrieve.h, csrc/retrieve.hip) under the criterion of tests/retrieve_ref.py --
every case in both forms, the same bits on a second call, pair-score bits that do not depend on the document's position, on B, M, k or the form,
an index added in ragged pieces, nir_retrieve_merge against the float64 merge, the non-finite rule, and one index beyond the 4 GiB byte offset."""
import numpy as np
import pytest
import torch

import retrieve_ref as R
from conftest import T

pytestmark = pytest.mark.gpu
DEV = "cuda"
FUSED, PLAIN = 1, 2


def _lib():
    from context_attentive_ir_amd import lib
    return lib, lib.load()


def _index(d, pieces=None, flag=None):
    """documents d [M, D] (numpy float32) -> (zero-initialised index buffer, capacity), added in `pieces` (sizes; default: one call)"""
    lib, L = _lib()
    M, D = d.shape
    buf = torch.zeros(max(L.nir_retrieve_index_bytes(M, D), 256), dtype=torch.uint8, device=DEV)
    dd = T(d, DEV)
    off = 0
    for m in (pieces or [M]):
        part = dd[off:off + m].contiguous()
        lib.check(L.nir_retrieve_add(lib.ptr(part), m, D, lib.ptr(buf), M, off, lib.ptr(flag), lib.stream()), "nir_retrieve_add")
        off += m
    assert off == M
    return buf


def _topk(q, buf, M, k, form, flag=None):
    lib, L = _lib()
    qq = T(q, DEV)
    B, D = q.shape
    val = torch.full((B, k), 7.0, device=DEV)
    idx = torch.full((B, k), -7, dtype=torch.int32, device=DEV)
    ws = torch.empty(max(L.nir_retrieve_topk_workspace_bytes(B, M, D, k, form), 256), dtype=torch.uint8, device=DEV)
    lib.check(L.nir_retrieve_topk(lib.ptr(qq), B, lib.ptr(buf), M, D, k, form, lib.ptr(ws), ws.numel(), lib.ptr(flag), lib.ptr(val), lib.ptr(idx),
                                  lib.stream()), "nir_retrieve_topk")
    return val.cpu().numpy(), idx.cpu().numpy()


C = None


def _c():
    global C
    if C is None:
        C = R.chunk_docs()
    return C


_CASES = {}


def _case(name):
    """the case, its index and nothing else: built once, shared by the forms, never changed"""
    if name not in _CASES:
        c = R.make_case(name, _c())
        _CASES[name] = (c, _index(c["d"]))
    return _CASES[name]


@pytest.mark.parametrize("form", [FUSED, PLAIN], ids=["fused", "plain"])
@pytest.mark.parametrize("name", [c[0] for c in R.case_list(4096)])          # (the names do not depend on the chunk size)
def test_every_case_meets_the_criterion_and_repeats_its_bits(name, form):
    c, buf = _case(name)
    val, idx = _topk(c["q"], buf, c["M"], c["k"], form)
    ok, why = R.accept(val, idx, c["q"], c["d"], c["k"])
    assert ok, why
    val2, idx2 = _topk(c["q"], buf, c["M"], c["k"], form)
    assert np.array_equal(val.view(np.uint32), val2.view(np.uint32)) and np.array_equal(idx, idx2)
    if c["planted"] and name not in ("zeros",):
        assert set(c["planted"]) <= set(idx[0].tolist())


def test_the_forms_agree_bit_for_bit():
    for name in ("d37", "m2C+1", "dups"):
        c, buf = _case(name)
        a, b = _topk(c["q"], buf, c["M"], c["k"], FUSED), _topk(c["q"], buf, c["M"], c["k"], PLAIN)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1], b[1])


def _pair_bits(val, idx, M):
    """[B, M] uint32: the score bits of every (query, document) pair of a k = M result"""
    out = np.zeros((val.shape[0], M), np.uint32)
    for b in range(val.shape[0]):
        assert sorted(idx[b].tolist()) == list(range(M))
        out[b, idx[b]] = val[b].view(np.uint32)
    return out


@pytest.mark.parametrize("D", [37, 128])
def test_pair_score_bits_do_not_depend_on_position_batch_or_k(D):
    rng = np.random.default_rng(D)
    M, B = 100, 65
    q = rng.standard_normal((B, D)).astype(np.float32)
    d = rng.standard_normal((M, D)).astype(np.float32)
    base = _pair_bits(*_topk(q, _index(d), M, M, FUSED), M)
    perm = rng.permutation(M)
    moved = _pair_bits(*_topk(q, _index(d[perm]), M, M, FUSED), M)                    # document perm[j] now sits at position j
    assert np.array_equal(moved, base[:, perm])
    one = _pair_bits(*_topk(q[:1], _index(d), M, M, FUSED), M)                        # B = 1 against B = 65 (another tile width)
    assert np.array_equal(one[0], base[0])
    last = _pair_bits(*_topk(q[64:], _index(d), M, M, PLAIN), M)
    assert np.array_equal(last[0], base[64])
    # a larger M and a smaller k: documents appended behind, the same pairs at the top
    more = np.concatenate([d, 0.01 * rng.standard_normal((_c() + 30, D)).astype(np.float32) - 5.0 * q[0] / np.linalg.norm(q[0])])
    val, idx = _topk(q[:1], _index(more), more.shape[0], 8, FUSED)
    want = np.sort(base[0].view(np.float32))[::-1][:8]
    assert (idx[0] < M).all() and np.array_equal(val[0], want)


def test_an_index_added_in_pieces_is_bit_equal_to_a_one_shot_build():
    rng = np.random.default_rng(2)
    for D in (5, 128):
        d = rng.standard_normal((300, D)).astype(np.float32)
        whole = _index(d)
        ragged = _index(d, [100, 29, 1, 2, 31, 33, 64, 40])
        assert torch.equal(whole, ragged)
        lib, L = _lib()
        rows = torch.empty(300, D, device=DEV)
        lib.check(L.nir_retrieve_export(lib.ptr(whole), 300, D, 0, 300, lib.ptr(rows), lib.stream()), "nir_retrieve_export")
        want = R.unit64(d)
        assert float((rows.cpu().double() - T(want)).abs().max()) < 4 * 2.0 ** -24
        back = torch.zeros_like(whole)
        for lo, m in ((0, 77), (77, 223)):
            part = rows[lo:lo + m].contiguous()
            lib.check(L.nir_retrieve_import(lib.ptr(part), m, D, lib.ptr(back), 300, lo, lib.stream()), "nir_retrieve_import")
        assert torch.equal(back, whole)                                               # export / import move the stored bits


@pytest.mark.parametrize("P,k", [(1, 8), (2, 1), (31, 128), (32, 64), (70, 8), (200, 100)])
def test_merge_against_the_float64_merge(P, k):
    lib, L = _lib()
    rng = np.random.default_rng(P * 131 + k)
    B, n = 3, 150
    vals = np.full((P, B, k), -np.inf, np.float32)
    idx = np.full((P, B, k), -1, np.int32)
    for p in range(P):
        for b in range(B):
            s = rng.standard_normal(n).round(1).astype(np.float32) + 0.0              # many equal values across the lists
            m = min(k, int(rng.integers(0, n)))                                       # ragged: some lists are short, some empty
            v, i = R.topk64(s.astype(np.float64)[:m] if m else np.zeros(0), k)
            vals[p, b], idx[p, b] = v, np.where(i >= 0, i + p * n, -1)
    ov = torch.empty(B, k, device=DEV)
    oi = torch.empty(B, k, dtype=torch.int32, device=DEV)
    tv, ti = T(vals, DEV), T(idx, DEV)
    lib.check(L.nir_retrieve_merge(lib.ptr(tv), lib.ptr(ti), P, B, k, lib.ptr(ov), lib.ptr(oi), lib.stream()), "nir_retrieve_merge")
    for b in range(B):
        wv, wi = R.merge64(vals[:, b], idx[:, b], k)
        assert np.array_equal(ov[b].cpu().numpy().astype(np.float64), wv) and np.array_equal(oi[b].cpu().numpy(), wi)


def test_non_finite_rows_count_as_zeros_and_raise_the_flag():
    rng = np.random.default_rng(8)
    q = rng.standard_normal((3, 16)).astype(np.float32)
    d = rng.standard_normal((20, 16)).astype(np.float32)
    d[4, 3], d[9, 0], q[2, 5] = np.inf, np.nan, -np.inf
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    buf = _index(d, flag=flag)
    assert int(flag.item()) == 1
    for form in (FUSED, PLAIN):
        flag.zero_()
        val, idx = _topk(q, buf, 20, 20, form, flag)
        assert int(flag.item()) == 2
        ok, why = R.accept(val, idx, q, d, 20)                                        # the restatement zeroes the same rows
        assert ok, why
        assert (val[2] == 0).all() and idx[2].tolist() == list(range(20))
        pos = {int(j): float(v) for v, j in zip(val[0], idx[0])}
        assert pos[4] == 0.0 and pos[9] == 0.0
    val, idx = _topk(q[:2], buf, 20, 20, FUSED, flag=None)                             # a null flag is allowed
    assert np.isfinite(val).all()


def test_an_empty_index_returns_empty_slots():
    q = np.ones((2, 8), np.float32)
    buf = torch.zeros(256, dtype=torch.uint8, device=DEV)
    for form in (FUSED, PLAIN):
        val, idx = _topk(q, buf, 0, 5, form)
        assert np.isneginf(val).all() and (idx == -1).all()


def test_an_index_beyond_the_4_gib_byte_offset():
    """D = 256, M = 2^22 + 64 documents: document 2^22 starts at byte 2^32 of the index.  The index is zero-filled on the device and a few rows are
    planted on both sides of that line, so the planted rows hold the only non-zero scores: the result is the planted rows with a positive cosine
    in the order of their cosines, then the zero documents 0, 1, 2 ... with a score of exactly 0."""
    lib, L = _lib()
    D, M, k = 256, (1 << 22) + 64, 8
    nbytes = L.nir_retrieve_index_bytes(M, D)
    assert nbytes > (1 << 32)
    free = torch.cuda.mem_get_info()[0]
    assert free > nbytes + (1 << 30), "the device has no room for a %.1f GB index" % (nbytes / 1e9)
    buf = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    rng = np.random.default_rng(4)
    q = rng.standard_normal((1, D)).astype(np.float32)
    p = rng.standard_normal(D).astype(np.float32)
    spots = [5, (1 << 22) - 1, 1 << 22, (1 << 22) + 1, M - 1, 2, 1 << 21]
    tilt = [0.9, 0.1, 0.5, 0.3, 0.7, None, 1.5]                                       # None: the row -q (cosine -1: behind every zero document)
    rows = np.stack([(-q[0] if t is None else q[0] + t * p * np.linalg.norm(q[0]) / np.linalg.norm(p)) for t in tilt]).astype(np.float32)
    for j, r in zip(spots, rows):
        rr = T(r[None], DEV)
        lib.check(L.nir_retrieve_add(lib.ptr(rr), 1, D, lib.ptr(buf), M, j, None, lib.stream()), "nir_retrieve_add")
    s = R.scores64(q, rows)[0]
    live = [(float(s[i]), spots[i]) for i in range(len(spots)) if tilt[i] is not None]
    want_idx = [j for _, j in sorted(live, key=lambda t: -t[0])] + [0, 1]             # 6 planted rows, then the first zero documents (2 is -q)
    s64 = np.zeros(M)
    s64[spots] = s
    for form in (FUSED, PLAIN):
        val, idx = _topk(q, buf, M, k, form)
        assert idx[0].tolist() == want_idx, (form, idx[0].tolist(), want_idx)
        ok, why = R.accept_row(val[0], idx[0], s64, k, D)
        assert ok, why
        assert (val[0, 6:] == 0).all()
    del buf
    torch.cuda.empty_cache()
