"""The acceptance criterion of corpus retrieval (include/neuroir_retrieve.h): an fp64 restatement of the clamp cosine, a
float64 top-k, the cases at every seam of the kernels, and a numpy model of honest and of faulty results.

Tolerance -- derived, not tuned.  With q^ = q / max(|q|, 1e-8) and d^ likewise, sum_i |q^_i d^_i| <= |q^| |d^| <= 1 (Cauchy-Schwarz), so ANY
order of an fp32 sum of the D products is off by at most about D u (u = 2^-24: one rounding per product and per addition, each relative to a
partial sum bounded by 1); the two normalisations (a sum of squares, a square root, a division per component) move every component by a handful
of ulps, i.e. the dot product by a handful of u more.  E_S = (D + 16) 2^-24.

A row is accepted iff, with s64 the float64 scores and t the k-th largest of them (the smallest when k > M):
  every returned index lies in [0, M) and is distinct;  |top_val - s64[top_idx]| <= E_S;  every j with s64[j] > t + 2 E_S is returned;  every
  returned j has s64[j] >= t - 2 E_S;  the device's own values are non-increasing;  equal device bits appear in ascending index order;  slots
  beyond M hold (-inf, -1).  No share of rows is exempt, so near-ties need no allowance.
"""
import numpy as np

EPS = 1e-8


def E_S(D):
    return (D + 16) * 2.0 ** -24


def chunk_docs():
    from context_attentive_ir_amd import lib
    return int(lib.load().nir_retrieve_chunk_docs())


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------------
def unit64(x):
    """rows of x / max(|x|, 1e-8) in float64; a row with a non-finite component counts as zeros"""
    x = np.asarray(x, np.float64)
    bad = ~np.isfinite(x).all(1)
    x = np.where(bad[:, None], 0.0, x)
    return x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), EPS)


def scores64(q, d):
    return unit64(q) @ unit64(d).T


def order_desc(vals, idx):
    """positions sorted by (value descending, index ascending)"""
    return np.lexsort((idx, -vals))


def topk64(s, k):
    """s [M] float64 -> (values [k], indices [k]); slots beyond M: (-inf, -1)"""
    M = s.shape[0]
    o = order_desc(s, np.arange(M))[:k]
    val = np.full(k, -np.inf)
    idx = np.full(k, -1, np.int64)
    val[:o.size], idx[:o.size] = s[o], o
    return val, idx


def merge64(vals, idx, k):
    """P partial lists vals / idx [P, k] of one query -> the merged (values [k], indices [k]) under the same rule; (-inf, -1) entries are empty"""
    v, i = np.asarray(vals, np.float64).reshape(-1), np.asarray(idx, np.int64).reshape(-1)
    keep = i >= 0
    v, i = v[keep], i[keep]
    o = order_desc(v, i)[:k]
    out_v, out_i = np.full(k, -np.inf), np.full(k, -1, np.int64)
    out_v[:o.size], out_i[:o.size] = v[o], i[o]
    return out_v, out_i


def accept_row(top_val, top_idx, s64, k, D):
    """-> (ok, reason) for one query"""
    M = s64.shape[0]
    E = E_S(D)
    n = min(k, M)
    top_val, top_idx = np.asarray(top_val), np.asarray(top_idx).astype(np.int64)
    if top_val.shape != (k,) or top_idx.shape != (k,):
        return False, "shape"
    val, idx = top_val[:n].astype(np.float64), top_idx[:n]
    if np.isnan(top_val.astype(np.float64)).any():
        return False, "nan"
    if not ((idx >= 0) & (idx < M)).all():
        return False, "index outside [0, M)"
    if np.unique(idx).size != n:
        return False, "index repeated"
    if not (np.isneginf(top_val[n:].astype(np.float64)).all() and (top_idx[n:] == -1).all()):
        return False, "slots beyond M are not (-inf, -1)"
    if n == 0:
        return True, ""
    if np.abs(val - s64[idx]).max() > E:
        return False, "value off by %.3g > %.3g" % (np.abs(val - s64[idx]).max(), E)
    t = np.sort(s64)[M - n]
    must = np.nonzero(s64 > t + 2 * E)[0]
    if not np.isin(must, idx).all():
        return False, "a document above t + 2 E_S is missing"
    if (s64[idx] < t - 2 * E).any():
        return False, "a document below t - 2 E_S is returned"
    if (np.diff(val) > 0).any():
        return False, "values increase"
    bits = top_val[:n].astype(np.float32).view(np.uint32)
    same = bits[1:] == bits[:-1]
    if (idx[1:][same] <= idx[:-1][same]).any():
        return False, "equal values out of index order"
    return True, ""


def accept(top_val, top_idx, q, d, k):
    """all queries: -> (ok, (row, reason) of the first failure or None)"""
    D = q.shape[1]
    s = scores64(q, d) if d.shape[0] else np.zeros((q.shape[0], 0))
    for b in range(q.shape[0]):
        ok, why = accept_row(top_val[b], top_idx[b], s[b], k, D)
        if not ok:
            return False, (b, why)
    return True, None


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------------
def case_list(C):
    """(name, B, M, D, k, plant): small shapes at every seam -- M around k, the 128-document step and the chunk C (D = 8 at the multi-chunk
    sizes), every D class, B around the 32- and 64-query tiles, every k class and k > M; then the planted contents"""
    return [
        ("m1", 1, 1, 8, 1, None), ("m_k-1", 2, 7, 8, 8, None), ("m_k", 2, 8, 8, 8, None), ("m127", 31, 127, 4, 8, None),
        ("m128", 32, 128, 8, 8, None), ("m129", 33, 129, 8, 2, None), ("mC-1", 1, C - 1, 8, 8, None), ("mC", 2, C, 8, 64, None),
        ("mC+1", 33, C + 1, 8, 8, None), ("m2C+1", 65, 2 * C + 1, 8, 128, None),
        ("d1", 3, 300, 1, 8, None), ("d4", 2, 131, 4, 1, None), ("d37", 5, 300, 37, 64, None), ("d128", 65, 257, 128, 128, None),
        ("d256", 33, 200, 256, 128, None), ("d256_two_tiles", 65, 130, 256, 8, None),
        ("k_gt_m", 3, 50, 16, 128, None), ("k2", 4, 129, 8, 2, None), ("k32", 33, 300, 16, 32, None), ("k33", 33, 300, 16, 33, None),
        ("one_chunk", 2, 2 * C + 1, 8, 64, "one_chunk"), ("spread", 2, 3 * C - 7, 8, 3, "spread"), ("dups", 2, C + 200, 8, 8, "dups"),
        ("zeros", 3, 40, 16, 40, "zeros"), ("best_last", 2, C + 77, 8, 2, "best_last"), ("best_first", 2, C + 77, 8, 2, "best_first"),
    ]


def make_case(name, C):
    """-> dict(q [B, D], d [M, D] float32 raw representations, k, planted: indices the plant concerns)"""
    name, B, M, D, k, plant = next(c for c in case_list(C) if c[0] == name)
    rng = np.random.default_rng(sum(map(ord, name)) * 7919 + 11)          # seeded by the name, not by Python's salted hash
    q = (rng.standard_normal((B, D)) * 1.7).astype(np.float32)
    d = (rng.standard_normal((M, D)) * 0.6).astype(np.float32)
    planted = []

    def near(v, eps):
        return (v * 2.5 + eps * rng.standard_normal(D)).astype(np.float32)
    if plant == "one_chunk":            # all of query 0's top-k inside chunk 1
        planted = list(range(C + 5, C + 5 + k))
        for j in planted:
            d[j] = near(q[0], 0.02)
    elif plant == "spread":             # one winner per chunk
        planted = [17, C + 4000, 2 * C + 1]
        for j in planted:
            d[j] = near(q[0], 0.01)
    elif plant == "dups":               # exact duplicates across a 32-document group, a 128-document step and the chunk seam
        planted = [31, 32, 127, 128, C - 1, C]
        v = near(q[0], 0.01)
        for j in planted:
            d[j] = v
    elif plant == "zeros":              # a zero document, a zero query, a row below the clamp
        d[3] = 0.0
        q[1] = 0.0
        d[5] = (q[0] / np.linalg.norm(q[0]) * 1e-9).astype(np.float32)
        planted = [3, 5]
    elif plant == "best_last":
        planted = [M - 1]
        d[M - 1] = near(q[0], 0.0)
    elif plant == "best_first":
        planted = [0]
        d[0] = near(q[0], 0.0)
    return dict(name=name, q=q, d=d, k=k, planted=planted, D=D, B=B, M=M)


# ---- a numpy float32 model of the result, honest or with one planted fault -------------------------------------------------------------------------
ORDERS = ("fwd", "rev", "pairwise", "blocks")
FAULTS = ("last_chunk_dropped", "padding_columns_returned", "chunk_base_not_added", "chunk_lists_truncated", "tie_order_reversed",
          "duplicate_emitted_twice", "clamp_missing", "query_not_normalised", "document_not_normalised", "k_gt_m_filled_with_zeros",
          "merge_not_stable")
# the case on which each fault must show
FAULT_CASE = {"last_chunk_dropped": "best_last", "padding_columns_returned": "k_gt_m", "chunk_base_not_added": "spread",
              "chunk_lists_truncated": "one_chunk", "tie_order_reversed": "dups", "duplicate_emitted_twice": "m_k", "clamp_missing": "zeros",
              "query_not_normalised": "m128", "document_not_normalised": "m128", "k_gt_m_filled_with_zeros": "k_gt_m", "merge_not_stable": "dups"}


def unit32(x, clamp=True):
    x = np.asarray(x, np.float32)
    n = np.sqrt((x * x).sum(1, keepdims=True, dtype=np.float32), dtype=np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return (x / (np.maximum(n, np.float32(EPS)) if clamp else n)).astype(np.float32)


def dot32(qh, dh, order):
    """float32 scores [B, M] under one summation order of the D products"""
    D = qh.shape[1]
    if order == "pairwise":
        return (qh[:, None, :] * dh[None, :, :]).sum(-1, dtype=np.float32)
    cols = {"fwd": range(D), "rev": range(D - 1, -1, -1),
            "blocks": [c for s in range(0, D, 8) for t in range(4) for c in (s + t, s + 4 + t) if c < D]}[order]
    s = np.zeros((qh.shape[0], dh.shape[0]), np.float32)
    for c in cols:
        s += qh[:, c, None] * dh[None, :, c]
    return s


def model_topk(q, d, k, C, order="fwd", fault=None):
    """what a chunked implementation returns: per chunk of C documents the k best (value desc, index asc), then the merge -> (val [B, k] float32,
    idx [B, k] int64).  fault: one of FAULTS."""
    B, M = q.shape[0], d.shape[0]
    qh = q.astype(np.float32) if fault == "query_not_normalised" else unit32(q, fault != "clamp_missing")
    dh = d.astype(np.float32) if fault == "document_not_normalised" else unit32(d, fault != "clamp_missing")
    if fault == "padding_columns_returned" and M % 128:          # the ragged step's padding documents score 0 and are not masked
        dh = np.concatenate([dh, np.zeros((128 - M % 128, dh.shape[1]), np.float32)])
    s = dot32(qh, dh, order) + np.float32(0)
    Mx = dh.shape[0]
    kk = max(1, k // 2) if fault == "chunk_lists_truncated" else k
    val, idx = np.full((B, k), -np.inf, np.float32), np.full((B, k), -1, np.int64)
    chunks = list(range(0, Mx, C))
    if fault == "last_chunk_dropped" and len(chunks) > 1:
        chunks = chunks[:-1]
    for b in range(B):
        lv, li = [], []
        for c0 in chunks:
            sc = s[b, c0:c0 + C]
            ids = np.arange(sc.size)
            o = np.lexsort((-ids if fault == "tie_order_reversed" else ids, -sc))[:kk]
            lv.append(sc[o])
            li.append(o if fault == "chunk_base_not_added" else o + c0)
        if fault == "merge_not_stable":                            # by value alone, the later list first among equal values
            lv, li = lv[::-1], li[::-1]
            v, i = np.concatenate(lv), np.concatenate(li)
            o = np.argsort(-v, kind="stable")[:k]
        else:
            v, i = np.concatenate(lv) if lv else np.zeros(0, np.float32), np.concatenate(li) if li else np.zeros(0, np.int64)
            o = np.lexsort((-i if fault == "tie_order_reversed" else i, -v))[:k]
        val[b, :o.size], idx[b, :o.size] = v[o], i[o]
        if fault == "duplicate_emitted_twice" and o.size > 1:
            val[b, o.size - 1], idx[b, o.size - 1] = val[b, o.size - 2], idx[b, o.size - 2]
        if fault == "k_gt_m_filled_with_zeros" and o.size < k:
            val[b, o.size:], idx[b, o.size:] = 0.0, 0
    return val, idx
