"""Corpus retrieval for the two-tower rankers (DSSM, CDSSM): a document index of unit rows on the device and the fused cosine top-k over it
(include/neuroir_retrieve.h, csrc/retrieve.hip).  The reference has no counterpart: its rankers only re-rank the
candidates handed in with each query.  The scores are the reference's cosine, x / max(|x|, 1e-8) . y / max(|y|, 1e-8).

    index = DocumentIndex(nout, device); index.add(net.encode_documents(doc_ids)); scores, ids = index.search(net.encode_queries(q_ids), k)
"""
import itertools

import torch

from . import lib

MAX_K, MAX_D = lib.RETRIEVE_MAX_K, lib.RETRIEVE_MAX_D
MIN_CAPACITY = 1024
FORMS = {"auto": lib.RETRIEVE_AUTO, "fused": lib.RETRIEVE_FUSED, "plain": lib.RETRIEVE_PLAIN}
_SERIAL = itertools.count(1)          # DocumentIndex.serial: never reused in a process, unlike id() of a collected object


def next_capacity(capacity, need):
    """geometric growth: the smallest of MIN_CAPACITY, 2 MIN_CAPACITY, 4 MIN_CAPACITY ... that holds `need` documents and is not below `capacity`"""
    cap = max(int(capacity), MIN_CAPACITY)
    while cap < need:
        cap *= 2
    return cap


def topk(queries, index_buf, count, dim, k, form="auto", err_flag=None):
    """nir_retrieve_topk over a raw index buffer -> (values [B, k] fp32, indices [B, k] int32); no synchronisation"""
    L = lib.load()
    lib.require_device(queries, index_buf)
    q = queries.detach().to(torch.float32).contiguous()
    B = q.shape[0]
    val = torch.empty(B, k, dtype=torch.float32, device=q.device)
    idx = torch.empty(B, k, dtype=torch.int32, device=q.device)
    f = FORMS[form] if isinstance(form, str) else int(form)
    ws = lib.workspace(L.nir_retrieve_topk_workspace_bytes(B, count, dim, k, f), q.device)
    lib.check(L.nir_retrieve_topk(lib.ptr(q), B, lib.ptr(index_buf), count, dim, k, f, lib.ptr(ws), ws.numel(), lib.ptr(err_flag), lib.ptr(val),
                                  lib.ptr(idx), lib.stream()), "nir_retrieve_topk")
    return val, idx


class DocumentIndex(object):
    """`count` unit rows of `dim` components in a device buffer of `capacity` rows (the library's opaque layout).

    add(reps) appends raw tower outputs [m, dim] (normalised by the kernel) and grows the buffer geometrically: growing copies the buffer's bytes,
    no document is added again.  search(query_reps, k) -> (scores [B, k] fp32, ids [B, k] int64), descending, the smaller id first among equal
    scores, (-inf, -1) beyond `count`; it enqueues on the current stream and never synchronises.  A row with a non-finite component is stored /
    searched as zeros and sets a bit of `err_flag` (bit 0: a document, bit 1: a query); check() is the synchronising read of that word.
    state_dict() holds the unit rows in plain [count, dim] order, load_state_dict() restores them bit for bit."""

    def __init__(self, dim, device=None, capacity=0):
        if not (1 <= int(dim) <= MAX_D):
            raise ValueError("DocumentIndex: dim %d unsupported (1 <= dim <= %d)" % (dim, MAX_D))
        self.dim, self.count, self.capacity, self.version = int(dim), 0, 0, 0
        # (serial, version) names one state of one index for as long as the process lives: the key of anything that bakes the buffer's address
        # in, such as a captured hipGraph (Ranker.search).  version moves with every add, growth and load.
        self.serial = next(_SERIAL)
        self.device = torch.device(device) if device is not None else None
        self.buf = self.err_flag = None
        if capacity:
            self.reserve(capacity)

    def __len__(self):
        return self.count

    def _device(self, t=None):
        if self.device is None:
            self.device = t.device if t is not None else torch.device("cuda")
        if self.device.type != "cuda":
            raise RuntimeError("context_attentive_ir_amd runs on a ROCm device only (got a %s index); there is no CPU fallback" % self.device)
        return self.device

    def reserve(self, need):
        """room for `need` documents in all (never shrinks)"""
        need = int(need)
        if need <= self.capacity and self.buf is not None:
            return
        cap = next_capacity(self.capacity, need)
        dev = self._device()
        L = lib.load()
        buf = torch.empty(L.nir_retrieve_index_bytes(cap, self.dim), dtype=torch.uint8, device=dev)
        if self.buf is not None and self.count:
            used = L.nir_retrieve_index_bytes(self.count, self.dim)          # a document's address does not depend on the capacity
            buf[:used].copy_(self.buf[:used])
        if self.err_flag is None:
            self.err_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        self.buf, self.capacity = buf, cap
        self.version += 1

    def _rows(self, reps, what):
        if reps.dim() != 2 or reps.shape[1] != self.dim:
            raise ValueError("DocumentIndex.%s: expected [m, %d] representations, got %s" % (what, self.dim, tuple(reps.shape)))
        self._device(reps)
        lib.require_device(reps)
        return reps.detach().to(torch.float32).contiguous()

    def add(self, reps):
        """append the documents reps [m, dim] -> the id of the first one"""
        r = self._rows(reps, "add")
        first, m = self.count, r.shape[0]
        if m == 0:
            return first
        self.reserve(first + m)
        lib.check(lib.load().nir_retrieve_add(lib.ptr(r), m, self.dim, lib.ptr(self.buf), self.capacity, first, lib.ptr(self.err_flag), lib.stream()),
                  "nir_retrieve_add")
        self.count += m
        self.version += 1
        return first

    def search(self, query_reps, k, form="auto"):
        if not (1 <= int(k) <= MAX_K):
            raise ValueError("DocumentIndex.search: k %d unsupported (1 <= k <= %d)" % (k, MAX_K))
        q = self._rows(query_reps, "search")
        if self.buf is None:
            self.reserve(1)
        val, idx = topk(q, self.buf, self.count, self.dim, int(k), form, self.err_flag)
        return val, idx.long()

    def check(self):
        """synchronising: raise if a document or a query since the last check held a non-finite component"""
        v = int(self.err_flag.item()) if self.err_flag is not None else 0
        if v:
            self.err_flag.zero_()
            raise RuntimeError("DocumentIndex: non-finite representation (%s); such rows count as zeros"
                               % " and ".join(n for b, n in ((1, "a document"), (2, "a query")) if v & b))

    def rows(self):
        """the stored unit rows in plain [count, dim] order (a fresh device tensor)"""
        out = torch.empty(self.count, self.dim, dtype=torch.float32, device=self._device())
        if self.count:
            lib.check(lib.load().nir_retrieve_export(lib.ptr(self.buf), self.capacity, self.dim, 0, self.count, lib.ptr(out), lib.stream()),
                      "nir_retrieve_export")
        return out

    def state_dict(self):
        return {"dim": self.dim, "count": self.count, "rows": self.rows().cpu() if self.count else torch.empty(0, self.dim)}

    def load_state_dict(self, state):
        check_state(state, self.dim)
        rows = state["rows"]
        self.count = 0
        m = rows.shape[0]
        if m:
            self.reserve(m)
            r = rows.to(self._device(), torch.float32).contiguous()
            lib.check(lib.load().nir_retrieve_import(lib.ptr(r), m, self.dim, lib.ptr(self.buf), self.capacity, 0, lib.stream()), "nir_retrieve_import")
        self.count = m
        self.version += 1
        return self


def check_state(state, dim):
    """host-side validation of a saved index"""
    rows = state.get("rows")
    if int(state.get("dim", -1)) != dim or not torch.is_tensor(rows) or rows.dim() != 2 or rows.shape[1] != dim or int(state.get("count", -1)) != rows.shape[0]:
        raise ValueError("DocumentIndex.load_state_dict: expected {dim: %d, count: m, rows: [m, %d]}" % (dim, dim))
