"""CDSSM (drop-in for neuroir.rankers.cdssm.CDSSM, /root/reference/neuroir/rankers/cdssm.py:8-77).

The reference concatenates rows t, t+1, t+2 of the embedded sequence (`_interleave_tensor`) and runs Conv1d(3E -> nhid, k=3) over that,
so every output position sees a 5-row window.  Here the conv weight is folded once per weight version into its 5-tap form
W5[o][m][e] = sum_{i+k=m} W[o][i E + e][k] (fold_taps) and the [B, L-2, 3E] interleave is never formed.
rep = max over the L-4 windows of tanh(sem(tanh(conv(window)))); score = cos(rep_q, rep_d).
Eval: one C-ABI call (nir_cdssm_score), two launches -- the fused tile kernel (gathered 5-tap conv, tanh, Linear(nhid -> nout), tanh and the
column max over a tile of 32 windows, query and document rows in one launch) and the max-over-tiles + cosine.  Like the reference the max
runs over ALL windows of the padded width; the all-PAD window's vector is folded into rows with a PAD tail instead of being recomputed.
Train mode: autograd.embed -> dropout -> linear over the 5-row windows (folded weight; its gradient unfolds through the fold's autograd)
-> linear -> max_pool -> cosine.
"""
import torch
import torch.nn as nn

from .. import autograd as A
from .. import lib
from ..constants import PAD
from ..modules import Embeddings

TAPS = 5
# The eval kernels' envelope (csrc/dssm.hip, nir_cdssm_score), checked at construction so that a model the training operators accept
# cannot fail later at its first eval forward: cdssm_tile_kernel owns one conv column per thread (320 threads), rank_finish_kernel
# holds 4 of the representation, and the tile kernel's LDS holds 40 staged floats per embedding column (2 x 20 window rows), within
# the 159 KiB the launch reserves.
MAX_NHID, MAX_NOUT, TILE_LDS_BYTES = 320, 256, 160 * 1024 - 1024
MAX_EMSIZE = TILE_LDS_BYTES // (40 * 4)


def check_arch(emsize, nhid, nout):
    if not (0 < emsize <= MAX_EMSIZE):
        raise ValueError("CDSSM: emsize %d unsupported (1 <= emsize <= %d: 160 bytes of LDS per column, %d bytes in all)"
                         % (emsize, MAX_EMSIZE, TILE_LDS_BYTES))
    if not (0 < nhid <= MAX_NHID):
        raise ValueError("CDSSM: nhid %d unsupported (1 <= nhid <= %d)" % (nhid, MAX_NHID))
    if not (0 < nout <= MAX_NOUT):
        raise ValueError("CDSSM: nout %d unsupported (1 <= nout <= %d)" % (nout, MAX_NOUT))


def fold_taps(weight, window=3):
    """Conv1d weight [O, window*E, k] over the `window`-row interleave -> the equivalent [O, window+k-1, E] weight over plain rows
    (differentiable: dW[o, i E + e, k] = dW5[o, i + k, e])."""
    O, K, k = weight.shape
    w = weight.view(O, window, K // window, k)
    return torch.stack([sum(w[:, i, :, m - i] for i in range(window) if 0 <= m - i < k) for m in range(window + k - 1)], 1)


class CDSSM(nn.Module, lib.IdCheck):
    def __init__(self, args):
        super().__init__()
        check_arch(args.emsize, args.nhid, args.nout)
        self.window = 3
        self.word_embeddings = Embeddings(args.emsize, args.src_vocab_size, PAD)
        self.emb_drop = nn.Dropout(p=args.dropout_emb)
        K = self.window * args.emsize
        self.query_conv = nn.Conv1d(K, args.nhid, 3)
        self.query_sem = nn.Linear(args.nhid, args.nout)
        self.doc_conv = nn.Conv1d(K, args.nhid, 3)
        self.doc_sem = nn.Linear(args.nhid, args.nout)
        self._pack = lib.PackCache()

    def _weights(self):
        def build():
            def w5t(conv):
                return fold_taps(conv.weight.detach(), self.window).reshape(conv.out_channels, -1).t()     # [5E][nhid]
            t = dict(q_w5t=w5t(self.query_conv), q_b=self.query_conv.bias, q_semt=self.query_sem.weight.t(), q_semb=self.query_sem.bias,
                     d_w5t=w5t(self.doc_conv), d_b=self.doc_conv.bias, d_semt=self.doc_sem.weight.t(), d_semb=self.doc_sem.bias)
            return lib.Packed(lib.CdssmWeights, t, dict(NH=self.query_conv.out_channels, NO=self.query_sem.out_features))
        params = [p for n, p in self.named_parameters() if not n.startswith("word_embeddings")]
        return self._pack.get(params, build)

    def _forward_train(self, q, d):
        B, QL = q.shape
        N, DL = d.shape[1], d.shape[2]
        table = self.word_embeddings.table
        eq = A.dropout(A.embed(q, table, PAD), self.emb_drop.p, True)
        ed = A.dropout(A.embed(d.reshape(B * N, DL), table, PAD), self.emb_drop.p, True)

        def tower(x, conv, sem):
            R, L, E = x.shape
            P = L - TAPS + 1
            rows = torch.cat([x[:, m:m + P] for m in range(TAPS)], 2).reshape(R * P, TAPS * E)
            h = A.linear(rows, fold_taps(conv.weight, self.window).reshape(conv.out_channels, -1), conv.bias, act="tanh")
            return A.max_pool(A.linear(h, sem.weight, sem.bias, act="tanh").view(R, P, -1))
        rq = tower(eq, self.query_conv, self.query_sem)
        rd = tower(ed, self.doc_conv, self.doc_sem)
        return A.cosine(rq, rd.view(B, N, -1))

    def forward(self, batch_queries, query_len, batch_docs, doc_len, return_reps=False):
        """scores [B,N]; return_reps: also the tower outputs rep_q [B,nout] / rep_d [B,N,nout] (eval only)."""
        assert batch_queries.shape[0] == batch_docs.shape[0]
        QL, DL = batch_queries.shape[1], batch_docs.shape[2]
        if QL < TAPS or DL < TAPS:
            # the reference fails for these widths too (cdssm.py:34 asserts >= 3; Conv1d(k=3) over L-2 < 3 rows raises)
            raise RuntimeError("CDSSM needs query and document widths >= %d (the conv over the 3-row interleave sees 5 tokens), got %d / %d"
                               % (TAPS, QL, DL))
        table = self.word_embeddings.table
        lib.require_device(batch_queries, batch_docs, table)
        q, d = self._clean_ids(batch_queries, batch_docs, table.shape[0])
        B, N = q.shape[0], d.shape[1]
        if self.training and not return_reps:
            return self._forward_train(q, d)
        L = lib.load()
        w = self._weights()
        dev = q.device
        NO = w.struct.NO
        scores = torch.empty(B, N, device=dev, dtype=torch.float32)
        rq = torch.empty(B, NO, device=dev, dtype=torch.float32) if return_reps else None
        rd = torch.empty(B, N, NO, device=dev, dtype=torch.float32) if return_reps else None
        if B > 0:
            ws = lib.workspace(L.nir_cdssm_workspace_bytes(B, N, QL, DL, NO), dev)
            lib.check(L.nir_cdssm_score(lib.ptr(q), lib.ptr(d), B, N, QL, DL, lib.ptr(table), table.shape[0], table.shape[1], PAD, w.ref(),
                                        lib.ptr(ws), ws.numel(), lib.ptr(scores), lib.ptr(rq), lib.ptr(rd), lib.stream()), "nir_cdssm_score")
        return (scores, rq, rd) if return_reps else scores

    # -- corpus retrieval (retrieval.DocumentIndex): each tower on its own ----------------------------------------------
    def _encode(self, ids, side):
        """one tower over the rows ids [R, L] -> [R, nout], through the scoring entry itself (nir_cdssm_score, return_reps): a tower row
        depends on nothing but its own ids, so these are the bits of rep_q / rep_d of any forward that holds the row.  The other tower gets
        one all-PAD row of the smallest width per call (documents) or per query (queries); its output is dropped."""
        if self.training:
            raise NotImplementedError("CDSSM.encode_queries / encode_documents run in eval mode only (call .eval())")
        if ids.dim() != 2:
            raise ValueError("CDSSM.encode_%s: expected ids [rows, width], got %s" % (side, tuple(ids.shape)))
        R = ids.shape[0]
        lib.require_device(ids, self.word_embeddings.table)
        if R == 0:
            return torch.empty(0, self._weights().struct.NO, device=ids.device, dtype=torch.float32)
        if side == "queries":
            other = torch.full((R, 1, TAPS), PAD, dtype=torch.int64, device=ids.device)
            return self.forward(ids, None, other, None, return_reps=True)[1]
        other = torch.full((1, TAPS), PAD, dtype=torch.int64, device=ids.device)
        return self.forward(other, None, ids.unsqueeze(0), None, return_reps=True)[2][0]

    def encode_queries(self, ids):
        """query tower: ids [B, QL] -> [B, nout], bit-identical to rep_q of forward(..., return_reps=True) on the same rows (eval only)"""
        return self._encode(ids, "queries")

    def encode_documents(self, ids):
        """document tower: ids [M, DL] -> [M, nout], bit-identical to rep_d of forward(..., return_reps=True) on the same rows (eval only)"""
        return self._encode(ids, "documents")
