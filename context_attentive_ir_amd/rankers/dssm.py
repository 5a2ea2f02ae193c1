"""DSSM (drop-in for neuroir.rankers.dssm.DSSM, /root/reference/neuroir/rankers/dssm.py:8-63).

rep = tanh(W2 tanh(W1 x + b1) + b2) per tower, x = max over ALL padded positions of the embedded ids; score = cos(rep_q, rep_d).
Eval: one C-ABI call (nir_dssm_score), two launches -- the tower kernel (query and document rows in one launch: gather + max, both
layers) and the cosine.  The lengths are ignored like in the reference; the max runs over the padded width, the PAD row included
wherever a row has padding (read from the table: a loaded state dict may hold a non-zero PAD row).
Train mode: autograd.embed -> dropout -> max_pool -> linear (x2) -> cosine, all on the HIP operators.
"""
import torch
import torch.nn as nn

from .. import autograd as A
from .. import lib
from ..constants import PAD
from ..modules import Embeddings

# The eval kernels' envelope (csrc/dssm.hip, nir_dssm_score), checked at construction so that a model the training operators accept
# cannot fail later at its first eval forward: a dssm_tower_kernel lane gathers 8 of the 64-column groups of an embedded row,
# rank_finish_kernel holds 4 of the representation, and the tower kernel keeps 4 E + E + nhid floats in 64 KiB of LDS.
MAX_EMSIZE, MAX_NOUT, TOWER_LDS_BYTES = 512, 256, 64 * 1024


def check_arch(emsize, nhid, nout):
    if not (0 < emsize <= MAX_EMSIZE):
        raise ValueError("DSSM: emsize %d unsupported (1 <= emsize <= %d)" % (emsize, MAX_EMSIZE))
    if not (0 < nout <= MAX_NOUT):
        raise ValueError("DSSM: nout %d unsupported (1 <= nout <= %d)" % (nout, MAX_NOUT))
    if nhid <= 0 or (5 * emsize + nhid) * 4 > TOWER_LDS_BYTES:
        raise ValueError("DSSM: nhid %d unsupported at emsize %d (1 <= nhid, (5 emsize + nhid) floats <= %d bytes of LDS)"
                         % (nhid, emsize, TOWER_LDS_BYTES))


class DSSM(nn.Module, lib.IdCheck):
    def __init__(self, args):
        super().__init__()
        check_arch(args.emsize, args.nhid, args.nout)
        self.word_embeddings = Embeddings(args.emsize, args.src_vocab_size, PAD)
        self.emb_drop = nn.Dropout(p=args.dropout_emb)
        self.query_mlp = nn.Sequential(nn.Linear(args.emsize, args.nhid), nn.Tanh(), nn.Linear(args.nhid, args.nout), nn.Tanh())
        self.doc_mlp = nn.Sequential(nn.Linear(args.emsize, args.nhid), nn.Tanh(), nn.Linear(args.nhid, args.nout), nn.Tanh())
        self._pack = lib.PackCache()

    def _weights(self):
        def build():
            q, d = self.query_mlp, self.doc_mlp
            t = dict(q_w1t=q[0].weight.t(), q_b1=q[0].bias, q_w2t=q[2].weight.t(), q_b2=q[2].bias,
                     d_w1t=d[0].weight.t(), d_b1=d[0].bias, d_w2t=d[2].weight.t(), d_b2=d[2].bias)
            return lib.Packed(lib.DssmWeights, t, dict(NH=q[0].out_features, NO=q[2].out_features))
        return self._pack.get(list(self.query_mlp.parameters()) + list(self.doc_mlp.parameters()), build)

    def _forward_train(self, q, d):
        B, QL = q.shape
        N, DL = d.shape[1], d.shape[2]
        table = self.word_embeddings.table
        eq = A.dropout(A.embed(q, table, PAD), self.emb_drop.p, True)
        ed = A.dropout(A.embed(d.reshape(B * N, DL), table, PAD), self.emb_drop.p, True)

        def mlp(x, m):
            return A.linear(A.linear(x, m[0].weight, m[0].bias, act="tanh"), m[2].weight, m[2].bias, act="tanh")
        rq = mlp(A.max_pool(eq), self.query_mlp)
        rd = mlp(A.max_pool(ed), self.doc_mlp)
        return A.cosine(rq, rd.view(B, N, -1))

    def forward(self, batch_queries, query_len, batch_docs, doc_len, return_reps=False):
        """scores [B,N]; return_reps: also the tower outputs rep_q [B,nout] / rep_d [B,N,nout] (eval only)."""
        assert batch_queries.shape[0] == batch_docs.shape[0]
        table = self.word_embeddings.table
        lib.require_device(batch_queries, batch_docs, table)
        q, d = self._clean_ids(batch_queries, batch_docs, table.shape[0])
        B, QL = q.shape
        N, DL = d.shape[1], d.shape[2]
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
            ws = lib.workspace(L.nir_dssm_workspace_bytes(B, N, NO), dev)
            lib.check(L.nir_dssm_score(lib.ptr(q), lib.ptr(d), B, N, QL, DL, lib.ptr(table), table.shape[0], table.shape[1], PAD, w.ref(),
                                       lib.ptr(ws), ws.numel(), lib.ptr(scores), lib.ptr(rq), lib.ptr(rd), lib.stream()), "nir_dssm_score")
        return (scores, rq, rd) if return_reps else scores

    # -- corpus retrieval (retrieval.DocumentIndex): each tower on its own ----------------------------------------------
    def _encode(self, ids, side):
        """one tower over the rows ids [R, L] -> [R, nout], through the scoring entry itself (nir_dssm_score, return_reps): a tower row
        depends on nothing but its own ids, so these are the bits of rep_q / rep_d of any forward that holds the row.  The other tower gets
        one all-PAD row of the smallest width per call (documents) or per query (queries); its output is dropped."""
        if self.training:
            raise NotImplementedError("DSSM.encode_queries / encode_documents run in eval mode only (call .eval())")
        if ids.dim() != 2:
            raise ValueError("DSSM.encode_%s: expected ids [rows, width], got %s" % (side, tuple(ids.shape)))
        R = ids.shape[0]
        lib.require_device(ids, self.word_embeddings.table)
        if R == 0:
            return torch.empty(0, self._weights().struct.NO, device=ids.device, dtype=torch.float32)
        if side == "queries":
            other = torch.full((R, 1, 1), PAD, dtype=torch.int64, device=ids.device)
            return self.forward(ids, None, other, None, return_reps=True)[1]
        other = torch.full((1, 1), PAD, dtype=torch.int64, device=ids.device)
        return self.forward(other, None, ids.unsqueeze(0), None, return_reps=True)[2][0]

    def encode_queries(self, ids):
        """query tower: ids [B, QL] -> [B, nout], bit-identical to rep_q of forward(..., return_reps=True) on the same rows (eval only)"""
        return self._encode(ids, "queries")

    def encode_documents(self, ids):
        """document tower: ids [M, DL] -> [M, nout], bit-identical to rep_d of forward(..., return_reps=True) on the same rows (eval only)"""
        return self._encode(ids, "documents")
