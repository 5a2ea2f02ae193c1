"""ARC-I (drop-in for neuroir.rankers.arci.ARCI, /root/reference/neuroir/rankers/arci.py:7-105).

Per tower (separate weights for queries and documents) a stack of Conv1d(k, padding k // 2) -> ReLU -> MaxPool1d(p) over the embedded ids,
the two flattened results concatenated (query first, index f * feats + t) and scored by mlp = Linear(inp, inp // 2) -> Linear(inp // 2, 1).
Like the reference, the lengths are ignored: the convolutions run over the padded width, a PAD id contributes the table's PAD row (a
loaded state dict may hold a non-zero one) while the conv's own edge padding is zeros, and any width whose pooled widths equal the ones
of construction is accepted (any other fails in the reference's mlp with a shape RuntimeError; here before anything is launched).

Eval: one C-ABI call (nir_arci_score), len(filters_1d) + 1 launches -- one gather/conv/bias/ReLU/max-pool kernel per layer for both towers
(csrc/arci.hip) and the finish.  mlp has no non-linearity, so it is folded once per weight version into one vector and one scalar
(fold_head); the last layer's kernel multiplies its pooled tile by that vector and never writes the features.
A layer runs on the two-term fp16 MFMA path when a bound on its input, computed at pack time from the table and the weights layer by
layer, is below 2^15 (the range of the split format), else in plain fp32.
Train mode: autograd.embed -> dropout -> per layer im2col_rows + linear(relu) + max_pool -> the unfolded mlp as two linear.
"""
import ctypes as C

import torch
import torch.nn as nn

from .. import autograd as A
from .. import lib
from ..constants import PAD
from ..modules import Embeddings

# The envelope of nir_conv1d_pool_f32 (csrc/arci.hip), checked at construction so that a model the training operators accept cannot fail
# at its first eval forward.  Kernel sizes are odd: an even k with padding k // 2 lengthens the output by one position per layer, a form the
# kernels do not have.
MAX_CHANNELS, MAX_FILTERS, MAX_KERNEL, MAX_POOL, MAX_LAYERS = 1024, 1024, 7, 64, lib.ARCI_MAX_LAYERS
SPLIT_RANGE = 32768.0


def check_arch(emsize, filters_1d, kernel_size_1d, maxpool_size_1d):
    if not (1 <= len(filters_1d) <= MAX_LAYERS):
        raise ValueError("ARCI: %d conv layers unsupported (1 <= layers <= %d)" % (len(filters_1d), MAX_LAYERS))
    if not (1 <= emsize <= MAX_CHANNELS):
        raise ValueError("ARCI: emsize %d unsupported (1 <= emsize <= %d)" % (emsize, MAX_CHANNELS))
    for f, k, p in zip(filters_1d, kernel_size_1d, maxpool_size_1d):
        if not (1 <= f <= MAX_FILTERS):
            raise ValueError("ARCI: filters_1d %d unsupported (1 <= filters <= %d)" % (f, MAX_FILTERS))
        if k < 1 or k % 2 == 0 or k > MAX_KERNEL:
            raise ValueError("ARCI: kernel_size_1d %d unsupported (odd kernel sizes 1 .. %d only: an even one changes the output width)"
                             % (k, MAX_KERNEL))
        if not (1 <= p <= MAX_POOL):
            raise ValueError("ARCI: maxpool_size_1d %d unsupported (1 <= pool <= %d)" % (p, MAX_POOL))


def pooled_widths(L, maxpool_size_1d):
    """the width after every layer's MaxPool1d (floor)"""
    out = []
    for p in maxpool_size_1d:
        L = L // p
        out.append(L)
    return out


def fold_head(mlp):
    """mlp = Linear(inp, inp // 2) -> Linear(inp // 2, 1), nothing in between (arci.py:55-58): score = w_eff . x + b_eff with
    w_eff = W2 W1, b_eff = W2 b1 + b2.  Formed in float64 and rounded once -> (w_eff [inp] fp32, b_eff [1] fp32)."""
    w1, b1 = mlp[0].weight.detach().double(), mlp[0].bias.detach().double()
    w2, b2 = mlp[1].weight.detach().double(), mlp[1].bias.detach().double()
    return (w2 @ w1).reshape(-1).float(), (w2 @ b1 + b2).reshape(1).float()


class PackedLayer(object):
    """lib.Conv1dLayer of one Conv1d + the device tensors behind its pointers"""

    def __init__(self, weight, bias, pool, path, flag):
        L = lib.load()
        w = weight.detach().float().contiguous()
        F, Cin, k = w.shape
        self.planes = torch.empty(max(1, L.nir_conv1d_planes_bytes(Cin, F, k)), dtype=torch.uint8, device=w.device)
        self.wt = torch.empty(k * Cin, F, dtype=torch.float32, device=w.device)
        self.bias = bias.detach().float().contiguous().clone()
        lib.check(L.nir_conv1d_pack(lib.ptr(w), Cin, F, k, lib.ptr(self.planes), lib.ptr(self.wt), lib.ptr(flag), lib.stream()), "nir_conv1d_pack")
        self.struct = lib.Conv1dLayer(self.planes.data_ptr(), self.wt.data_ptr(), self.bias.data_ptr(), Cin, F, k, int(pool), int(path))

    def ref(self):
        return C.byref(self.struct)


def weight_range_error():
    return RuntimeError("ARCI: a convolution weight is outside the fp16 range of the split-fp16 MFMA path (|w| >= 2^15) or not finite")


def pack_tower(layers, pools, in_bound):
    """[PackedLayer] of one tower.  in_bound: max |input| of layer 0; a layer's outputs are bounded by max_f(sum |w_f|) max|input| + max|b|,
    which bounds the next layer's input (ReLU and the max only shrink it).  A layer takes the split path when its input bound is < 2^15.
    Synchronises (pack time only); RuntimeError when a weight is >= 2^15."""
    dev = layers[0][0].weight.device
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    out, bound = [], float(in_bound)
    for seq, p in zip(layers, pools):
        conv = seq[0]
        path = lib.CONV1D_SPLIT if bound < SPLIT_RANGE else lib.CONV1D_FP32
        out.append(PackedLayer(conv.weight, conv.bias, p, path, flag))
        w = conv.weight.detach().double().abs()
        bound = float(w.sum((1, 2)).max()) * bound + float(conv.bias.detach().double().abs().max())
    if int(flag.item()) & 2:
        raise weight_range_error()
    return out


def conv1d_pool(x, ids, layer, act="relu", head_w=None, M=None, L=None):
    """nir_conv1d_pool_f32 on a PackedLayer: ids [M, L] + table x [V, C], or the dense x [M, L, C].  -> [M, L // p, F], or with head_w
    [F, L // p] the partial list [M, L // p, ceil(F / 128), 2]."""
    Lb = lib.load()
    if ids is not None:
        M, L = ids.shape
    else:
        M, L = x.shape[0], x.shape[1]
    st = layer.struct
    n = Lb.nir_conv1d_pool_out_floats(M, L, st.F, st.p, int(head_w is not None))
    out = torch.empty(n, dtype=torch.float32, device=x.device)
    lib.check(Lb.nir_conv1d_pool_f32(lib.ptr(ids), lib.ptr(x), M, L, layer.ref(), A.ACT[act], lib.ptr(head_w), lib.ptr(out), lib.stream()),
              "nir_conv1d_pool_f32")
    Lp = L // st.p
    return out.view(M, Lp, (st.F + 127) // 128, 2) if head_w is not None else out.view(M, Lp, st.F)


class _Pack(object):
    def __init__(self, net):
        table = net.word_embeddings.table
        tmax = float(table.detach().abs().max())
        self.q = pack_tower(net.query_conv1d_layers, net.maxpool_size_1d, tmax)
        self.d = pack_tower(net.doc_conv1d_layers, net.maxpool_size_1d, tmax)
        w_eff, self.head_b = fold_head(net.mlp)
        nq = net.filters_1d[-1] * net.query_feats
        self.head_wq, self.head_wd = w_eff[:nq].contiguous(), w_eff[nq:].contiguous()
        s = self.struct = lib.ArciWeights()
        for i, (lq, ld) in enumerate(zip(self.q, self.d)):
            s.q[i], s.d[i] = lq.struct, ld.struct
        s.head_wq, s.head_wd, s.head_b = self.head_wq.data_ptr(), self.head_wd.data_ptr(), self.head_b.data_ptr()
        s.n_layers, s.q_feats, s.d_feats = len(self.q), net.query_feats, net.doc_feats

    def ref(self):
        return C.byref(self.struct)


class ARCI(nn.Module, lib.IdCheck):
    def __init__(self, args):
        super().__init__()
        num_conv1d_layers = len(args.filters_1d)
        assert num_conv1d_layers == len(args.kernel_size_1d)
        assert num_conv1d_layers == len(args.maxpool_size_1d)
        check_arch(args.emsize, args.filters_1d, args.kernel_size_1d, args.maxpool_size_1d)
        self.word_embeddings = Embeddings(args.emsize, args.src_vocab_size, PAD)
        self.emb_drop = nn.Dropout(p=args.dropout_emb)
        self.filters_1d, self.kernel_size_1d = list(args.filters_1d), list(args.kernel_size_1d)
        self.maxpool_size_1d = list(args.maxpool_size_1d)

        query_feats, doc_feats = args.max_query_len, args.max_doc_len
        query_conv1d_layers, doc_conv1d_layers = [], []
        for i in range(num_conv1d_layers):
            inpsize = args.emsize if i == 0 else args.filters_1d[i - 1]
            pad = args.kernel_size_1d[i] // 2
            for tower in (query_conv1d_layers, doc_conv1d_layers):
                tower.append(nn.Sequential(nn.Conv1d(inpsize, args.filters_1d[i], args.kernel_size_1d[i], padding=pad), nn.ReLU(inplace=True),
                                           nn.MaxPool1d(args.maxpool_size_1d[i])))
            doc_feats = doc_feats // args.maxpool_size_1d[i]
            query_feats = query_feats // args.maxpool_size_1d[i]
            assert query_feats != 0 and doc_feats != 0
        self.query_conv1d_layers = nn.ModuleList(query_conv1d_layers)
        self.doc_conv1d_layers = nn.ModuleList(doc_conv1d_layers)
        self.query_feats, self.doc_feats = query_feats, doc_feats
        inpsize = (args.filters_1d[-1] * query_feats) + (args.filters_1d[-1] * doc_feats)
        self.mlp = nn.Sequential(nn.Linear(inpsize, inpsize // 2), nn.Linear(inpsize // 2, 1))
        self._pack = lib.PackCache()

    def _weights(self):
        return self._pack.get(list(self.parameters()), lambda: _Pack(self))

    def _check_widths(self, QL, DL):
        """arci.py:104: the reference accepts any widths that pool to the feature counts of construction and fails in mlp otherwise"""
        wq, wd = pooled_widths(QL, self.maxpool_size_1d), pooled_widths(DL, self.maxpool_size_1d)
        if wq[-1] != self.query_feats or wd[-1] != self.doc_feats or 0 in wq or 0 in wd:
            F = self.filters_1d[-1]
            raise RuntimeError("ARCI: mat1 and mat2 shapes cannot be multiplied: widths %d / %d pool to %d / %d positions (%d features), mlp was "
                               "built for %d / %d (%d)" % (QL, DL, wq[-1], wd[-1], F * (wq[-1] + wd[-1]), self.query_feats, self.doc_feats,
                                                           F * (self.query_feats + self.doc_feats)))

    def _tower_train(self, x, layers):
        """x [M, L, C] -> [M, F_last * feats] (channel-major flatten)"""
        for seq, k, p in zip(layers, self.kernel_size_1d, self.maxpool_size_1d):
            conv = seq[0]
            M, L, Cin = x.shape
            rows = A.im2col_rows(x.transpose(1, 2).reshape(M, Cin, 1, L), (1, k), (0, k // 2))          # [M L, C k]
            y = A.linear(rows, conv.weight.reshape(conv.out_channels, -1), conv.bias, act="relu").view(M, L, -1)
            Lp = L // p
            x = A.max_pool(y[:, :Lp * p].reshape(M * Lp, p, -1)).view(M, Lp, -1)
        return x.transpose(1, 2).reshape(x.shape[0], -1)

    def _forward_train(self, q, d):
        B, QL = q.shape
        N, DL = d.shape[1], d.shape[2]
        table = self.word_embeddings.table
        eq = A.dropout(A.embed(q, table, PAD), self.emb_drop.p, True)
        ed = A.dropout(A.embed(d.reshape(B * N, DL), table, PAD), self.emb_drop.p, True)
        fq = self._tower_train(eq, self.query_conv1d_layers)
        fd = self._tower_train(ed, self.doc_conv1d_layers)
        com = torch.cat((fq.unsqueeze(1).expand(B, N, fq.shape[1]).reshape(B * N, -1), fd), 1)
        h = A.linear(com, self.mlp[0].weight, self.mlp[0].bias)
        return A.linear(h, self.mlp[1].weight, self.mlp[1].bias).view(B, N)

    def forward(self, batch_queries, query_len, batch_docs, doc_len):
        """scores [B, N] (arci.py:60-105); query_len / doc_len are not read, like in the reference"""
        assert batch_queries.shape[0] == batch_docs.shape[0]
        QL, DL = batch_queries.shape[1], batch_docs.shape[2]
        self._check_widths(QL, DL)
        table = self.word_embeddings.table
        lib.require_device(batch_queries, batch_docs, table)
        q, d = self._clean_ids(batch_queries, batch_docs, table.shape[0])
        B, N = q.shape[0], d.shape[1]
        if self.training:
            return self._forward_train(q, d)
        L = lib.load()
        w = self._weights()
        scores = torch.empty(B, N, device=q.device, dtype=torch.float32)
        if B > 0:
            ws = lib.workspace(L.nir_arci_workspace_bytes(B, N, QL, DL, w.ref()), q.device)
            lib.check(L.nir_arci_score(lib.ptr(q), lib.ptr(d), B, N, QL, DL, lib.ptr(table), table.shape[0], table.shape[1], w.ref(),
                                       lib.ptr(ws), ws.numel(), lib.ptr(scores), lib.stream()), "nir_arci_score")
        return scores
