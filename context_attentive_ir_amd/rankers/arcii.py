"""ARC-II (drop-in for neuroir.rankers.arcii.ARCII, neuroir/rankers/arcii.py:8-111).

Eq = conv_query(embed(q)) [B, F1, QL] and Ed = conv_doc(embed(d)) [B N, F1, DL] (separate weights, no activation), the grid
X[m, f, i, j] = Ed[m, f, i] + Eq[m // N, f, j] (document axis first) through MaxPool2d((2, 2)), then per layer
Conv2d(kernel_size_2d[i], padding (kh // 2, kw // 2)) -> ReLU -> MaxPool2d(maxpool_size_2d[i]) (index 0 of a kernel or pool size runs
along the document axis), flatten(1) (feature f Hd Hq + i Hq + j) and mlp = Linear(inp, inp // 2) -> Linear(inp // 2, 1).
Like the reference, the lengths are ignored, a PAD id contributes the table's PAD row while the convolutions' own edge padding is zeros
-- for the 2-D layers zeros of the GRID, not a one-sided sum -- and any runtime widths whose final grid has the PRODUCT F_last Hd Hq of
construction are accepted: the individual sides need not match (any other fails in the reference's mlp with a shape RuntimeError; here
before anything is launched), and the head is indexed with the runtime Hd, Hq.

Eval: one C-ABI call (nir_arcii_score), 2 + len(filters_2d) launches.  The first pool is separable bit for bit in fp32,
max_pool2d(Ed + Eq, 2 x 2) == max_pool1d(Ed, 2) + max_pool1d(Eq, 2) (fp32 addition is monotone in each operand), so stage 1 is ARC-I's
gather/conv/max-pool kernel over both towers and the [B N, F1, DL, QL] grid is never formed; the first 2-D layer adds the two pooled
terms while it loads them (csrc/arcii.hip).  mlp has no non-linearity and is folded like ARC-I's (arci.fold_head); the last layer's kernel
multiplies its pooled tile by that vector.  A layer runs on the two-term fp16 MFMA path when a bound on its input, computed at pack time,
is below 2^15, else in plain fp32; the first 2-D layer's input bound is the sum of the two towers' output bounds.
Train mode: autograd.embed -> dropout -> im2col_rows + linear (1-D conv) -> max_pool over pairs -> the broadcast add -> per 2-D layer
im2col_rows + linear(relu) + max_pool over row-major windows -> the (f, i, j) flatten -> the unfolded mlp as two linear.
"""
import ctypes as C

import torch
import torch.nn as nn

from .. import autograd as A
from .. import lib
from ..constants import PAD
from ..modules import Embeddings
from .arci import MAX_CHANNELS, MAX_FILTERS, MAX_KERNEL, MAX_POOL, SPLIT_RANGE, PackedLayer, fold_head

MAX_LAYERS = lib.ARCII_MAX_LAYERS
FIRST_POOL = 2            # self.maxpool1 = nn.MaxPool2d((2, 2)) (arcii.py:27)


def _odd_kernel(k):
    return 1 <= k <= MAX_KERNEL and k % 2 == 1


def check_arch(emsize, filters_1d, kernel_size_1d, filters_2d, kernel_size_2d, maxpool_size_2d):
    """the envelope of nir_conv1d_pool_f32 / nir_conv2d_pool_f32, checked at construction.  Kernel sizes are odd: an even kernel_size_1d
    makes the reference's own forward fail (the two towers' widths no longer match the broadcast add), an even kernel_size_2d grows the
    grid by one per layer, a form the kernels do not have."""
    if not (1 <= len(kernel_size_2d) <= MAX_LAYERS):
        raise ValueError("ARCII: %d conv2d layers unsupported (1 <= layers <= %d)" % (len(kernel_size_2d), MAX_LAYERS))
    if len(filters_2d) != len(kernel_size_2d):
        raise ValueError("ARCII: filters_2d has %d entries for %d conv2d layers" % (len(filters_2d), len(kernel_size_2d)))
    if not (1 <= emsize <= MAX_CHANNELS):
        raise ValueError("ARCII: emsize %d unsupported (1 <= emsize <= %d)" % (emsize, MAX_CHANNELS))
    if not (1 <= filters_1d <= MAX_FILTERS):
        raise ValueError("ARCII: filters_1d %d unsupported (1 <= filters <= %d)" % (filters_1d, MAX_FILTERS))
    if not _odd_kernel(kernel_size_1d):
        raise ValueError("ARCII: kernel_size_1d %d unsupported (odd kernel sizes 1 .. %d only: an even one changes the output width)"
                         % (kernel_size_1d, MAX_KERNEL))
    for f, k, p in zip(filters_2d, kernel_size_2d, maxpool_size_2d):
        if not (1 <= f <= MAX_FILTERS):
            raise ValueError("ARCII: filters_2d %d unsupported (1 <= filters <= %d)" % (f, MAX_FILTERS))
        if len(k) != 2 or not (_odd_kernel(k[0]) and _odd_kernel(k[1])):
            raise ValueError("ARCII: kernel_size_2d %s unsupported (two odd kernel sizes 1 .. %d only: an even one changes the grid)"
                             % (list(k), MAX_KERNEL))
        if len(p) != 2 or p[0] < 1 or p[1] < 1 or p[0] * p[1] > MAX_POOL:
            raise ValueError("ARCII: maxpool_size_2d %s unsupported (1 <= ph * pw <= %d)" % (list(p), MAX_POOL))


def pooled_grids(QL, DL, maxpool_size_2d):
    """[(Hd, Hq)] after the first pool and after every 2-D layer's MaxPool2d (floor)"""
    hd, hq = DL // FIRST_POOL, QL // FIRST_POOL
    out = [(hd, hq)]
    for ph, pw in maxpool_size_2d:
        hd, hq = hd // ph, hq // pw
        out.append((hd, hq))
    return out


class PackedLayer2d(object):
    """lib.Conv2dLayer of one Conv2d + the device tensors behind its pointers"""

    def __init__(self, weight, bias, pool, path, flag):
        L = lib.load()
        w = weight.detach().float().contiguous()
        F, Cin, kh, kw = w.shape
        self.planes = torch.empty(max(1, L.nir_conv2d_planes_bytes(Cin, F, kh, kw)), dtype=torch.uint8, device=w.device)
        self.wt = torch.empty(kh * kw * Cin, F, dtype=torch.float32, device=w.device)
        self.bias = bias.detach().float().contiguous().clone()
        lib.check(L.nir_conv2d_pack(lib.ptr(w), Cin, F, kh, kw, lib.ptr(self.planes), lib.ptr(self.wt), lib.ptr(flag), lib.stream()),
                  "nir_conv2d_pack")
        self.struct = lib.Conv2dLayer(self.planes.data_ptr(), self.wt.data_ptr(), self.bias.data_ptr(), Cin, F, kh, kw, int(pool[0]), int(pool[1]),
                                      int(path))

    def ref(self):
        return C.byref(self.struct)


def _out_bound(conv, in_bound):
    """max_f(sum |w_f|) max|input| + max|b|: a bound on the outputs of a convolution (ReLU and the max only shrink it)"""
    w = conv.weight.detach().double().abs()
    return float(w.reshape(w.shape[0], -1).sum(1).max()) * in_bound + float(conv.bias.detach().double().abs().max())


def _path(bound):
    return lib.CONV1D_SPLIT if bound < SPLIT_RANGE else lib.CONV1D_FP32


def pack_layers2d(convs, pools, in_bound):
    """[PackedLayer2d] of a Conv2d stack whose first input is bounded by in_bound; a layer takes the split path when its input bound is
    < 2^15.  Synchronises (pack time only); RuntimeError when a weight is >= 2^15."""
    flag = torch.zeros(1, dtype=torch.int32, device=convs[0].weight.device)
    out, bound = [], float(in_bound)
    for conv, p in zip(convs, pools):
        out.append(PackedLayer2d(conv.weight, conv.bias, p, _path(bound), flag))
        bound = _out_bound(conv, bound)
    if int(flag.item()) & 2:
        raise weight_range_error()
    return out


def weight_range_error():
    return RuntimeError("ARCII: a convolution weight is outside the fp16 range of the split-fp16 MFMA path (|w| >= 2^15) or not finite")


def conv2d_pool(layer, x=None, pd=None, pq=None, act="relu", head_w=None):
    """nir_conv2d_pool_f32 on a PackedLayer2d: the dense x [M, H, W, C], or the outer sum of pd [M, H, C] and pq [M // N, W, C].
    -> [M, H // ph, W // pw, F], or with head_w [F, H // ph, W // pw] the partial list [M, H // ph, W // pw, ceil(F / 128), 2]."""
    Lb = lib.load()
    if x is not None:
        M, H, W, N = x.shape[0], x.shape[1], x.shape[2], 1
        dev = x.device
    else:
        M, H, W = pd.shape[0], pd.shape[1], pq.shape[1]
        N = M // max(1, pq.shape[0])
        dev = pd.device
    st = layer.struct
    out = torch.empty(Lb.nir_conv2d_pool_out_floats(M, H, W, st.F, st.ph, st.pw, int(head_w is not None)), dtype=torch.float32, device=dev)
    lib.check(Lb.nir_conv2d_pool_f32(lib.ptr(x), lib.ptr(pd), lib.ptr(pq), M, N, H, W, layer.ref(), A.ACT[act], lib.ptr(head_w), lib.ptr(out),
                                     lib.stream()), "nir_conv2d_pool_f32")
    Hp, Wp = H // st.ph, W // st.pw
    return out.view(M, Hp, Wp, (st.F + 127) // 128, 2) if head_w is not None else out.view(M, Hp, Wp, st.F)


class _Pack(object):
    def __init__(self, net):
        tmax = float(net.word_embeddings.table.detach().abs().max())
        flag = torch.zeros(1, dtype=torch.int32, device=net.conv_query.weight.device)
        self.q = PackedLayer(net.conv_query.weight, net.conv_query.bias, FIRST_POOL, _path(tmax), flag)
        self.d = PackedLayer(net.conv_doc.weight, net.conv_doc.bias, FIRST_POOL, _path(tmax), flag)
        if int(flag.item()) & 2:
            raise weight_range_error()
        # a grid value is one document term + one query term
        grid_bound = _out_bound(net.conv_query, tmax) + _out_bound(net.conv_doc, tmax)
        self.l = pack_layers2d([seq[0] for seq in net.conv2d_layers], net.maxpool_size_2d, grid_bound)
        self.head_w, self.head_b = fold_head(net.mlp)
        s = self.struct = lib.ArciiWeights()
        s.q, s.d = self.q.struct, self.d.struct
        for i, ly in enumerate(self.l):
            s.l[i] = ly.struct
        s.head_w, s.head_b = self.head_w.data_ptr(), self.head_b.data_ptr()
        s.n_layers, s.feats = len(self.l), net.mlp[0].in_features

    def ref(self):
        return C.byref(self.struct)


class ARCII(nn.Module, lib.IdCheck):
    def __init__(self, args):
        super().__init__()
        num_conv2d_layers = len(args.kernel_size_2d)
        assert num_conv2d_layers == len(args.maxpool_size_2d)
        check_arch(args.emsize, args.filters_1d, args.kernel_size_1d, args.filters_2d, args.kernel_size_2d, args.maxpool_size_2d)
        self.word_embeddings = Embeddings(args.emsize, args.src_vocab_size, PAD)
        self.emb_drop = nn.Dropout(p=args.dropout_emb)
        pad = args.kernel_size_1d // 2
        self.conv_query = nn.Conv1d(args.emsize, args.filters_1d, args.kernel_size_1d, padding=pad)
        self.conv_doc = nn.Conv1d(args.emsize, args.filters_1d, args.kernel_size_1d, padding=pad)
        self.maxpool1 = nn.MaxPool2d((FIRST_POOL, FIRST_POOL))
        self.filters_1d, self.kernel_size_1d = args.filters_1d, args.kernel_size_1d
        self.filters_2d = list(args.filters_2d)
        self.kernel_size_2d = [tuple(k) for k in args.kernel_size_2d]
        self.maxpool_size_2d = [tuple(p) for p in args.maxpool_size_2d]

        doc_feats, query_feats = args.max_doc_len // FIRST_POOL, args.max_query_len // FIRST_POOL
        conv2d_layers = []
        for i in range(num_conv2d_layers):
            inpsize = args.filters_1d if i == 0 else args.filters_2d[i - 1]
            kh, kw = self.kernel_size_2d[i]
            conv2d_layers.append(nn.Sequential(nn.Conv2d(inpsize, args.filters_2d[i], (kh, kw), padding=(kh // 2, kw // 2)), nn.ReLU(inplace=True),
                                               nn.MaxPool2d(self.maxpool_size_2d[i])))
            doc_feats = doc_feats // self.maxpool_size_2d[i][0]
            query_feats = query_feats // self.maxpool_size_2d[i][1]
            assert query_feats != 0 and doc_feats != 0
        self.conv2d_layers = nn.ModuleList(conv2d_layers)
        self.query_feats, self.doc_feats = query_feats, doc_feats
        inpsize = args.filters_2d[-1] * query_feats * doc_feats
        self.mlp = nn.Sequential(nn.Linear(inpsize, inpsize // 2), nn.Linear(inpsize // 2, 1))
        self._pack = lib.PackCache()

    def _weights(self):
        return self._pack.get(list(self.parameters()), lambda: _Pack(self))

    def _check_widths(self, QL, DL):
        """arcii.py:108-110: the reference accepts any widths whose final grid flattens to the feature count of construction -- the product
        F_last Hd Hq, not the two sides -- and fails in mlp otherwise"""
        grids = pooled_grids(QL, DL, self.maxpool_size_2d)
        hd, hq = grids[-1]
        feats, want = self.filters_2d[-1] * hd * hq, self.mlp[0].in_features
        if feats != want or any(0 in g for g in grids):
            raise RuntimeError("ARCII: mat1 and mat2 shapes cannot be multiplied: widths %d / %d pool to a %d x %d grid (%d features), mlp was "
                               "built for %d" % (QL, DL, hd, hq, feats, want))

    def _conv1d_train(self, x, conv):
        """x [M, L, C] -> MaxPool1d(2) of the convolution, position-major [M, L // 2, F1] (no activation)"""
        M, L, Cin = x.shape
        k = self.kernel_size_1d
        rows = A.im2col_rows(x.transpose(1, 2).reshape(M, Cin, 1, L), (1, k), (0, k // 2))              # [M L, C k]
        y = A.linear(rows, conv.weight.reshape(conv.out_channels, -1), conv.bias).view(M, L, -1)
        Lp = L // FIRST_POOL
        return A.max_pool(y[:, :Lp * FIRST_POOL].reshape(M * Lp, FIRST_POOL, -1)).view(M, Lp, -1)

    def _forward_train(self, q, d):
        B, QL = q.shape
        N, DL = d.shape[1], d.shape[2]
        M = B * N
        table = self.word_embeddings.table
        eq = A.dropout(A.embed(q, table, PAD), self.emb_drop.p, True)
        ed = A.dropout(A.embed(d.reshape(M, DL), table, PAD), self.emb_drop.p, True)
        pq = self._conv1d_train(eq, self.conv_query)                                  # [B, Hq, F1]
        pd = self._conv1d_train(ed, self.conv_doc)                                    # [M, Hd, F1]
        # the separable form of MaxPool2d((2, 2)) over the grid: the first maximum of each term is the element the 2-D row-major scan keeps
        x = pd.view(B, N, pd.shape[1], 1, -1) + pq.view(B, 1, 1, pq.shape[1], -1)     # [B, N, Hd, Hq, F1]
        x = x.reshape(M, pd.shape[1], pq.shape[1], -1)
        for seq, (kh, kw), (ph, pw) in zip(self.conv2d_layers, self.kernel_size_2d, self.maxpool_size_2d):
            conv = seq[0]
            _, H, W, _ = x.shape
            rows = A.im2col_rows(x.permute(0, 3, 1, 2), (kh, kw), (kh // 2, kw // 2))               # [M H W, C kh kw]
            y = A.linear(rows, conv.weight.reshape(conv.out_channels, -1), conv.bias, act="relu").view(M, H, W, -1)
            Hp, Wp = H // ph, W // pw
            win = y[:, :Hp * ph, :Wp * pw].reshape(M, Hp, ph, Wp, pw, -1).permute(0, 1, 3, 2, 4, 5)      # row-major inside a window
            x = A.max_pool(win.reshape(M * Hp * Wp, ph * pw, -1)).view(M, Hp, Wp, -1)
        com = x.permute(0, 3, 1, 2).reshape(M, -1)                                     # flatten(1): f Hd Hq + i Hq + j
        h = A.linear(com, self.mlp[0].weight, self.mlp[0].bias)
        return A.linear(h, self.mlp[1].weight, self.mlp[1].bias).view(B, N)

    def forward(self, batch_queries, query_len, batch_docs, doc_len):
        """scores [B, N] (arcii.py:58-111); query_len / doc_len are not read, like in the reference"""
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
            ws = lib.workspace(L.nir_arcii_workspace_bytes(B, N, QL, DL, w.ref()), q.device)
            lib.check(L.nir_arcii_score(lib.ptr(q), lib.ptr(d), B, N, QL, DL, lib.ptr(table), table.shape[0], table.shape[1], w.ref(),
                                        lib.ptr(ws), ws.numel(), lib.ptr(scores), lib.stream()), "nir_arcii_score")
        return scores
