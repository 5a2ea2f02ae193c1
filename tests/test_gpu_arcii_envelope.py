"""GPU (-m gpu): nir_conv2d_pool_f32 (csrc/arcii.hip) at the C ABI against float64 F.conv2d / max_pool2d, under the bound of
tests/arcii_ref.py, over its envelope: channel and filter counts on both sides of the 32-wide k-step, the 16-wide column tile and the
128-filter block, the dense and the outer-sum input (N = 1 and N = 3), asymmetric kernels, pool windows that divide the 64-row tile and
that do not, floor-dropped rows and columns, grids that pool to width 1, window counts around a tile so that tiles cross pair ends, both
activations, the folded-head epilogue with one and two filter blocks, the fp32 path, the zero padding of the GRID in the outer-sum mode,
and every limit of the entry at its negative return."""
import ctypes as C

import pytest
import torch

import arcii_ref
import gemm_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 64


def _layer(w, b, pool, path=0):
    from context_attentive_ir_amd.rankers import arcii
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    layer = arcii.PackedLayer2d(w.to(DEV), b.to(DEV), pool, path, flag)
    assert int(flag.item()) == 0
    return layer


def _run(M, H, W, Cin, Fo, kernel=(3, 3), pool=(2, 2), act="relu", fam="randn", N=0, head=False, path=0, seed=0):
    """N == 0: the dense input [M, H, W, C]; N >= 1: the outer sum of pd [M, H, C] and pq [M / N, W, C] (each term half the family's range,
    so that the sums stay inside the split format)"""
    from context_attentive_ir_amd.rankers import arcii
    g = torch.Generator().manual_seed(2000 + seed)
    kh, kw = kernel
    K = Cin * kh * kw
    w = gemm_ref.family(fam, g, Fo, K, "w").reshape(Fo, Cin, kh, kw)
    b = gemm_ref.family("randn", g, 1, Fo, "a")[0]
    layer = _layer(w, b, pool, path)
    Hp, Wp = H // pool[0], W // pool[1]
    hw = torch.randn(Fo, Hp, Wp, generator=g) if head else None
    hwd = hw.to(DEV) if head else None
    if N == 0:
        x = gemm_ref.family(fam, g, M * H * W, K, "a", cols=Cin).reshape(M, H, W, Cin)
        got = arcii.conv2d_pool(layer, x=x.to(DEV), act=act, head_w=hwd)
        x32, x64 = x, x.double()
    else:
        assert M % N == 0
        pd = 0.5 * gemm_ref.family(fam, g, M * H, K, "a", cols=Cin).reshape(M, H, Cin)
        pq = 0.5 * gemm_ref.family(fam, g, (M // N) * W, K, "a", cols=Cin).reshape(M // N, W, Cin)
        got = arcii.conv2d_pool(layer, pd=pd.to(DEV), pq=pq.to(DEV), act=act, head_w=hwd)
        x32, x64 = arcii_ref.outer_sum(pd, pq, N), arcii_ref.outer_sum(pd.double(), pq.double(), N)
    ref = arcii_ref.conv2d_pool(x64, w.double(), b.double(), pool, act)
    chain = arcii_ref.conv2d_pool(x32, w, b, pool, act)
    assert ref.shape == (M, Hp, Wp, Fo)
    if head:
        got = got.sum((3, 4))
        ref = (ref * hw.double().permute(1, 2, 0)).sum(3)
        chain = (chain * hw.permute(1, 2, 0)).sum(3)
    ok, fig = arcii_ref.accept(got, ref, chain, 1 if path == 0 else 0)
    print("conv2d_pool M=%d H=%d W=%d C=%d F=%d k=%s p=%s %s %s N=%d head=%d path=%d: ratio %.3f e %.3g e_chain %.3g"
          % (M, H, W, Cin, Fo, kernel, pool, act, fam, N, head, path, fig["ratio"], fig["e"], fig["e_chain"]))
    assert ok, fig


@pytest.mark.parametrize("N", [0, 1, 3])
@pytest.mark.parametrize("Cin", [1, 31, 32, 33, 300])
def test_channel_counts(Cin, N):
    _run(3, 5, 4, Cin, 17, N=N, seed=Cin)


@pytest.mark.parametrize("N", [0, 3])
@pytest.mark.parametrize("Fo", [1, 15, 16, 17, 130, 256])
def test_filter_counts(Fo, N):
    _run(3, 5, 4, 33, Fo, N=N, seed=Fo)


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("kernel", [(1, 1), (3, 3), (5, 3), (1, 7), (7, 1)])
def test_kernel_sizes_and_activations(kernel, act):
    """an asymmetric kernel on an asymmetric grid: a transposed tap order or axis shows; then grids smaller than the kernel, where every
    tap but the centre falls outside somewhere"""
    s = 10 * kernel[0] + kernel[1]
    _run(2, 7, 5, 20, 24, kernel, (2, 2), act=act, seed=s)
    _run(3, 6, 5, 20, 24, kernel, (1, 1), act=act, N=3, seed=s + 1)
    for H, W in ((1, 1), (2, 1), (1, 3)):
        _run(2, H, W, 20, 24, kernel, (1, 1), act=act, seed=s + 2 + H + W)
        _run(2, H, W, 20, 24, kernel, (1, 1), act=act, N=2, seed=s + 5 + H + W)


@pytest.mark.parametrize("pool,H,W", [((1, 1), 5, 3), ((2, 2), 6, 4), ((2, 2), 7, 5), ((3, 2), 7, 5), ((3, 2), 9, 2), ((1, 3), 4, 7), ((1, 3), 5, 3),
                                      ((2, 1), 9, 1), ((8, 8), 17, 9), ((8, 8), 8, 8), ((64, 1), 70, 2), ((1, 64), 1, 64)])
def test_pool_sizes_and_floor_dropped_tails(pool, H, W):
    """(3, 2): 10 windows = 60 rows per tile, 4 rows idle; (7, 5) under (3, 2) drops one row and one column; (9, 2) and (5, 3) pool to
    width 1; (8, 8) and (64, 1) are the limit, one window per tile"""
    s = 1000 * pool[0] + 100 * pool[1] + 10 * H + W
    _run(3, H, W, 33, 17, (3, 3), pool, seed=s)
    _run(3, H, W, 33, 17, (3, 3), pool, N=3, seed=s + 1)
    _run(3, H, W, 33, 17, (3, 3), pool, N=1, head=True, seed=s + 2)


@pytest.mark.parametrize("pool,M,H,W", [((2, 2), 3, 10, 2), ((2, 2), 2, 8, 4), ((2, 2), 1, 34, 2), ((2, 2), 3, 14, 2), ((2, 2), 5, 7, 7),
                                        ((3, 2), 3, 9, 2), ((3, 2), 2, 15, 2), ((3, 2), 1, 33, 2), ((3, 2), 3, 21, 3), ((1, 1), 3, 7, 3),
                                        ((1, 1), 1, 8, 8), ((1, 1), 5, 13, 1)])
def test_window_counts_around_a_tile(pool, M, H, W):
    """(2, 2): 16 windows per tile -- 15, 16, 17 and 21 windows (three pairs of 7: the first tile ends inside the third pair); (3, 2): 10
    windows per tile -- 9, 10, 11, 21; (1, 1): 64 -- 63, 64, 65"""
    s = 100 * pool[0] + 10 * M + H + W
    _run(M, H, W, 40, 130, (3, 3), pool, seed=s)                        # two filter blocks
    _run(M, H, W, 40, 17, (5, 3), pool, N=1, seed=s + 1)
    if M % 3 == 0:
        _run(M, H, W, 40, 17, (3, 5), pool, N=3, seed=s + 2)


@pytest.mark.parametrize("Fo", [40, 130])
@pytest.mark.parametrize("N", [0, 1, 3])
def test_head_epilogue(Fo, N):
    """the folded head over a 3 x 2 final grid (an i / j transposition of the head index shows), one and two 128-filter blocks"""
    _run(6, 7, 5, 33, Fo, (3, 3), (2, 2), N=N, head=True, seed=Fo + N)
    _run(3, 9, 4, 33, Fo, (3, 1), (3, 2), act="none", N=N, head=True, seed=Fo + N + 1)


@pytest.mark.parametrize("fam", ["randn", "mixed", "edge", "tiny"])
@pytest.mark.parametrize("N", [0, 2])
def test_input_families(fam, N):
    _run(4, 9, 5, 300, 256, (3, 3), (2, 2), fam=fam, N=N, seed=len(fam))            # 32 windows: two row tiles, two filter blocks
    _run(2, 9, 5, 64, 40, (3, 3), (2, 2), fam=fam, N=N, head=True, seed=len(fam) + 1)


@pytest.mark.parametrize("fam", ["randn", "mixed", "edge"])
def test_fp32_path(fam):
    _run(3, 7, 5, 33, 17, (3, 3), (2, 2), fam=fam, path=1, seed=3)
    _run(3, 7, 5, 33, 17, (5, 3), (3, 2), fam=fam, N=3, path=1, seed=4)
    _run(2, 7, 5, 70, 300, (3, 5), (3, 2), fam=fam, N=1, head=True, path=1, seed=5)


def test_outer_sum_pads_the_grid_with_zeros():
    """a constant document term and a zero query term: with zero padding of the GRID the border outputs differ from the interior ones; a
    loader that adds first and bounds-checks one axis would read Pd[i] + 0 beyond the query edge and make every column equal"""
    from context_attentive_ir_amd.rankers import arcii
    Cin, Fo, H, W = 8, 16, 4, 5
    w = torch.ones(Fo, Cin, 3, 3)
    layer = _layer(w, torch.zeros(Fo), (1, 1))
    pd, pq = torch.ones(1, H, Cin), torch.zeros(1, W, Cin)
    got = arcii.conv2d_pool(layer, pd=pd.to(DEV), pq=pq.to(DEV), act="none").cpu()
    taps = lambda n, i: 3 - (i == 0) - (i == n - 1)
    want = torch.tensor([[float(Cin * taps(H, i) * taps(W, j)) for j in range(W)] for i in range(H)])
    assert torch.equal(got[0, :, :, 0], want) and torch.equal(got[0, :, :, Fo - 1], want)


def _conv_seq(w, b):
    conv = torch.nn.Conv2d(w.shape[1], w.shape[0], tuple(w.shape[2:]), padding=(w.shape[2] // 2, w.shape[3] // 2)).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    return conv


def test_pack_time_bound_picks_the_path():
    """max_f(sum |w_f|) max|input| + max|b| layer by layer: below 2^15 the next layer splits, above it runs in fp32 -- and is still right"""
    from context_attentive_ir_amd.rankers import arcii
    g = torch.Generator().manual_seed(5)
    Cin, F1, F2, H, W = 24, 20, 12, 8, 6
    w1, b1 = torch.randn(F1, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5, torch.randn(F1, generator=g)
    w2, b2 = torch.randn(F2, F1, 3, 3, generator=g) / (9 * F1) ** 0.5, torch.randn(F2, generator=g)
    x = torch.randn(2, H, W, Cin, generator=g)
    s1 = float(w1.abs().sum((1, 2, 3)).max())
    for scale, want in ((1.0, 0), (40000.0, 1)):
        ws, bs = [w1 * scale, w2], [b1, b2]
        in_bound = float(x.abs().max())
        assert ((s1 * scale * in_bound + float(b1.abs().max())) >= 32768.0) == bool(want)
        packed = arcii.pack_layers2d([_conv_seq(a, b) for a, b in zip(ws, bs)], [(2, 2), (2, 1)], in_bound)
        assert [l.struct.path for l in packed] == [0, want]
        got = arcii.conv2d_pool(packed[1], x=arcii.conv2d_pool(packed[0], x=x.to(DEV)))
        f = lambda t: arcii_ref.conv2d_pool(arcii_ref.conv2d_pool(x.to(t), ws[0].to(t), bs[0].to(t), (2, 2)), ws[1].to(t), bs[1].to(t), (2, 1))
        if want:
            assert float(f(torch.float64).abs().max()) > 32768.0
        ok, fig = arcii_ref.accept(got, f(torch.float64), f(torch.float32), 2 - want)
        print("pack-time bound scale %g -> paths %s: %s" % (scale, [l.struct.path for l in packed], fig))
        assert ok, fig
    convs = [_conv_seq(w1, b1), _conv_seq(w2, b2)]
    assert [l.struct.path for l in arcii.pack_layers2d(convs, [(2, 2), (2, 1)], 32768.0)] == [1, 1]
    assert arcii.pack_layers2d(convs, [(2, 2), (2, 1)], 32767.0)[0].struct.path == 0


def test_network_pack_bounds_the_grid_by_the_sum_of_the_towers():
    """layer 0 of the 2-D stack reads Pd + Pq: its input bound is the sum of the two towers' output bounds"""
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.rankers import ARCII
    net = ARCII(default_args("ARCII", src_vocab_size=30, emsize=8, filters_1d=6, filters_2d=[6, 4], max_query_len=9, max_doc_len=23))
    fill_module_(net)
    net.to(DEV).eval()
    assert [l.struct.path for l in net._weights().l] == [0, 0]
    tmax = float(net.word_embeddings.table.detach().abs().max())
    one = float(net.conv_doc.weight.detach().abs().sum((1, 2)).max()) * tmax
    with torch.no_grad():                     # each tower's bound lands between 2^14 and 2^15: only their sum passes the limit
        net.conv_doc.weight.mul_(24000.0 / one)
        net.conv_query.weight.mul_(24000.0 / (float(net.conv_query.weight.abs().sum((1, 2)).max()) * tmax))
    w = net._weights()
    assert (w.q.struct.path, w.d.struct.path) == (0, 0) and [l.struct.path for l in w.l][0] == 1
    q, d = torch.randint(1, 30, (2, 9)), torch.randint(1, 30, (2, 3, 23))
    got = net(q.to(DEV), None, d.to(DEV), None)
    ok, fig = arcii_ref.accept_scores(got, net.state_dict(), q, d, net.maxpool_size_2d, n_split=1 + sum(1 for l in w.l if l.struct.path == 0))
    print("arcii with an fp32 first 2-D layer: %s" % fig)
    assert ok, fig


def test_weight_at_the_range_limit_raises():
    from context_attentive_ir_amd.rankers import arcii
    w = torch.zeros(4, 5, 3, 1)
    b = torch.zeros(4)
    w[2, 3, 1, 0] = 32767.0
    arcii.pack_layers2d([_conv_seq(w, b)], [(1, 1)], 1.0)
    w[2, 3, 1, 0] = -32768.0
    with pytest.raises(RuntimeError, match="2\\^15"):
        arcii.pack_layers2d([_conv_seq(w, b)], [(1, 1)], 1.0)


@pytest.mark.parametrize("field,bad", [("C_in", 0), ("C_in", 1025), ("F", 0), ("F", 1025), ("kh", 0), ("kh", 2), ("kh", 9), ("kw", 0), ("kw", 4),
                                       ("kw", 9), ("ph", 0), ("pw", 0), ("ph", 65), ("pw", 33), ("path", 2), ("act", 1), ("H", 0), ("W", 0),
                                       ("N", 0), ("N", 2)])
def test_entry_refuses_what_is_outside_its_limits(field, bad):
    """the inside of every limit runs in the tests above or in test_limits_inside; the outside is a negative code and no launch (pw 33
    with ph 2 is a window of 66; N 2 does not divide M 3)"""
    from context_attentive_ir_amd import lib
    L = lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    out = torch.full((1 << 16,), -7.0, device=DEV)
    v = dict(C_in=8, F=8, kh=3, kw=3, ph=2, pw=2, path=0, act=2, H=8, W=4, N=1)
    v[field] = bad
    st = lib.Conv2dLayer(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), v["C_in"], v["F"], v["kh"], v["kw"], v["ph"], v["pw"], v["path"])
    rc = L.nir_conv2d_pool_f32(None, lib.ptr(buf), lib.ptr(buf), 3, v["N"], v["H"], v["W"], C.byref(st), v["act"], None, lib.ptr(out), lib.stream())
    torch.cuda.synchronize()
    assert rc < 0 and L.nir_last_error_string()
    assert bool((out == -7.0).all())
    if field != "N":
        rc = L.nir_conv2d_pool_f32(lib.ptr(buf), None, None, 3, 1, v["H"], v["W"], C.byref(st), v["act"], None, lib.ptr(out), lib.stream())
        torch.cuda.synchronize()
        assert rc < 0 and bool((out == -7.0).all())
    if field in ("C_in", "F", "kh", "kw"):
        rc = L.nir_conv2d_pack(lib.ptr(buf), v["C_in"], v["F"], v["kh"], v["kw"], lib.ptr(out), lib.ptr(out), lib.ptr(out), lib.stream())
        assert rc < 0


def test_entry_refuses_mixed_input_modes():
    from context_attentive_ir_amd import lib
    L = lib.load()
    buf = torch.zeros(1 << 12, device=DEV)
    out = torch.full((1 << 12,), -7.0, device=DEV)
    st = lib.Conv2dLayer(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), 8, 8, 3, 3, 2, 2, 0)
    for x, pd, pq in ((buf, buf, buf), (buf, buf, None), (None, buf, None), (None, None, None)):
        rc = L.nir_conv2d_pool_f32(lib.ptr(x), lib.ptr(pd), lib.ptr(pq), 2, 1, 4, 4, C.byref(st), 2, None, lib.ptr(out), lib.stream())
        assert rc < 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())


def test_limits_inside():
    """C_in 1024, F 1024 and a 7 x 7 kernel, each at a small size of the rest"""
    _run(1, 3, 2, 1024, 17, (1, 1), (1, 1), seed=1)
    _run(1, 3, 2, 8, 1024, (1, 1), (1, 1), N=1, seed=2)
    _run(2, 4, 9, 5, 17, (7, 7), (2, 3), seed=3)
