"""GPU (-m gpu): nir_conv1d_pool_f32 (csrc/arci.hip) at the C ABI against float64, under the bound of tests/arci_ref.py, over its envelope:
channel and filter counts on both sides of the 32-wide k-step, the 16-wide column tile and the 128-filter block up to the maxima, gathered
and dense A, every kernel size, pool sizes with every remainder, widths around the 64-row tile (a pool of 3 does not divide it), one
sequence and a partial last workgroup, both activations, the folded-head epilogue, the pack-time choice between the split and the fp32
path on both sides of 2^15, and every limit of the entry at its negative return."""
import ctypes as C

import pytest
import torch

import arci_ref
import gemm_ref

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILE = 64


def _layer(w, b, p, path=0):
    from context_attentive_ir_amd.rankers import arci
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    layer = arci.PackedLayer(w.to(DEV), b.to(DEV), p, path, flag)
    assert int(flag.item()) == 0
    return layer


def _run(M, L, Cin, Fo, k, p, act="relu", fam="randn", gathered=True, head=False, path=0, seed=0):
    from context_attentive_ir_amd.rankers import arci
    g = torch.Generator().manual_seed(1000 + seed)
    K = Cin * k
    w = gemm_ref.family(fam, g, Fo, K, "w").reshape(Fo, Cin, k)
    b = gemm_ref.family("randn", g, 1, Fo, "a")[0]
    if gathered:
        V = 37
        table = gemm_ref.family(fam, g, V, K, "a", cols=Cin)
        ids = torch.randint(0, V, (M, L), generator=g)
        x = table[ids]
    else:
        x = gemm_ref.family(fam, g, M * L, K, "a", cols=Cin).reshape(M, L, Cin)
    layer = _layer(w, b, p, path)
    Lp = L // p
    hw = torch.randn(Fo, Lp, generator=g) if head else None
    got = arci.conv1d_pool(table.to(DEV) if gathered else x.to(DEV), ids.to(DEV) if gathered else None, layer, act,
                           hw.to(DEV) if head else None)
    ref = arci_ref.conv_pool(x.double(), w.double(), b.double(), p, act)
    chain = arci_ref.conv_pool(x, w, b, p, act)
    assert ref.shape == (M, Lp, Fo)
    if head:
        got = got.sum((2, 3))
        ref = (ref * hw.double().t()).sum(2)
        chain = (chain * hw.t()).sum(2)
    ok, fig = arci_ref.accept(got, ref, chain, 1 if path == 0 else 0)
    print("conv1d_pool M=%d L=%d C=%d F=%d k=%d p=%d %s %s %s head=%d path=%d: ratio %.3f e %.3g e_chain %.3g"
          % (M, L, Cin, Fo, k, p, act, fam, "gathered" if gathered else "dense", head, path, fig["ratio"], fig["e"], fig["e_chain"]))
    assert ok, fig


@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("Cin", [1, 31, 32, 33, 300, 1024])
def test_channel_counts(Cin, gathered):
    _run(3, 9, Cin, 17, 3, 2, gathered=gathered, seed=Cin)


@pytest.mark.parametrize("gathered", [True, False])
@pytest.mark.parametrize("Fo", [1, 15, 16, 17, 256, 1024])
def test_filter_counts(Fo, gathered):
    _run(3, 9, 33, Fo, 3, 2, gathered=gathered, seed=Fo)


@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("k", [1, 3, 5, 7])
def test_kernel_sizes_and_activations(k, act):
    _run(2, 11, 20, 24, k, 2, act=act, seed=k)
    for L in sorted({1, 2, max(1, k - 1)}):                    # widths below the kernel: every tap but the centre falls outside somewhere
        _run(2, L, 20, 24, k, 1, act=act, seed=10 * k + L)


@pytest.mark.parametrize("p,L", [(1, 9), (2, 8), (2, 9), (3, 9), (3, 10), (3, 11), (64, 130)])
def test_pool_sizes_and_remainders(p, L):
    _run(3, L, 33, 17, 3, p, seed=p * 100 + L)
    _run(3, L, 33, 17, 3, p, gathered=False, head=True, seed=p * 100 + L + 1)


@pytest.mark.parametrize("p", [1, 2, 3])
@pytest.mark.parametrize("L", [TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_widths_around_the_row_tile(L, p):
    """p = 3 does not divide the 64-row tile: a tile then holds 21 windows and the next one starts at window 21, never inside a window"""
    _run(1, L, 33, 17, 3, p, seed=L + p)
    _run(3, L, 40, 130, 5, p, gathered=False, seed=L + p + 7)              # three sequences: tiles straddle sequence ends; two filter blocks


@pytest.mark.parametrize("fam", ["randn", "mixed", "edge", "tiny"])
@pytest.mark.parametrize("gathered", [True, False])
def test_input_families(fam, gathered):
    _run(3, 50, 300, 256, 3, 2, fam=fam, gathered=gathered, seed=len(fam))          # 150 rows: a partial last workgroup
    _run(1, 50, 64, 40, 3, 2, fam=fam, gathered=gathered, head=True, seed=len(fam) + 1)


@pytest.mark.parametrize("fam", ["randn", "mixed", "edge"])
def test_fp32_path(fam):
    _run(3, 21, 33, 17, 3, 2, fam=fam, path=1, seed=3)
    _run(2, 21, 70, 300, 5, 3, fam=fam, gathered=False, head=True, path=1, seed=4)


def _tower(ws, bs):
    out = []
    for w, b in zip(ws, bs):
        conv = torch.nn.Conv1d(w.shape[1], w.shape[0], w.shape[2], padding=w.shape[2] // 2).to(DEV)
        with torch.no_grad():
            conv.weight.copy_(w)
            conv.bias.copy_(b)
        out.append([conv])
    return out


def test_pack_time_bound_picks_the_path():
    """max_f(sum |w_f|) max|input| + max|b| layer by layer: below 2^15 the next layer splits, above it runs in fp32 -- and is still right"""
    from context_attentive_ir_amd.rankers import arci
    g = torch.Generator().manual_seed(5)
    Cin, F1, F2, L = 24, 20, 12, 16
    w1, b1 = torch.randn(F1, Cin, 3, generator=g) / (3 * Cin) ** 0.5, torch.randn(F1, generator=g)
    w2, b2 = torch.randn(F2, F1, 3, generator=g) / (3 * F1) ** 0.5, torch.randn(F2, generator=g)
    x = torch.randn(2, L, Cin, generator=g)
    s1 = float(w1.abs().sum((1, 2)).max())
    for scale, want in ((1.0, 0), (40000.0, 1)):
        # the first layer's weights scaled so that its outputs really pass 2^15 in the second case
        ws, bs = [w1 * scale, w2], [b1, b2]
        in_bound = float(x.abs().max())
        assert ((s1 * scale * in_bound + float(b1.abs().max())) >= 32768.0) == bool(want)
        packed = arci.pack_tower(_tower(ws, bs), [2, 2], in_bound)
        assert [l.struct.path for l in packed] == [0, want]
        h = arci.conv1d_pool(x.to(DEV), None, packed[0])
        got = arci.conv1d_pool(h, None, packed[1])
        f = lambda t: arci_ref.conv_pool(arci_ref.conv_pool(x.to(t), ws[0].to(t), bs[0].to(t), 2), ws[1].to(t), bs[1].to(t), 2)
        if want:
            assert float(f(torch.float64).abs().max()) > 32768.0
        ok, fig = arci_ref.accept(got, f(torch.float64), f(torch.float32), 2 - want)
        print("pack-time bound scale %g -> paths %s: %s" % (scale, [l.struct.path for l in packed], fig))
        assert ok, fig
    # an input bound at the limit itself: fp32 from the first layer on
    assert [l.struct.path for l in arci.pack_tower(_tower([w1, w2], [b1, b2]), [2, 2], 32768.0)] == [1, 1]
    assert arci.pack_tower(_tower([w1, w2], [b1, b2]), [2, 2], 32767.0)[0].struct.path == 0


def test_weight_at_the_range_limit_raises():
    from context_attentive_ir_amd.rankers import arci
    w = torch.zeros(4, 5, 3)
    b = torch.zeros(4)
    w[2, 3, 1] = 32767.0
    arci.pack_tower(_tower([w], [b]), [1], 1.0)
    w[2, 3, 1] = -32768.0
    with pytest.raises(RuntimeError, match="2\\^15"):
        arci.pack_tower(_tower([w], [b]), [1], 1.0)


@pytest.mark.parametrize("field,bad", [("C_in", 0), ("C_in", 1025), ("F", 0), ("F", 1025), ("k", 0), ("k", 2), ("k", 9), ("p", 0), ("p", 65),
                                       ("path", 2), ("act", 1), ("L", 0)])
def test_entry_refuses_what_is_outside_its_limits(field, bad):
    """the inside of every limit runs in the tests above (C_in 1024, F 1024, k 7, p 64); the outside is a negative code and no launch"""
    from context_attentive_ir_amd import lib
    L = lib.load()
    buf = torch.zeros(1 << 16, device=DEV)
    out = torch.full((1 << 16,), -7.0, device=DEV)
    v = dict(C_in=8, F=8, k=3, p=2, path=0, act=2, L=8)
    v[field] = bad
    st = lib.Conv1dLayer(buf.data_ptr(), buf.data_ptr(), buf.data_ptr(), v["C_in"], v["F"], v["k"], v["p"], v["path"])
    rc = L.nir_conv1d_pool_f32(None, lib.ptr(buf), 2, v["L"], C.byref(st), v["act"], None, lib.ptr(out), lib.stream())
    torch.cuda.synchronize()
    assert rc < 0 and L.nir_last_error_string()
    assert bool((out == -7.0).all())
    if field in ("C_in", "F", "k"):
        rc = L.nir_conv1d_pack(lib.ptr(buf), v["C_in"], v["F"], v["k"], lib.ptr(out), lib.ptr(out), lib.ptr(out), lib.stream())
        assert rc < 0
