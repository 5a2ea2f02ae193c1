"""GPU (-m gpu): nir_tf_attend driven directly (include/neuroir_teacher.h, csrc/tf_attend.hip), both forms against the float64 restatement
under session_score_ref's attention bound, over the shapes at which the kernels take another path: rows per group around the 16-row tile and the
64-row block, one group and more groups than CUs, QL around the position tiles and the largest fusable one, every H class, every kind of
length, the three kinds of row map, dominant and vanishing scores, the dot form, the optional attention row with a wide stride, guard values,
the same bits twice, and the form taken."""
import ctypes as C
import re

import pytest
import torch

import session_score_ref as SS

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = -7.25


def _lib():
    from context_attentive_ir_amd import lib
    return lib, lib.load()


def _profiled(L, fn):
    buf = C.create_string_buffer(1 << 16)
    L.nir_profile_report(buf, len(buf))                     # drop what earlier tests left
    L.nir_profile_enable(1)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        L.nir_profile_enable(0)
    L.nir_profile_report(buf, len(buf))
    return [re.sub(r"\[M=[^\]]*\]$", "", ln.rsplit(",", 2)[0]) for ln in buf.value.decode().strip().splitlines()]


def _inputs(seed, ngroups, G, rows_src, QL, H, lens="mixed", rowmap="perm", dot=False, spike=False):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(ngroups * G, H, generator=g) * 0.5
    mem = torch.randn(rows_src, QL, H, generator=g)
    sb = mem if dot else torch.randn(rows_src, QL, H, generator=g) * 0.5
    if lens == "mixed":                                      # 1, QL, above QL (clamped), 0, then ragged
        ln = torch.randint(1, QL + 1, (rows_src,), generator=g)
        for i, v in enumerate((1, QL, QL + 5, 0)[:rows_src]):
            ln[i] = v
    else:
        ln = torch.full((rows_src,), QL if lens == "full" else int(lens), dtype=torch.int64)
    if rowmap == "perm":                                     # every bank row once, then again
        rm = torch.randperm(rows_src, generator=g).repeat((ngroups + rows_src - 1) // rows_src)[:ngroups]
    elif rowmap == "one":                                    # many groups onto one source row
        rm = torch.full((ngroups,), rows_src - 1, dtype=torch.int64)
    else:
        rm = None
    if spike:                                                # one score 80 above the rest, one 80 below: every row of h carries 4.0 in feature 0
        h[:, 0] = 4.0
        sb = sb.clone()
        sb[:, 0, 0] += 20.0
        if QL > 2:
            sb[:, 2, 0] -= 20.0
    return h, mem, sb, ln, rm, G


def _call(L, lib, h, mem, sb, lens, rowmap, G, with_attn=True, stride_extra=3):
    """-> (cat [R, 2H], attn [R, QL] or None) on the CPU, after checking the guard values behind and between the outputs"""
    R, H = h.shape
    rows_src, QL, _ = mem.shape
    d = [t.to(DEV).contiguous() if t is not None else None for t in (h, mem, sb, lens, rowmap)]
    if sb is mem:
        d[2] = d[1]                                          # the dot form: ONE bank
    cat = torch.full((R + 2, 2 * H), GUARD, device=DEV)
    stride = QL + stride_extra
    attn = torch.full((R + 2, stride), GUARD, device=DEV) if with_attn else None
    ws = torch.empty(max(1, L.nir_tf_attend_workspace_bytes(R // G, G, QL, H)), dtype=torch.uint8, device=DEV)
    lib.check(L.nir_tf_attend(lib.ptr(d[0]), lib.ptr(d[1]), lib.ptr(d[2]), lib.ptr(d[3]), lib.ptr(d[4]), R // G, G, rows_src, QL, H, lib.ptr(cat),
                              lib.ptr(attn), stride, lib.ptr(ws), ws.numel(), lib.stream()), "nir_tf_attend")
    torch.cuda.synchronize()
    cat = cat.cpu()
    assert bool((cat[R:] == GUARD).all()), "cat written past its rows"
    if attn is not None:
        attn = attn.cpu()
        assert bool((attn[R:] == GUARD).all()) and bool((attn[:R, QL:] == GUARD).all()), "attn written past its rows or between them"
        attn = attn[:R, :QL]
    return cat[:R], attn


def _check(tag, inputs, forms=("fused", "plain"), with_attn=True, expect_fused=True):
    lib, L = _lib()
    h, mem, sb, lens, rowmap, G = inputs
    QL, H = mem.shape[1], mem.shape[2]
    ref = SS.tf_attend(h, mem, sb, lens, rowmap, G)
    chain = SS.tf_attend(h, mem, sb, lens, rowmap, G, torch.float32)
    fusable = bool(L.nir_tf_attend_fusable(QL, H, int(sb is mem)))
    assert fusable == expect_fused, (tag, QL, H)
    fusable = fusable and G >= SS.TF_MIN_G                  # the entry's own rule: the fused form from two full row blocks a group on
    for form in forms:
        if form == "fused" and not fusable:
            continue
        out = {}

        def run():
            out["a"] = _call(L, lib, h, mem, sb, lens, rowmap, G, with_attn)
            out["b"] = _call(L, lib, h, mem, sb, lens, rowmap, G, with_attn)
        if form == "plain":
            with lib.tunable("exact_f32", 1, 0):
                names = _profiled(L, run)
        else:
            names = _profiled(L, run)
        want = "tf_attend_fused_kernel" if form == "fused" else "tf_attend_plain_kernel"
        assert names == [want], (tag, form, names)                             # the form taken, and nothing else launched
        (cat, attn), (cat2, attn2) = out["a"], out["b"]
        assert torch.equal(cat.view(torch.int32), cat2.view(torch.int32)), "the same inputs, other bits"          # NaN rows included
        if attn is not None:
            assert torch.equal(attn.view(torch.int32), attn2.view(torch.int32))
        ok, fig = SS.accept_attend(cat, attn, h, ref, chain, 2 if form == "fused" else 0)
        print("tf_attend %s %s: %s" % (tag, form, {k: (round(v["ratio"], 3), v["e"], v["bound"]) for k, v in fig.items() if isinstance(v, dict)}))
        assert ok, (tag, form, fig)


@pytest.mark.parametrize("G", [1, 15, 16, 17, 63, 64, 65, 127, 128, 130])
def test_rows_per_group_around_the_tile_and_the_block(G):
    """below 128 rows a group the entry runs its plain form alone"""
    _check("G=%d" % G, _inputs(G, 3, G, 4, 5, 64))


@pytest.mark.parametrize("last", [1, 15, 16, 17, 63, 64, 65])
def test_the_fused_forms_last_block_around_the_tile_and_the_block(last):
    """the same edges where the fused form runs: two full 64-row blocks and `last` rows behind them"""
    _check("G=128+%d" % last, _inputs(100 + last, 3, 128 + last, 4, 5, 64))


def test_one_group_and_more_groups_than_cus():
    _check("ngroups=1", _inputs(1, 1, 145, 4, 5, 64, rowmap="perm"))
    _check("ngroups=1 no map", _inputs(2, 1, 129, 1, 5, 64, lens="full", rowmap=None))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    _check("ngroups=CUs+1 onto one row", _inputs(3, cus + 1, 129, 2, 5, 32, lens=4, rowmap="one"))
    _check("ngroups=CUs+1 no map", _inputs(4, cus + 1, 130, cus + 1, 3, 32, rowmap=None))


@pytest.mark.parametrize("QL", [1, 5, 16, 17, 32, 33])
def test_ql_around_the_position_tiles_at_h_512(QL):
    _check("QL=%d" % QL, _inputs(10 + QL, 2, 130, 4, QL, 512), expect_fused=QL <= 32)     # 32: the largest fusable at H 512; 33: the plain form takes it


def test_ql_beyond_the_fused_range_at_a_small_h():
    _check("QL=48 H=64", _inputs(7, 2, 129, 4, 48, 64))
    _check("QL=64 H=32", _inputs(8, 2, 129, 4, 64, 32))
    _check("QL=65 H=32", _inputs(9, 2, 129, 4, 65, 32), expect_fused=False)


@pytest.mark.parametrize("H", [32, 64, 288, 512, 1024, 36])
def test_every_class_of_h(H):
    _check("H=%d" % H, _inputs(20 + H, 2, 145, 4, 10, H), expect_fused=H != 36)


def test_dominant_and_vanishing_scores():
    _check("spike", _inputs(31, 3, 145, 4, 5, 64, lens="full", spike=True))


def test_the_dot_form_reads_one_bank():
    _check("dot", _inputs(32, 3, 145, 4, 5, 64, dot=True))
    _check("dot H=512", _inputs(33, 2, 170, 4, 10, 512, dot=True))


def test_without_the_attention_row():
    _check("attn NULL", _inputs(34, 3, 145, 4, 5, 64), with_attn=False)


def test_a_map_entry_outside_the_bank_rows_is_clamped():
    lib, L = _lib()
    h, mem, sb, lens, _, G = _inputs(35, 3, 130, 4, 5, 64)
    far, near = torch.tensor([9, -2, 2]), torch.tensor([3, 0, 2])
    for plain in (False, True):
        if plain:
            with lib.tunable("exact_f32", 1, 0):
                a, b = _call(L, lib, h, mem, sb, lens, far, G), _call(L, lib, h, mem, sb, lens, near, G)
        else:
            a, b = _call(L, lib, h, mem, sb, lens, far, G), _call(L, lib, h, mem, sb, lens, near, G)
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
