"""GPU (-m gpu): the sampling entries at the C ABI (csrc/sample.hip, include/neuroir_sample.h) against the float64 restatement of
tests/sample_ref.py.  nir_sample_noise: the Philox words bit for bit and |g - g64| <= E_G over more than 2^22 draws; nir_sample_gen, both
forms, on sample_ref.GEN_CASES: the float64 token wherever its gap exceeds 2 (E_y / tau + E_G), a near-tie candidate elsewhere (at most 1 % of
a case's rows), logp and lse by score_ref's token bound at the device's token, the same bits twice; nir_sample_topk_select: the float64
restriction to top_idx, K = 1 the first entry; and the chi-square of 16 384 draws against softmax64(y / tau), both forms."""
import numpy as np
import pytest
import torch

import sample_ref as R
import score_ref
from context_attentive_ir_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pack(w):
    L = lib.load()
    VT, K = w.shape
    nb = L.nir_seq2seq_gen_frag_bytes(VT, K)
    if not nb:
        return None
    frag = torch.empty(nb, dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.check(L.nir_seq2seq_pack_gen_frag(lib.ptr(w), VT, K, lib.ptr(frag), lib.ptr(flag), lib.stream()), "nir_seq2seq_pack_gen_frag")
    assert int(flag.item()) == 0
    return frag


def _noise(seed, step, nsrc, rows, VT, with_words=True):
    g = torch.full((rows, VT), float("nan"), device=DEV)
    wd = torch.zeros(rows, VT, dtype=torch.int32, device=DEV) if with_words else None
    lib.check(lib.load().nir_sample_noise(seed, step, nsrc, rows, VT, lib.ptr(g), lib.ptr(wd), lib.stream()), "nir_sample_noise")
    return g.cpu().numpy(), (wd.cpu().numpy().view(np.uint32) if with_words else None)


def _gen(x, w, b, frag, nsrc, tau, seed, step, with_lse=True):
    L = lib.load()
    rows, K = x.shape
    VT = w.shape[0]
    nb = L.nir_sample_gen_workspace_bytes(rows, K, VT, 1 if frag is not None else 0)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    tok = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((rows,), float("nan"), device=DEV)
    lse = torch.full((rows,), float("nan"), device=DEV) if with_lse else None
    lib.check(L.nir_sample_gen(lib.ptr(x), rows, nsrc, K, lib.ptr(w), lib.ptr(b), lib.ptr(frag), VT, 1.0 / tau, seed, step, lib.ptr(ws), nb, lib.ptr(tok),
                               lib.ptr(lp), lib.ptr(lse), lib.stream()), "nir_sample_gen")
    return tok, lp, lse


# ---- the noise -----------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def worst():
    w = {"E_G": 0.0, "draws": 0}
    yield w
    print("sample envelope: max |g - g64| = %.3g = 2^%.2f over %d draws" % (w["E_G"], np.log2(max(w["E_G"], 1e-30)), w["draws"]))


@pytest.mark.parametrize("seed", [0, 1, (1 << 63) + 5])
@pytest.mark.parametrize("step", [0, 1, 1 << 20])
def test_noise_words_are_the_numpy_words_and_the_gumbel_is_accurate(seed, step, worst):
    for nsrc, rows, VT in ((1, 3, 5), (3, 7, 37), (3, 12, 4099), (1, 2, 4099)):
        g, wd = _noise(seed, step, nsrc, rows, VT)
        want = R.words(seed, step, nsrc, rows, VT)
        assert np.array_equal(wd, want), (seed, step, nsrc, rows, VT)
        err = float(np.abs(g.astype(np.float64) - R.gumbel(want)).max())
        worst["E_G"], worst["draws"] = max(worst["E_G"], err), worst["draws"] + g.size
        assert err <= R.E_G, (err, seed, step)


def test_the_gumbel_bound_over_four_million_draws(worst):
    assert R.E_G <= R.E_G_CAP
    rows, VT = 1040, 4099                                                         # > 2^22 draws
    g, wd = _noise(12345, 3, 16, rows, VT)
    assert g.size >= 1 << 22
    want = R.words(12345, 3, 16, rows, VT)
    assert np.array_equal(wd, want)
    g64 = R.gumbel(want)
    err = np.abs(g.astype(np.float64) - g64)
    worst["E_G"], worst["draws"] = max(worst["E_G"], float(err.max())), worst["draws"] + g.size
    top = g64 > 12                                                                # u -> 1: where the winners come from
    print("noise: max |g - g64| %.3g (2^%.2f); over the %d draws with g > 12: %.3g; largest g %.3f, smallest %.3f"
          % (err.max(), np.log2(err.max()), int(top.sum()), err[top].max() if top.any() else 0.0, g64.max(), g64.min()))
    assert float(err.max()) <= R.E_G
    g2, none = _noise(12345, 3, 16, rows, VT, with_words=False)
    assert none is None and np.array_equal(g2, g)                                 # the words are optional; the same bits


# ---- nir_sample_gen ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ratios():
    w = {"fused": 0.0, "plain": 0.0, "fused_lse": 0.0, "plain_lse": 0.0, "near": 0}
    yield w
    print("sample envelope: largest ratios %s" % {k: round(v, 3) for k, v in w.items()})


@pytest.mark.parametrize("ci", range(len(R.GEN_CASES)))
def test_gen_both_forms_against_fp64(ci, ratios):
    rows, K, VT, tau, bias, nsrc = R.GEN_CASES[ci]
    seed, step = R.GEN_SEEDS[ci], R.GEN_STEPS[ci]
    x, w, b, dom = R.gen_problem(ci)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    frag = _pack(wd)
    assert (frag is None) == (K % 32 != 0)
    for form, f, n_split in (("fused", frag, 1), ("plain", None, 0)):
        if form == "fused" and f is None:
            continue
        tag = "rows=%d K=%d VT=%d tau=%g %s %s" % (rows, K, VT, tau, bias, form)
        d = R.gen_reference(ci, n_split)
        tok, lp, lse = _gen(xd, wd, bd, f, nsrc, tau, seed, step)
        tok2, lp2, lse2 = _gen(xd, wd, bd, f, nsrc, tau, seed, step)
        assert torch.equal(tok, tok2) and torch.equal(lp, lp2) and torch.equal(lse, lse2), tag       # the same inputs give the same bits
        tok3, lp3, none = _gen(xd, wd, bd, f, nsrc, tau, seed, step, with_lse=False)
        assert none is None and torch.equal(tok, tok3) and torch.equal(lp, lp3), tag                 # lse is optional
        tok, lp, lse = tok.cpu().long(), lp.cpu(), lse.cpu()
        assert bool(((tok >= 0) & (tok < VT)).all()) and bool(torch.isfinite(lp).all()) and bool(torch.isfinite(lse).all()), tag
        ok, near = R.accept_tokens(tok, d["ref"], d["e_p"])
        print("%s: e_y %.3g e_p %.3g near-tie rows %d, tokens differing from fp64 %d" % (tag, d["e_y"], d["e_p"], near, int((tok != d["ref"]["token"]).sum())))
        ratios["near"] += near
        assert ok, tag
        assert near <= rows // 100, tag
        if dom is not None:
            assert bool((tok == dom).all()), tag
        ref = score_ref.gen_target(x, w, b, tok, pad=-1)                           # (a sampled PAD counts like any token)
        chain = score_ref.gen_target(x, w, b, tok, pad=-1, dtype=torch.float32)
        ok, fig = score_ref.accept_rows(lp, ref, chain, 2 * n_split)
        print("%s: logp e %.3g e_chain %.3g ratio %.3g" % (tag, fig["e"], fig["e_chain"], fig["ratio"]))
        ratios[form] = max(ratios[form], fig["ratio"])
        assert ok, (tag, fig)
        ok, fig = score_ref.accept_rows(lse, (ref[1], None, ref[2]), (chain[1],), n_split)
        ratios[form + "_lse"] = max(ratios[form + "_lse"], fig["ratio"])
        assert ok, (tag, "lse", fig)


def test_the_draw_moves_with_seed_step_and_row_keying_and_not_with_the_form_of_the_rows():
    ci = 4                                                                        # 63 rows, K 1024, VT 4099, nsrc 3
    rows, K, VT, tau, bias, nsrc = R.GEN_CASES[ci]
    x, w, b, _ = R.gen_problem(ci)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    frag = _pack(wd)
    base = _gen(xd, wd, bd, frag, nsrc, tau, 5, 2)[0].cpu()
    for kw in (dict(seed=6, step=2, nsrc=nsrc), dict(seed=5, step=3, nsrc=nsrc), dict(seed=5, step=2, nsrc=7), dict(seed=5 + (1 << 32), step=2, nsrc=nsrc)):
        assert not torch.equal(_gen(xd, wd, bd, frag, kw["nsrc"], tau, kw["seed"], kw["step"])[0].cpu(), base), kw
    # rows 3 .. 5 of a call over nsrc = 3 source rows are sample 1 of source rows 0 .. 2: the same draws as rows 7 .. 9 of a call over 7
    big = torch.cat((xd[:3], xd[:4], xd[3:6], xd[:4]))                           # rows n 7 + b: (b, n) = (0..2, 1) at rows 7 .. 9
    other = _gen(big, wd, bd, frag, 7, tau, 5, 2)[0].cpu()
    assert torch.equal(other[7:10], base[3:6])
    with lib.tunable("exact_f32", 1, 0):
        exact = _gen(xd, wd, bd, frag, nsrc, tau, 5, 2)
    plain = _gen(xd, wd, bd, None, nsrc, tau, 5, 2)
    assert torch.equal(exact[0], plain[0]) and torch.equal(exact[1], plain[1])    # the fragment is ignored under the tunable


# ---- nir_sample_topk_select ----------------------------------------------------------------------------------------------------------------------------
def _topk_select(x, w, b, frag, nsrc, K_top, tau, seed, step):
    L = lib.load()
    rows, K = x.shape
    VT = w.shape[0]
    nb = L.nir_beam_gen_topk_workspace_bytes(rows, K, VT, K_top, 1 if frag is not None else 0)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    tv, ti = torch.empty(rows, K_top, device=DEV), torch.empty(rows, K_top, dtype=torch.int32, device=DEV)
    lse = torch.empty(rows, device=DEV)
    lib.check(L.nir_beam_gen_topk(lib.ptr(x), rows, K, lib.ptr(w), lib.ptr(b), lib.ptr(frag), VT, K_top, lib.ptr(ws), nb, lib.ptr(tv), lib.ptr(ti), lib.ptr(lse),
                                  lib.stream()), "nir_beam_gen_topk")
    tok = torch.full((rows,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((rows,), float("nan"), device=DEV)
    lib.check(L.nir_sample_topk_select(lib.ptr(tv), lib.ptr(ti), lib.ptr(lse), rows, nsrc, K_top, 1.0 / tau, seed, step, lib.ptr(tok), lib.ptr(lp),
                                       lib.stream()), "nir_sample_topk_select")
    return tok.cpu().long(), lp.cpu(), tv.cpu(), ti.cpu().long(), lse.cpu()


@pytest.mark.parametrize("ci,K_top", [(4, 3), (7, 8), (5, 5), (12, 2)])
def test_topk_select_is_the_fp64_restriction_to_the_lists(ci, K_top):
    rows, K, VT, tau, bias, nsrc = R.GEN_CASES[ci]
    x, w, b, _ = R.gen_problem(ci)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    for frag in ((_pack(wd), None) if K % 32 == 0 else (None,)):
        tok, lp, tv, ti, lse = _topk_select(xd, wd, bd, frag, nsrc, K_top, tau, 9, 4)
        # the float64 choice among the DEVICE's lists: the noise of the ids, the fp32 values as they are
        g = torch.from_numpy(R.gumbel(R.words(9, 4, nsrc, rows, VT, ti.numpy())))
        p = tv.double() * float(np.float32(1.0 / tau)) + g
        best = p.max(1, keepdim=True)[0]
        want = torch.where(p == best, ti, torch.full_like(ti, 1 << 40)).min(1)[0]
        srt = torch.sort(p, 1, descending=True)[0]
        clear = (srt[:, 0] - srt[:, 1]) > 2 * (R.E_G + 2.0 ** -23 * float(p.abs().max()))
        assert bool(clear.all())                                                   # (seed 9 leaves no near-tie in these cases)
        assert torch.equal(tok, want)
        pos = (ti == tok.unsqueeze(1)).long().argmax(1)
        assert torch.equal(lp, tv.gather(1, pos.unsqueeze(1)).squeeze(1) - lse)      # the same fp32 subtraction
        for seed in (1, 2, 3):
            one = _topk_select(xd, wd, bd, frag, nsrc, 1, tau, seed, 0)
            assert torch.equal(one[0], one[3][:, 0])                              # K = 1: the greedy token, whatever the seed


# ---- the statistical criterion -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_chi_square_of_the_draws_against_the_softmax(tau):
    x, w, b = R.stat_problem()
    rows = x.shape[0]
    l64 = x[:1].double() @ w.double().t() + b.double()
    probs = torch.softmax(l64[0] / tau, 0).numpy()
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    for form, frag in (("fused", _pack(wd)), ("plain", None)):
        for seed in (21, 22):
            tok = _gen(xd, wd, bd, frag, 128, tau, seed, 0)[0].cpu().numpy()
            v = R.chi_square(tok, probs)
            pv, df, thr = R.chi_square_pooled(tok, probs)                        # cells below five expected draws taken as one (tau = 0.5)
            print("chi-square %s tau=%g seed=%d rows=%d: %.1f (threshold %g); pooled %.1f at %d degrees of freedom (threshold %.1f)"
                  % (form, tau, seed, rows, v, R.CHI2_THRESHOLD, pv, df, thr))
            assert v < R.CHI2_THRESHOLD, (form, tau, seed)
            assert pv < thr, (form, tau, seed, "pooled")
