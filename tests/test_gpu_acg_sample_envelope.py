"""GPU (-m gpu): one draw per row of ACG's collapsed extended distribution at the C ABI (nir_acg_sample_gen_select; csrc/sample.hip:
sample_gen_kernel<.., PAD>, sample_row_kernel<PAD>, acg_sample_row_kernel, and the top-k form on nir_acg_beam_gen_select's lists) against the
float64 restatement of tests/acg_sample_ref.py, which forms the full collapsed row, across the envelope and in both generator forms.

Problems: acg_sample_ref.gen_problem -- per row one class is planted so that its winner does not depend on the noise (vocabulary-only winner,
slot-only winner, a target entering by its mass, the raw perturbed winner being a target, two slots sharing a target, PAD as raw winner, PAD as
target) next to generic rows; slots without a position (mass 0), source rows of length 0 and map entries outside [0, CV) are part of every problem
that has room for them.  Before the GPU is asked, float64 asserts that every planted row's winner is the planted id with a gap above the bound,
and that at most 1 % of a case's rows are near ties.

Tokens: the float64 token wherever the float64 top-two gap of the perturbed values exceeds 2 E_p, E_p = E_y / tau + E_G + 2^-23 max |p|
(sample_ref.perturbed_bound, section 28's: E_y from the float32 restatement's logits with one split product in the fused form, and one fp32
rounding of the perturbed value itself at the largest |p| of the case); elsewhere one of the candidates inside the bound.  logp: score_ref.accept_rows-
style at the device's token.  The statistical case: 16384 identical rows against P^(1/tau) by Pearson's chi-square."""
import numpy as np
import pytest
import torch

import acg_sample_ref as R
import acg_score_ref as SC
import sample_ref as SR
from context_attentive_ir_amd import lib
from test_gpu_seq2seq_envelope import _pack

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG, BAD_WS = -1, -3
#          K     VT    rows CV    QL  tau   top_k
CONFIGS = [(32, 5, 1, 2, 1, 1.0, 0), (32, 37, 17, 3, 7, 0.25, 1), (48, 37, 65, 10, 7, 4.0, 0), (48, 4099, 17, 65, 65, 1.0, 3),
           (96, 37, 65, 10, 7, 0.25, 0), (96, 4099, 65, 1024, 65, 1.0, 8), (96, 37, 17, 65, 65, 4.0, 3), (1024, 4099, 65, 65, 65, 4.0, 0),
           (1024, 37, 17, 10, 7, 1.0, 8), (1024, 5, 65, 3, 1, 0.25, 3), (96, 4099, 17, 10, 65, 1.0, 0)]


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _draw(d, nsrc, tau, top_k, seed, step, fused, bytes_=None, rows=None, stats=False):
    """-> (rc, token [R], logp [R], (gen_max, gen_lse) or None); the outputs start at -7"""
    L = lib.load()
    o, Wg = d["o"], d["gen_w"]
    n = o.shape[0]
    rows = n if rows is None else rows
    K, VT, QL, CV = o.shape[1], Wg.shape[0], d["attn"].shape[1], d["e2t"].shape[1]
    frag = None
    if fused:
        frag, flag = _pack(Wg.to(DEV))
        assert frag is not None and flag == 0
    t = [_dev(d[k]) for k in ("o", "gen_w", "gen_b", "copy_w", "copy_b", "attn", "lens", "smap", "e2t")]
    e2s = torch.ones(nsrc, CV, dtype=torch.long, device=DEV)
    nb = L.nir_acg_sample_gen_select_workspace_bytes(max(rows, 1), K, VT, top_k, int(fused))
    ws = torch.empty(max(1, nb if bytes_ is None else bytes_), dtype=torch.uint8, device=DEV)
    tok = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    lp = torch.full((n,), -7.0, device=DEV)
    gm, gl = (torch.full((n,), -7.0, device=DEV), torch.full((n,), -7.0, device=DEV)) if stats else (None, None)
    rc = L.nir_acg_sample_gen_select(lib.ptr(t[0]), rows, nsrc, K, lib.ptr(t[1]), lib.ptr(t[2]), lib.ptr(frag), VT, top_k, 1.0 / tau, seed, step,
                                     lib.ptr(t[3]), lib.ptr(t[4]), lib.ptr(t[5]), QL, lib.ptr(t[6]), QL, lib.ptr(t[7]), lib.ptr(t[8]), lib.ptr(e2s), CV,
                                     lib.ptr(ws), ws.numel() if bytes_ is None else bytes_, lib.ptr(tok), lib.ptr(lp), lib.ptr(gm), lib.ptr(gl),
                                     lib.stream())
    torch.cuda.synchronize()
    return rc, tok.cpu().long(), lp.cpu(), ((gm.cpu(), gl.cpu()) if stats else None)


def _problem(K, VT, rows, nsrc, CV, QL, tau, top_k):
    """the first problem seed whose float64 reference has at most 1 % near-tie rows under the fused form's bound (the wider one)"""
    for ps in range(8):
        d = R.gen_problem(rows, nsrc, K, VT, CV, QL, seed=ps * 101 + K + VT + rows)
        g = R.gen_reference(d, nsrc, 1000 + K + CV, (3, 1 << 20, 0, 7)[ps % 4], tau, top_k, 1)
        near = int((g["ref"]["gap"] <= 2 * g["e_p"]).sum())
        if near <= rows // 100:
            return d, ps, near
    raise AssertionError("no problem seed with at most 1 % near ties")


def _logp_ok(d, nsrc, tok, lp, n_split):
    """score_ref.accept_rows' bound on log P at the device's token, float64 against the float32 restatement, the same for every kind of token"""
    l64, live, lg, _ = R.gen_rows(d, nsrc)
    l32 = R.gen_rows(d, nsrc, torch.float32)[0]
    ref = l64.gather(1, tok.unsqueeze(1)).squeeze(1)
    chain = l32.gather(1, tok.unsqueeze(1)).squeeze(1)
    assert bool(live.gather(1, tok.unsqueeze(1)).all()), "a collapsed slot was drawn"
    assert bool(torch.isfinite(ref).all()), "an entry of probability 0 was drawn"
    return SC.accept_rows(lp, ref, chain, float(lg.abs().max()), n_split)


@pytest.mark.parametrize("K,VT,rows,CV,QL,tau,top_k", CONFIGS)
def test_tokens_and_logp_against_fp64_in_both_forms(K, VT, rows, CV, QL, tau, top_k):
    seen = set()
    for nsrc in sorted({1, rows}):
        d, ps, near0 = _problem(K, VT, rows, nsrc, CV, QL, tau, top_k)
        seed, step = 1000 + K + CV, (3, 1 << 20, 0, 7)[ps % 4]
        seen.update(R.GEN_CLASSES[i] for i in d["cls"].tolist())
        planted = d["want"] >= 0
        for fused in ((True, False) if K % 32 == 0 else (False,)):
            g = R.gen_reference(d, nsrc, seed, step, tau, top_k, 1 if fused else 0)
            ref = g["ref"]
            assert bool(torch.equal(ref["token"][planted], d["want"][planted])) and bool((ref["gap"][planted] > 2 * g["e_p"]).all())
            rc, tok, lp, st = _draw(d, nsrc, tau, top_k, seed, step, fused, stats=top_k == 0)
            assert rc == 0
            ok, near = R.accept_tokens(tok, g)
            print("acg sample envelope K=%d VT=%d rows=%d nsrc=%d CV=%d QL=%d tau=%g top_k=%d fused=%s: e_p %.3g near ties %d" %
                  (K, VT, rows, nsrc, CV, QL, tau, top_k, fused, g["e_p"], near))
            assert ok and near <= rows // 100, (tok != ref["token"]).nonzero().flatten()[:8]
            ok, fig = _logp_ok(d, nsrc, tok, lp, 1 if fused else 0)
            assert ok, fig
            if st is not None:                                                      # m and m + log Z of the PAD-substituted logits
                lg = R.gen_rows(d, nsrc)[2]
                e_st = 2 * g["e_y"]                                                 # E_y bounds a logit: the maximum and the log-sum-exp move no further
                assert float((st[0].double() - lg.max(1)[0]).abs().max()) <= e_st
                assert float((st[1].double() - torch.logsumexp(lg, 1)).abs().max()) <= e_st + 1e-5
            again = _draw(d, nsrc, tau, top_k, seed, step, fused)
            assert torch.equal(again[1], tok) and torch.equal(again[2], lp)         # the same bits
            if top_k == 1:                                                          # the arg-max of P, whatever the seed and the temperature
                other = _draw(d, nsrc, 4.0, 1, seed + 99, step + 1, fused)
                assert torch.equal(other[1], tok)
    print("acg sample envelope K=%d VT=%d rows=%d CV=%d QL=%d: classes %s" % (K, VT, rows, CV, QL, sorted(seen)))


def test_every_class_is_planted_somewhere():
    seen = set()
    for K, VT, rows, CV, QL, tau, top_k in CONFIGS:
        for nsrc in sorted({1, rows}):
            seen.update(R.GEN_CLASSES[i] for i in R.gen_problem(rows, nsrc, K, VT, CV, QL, seed=K + VT + rows)["cls"].tolist())
    assert seen == set(R.GEN_CLASSES), set(R.GEN_CLASSES) - seen


# ---- the statistical case: 16384 rows of identical o, nsrc = 1, K 32, VT 37, CV 5 --------------------------------------------------------------------
@pytest.mark.parametrize("tau", [0.5, 1.0, 2.0])
def test_chi_square_against_the_tempered_collapsed_distribution(tau):
    d = R.stat_problem()
    VT, CV = R.STAT_VT, R.STAT_CV
    one = {k: (v[:1] if k in ("o", "attn") else v) for k, v in d.items()}
    logp, live, _, _ = R.gen_rows(one, 1)
    q = torch.where(live[0], logp[0] / tau, torch.full_like(logp[0], float("-inf")))
    probs = torch.softmax(q, 0).numpy()
    dead = [VT + 1, VT + 2, VT + 3, VT + 4]                                         # the empty slot and the three collapsed ones
    assert all(probs[e] == 0 for e in dead) and probs[VT] > 0 and int((probs > 0).sum()) == VT + 1
    df = int((probs > 0).sum()) - 1
    threshold = SR.wilson_hilferty(df, SR.Z_1E6)
    for fused in (True, False):
        rc, tok, lp, _ = _draw(d, 1, tau, 0, 77 + int(tau * 10), 2, fused)
        assert rc == 0
        counts = np.bincount(tok.numpy(), minlength=VT + CV)
        assert all(counts[e] == 0 for e in dead)                                    # no collapsed or empty slot is ever drawn
        keep = probs > 0
        stat = SR.chi_square(np.searchsorted(np.nonzero(keep)[0], tok.numpy()), probs[keep])
        pooled, pdf, pthr = SR.chi_square_pooled(np.searchsorted(np.nonzero(keep)[0], tok.numpy()), probs[keep])
        print("acg sample chi-square tau=%g fused=%s: %.1f (df %d, threshold %.1f); pooled %.1f (df %d, threshold %.1f)" %
              (tau, fused, stat, df, threshold, pooled, pdf, pthr))
        assert stat <= threshold and pooled <= pthr


def test_empty_batch_and_bad_arguments_leave_the_outputs_untouched():
    d = R.gen_problem(6, 2, 32, 17, 3, 7, seed=1)
    untouched = lambda r: bool((r[1] == -7).all()) and bool((r[2] == -7).all())      # noqa: E731
    for fused in (True, False):
        for top_k in (0, 3):
            r = _draw(d, 2, 1.0, top_k, 1, 0, fused, rows=0)                       # rows = 0 over live buffers
            assert r[0] == 0 and untouched(r)
            r = _draw(d, 2, 1.0, top_k, 1, 0, fused, bytes_=16)
            assert r[0] == BAD_WS and untouched(r)
    for kw in (dict(top_k=9), dict(top_k=-1), dict(nsrc=7), dict(tau=float("inf")), dict(step=-1), dict(step=1 << 32)):
        a = dict(nsrc=2, tau=1.0, top_k=0, seed=1, step=0)
        a.update(kw)
        r = _draw(d, a["nsrc"], a["tau"], a["top_k"], a["seed"], a["step"], False)
        assert r[0] == BAD_ARG and untouched(r), kw
    r = _draw(d, 2, 1.0, 3, 1, 0, False, stats=True)                               # the pair belongs to the whole-distribution form
    assert r[0] == BAD_ARG and untouched(r) and bool((r[3][0] == -7).all())
    L = lib.load()
    p = lib.C.c_void_p(16)
    f = L.nir_acg_sample_gen_select
    assert f(p, 2, 1, 96, p, p, None, 10, 0, 1.0, 0, 0, p, p, p, 7, p, 7, p, p, p, 1, p, 1 << 20, p, p, None, None, None) == BAD_ARG        # CV
    assert f(p, 2, 1, 96, p, p, None, 10, 0, 1.0, 0, 0, p, p, p, 5000, p, 5000, p, p, p, 5, p, 1 << 20, p, p, None, None, None) == BAD_ARG  # QL
    assert f(p, 2, 1, 96, p, p, None, 10, 0, 0.0, 0, 0, p, p, p, 7, p, 7, p, p, p, 5, p, 1 << 20, p, p, None, None, None) == BAD_ARG        # 1 / tau
    assert f(None, 2, 1, 96, p, p, None, 10, 0, 1.0, 0, 0, p, p, p, 7, p, 7, p, p, p, 5, p, 1 << 20, p, p, None, None, None) == BAD_ARG     # null
    assert f(p, 2, 1, 98, p, p, None, 10, 0, 1.0, 0, 0, p, p, p, 7, p, 7, p, p, p, 5, p, 1 << 20, p, p, None, None, None) == BAD_ARG        # K % 4
    assert f(p, 2, 1, 96, p, p, None, 10, 0, 1.0, 0, 0, p, p, p, 6, p, 7, p, p, p, 5, p, 1 << 20, p, p, None, None, None) == BAD_ARG        # stride < QL
