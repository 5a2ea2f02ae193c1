"""GPU (-m gpu): nir_score_gen_target and nir_score_sequences at the C ABI (csrc/score.hip), both forms of the generator judged by
score_ref's criterion against float64 (n_split = 2 per token log-probability and 1 per lse on the fused form, 0 on the plain form).

The cases are a list, not a cross product: rows at the row-tile and row-block edges (16 / 64 rows at K <= 512, 32 beyond), K at one k-step, a
full chunk, the clamped chunk (288 = nine k-steps), the NBT switch (512 | 544) and the largest, VT from one tile with three idle waves (5) to
several vocabulary ranges (4099), and four row counts computed from the device: enough row blocks that the number of ranges that fills the
chip once stays under its cap; more row blocks than CUs, where the grid runs in several rounds and the ranges are few and long (at K = 1024 and
at K = 32); and one past the host's row chunk.  Every case carries the targets 0 (PAD), 1, 15, 16, VT - 1, VT and -1 (the last two, and whatever else lies past VT, are
flagged and read 0) among random ones, and a duplicate of row 0 in its last row.  Operand families: gemm_ref.family inputs; the bias random,
ascending in v (the running maximum moves at every tile), descending, or with one logit dominant by +80 -- with the target on it, and with the
target 80 below the rest (lse = max, log-probability ~ -160, finite).  Large cases are judged on a sample of rows (rows are independent)."""
import pytest
import torch

import gemm_ref
import score_ref as R
from context_attentive_ir_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 1 << 18


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _nbt(K):
    return 4 if K <= 512 else 2


def _nvr(rows, K, VT, cu):
    """score_nvr of csrc/score.hip, restated -> (ranges, row blocks, rounds of workgroups over the CUs, the cap)"""
    nrb, ntiles = -(-rows // (16 * _nbt(K))), -(-VT // 16)
    cap = max(1, min(256, (ntiles + 7) // 8))
    nvr = min(range(1, cap + 1), key=lambda n: (-(-nrb * n // cu) * (12 + -(-ntiles // n)), n))
    return nvr, nrb, -(-nrb * nvr // cu), cap


def _cases():
    cu = _cu()
    big2, big4 = 32 * (cu + 1) + 1, 64 * (cu + 1) + 1
    mid = 64 * -(-cu // 24) - 5                     # ~11 row blocks: enough ranges to fill the chip once, under the cap
    return [(1, 32, 5, "randn", "rand"), (16, 64, 16, "randn", "asc"), (17, 256, 17, "randn", "desc"), (63, 288, 250, "randn", "rand"),
            (64, 512, 250, "positive", "asc"), (65, 544, 250, "randn", "desc"), (129, 1024, 250, "randn", "rand"), (129, 32, 4099, "randn", "asc"),
            (65, 512, 4099, "positive", "desc"), (17, 544, 4099, "randn", "rand"), (64, 1024, 4099, "tiny", "asc"), (1, 288, 4099, "randn", "desc"),
            (63, 64, 5, "randn", "asc"), (129, 256, 17, "tiny", "rand"), (16, 1024, 16, "randn", "desc"), (32, 544, 5, "randn", "rand"),
            (33, 1024, 4099, "randn", "rand"), (mid, 96, 4099, "randn", "asc"), (64, 48, 250, "randn", "rand"),
            (65, 32, 250, "randn", "dom_on"), (65, 512, 4099, "randn", "dom_off"), (17, 288, 17, "randn", "dom_on"), (129, 544, 250, "randn", "dom_off"),
            (big2, 1024, 4099, "randn", "rand"), (big4, 32, 250, "randn", "asc"), (CHUNK + 17, 32, 5, "randn", "rand")]


def _problem(rows, K, VT, fam, bias):
    g = torch.Generator().manual_seed(rows * 31 + K * 7 + VT)
    x, w = gemm_ref.family(fam, g, rows, K, "a"), gemm_ref.family(fam, g, VT, K, "w")
    special = torch.tensor([0, 1, 15, 16, VT - 1, VT, -1])
    tg = torch.randint(0, VT, (rows,), generator=g)
    pos = torch.randperm(rows, generator=g)[:7]
    tg[pos] = special[:pos.numel()]
    if bias == "asc":
        b = torch.arange(VT).float() / 4
    elif bias == "desc":
        b = -torch.arange(VT).float() / 4
    else:
        b = torch.randn(VT, generator=g)
    if bias.startswith("dom"):
        top, low = (VT * 2) // 3, VT // 3
        b[top] += 80
        b[low] -= 80
        tg[::2] = top if bias == "dom_on" else low
    if rows > 1:
        x[rows - 1], tg[rows - 1] = x[0], tg[0]
    return x, w, b, tg


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


def _score(x, w, b, frag, tg, pad=R.PAD, with_lse=True):
    L = lib.load()
    rows, K = x.shape
    VT = w.shape[0]
    nb = L.nir_score_gen_target_workspace_bytes(rows, K, VT, 1 if frag is not None else 0)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    lp = torch.full((rows,), float("nan"), device=DEV)
    lse = torch.full((rows,), float("nan"), device=DEV) if with_lse else None
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.check(L.nir_score_gen_target(lib.ptr(x), rows, K, lib.ptr(w), lib.ptr(b), lib.ptr(frag), VT, lib.ptr(tg), pad, lib.ptr(ws), nb, lib.ptr(lp),
                                     lib.ptr(lse), lib.ptr(flag), lib.stream()), "nir_score_gen_target")
    return lp, lse, int(flag.item())


def _sample(rows):
    if rows <= 512:
        return torch.arange(rows)
    g = torch.Generator().manual_seed(rows)
    edge = torch.arange(CHUNK - 3, CHUNK + 3) if rows > CHUNK + 3 else torch.arange(0)          # either side of the host's row chunk
    return torch.unique(torch.cat([torch.arange(70), torch.arange(rows - 70, rows), edge, torch.randint(0, rows, (300,), generator=g)]))


@pytest.fixture(scope="module")
def worst():
    w = {"fused": 0.0, "plain": 0.0, "fused_lse": 0.0, "plain_lse": 0.0}
    yield w
    print("score envelope: largest ratios %s" % {k: round(v, 3) for k, v in w.items()})


@pytest.mark.parametrize("ci", range(26))
def test_gen_target_both_forms_against_fp64(ci, worst):
    rows, K, VT, fam, bias = _cases()[ci]
    x, w, b, tg = _problem(rows, K, VT, fam, bias)
    keep = _sample(rows)
    ref = R.gen_target(x[keep], w, b, tg[keep])
    chain = R.gen_target(x[keep], w, b, tg[keep], dtype=torch.float32)
    if bias == "dom_off":
        assert float(ref[0].min()) < -150
    xd, wd, bd, td = x.to(DEV), w.to(DEV), b.to(DEV), tg.to(DEV)
    frag = _pack(wd)
    assert (frag is None) == (K % 32 != 0)
    bad_any = bool(((tg < 0) | (tg >= VT)).any())
    for form, f in (("fused", frag), ("plain", None)):
        if form == "fused" and f is None:
            continue
        tag = "rows=%d K=%d VT=%d %s %s %s" % (rows, K, VT, fam, bias, form)
        lp, lse, flag = _score(xd, wd, bd, f, td)
        lp2, lse2, _ = _score(xd, wd, bd, f, td)
        assert torch.equal(lp, lp2) and torch.equal(lse, lse2), tag                # the same inputs give the same bits
        assert flag == int(bad_any), tag
        lp, lse = lp.cpu(), lse.cpu()
        assert bool(torch.isfinite(lp).all()) and bool(torch.isfinite(lse).all()), tag
        masked = (tg == R.PAD) | (tg < 0) | (tg >= VT)
        assert bool((lp[masked] == 0).all()), tag
        ok, fig = R.accept_rows(lp[keep], ref, chain, 2 if form == "fused" else 0)
        print("%s: logp e %.3g e_chain %.3g ratio %.3g" % (tag, fig["e"], fig["e_chain"], fig["ratio"]))
        worst[form] = max(worst[form], fig["ratio"])
        assert ok, (tag, fig)
        if rows > 1:                                                               # the duplicate of row 0 at the far end: both inside row 0's bound
            assert abs(float(lp[rows - 1]) - float(lp[0])) <= 2 * fig["bound"] * fig["s"], tag
        ok, fig = R.accept_rows(lse[keep], (ref[1], None, ref[2]), (chain[1],), 1 if form == "fused" else 0)
        worst[form + "_lse"] = max(worst[form + "_lse"], fig["ratio"])
        assert ok, (tag, "lse", fig)


def test_the_cases_take_every_branch_of_the_geometry():
    """recomputed from this device's CU count: one range and several, each with more than one row block (both coordinates of the grid mapping
    move); grids of one round and of several; the number of ranges at its cap and under it"""
    cu = _cu()
    seen = set()
    for rows, K, VT, _, _ in _cases():
        if K % 32:
            continue
        for n_rows in ([rows] if rows <= CHUNK else [CHUNK, rows - CHUNK]):
            nvr, nrb, rounds, cap = _nvr(n_rows, K, VT, cu)
            seen.add(("one range" if nvr == 1 else "ranges", "row blocks" if nrb > 1 else "one row block"))
            seen.add("rounds" if rounds > 1 else "one round")
            seen.add("cap" if nvr == cap else "under the cap")
            if nvr > 1 and rounds > 1:
                seen.add("ranges over several rounds")
    assert {("one range", "row blocks"), ("ranges", "row blocks"), ("ranges", "one row block"), "rounds", "one round", "cap", "under the cap",
            "ranges over several rounds"} <= seen, seen
    big2 = _nvr(_cases()[-3][0], 1024, 4099, cu)
    assert big2[1] > cu and big2[2] > 1                                            # more row blocks than CUs


def test_the_mask_follows_the_pad_argument_and_lse_is_optional():
    rows, K, VT = 65, 64, 250
    x, w, b, tg = _problem(rows, K, VT, "randn", "rand")
    tg[3], tg[4] = 7, 0
    xd, wd, bd, td = x.to(DEV), w.to(DEV), b.to(DEV), tg.to(DEV)
    for f in (_pack(wd), None):
        lp0, _, _ = _score(xd, wd, bd, f, td, pad=0)
        lp7, none, _ = _score(xd, wd, bd, f, td, pad=7, with_lse=False)
        assert none is None
        assert float(lp0[3]) != 0 and float(lp0[4]) == 0 and float(lp7[3]) == 0 and float(lp7[4]) != 0
        rest = (tg != 0) & (tg != 7)
        assert torch.equal(lp0.cpu()[rest], lp7.cpu()[rest])


def test_the_plain_form_runs_under_exact_f32_and_without_a_fragment():
    rows, K, VT = 65, 64, 250
    x, w, b, tg = _problem(rows, K, VT, "randn", "rand")
    xd, wd, bd, td = x.to(DEV), w.to(DEV), b.to(DEV), tg.to(DEV)
    frag = _pack(wd)
    plain = _score(xd, wd, bd, None, td)[0]
    fused = _score(xd, wd, bd, frag, td)[0]
    with lib.tunable("exact_f32", 1, 0):
        exact = _score(xd, wd, bd, frag, td)[0]
        exact_plain = _score(xd, wd, bd, None, td)[0]
    assert torch.equal(exact, exact_plain)                                         # the fragment is ignored under the tunable
    assert not torch.equal(fused, plain)                                           # two different kernels ran


@pytest.mark.parametrize("pad,eos", [(0, 3), (9, 3), (0, -1)])
def test_sequences_against_the_restatement(pad, eos):
    g = torch.Generator().manual_seed(5)
    nseq, Tn = 300, 7                                                              # two blocks of 256 threads
    tg = torch.randint(-1, 12, (nseq, Tn), generator=g)
    lp = -torch.rand(nseq, Tn, generator=g) * 9
    want = R.sequences(lp, tg, pad, eos)
    lpd, sc, ln = lp.to(DEV), torch.empty(nseq, device=DEV), torch.empty(nseq, dtype=torch.int64, device=DEV)
    lib.check(lib.load().nir_score_sequences(lib.ptr(lpd), lib.ptr(tg.to(DEV)), nseq, Tn, pad, eos, lib.ptr(sc), lib.ptr(ln), lib.stream()),
              "nir_score_sequences")
    assert torch.equal(lpd.cpu(), want[0]) and torch.equal(ln.cpu(), want[2])
    assert torch.equal(sc.cpu(), want[1])                                          # fp32 sums in position order on both sides
