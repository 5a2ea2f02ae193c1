"""GPU (-m gpu): nir_acg_score_gen_target at the C ABI (csrc/score.hip), both forms judged by acg_score_ref's criterion against float64
(n_split = 2 per token on the fused form, 0 on the plain form).

The cases are a list, not a cross product; each is one vocabulary-wide row set of acg_score_ref.planted, which cycles every target class its
shape can hold over the rows (PAD; a PAD-substituted word reached through a slot that collapses onto id 0; a word without copy mass; a word
with one slot on two positions; a word shared by two slots; an un-collapsed slot; a collapsed slot id; slots 0 and 1; a slot without a position:
log 0; VT + CV: flagged; -1) and poisons the map and the attention behind the length.  Rows 1, 15, 16, 17, 65, 129 and one case past the
host's chunk of 2^18 rows; rows_per_src 1, 3 and rows; K 32, 288, 512, 1024 and the plain-only 48; VT 5, 17, 4099; CV 2, 9, 1024; QL 1, 7, 64
and 4096; lengths 1 and QL; switch logit 0, +40, -40; one logit dominant by +80 with the target on it and below it.  The large case is judged
on a sample of rows (rows are independent); the number of -inf outputs is counted over all rows."""
import pytest
import torch

import acg_score_ref as R
from context_attentive_ir_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
CHUNK = 1 << 18

#        rows, rows_per_src, K, VT, CV, QL, length, switch, dominant
CASES = [(1, 1, 32, 5, 2, 1, "full", 0.0, False),
         (15, 3, 288, 17, 9, 7, "mixed", 0.0, False),
         (16, 16, 512, 4099, 9, 7, "full", 40.0, False),
         (17, 1, 1024, 17, 1024, 64, "full", -40.0, False),
         (65, 65, 32, 4099, 9, 7, "one", 0.0, True),
         (129, 3, 512, 17, 9, 4096, "full", 0.0, False),
         (66, 3, 48, 17, 9, 7, "mixed", 0.0, False),
         (129, 1, 1024, 4099, 1024, 64, "mixed", 0.0, True),
         (65, 1, 288, 5, 2, 7, "full", -40.0, False),
         (CHUNK + 16, (CHUNK + 16) // 16, 32, 17, 9, 7, "mixed", 0.0, False)]


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


def _device(c):
    return {k: (v.to(DEV).contiguous() if torch.is_tensor(v) else v) for k, v in c.items()}


def _score(d, frag, target=None, pad=R.PAD):
    L = lib.load()
    rows, K = d["o"].shape
    VT, CV, QL = d["gen_w"].shape[0], d["e2t"].shape[1], d["smap"].shape[1]
    nb = L.nir_acg_score_gen_target_workspace_bytes(rows, K, VT, 1 if frag is not None else 0)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    lp = torch.full((rows,), float("nan"), device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    tg = d["target"] if target is None else target
    lib.check(L.nir_acg_score_gen_target(lib.ptr(d["o"]), rows, d["rows_per_src"], K, lib.ptr(d["gen_w"]), lib.ptr(d["gen_b"]), lib.ptr(frag), VT,
                                         lib.ptr(d["copy_w"]), lib.ptr(d["copy_b"]), lib.ptr(d["attn"]), QL, lib.ptr(d["lens"]), QL, lib.ptr(d["smap"]),
                                         lib.ptr(d["e2t"]), CV, lib.ptr(tg), pad, lib.ptr(ws), nb, lib.ptr(lp), lib.ptr(flag), lib.stream()),
              "nir_acg_score_gen_target")
    return lp, int(flag.item())


def _sample(rows):
    if rows <= 512:
        return None
    g = torch.Generator().manual_seed(rows)
    edge = torch.arange(CHUNK - 3, CHUNK + 3)                                     # either side of the host's row chunk
    return torch.unique(torch.cat([torch.arange(70), torch.arange(rows - 70, rows), edge, torch.randint(0, rows, (300,), generator=g)]))


@pytest.fixture(scope="module")
def worst():
    w = {"fused": 0.0, "plain": 0.0}
    yield w
    print("acg score envelope: largest ratios %s" % {k: round(v, 3) for k, v in w.items()})


@pytest.mark.parametrize("ci", range(len(CASES)))
def test_gen_target_both_forms_against_fp64(ci, worst):
    rows, rps, K, VT, CV, QL, length, switch, dom = CASES[ci]
    c = R.planted(rows, rps, K, VT, CV, QL, seed=ci, length=length, switch=switch, dominant=dom)
    keep = _sample(rows)
    ref, chain = R.planted_ref(c, keep=keep), R.planted_ref(c, torch.float32, keep=keep)
    s = float(ref[1].abs().max())
    k = slice(None) if keep is None else keep
    tg, cls = c["target"], c["classes"]
    if dom:
        assert float(ref[0][torch.isfinite(ref[0])].min()) < -70 and s > 75
    if abs(switch) == 40:                                                          # a saturated switch keeps its small side: finite, not log 0
        small = ("word_no_mass",) if switch > 0 else ("slot", "slot0", "slot1")
        v = ref[0][torch.isin(cls[k], torch.tensor([R.CLASSES.index(n) for n in small]))]
        v = v[torch.isfinite(v)]
        assert v.numel() > 0 and float(v.max()) < -30
    d = _device(c)
    frag = _pack(d["gen_w"])
    assert (frag is None) == (K % 32 != 0)
    rows_src = torch.arange(rows) // rps
    canon = torch.where((tg >= 0) & (tg < VT + CV), R.canonical(tg, c["e2t"][rows_src], VT), tg)
    canon = torch.where(canon == R.PAD, tg, canon).to(DEV)                         # (id 0 itself is PAD and masked: that slot keeps its spelling)
    for form, f in (("fused", frag), ("plain", None)):
        if form == "fused" and f is None:
            continue
        tag = "rows=%d rps=%d K=%d VT=%d CV=%d QL=%d %s switch=%g dom=%d %s" % (rows, rps, K, VT, CV, QL, length, switch, dom, form)
        lp, flag = _score(d, f)
        lp2, _ = _score(d, f)
        assert torch.equal(lp, lp2), tag                                           # the same inputs give the same bits
        assert flag == int(bool((tg >= VT + CV).any())), tag
        lpc, _ = _score(d, f, canon)                                               # a collapsed slot id: its word's value to the bit
        assert torch.equal(lp, lpc), tag
        lp = lp.cpu()
        assert not bool(torch.isnan(lp).any()) and not bool(torch.isposinf(lp).any()), tag
        masked = (tg == R.PAD) | (tg < 0) | (tg >= VT + CV)
        assert bool((lp[masked] == 0).all()), tag
        assert int(torch.isneginf(lp).sum()) == c["n_inf"], (tag, int(torch.isneginf(lp).sum()), c["n_inf"])     # only the planted zero-mass rows
        ok, fig = R.accept_rows(lp[k], ref[0], chain[0], s, 2 if form == "fused" else 0)
        print("%s: logp e %.3g e_chain %.3g ratio %.3g" % (tag, fig["e"], fig["e_chain"], fig["ratio"]))
        worst[form] = max(worst[form], fig["ratio"])
        assert ok, (tag, fig)
    if rps == 1 and rows > 1:                                                      # -1 is not flagged: the same call without VT + CV
        tg2 = torch.where(tg >= VT + CV, torch.full_like(tg, -1), tg).to(DEV)
        assert bool((tg2 < 0).any()) and _score(d, frag, tg2)[1] == 0


def test_the_mask_follows_the_pad_argument():
    c = R.planted(65, 1, 64, 17, 9, 7, seed=3)
    c["target"][5] = 7
    d = _device(c)
    tg = c["target"]
    for f in (_pack(d["gen_w"]), None):
        lp0, lp7 = _score(d, f, pad=0)[0].cpu(), _score(d, f, pad=7)[0].cpu()
        assert bool((lp0[tg == 0] == 0).all()) and bool((lp7[tg == 0] != 0).all()) and bool((lp7[tg == 7] == 0).all())
        rest = (tg != 0) & (tg != 7)
        assert torch.equal(lp0[rest], lp7[rest])


def test_the_plain_form_runs_under_exact_f32_and_without_a_fragment():
    c = R.planted(65, 5, 64, 250, 9, 7, seed=4)
    d = _device(c)
    frag = _pack(d["gen_w"])
    plain, fused = _score(d, None)[0], _score(d, frag)[0]
    with lib.tunable("exact_f32", 1, 0):
        exact, exact_plain = _score(d, frag)[0], _score(d, None)[0]
    assert torch.equal(exact, exact_plain) and torch.equal(exact, plain)           # the fragment is ignored under the tunable
    assert not torch.equal(fused, plain)                                           # two different kernels ran
