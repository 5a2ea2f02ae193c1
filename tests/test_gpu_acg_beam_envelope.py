"""GPU (-m gpu): the per-row launches and the selection of ACG's beam at the C ABI (nir_acg_beam_gen_select, nir_acg_beam_select; csrc/beam.hip)
against float64, across their envelope, on exactly representable inputs.

Inputs.  The generator's rows are one-hot: a set of "carrier" words spread over [0, VT) reads one feature each (all of [0, VT) when VT fits),
every other word has zero weights and a bias near -12.  Features hold odd multiples of 1/8 within 10 of zero, the bias multiples of 1/64: every logit is one
exact product plus one exact sum, the same number in the split-fp16 MFMA form, in the fp32 GEMM and in float64.  A row's carriers are ranked by a
permutation of its own, 1/4 apart -- adjacent vocabulary entries differ by e^(1/4).  The last feature carries the switch logit.  The raw PAD logit
is 1000 through its bias: it must neither win nor count.  Attention values are multiples of 1/64; garbage sits behind every length.

Per source row one class is planted (cycled; a class that does not fit QL / CV / the carriers gives way to "vocab"):
    vocab       z -> 0: vocabulary-only winners          slots       z -> 1: slot-only winners (as many as fit)
    enters      a collapse target outside the raw top-W enters by its mass
    once        a collapse target inside the raw top-W, offered once with its mass added
    shared      two slots share one target               pad_top     PAD (-1e-20) inside the top-W
    pad_target  PAD is a collapse target                 zero        slots without any position: log 0, never ahead of a finite candidate
    tie         two slots hold the same mass exactly: the lower extended id first
    empty       len = 0: no copy mass at all             outside     map entries outside [0, CV) at j < len are ignored
Before the GPU is asked, float64 asserts that adjacent entries among the top W + 1 of every row are either exactly equal (the planted tie, and
candidates at log 0) or at least 1e-3 apart relative; the ids are then compared exactly, and log P to 1e-5 absolute + relative.

Sizes: K in {32, 48 (plain only), 96, 1024} x VT in {8, 17, 200, 4099} x rows in {1, 17, 65, 97} x nsrc in {1, rows / W} x CV in {2, 3, 10, 65, 1024}
x QL in {1, 7, 65} x W in {1, 3, 8}, every value in at least one configuration, both forms wherever the fused one exists."""
import pytest
import torch

from context_attentive_ir_amd import lib
from test_gpu_seq2seq_envelope import _pack

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG, BAD_WS = -1, -3
PAD_LOGIT = -1e-20
CLASSES = ("vocab", "slots", "enters", "once", "shared", "pad_top", "pad_target", "zero", "tie", "empty", "outside")
#          K     VT   rows CV    QL  W
CONFIGS = [(32, 8, 1, 2, 1, 1), (32, 17, 17, 3, 7, 3), (48, 200, 65, 10, 7, 8), (96, 200, 65, 65, 65, 3), (96, 4099, 97, 10, 7, 8),
           (96, 17, 17, 1024, 65, 1), (1024, 17, 17, 3, 1, 8), (1024, 4099, 1, 65, 7, 3)]


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _inputs(K, VT, rows, nsrc, CV, QL, W, seed):
    g = torch.Generator().manual_seed(seed)
    NC = min(VT, K - 1)                                                      # carriers: word car[k] reads feature k
    car = torch.arange(VT) if VT <= K - 1 else torch.cat([torch.zeros(1, dtype=torch.long), 1 + torch.randperm(VT - 1, generator=g)[:NC - 1]])
    Wg = torch.zeros(VT, K)
    Wg[car, torch.arange(NC)] = 1.0
    b = -12.0 - (torch.arange(VT) % 64).float() / 64
    b[car] = 0.0
    b[0] = 1000.0                                                            # the raw PAD logit is the largest of every row
    o = torch.zeros(rows, K)
    rank = torch.stack([torch.randperm(NC, generator=g) for _ in range(rows)])              # rank[r, k]: 0 = the row's best carrier
    o[:, :NC] = 2.125 - 0.25 * rank.clamp(max=40).float()                    # never 0: PAD's -1e-20 has no near neighbour; eight carriers above it
    zl = torch.zeros(rows)
    attn = torch.zeros(rows, QL)
    lens = torch.zeros(nsrc, dtype=torch.long)
    smap = torch.zeros(nsrc, QL, dtype=torch.long)
    e2t = torch.full((nsrc, CV), -1, dtype=torch.long)
    e2t[:, :2] = int(car[min(1, NC - 1)])                                    # slots 0 and 1 are never collapsed, whatever their entry says
    names = []
    for s in range(nsrc):
        cls = CLASSES[(s + seed) % len(CLASSES)]
        n = int(torch.randint(1, QL + 1, (1,), generator=g))
        fits = dict(slots=CV >= 3, enters=CV >= 3 and NC >= W + 3, once=CV >= 3 and NC >= 3, shared=CV >= 4 and QL >= 2, pad_target=CV >= 3,
                    zero=CV >= 3, tie=CV >= 4 and QL >= 2, outside=QL >= 2)
        if not fits.get(cls, True):
            cls = "vocab"
        if cls in ("shared", "tie", "outside"):
            n = max(n, 2)
        names.append(cls)
        lens[s] = 0 if cls == "empty" else n
        # background: slot 0, the only slot whose mass is a sum of several positions unless a class says otherwise (two sums that are equal in
        # exact arithmetic would be an unplanted tie whose fp32 bits depend on the order of the terms)
        if cls in ("slots", "zero"):
            m = min(n, CV - 1)
            smap[s, :m] = torch.arange(m) + (1 if cls == "slots" else 0)     # one position per slot; zero: the last slot has none
        smap[s, n:] = torch.tensor([10 ** 9, -5, 2, CV - 1] * QL)[:QL - n]   # garbage behind the length: never read
    for r in range(rows):
        s = r % nsrc
        cls, n = names[s], int(lens[s])
        a = torch.randperm(64, generator=g)[:QL].float() + 1 if QL <= 64 else torch.arange(QL).float() % 61 + 1         # distinct where they can be
        attn[r] = a / 64
        attn[r, n:] = 0.77
        zl[r] = {"vocab": -40.0, "slots": 40.0, "pad_top": -1.0}.get(cls, float(torch.randint(-1, 2, (1,), generator=g)))
        if cls == "enters":
            attn[r, 0] = 1.0 + 1.0 / 128                                     # the mass that lifts the target into the list (no multiple of 1/64)
        if cls == "pad_top":
            o[r, :NC] -= 1.5                                                 # three carriers above 0, the next below: PAD is the row's fourth logit
    # the collapse targets depend on a ROW's ranks but live in the SOURCE row's maps: they are planted from the first beam row of a source row
    for s in range(nsrc):
        cls, n = names[s], int(lens[s])
        by_rank = car[torch.argsort(rank[s])]
        by_rank = by_rank[by_rank != 0]
        if cls == "enters":
            smap[s, 0], e2t[s, 2] = 2, int(by_rank[min(len(by_rank) - 1, W + 1)])
        elif cls == "once":
            smap[s, 0], e2t[s, 2] = 2, int(by_rank[0])
        elif cls == "shared":
            smap[s, 0], smap[s, 1] = 2, 3
            e2t[s, 2] = e2t[s, 3] = int(by_rank[min(len(by_rank) - 1, 2)])
        elif cls == "pad_target":
            smap[s, 0], e2t[s, 2] = 2, 0
        elif cls == "tie":
            smap[s, 0], smap[s, 1] = 3, 2
            for r in range(s, rows, nsrc):
                attn[r, 1] = attn[r, 0]
        elif cls == "outside":
            smap[s, 0], smap[s, 1] = 10 ** 9, -5
    if CV > 4:
        e2t[:, CV - 1] = VT + 5                                              # a target id outside [0, VT): not collapsed
    o[:, K - 1] = zl
    cw = torch.zeros(K)
    cw[K - 1] = 1.0
    return dict(o=o, Wg=Wg, b=b, cw=cw, cb=torch.zeros(1), attn=attn, lens=lens, smap=smap, e2t=e2t, names=names)


def _ref(d, nsrc, W):
    """float64: the whole collapsed distribution of every row -> (ids [rows, W], log P [rows, W]), the planted gaps asserted"""
    o, Wg, b = d["o"].double(), d["Wg"].double(), d["b"].double()
    rows, VT, CV = o.shape[0], Wg.shape[0], d["e2t"].shape[1]
    l = o @ Wg.t() + b
    l[:, 0] = PAD_LOGIT
    zl = o @ d["cw"].double()
    ids, vals = [], []
    for r in range(rows):
        s = r % nsrc
        P = torch.cat([torch.sigmoid(-zl[r]) * torch.softmax(l[r], 0), torch.zeros(CV, dtype=torch.float64)])
        live = torch.ones(VT + CV, dtype=torch.bool)
        z = torch.sigmoid(zl[r])
        for j in range(int(d["lens"][s])):
            c = int(d["smap"][s, j])
            if 0 <= c < CV:
                P[VT + c] += z * float(d["attn"][r, j])
        for c in range(2, CV):
            t = int(d["e2t"][s, c])
            if 0 <= t < VT:
                P[t] += P[VT + c]
                live[VT + c] = False
        lp = torch.log(P).masked_fill(~live, float("nan"))
        order = sorted((e for e in range(VT + CV) if bool(live[e])), key=lambda e: (-float(lp[e]), e))[:W + 1]
        for x, y in zip(order[:W], order[1:]):
            px, py = float(P[x]), float(P[y])
            assert px == py or px - py >= 1e-3 * px, (d["names"][s], r, x, y, px, py)
        ids.append(order[:W])
        vals.append([float(lp[e]) for e in order[:W]])
    return torch.tensor(ids), torch.tensor(vals, dtype=torch.float64)


def _gen_select(d, nsrc, W, fused, bytes_=None, rows=None):
    L = lib.load()
    o, Wg = d["o"], d["Wg"]
    rows = o.shape[0] if rows is None else rows
    K, VT, QL, CV = o.shape[1], Wg.shape[0], d["attn"].shape[1], d["e2t"].shape[1]
    frag = None
    if fused:
        frag, flag = _pack(Wg.to(DEV))
        assert frag is not None and flag == 0
    t = [_dev(d[k]) for k in ("o", "Wg", "b", "cw", "cb", "attn", "lens", "smap", "e2t")]
    e2s = torch.ones(nsrc, CV, dtype=torch.long, device=DEV)
    nb = L.nir_acg_beam_gen_select_workspace_bytes(max(rows, 1), K, VT, W, int(fused))
    ws = torch.empty(max(1, nb if bytes_ is None else bytes_), dtype=torch.uint8, device=DEV)
    tv = torch.full((o.shape[0], W), -7.0, device=DEV)
    ti = torch.full((o.shape[0], W), -7, dtype=torch.int32, device=DEV)
    rc = L.nir_acg_beam_gen_select(lib.ptr(t[0]), rows, nsrc, K, lib.ptr(t[1]), lib.ptr(t[2]), lib.ptr(frag), VT, W, lib.ptr(t[3]), lib.ptr(t[4]),
                                   lib.ptr(t[5]), QL, lib.ptr(t[6]), QL, lib.ptr(t[7]), lib.ptr(t[8]), lib.ptr(e2s), CV, lib.ptr(ws),
                                   ws.numel() if bytes_ is None else bytes_, lib.ptr(tv), lib.ptr(ti), lib.stream())
    torch.cuda.synchronize()
    return rc, tv.cpu(), ti.cpu().long()


@pytest.mark.parametrize("K,VT,rows,CV,QL,W", CONFIGS)
def test_row_lists_against_fp64(K, VT, rows, CV, QL, W):
    seen = set()
    for nsrc in sorted({1, max(1, rows // W)}):
        for seed in range(3 if nsrc == 1 else 1):                            # (one source row holds one class: a few seeds cycle them)
            d = _inputs(K, VT, rows, nsrc, CV, QL, W, 5 * seed + K + VT)
            seen.update(d["names"])
            ids, vals = _ref(d, nsrc, W)
            assert all(len(set(row)) == W for row in ids.tolist())          # a word is offered once
            for fused in ((True, False) if K % 32 == 0 else (False,)):
                rc, tv, ti = _gen_select(d, nsrc, W, fused)
                assert rc == 0
                assert torch.equal(ti, ids), (nsrc, seed, fused, d["names"], (ti != ids).nonzero()[:4])
                fin = torch.isfinite(vals)
                assert torch.equal(torch.isfinite(tv), fin)                  # log 0 is -inf on both sides
                err = (tv.double()[fin] - vals[fin]).abs() / (1 + vals[fin].abs())
                assert float(err.max()) <= 1e-5, float(err.max())
                again = _gen_select(d, nsrc, W, fused)
                assert torch.equal(again[1], tv) and torch.equal(again[2], ti)          # the same bits
    print("acg beam envelope K=%d VT=%d rows=%d CV=%d QL=%d W=%d: classes %s" % (K, VT, rows, CV, QL, W, sorted(seen)))


def test_every_class_is_planted_somewhere():
    seen = set()
    for K, VT, rows, CV, QL, W in CONFIGS:
        for nsrc in sorted({1, max(1, rows // W)}):
            for seed in range(3 if nsrc == 1 else 1):
                seen.update(_inputs(K, VT, rows, nsrc, CV, QL, W, 5 * seed + K + VT)["names"])
    assert seen == set(CLASSES), set(CLASSES) - seen


def _select(tv, ti, B, W, VT, CV, lut, e2s, V, cum, fin):
    L = lib.load()
    t = [_dev(x) for x in (tv, ti.int(), lut, e2s, cum.clone(), fin.int())]
    n = max(B, 2)                                                            # (live buffers for B = 0 too)
    bp = torch.full((n, W), -7, dtype=torch.int32, device=DEV)
    tok = torch.full((n, W), -7, dtype=torch.int32, device=DEV)
    nxt = torch.full((n * W,), -7, dtype=torch.int64, device=DEV)
    rc = L.nir_acg_beam_select(lib.ptr(t[0]), lib.ptr(t[1]), None, B, W, VT, CV, lib.ptr(t[2]), lib.ptr(t[3]), V, lib.ptr(t[4]), lib.ptr(t[5]), lib.ptr(bp),
                               lib.ptr(tok), lib.ptr(nxt), lib.stream())
    torch.cuda.synchronize()
    return rc, t[4].cpu(), t[5].cpu(), bp.cpu(), tok.cpu(), nxt.cpu()


@pytest.mark.parametrize("B,W", [(1, 1), (5, 3), (17, 8)])
def test_select_feeds_slots_back_through_the_source_rows_dictionary(B, W):
    VT, CV, V = 20, 6, 50
    g = torch.Generator().manual_seed(B + W)
    # per decode row k B + b: W distinct extended ids, log P on a grid of 1/8 (sums with cum exact: the order is float64's); EOS and slots among them
    ti = torch.stack([torch.randperm(VT + CV, generator=g)[:W] for _ in range(B * W)])
    ti[0, 0] = VT + CV - 1
    tv = -(torch.stack([torch.randperm(64, generator=g)[:W] for _ in range(B * W)]).float().sort(1).values) / 8
    cum = -(torch.randperm(B * W * 4, generator=g)[:B * W].float().view(B, W)) * 16
    fin = torch.zeros(B, W, dtype=torch.long)
    if W > 1:
        fin[:, 1] = 1
        cum[0, 1] = float("-inf")
    lut = torch.randint(0, V, (VT,), generator=g)
    lut[5] = V + 3                                                           # outside the source vocabulary: <unk>
    e2s = torch.randint(0, V, (B, CV), generator=g)
    e2s[:, CV - 1] = -2                                                      # likewise
    rc, ncum, nfin, bp, tok, nxt = _select(tv, ti, B, W, VT, CV, lut, e2s, V, cum, fin)
    assert rc == 0
    slots = 0
    for b in range(B):
        cand = []
        for k in range(W):
            if fin[b, k]:
                cand.append((float(cum[b, k]), k, 3))
            else:
                cand.extend((float(cum[b, k]) + float(tv[k * B + b, j]), k, int(ti[k * B + b, j])) for j in range(W))
        cand.sort(key=lambda x: (-x[0], x[1], x[2]))
        for j, (sc, k, e) in enumerate(cand[:W]):
            assert (int(bp[b, j]), int(tok[b, j]), int(nfin[b, j])) == (k, e, int(e == 3)), (b, j)
            assert float(ncum[b, j]) == sc
            want = int(lut[e]) if e < VT else int(e2s[b, e - VT])
            assert int(nxt[j * B + b]) == (want if 0 <= want < V else 1)
            slots += e >= VT
    assert slots >= 1


def test_empty_batch_and_bad_arguments_leave_the_outputs_untouched():
    d = _inputs(32, 17, 6, 2, 3, 7, 3, 1)
    for fused in (True, False):
        rc, tv, ti = _gen_select(d, 2, 3, fused, rows=0)                     # B = 0 over live buffers
        assert rc == 0 and bool((tv == -7).all()) and bool((ti == -7).all())
        rc, tv, ti = _gen_select(d, 2, 3, fused, bytes_=16)
        assert rc == BAD_WS and bool((tv == -7).all()) and bool((ti == -7).all())
    for W, nsrc in ((9, 2), (3, 7)):                                         # the width; more source rows than rows
        rc, tv, ti = _gen_select(d, nsrc, W, False)
        assert rc == BAD_ARG and bool((tv == -7).all()) and bool((ti == -7).all())
    L = lib.load()
    p = lib.C.c_void_p(16)
    assert L.nir_acg_beam_gen_select(p, 2, 1, 96, p, p, None, 10, 0, p, p, p, 7, p, 7, p, p, p, 5, p, 1 << 20, p, p, None) == BAD_ARG
    assert L.nir_acg_beam_gen_select(p, 2, 1, 96, p, p, None, 10, 3, p, p, p, 7, p, 7, p, p, p, 1, p, 1 << 20, p, p, None) == BAD_ARG       # CV
    assert L.nir_acg_beam_gen_select(p, 2, 1, 96, p, p, None, 10, 3, p, p, p, 5000, p, 5000, p, p, p, 5, p, 1 << 20, p, p, None) == BAD_ARG # QL
    assert L.nir_acg_beam_gen_select(None, 2, 1, 96, p, p, None, 10, 3, p, p, p, 7, p, 7, p, p, p, 5, p, 1 << 20, p, p, None) == BAD_ARG    # null
    cum, fin = torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.long)
    rc, ncum, nfin, bp, tok, nxt = _select(torch.zeros(6, 3), torch.zeros(6, 3).long(), 0, 3, 20, 6, torch.arange(20), torch.ones(2, 6).long(), 50, cum, fin)
    assert rc == 0 and bool((bp == -7).all()) and bool((tok == -7).all()) and bool((nxt == -7).all())
