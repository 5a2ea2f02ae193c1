"""The acceptance criterion of the DUET document branch (nir_duet_document_branch; csrc/duet_fused.hip: duet_doc_kernel<RT, POOL, PL>,
duet_doc_finish_kernel; csrc/duet.hip: the GEMM-per-layer chain): a float64 reference written from the operation's definition, seeded weight
families, a restatement of the kernel's tiling, the bound a result has to meet, the case list shared by the CPU and the GPU test, and a numpy
emulation of every kernel form with single faults (tests/test_duet_doc_criterion_host.py shows on the CPU that the bound accepts the honest
forms and rejects the faults).

Operation (rankers/duet.py, the document side of the distributed model):  x[m,t] = table[d_ids[m,t]];  c1 = tanh(conv_d1(x)) (k = 3,
[M, DL-2, NF]);  p = max_pool1d(c1, P, stride 1) ([M, PL, NF], PL = DL - 1 - P);  dd = tanh(conv_d2(p)) (1x1);
m1[m,f] = tanh(fc2_b + sum_t fc2_w[t] qv[m // N, f] dd[m,t,f]).  The caller supplies qv [B, NF].

Forms (FORMS) -- which path a case is judged as, and how a case selects it (`sel`):
    f96  fused kernel, plane mode, 96-row tiles            sel planes (documents of >= 98 - P positions)
    p64  fused kernel, plane mode, 64-row tiles            sel planes (short documents; E whose 96-row token tile exceeds 160 KB), sel rows64
    t64  fused kernel, fp32 table, 64-row tiles            sel noplanes (no table planes attached), sel planes with an E whose planes do not fit
    hp   layer chain on pre-split planes                   sel presplit
    ch   layer chain, tunable duet_unfused                 sel unfused
    ex   layer chain, tunable exact_f32                    sel exact
    un   layer chain, fragments attached but bounded = 0   sel unbounded
predicted_form() restates the dispatch predicates of csrc/duet.hip / csrc/duet_fused.hip; tiling() restates duet_doc_tiling, the row -> (document,
position) map, the row weights and the finish kernel's (tile, slot) walk.  The GPU test compares tiles x tile height with the [M=...] suffix of
the duet_doc_kernel launch, so the restatement and the kernel cannot drift apart unnoticed.

Three-document tiles: a flattened tile starts at row t00 <= Tc - 1 of its first document and reaches into a third one when t00 + rows > 2 Tc,
i.e. Tc <= rows - 2 = cap + P - 3; with Tc == cap every tile starts at t00 = 0, so the lengths lie in Tc in [cap + 1, cap + P - 3] (whether a
tile start b cap mod Tc gets there depends on the length; at Tc == cap + 1 tile 1 starts at Tc - 1 and does): DL = 63 / 95 at P = 5, DL = 64 /
96 at P = 4, and none at P <= 3 (P = 3 gets the two thresholds Tc == cap - 1 and Tc == cap instead).  The rows of the third
document lie past the tile's own rows (they are >= Tc + 1 > cap) and only feed pooled rows whose window has left the second document, which
carry weight 0: what such a tile reads there cannot reach m1 (fault 12 below).

Bound: with e = max |got - ref64| over m1 and e32 the same figure for torch's CPU fp32 chain in the reference's order,

    e <= margin[form] * max(e32, 2^-23) + fmt + floor

fmt (split forms; 0 for ex / un) is what the two-term fp16 split costs, derived from the reference: g = gemm_ref.FMT["fp16x2"] = 3 * 2^-22 per
product, one residual per product with independent signs (quadrature, as in mt_head_ref.fmt_term):
    d_z1(m,t,f)  = g sqrt(sum_k (a_k W1[f,k])^2)                            d_c1 = (1 - c1^2) d_z1
    d_p(m,t,f)   = max over the pooling window of d_c1                       (max is 1-Lipschitz in the sup norm)
    d_z2(m,t,f)  = sqrt(sum_j (W2[f,j] d_p_j)^2 + g^2 sum_j (W2[f,j] p_j)^2)  d_dd = (1 - dd^2) d_z2
    d_m1(m,f)    = (1 - m1^2) |qv| sqrt(sum_t (fc2_w[t] d_dd)^2),            fmt = max over (m, f).
floor covers the tanh on v_exp_f32 / v_rcp_f32 (1 - 2 rcp(1 + exp2(z)): one ulp each on a quantity of at most 2, DELTA = 2^-22 absolute per
tanh output), through the same derivatives, the per-output errors of the inner layers in quadrature and the last tanh's own DELTA added:
    floor = max (1 - m1^2) |qv| sqrt(sum_t fc2_w[t]^2 DELTA^2 (1 + (1 - dd^2)^2 sum_j W2[f,j]^2)) + DELTA,
the sum over j leaving out filters that are dead in the reference (pre-activation 0 everywhere: both tanh forms give exactly 0 there).
margin: never fixed in advance and never above MARGIN_CAP = 4.  MEASURED holds, per form, the largest r = e / max(e32, 2^-23) and the largest
ratio = (e - fmt - floor) / max(e32, 2^-23) over CASES on the MI355X (profiles/duet_doc_criterion_mi355x.log has the per-case lines).  r is
1.7 on the chain forms, 2.6 on the pre-split chain and 4.3 / 4.4 / 5.9 on the fused forms p64 / t64 / f96 (`trained`, E = NF = 4 at 96 rows: e32
is below 2^-23 there and e = 7.0e-7 is the split's own cost, which fmt prices at 1.8e-6): r alone would ask the fused forms for more than the cap, and the
cap holds -- what the criterion needs from the margin is ratio, which is negative on every split form and 0.135 at most (ex / un, E = NF = 300).
MARGIN is ratio doubled and rounded up to a power of two, at least 1: 1 on every form.

Weight families: model (detinit scale), trained (conv pre-activations reach |z| of 2 - 3), negative (conv_d1 bias strongly negative: every
pooled value below 0), seam (O(1) fc2_w with its largest entries on the first and last pooled row and on both sides of every tile seam,
distinctive table rows under those positions), large (table and conv weights just under 2^15 where the other operand is small; large_over is
the companion just over it, which must not be `bounded`)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import gemm_ref as G

EPS = 2.0 ** -23
MARGIN_CAP = 4.0
G16 = G.FMT["fp16x2"]
DELTA = 2.0 ** -22
FORMS = ("f96", "p64", "t64", "hp", "ch", "ex", "un")
FUSED = ("f96", "p64", "t64")
PLANE = ("f96", "p64")
SPLIT = FUSED + ("hp", "ch")
FAMILIES = ("model", "trained", "negative", "seam", "large")
FAULTS = tuple(range(1, 18))
# form -> (largest e / max(e32, 2^-23), largest (e - fmt - floor) / max(e32, 2^-23)) over CASES on the MI355X
MEASURED = {"f96": (5.855, -1.574), "p64": (4.328, -2.093), "t64": (4.397, -2.068), "hp": (2.607, -4.758), "ch": (1.692, -4.401), "ex": (1.692, 0.135),
            "un": (1.692, 0.135)}
MARGIN = {"f96": 1.0, "p64": 1.0, "t64": 1.0, "hp": 1.0, "ch": 1.0, "ex": 1.0, "un": 1.0}
PAD = 0
NFP = 320
HEAVY = 1.0                      # |fc2_w[t]| of a heavy row (seam family: 1.5)
HEAVY_SHARE = 0.25               # ... and max_f |fc2_w[t] dd[m,t,f]| it has to reach in the reference
LDS_LIMIT = 160 * 1024


# ------------------------------------------------------------------ kernel geometry (csrc/duet_fused.hip, csrc/duet.hip)
def ept(E):
    return (E + 63) // 64 * 64


def pl_lds(rows, C):
    """duet_pl_lds<rows / 16>(C): the token tile (C column chunks) or the P planes that take its place, + ids, fc2 weights and flags"""
    RP = rows + 6
    NI = (8 * RP + 63) // 64
    KG = rows * 8 + 32
    return max(C * NI * 1024, 2 * 10 * 4 * KG * 2) + 1536


def planes_fit(EPT):
    return EPT > 0 and EPT % 64 == 0 and EPT // 32 <= 32 and pl_lds(64, EPT // 32) <= LDS_LIMIT


def tile_rows(planes, DL, P, EPT, rows64=False):
    return 96 if planes and not rows64 and DL - 2 >= 96 - (P - 1) and pl_lds(96, EPT // 32) <= LDS_LIMIT else 64


def predicted_form(d):
    """(form, tile height or None) the dispatch gives case d"""
    sel, E, NF, P, DL = d["sel"], d["E"], d["NF"], d["P"], d["DL"]
    if sel in ("presplit", "unfused", "exact", "unbounded"):
        return {"presplit": "hp", "unfused": "ch", "exact": "ex", "unbounded": "un"}[sel], None
    assert NF <= NFP and NF % 4 == 0 and 1 <= P <= 5 and E % 4 == 0 and E >= 4 and DL >= P + 2      # duet_doc_usable
    planes = sel in ("planes", "rows64") and planes_fit(ept(E))
    rows = tile_rows(planes, DL, P, ept(E), sel == "rows64")
    return ("t64" if not planes else ("f96" if rows == 96 else "p64")), rows


def tiling(M, DL, P, rows):
    """duet_doc_tiling + the kernel's row map: dict(Tc, PL, cap, flat, ntile, TPv, own, n, tiles, finish).  tiles[b] = dict(doc0, t00, doc [rows],
    t [rows] (the conv row each tile row computes, clamps included), slot [rows], tw [rows] (the position the row weight is looked up at),
    ok [rows] (an own pooled row whose window stays inside its document), touches (the documents its rows lie in)).  finish[pair] = the
    (tile, slot) partials duet_doc_finish_kernel adds, in its order."""
    Tc, PL, cap = DL - 2, DL - 1 - P, rows - (P - 1)
    flat = Tc >= cap
    ntile = (PL + cap - 1) // cap
    TPv = (PL + ntile - 1) // ntile
    n = (M * Tc + cap - 1) // cap if flat else M * ntile
    own = cap if flat else TPv
    pr = np.arange(rows)
    tiles = []
    for b in range(n):
        if flat:
            doc0, t00 = divmod(b * cap, Tc)
        else:
            doc0, t00 = b // ntile, (b % ntile) * TPv
        t, dd = t00 + pr, np.zeros(rows, dtype=np.int64)
        if flat:
            for k in (1, 2):
                over = t >= Tc
                t, dd = np.where(over, t - Tc, t), np.where(over, k, dd)
            touches = sorted(set((doc0 + dd)[doc0 + dd < M].tolist()))
            past = doc0 + dd >= M
            dd, t = np.where(past, M - 1 - doc0, dd), np.where(past, Tc - 1, t)
        else:
            t = np.minimum(t, Tc - 1)
            touches = [doc0]
        slot = (t00 + pr >= Tc).astype(np.int64) if flat else np.zeros(rows, dtype=np.int64)
        tw = t00 + pr - Tc * slot
        ok = (pr < own) & (tw < PL) & (doc0 + slot < M)
        tiles.append(dict(doc0=doc0, t00=t00, doc=doc0 + dd, t=t, slot=slot, tw=tw, ok=ok, touches=touches))
    finish = []
    for pair in range(M):
        if flat:
            ta, tb = pair * Tc // cap, (pair * Tc + PL - 1) // cap
            finish.append([(b, pair - b * cap // Tc) for b in range(ta, tb + 1)])
        else:
            finish.append([(pair * ntile + b, 0) for b in range(ntile)])
    return dict(Tc=Tc, PL=PL, cap=cap, flat=flat, ntile=ntile, TPv=TPv, own=own, n=n, tiles=tiles, finish=finish, rows=rows)


def case_tiling(d):
    return tiling(d["B"] * d["N"], d["DL"], d["P"], d["rows"]) if d["rows"] else None


def owners(tl, M):
    """(doc, t) -> list of the (tile, slot) whose weights count pooled row t of document doc"""
    out = {}
    for b, T in enumerate(tl["tiles"]):
        for r in np.nonzero(T["ok"])[0]:
            out.setdefault((int(T["doc0"] + T["slot"][r]), int(T["tw"][r])), []).append((b, int(T["slot"][r])))
    return out


def seam_rows(d):
    """the pooled positions t the seam family makes heavy: first and last pooled row, and the first and last own row of every (tile, slot)"""
    M, PL = d["B"] * d["N"], d["DL"] - 1 - d["P"]
    heavy = {0, PL - 1}
    tl = case_tiling(d) or tiling(M, d["DL"], d["P"], 64)            # chain forms: the 64-row tiling's seams, so that the families agree
    by = {}
    for (doc, t), own in owners(tl, M).items():
        by.setdefault(own[0], []).append(t)
    for ts in by.values():
        heavy |= {min(ts), max(ts)}
    return sorted(heavy)


# ------------------------------------------------------------------ cases
def c(form, fam, B, N, DL, E=20, NF=20, P=5, sel=None, rows=None, tiles=None, V=211, seed=0):
    """One case: the form it is judged as, how it selects it, and for the fused forms the tile height and tile count it is expected to run at"""
    sel = sel or {"f96": "planes", "p64": "planes", "t64": "noplanes", "hp": "presplit", "ch": "unfused", "ex": "exact", "un": "unbounded"}[form]
    d = dict(form=form, fam=fam, B=B, N=N, DL=DL, E=E, NF=NF, P=P, sel=sel, rows=rows, tiles=tiles, V=V, seed=seed)
    d["id"] = "%s-%s-%s-B%dN%d-D%d-E%d-F%d-P%d" % (form, sel, fam, B, N, DL, E, NF, P) + ("-s%d" % seed if seed else "")
    return d


def _cases():
    out = []
    # ---- document length at P = 5 (E = NF = 20): thresholds of the tilings, three-document tiles, the tail tile
    for DL, tiles in ((7, 3), (61, 3), (62, 3), (63, 4), (64, 4), (93, 5)):
        out.append(c("p64", "seam", 1, 3, DL, rows=64, tiles=tiles))
    for DL, tiles in ((7, 3), (62, 3), (63, 4), (64, 4)):
        out.append(c("t64", "seam", 1, 3, DL, rows=64, tiles=tiles))
    for DL, tiles in ((94, 3), (95, 4), (97, 4), (200, 7)):
        out.append(c("f96", "seam", 1, 3, DL, rows=96, tiles=tiles))
    out += [c("f96", "seam", 1, 1, 95, rows=96, tiles=2), c("f96", "trained", 1, 1, 95, rows=96, tiles=2), c("p64", "seam", 1, 1, 63, rows=64, tiles=2)]
    for fam in ("seam", "negative", "trained"):                        # B = 2, N = 3: pair // N differs from pair % B; three-document tiles
        out += [c("p64", fam, 2, 3, 63, rows=64, tiles=7), c("t64", fam, 2, 3, 63, rows=64, tiles=7), c("f96", fam, 2, 3, 95, rows=96, tiles=7)]
    out += [c("p64", "seam", 2, 3, 95, sel="rows64", rows=64, tiles=10), c("p64", "negative", 1, 3, 7, rows=64, tiles=3), c("t64", "negative", 1, 3, 7, rows=64, tiles=3)]
    # ---- pool window 1 .. 4 (the run-time-window instantiation): per-document and flattened; three-document lengths at P = 4, thresholds at P = 3
    for P, lens in ((1, ((20, 3), (70, 4))), (2, ((30, 3), (80, 4))), (3, ((25, 3), (63, 3), (64, 3), (65, 4))), (4, ((30, 3), (64, 4)))):
        for DL, tiles in lens:
            out += [c("p64", "seam", 1, 3, DL, P=P, rows=64, tiles=tiles), c("t64", "seam", 1, 3, DL, P=P, rows=64, tiles=tiles)]
    out += [c("f96", "seam", 1, 3, 100, P=1, rows=96, tiles=4), c("f96", "seam", 1, 3, 100, P=2, rows=96, tiles=4), c("f96", "seam", 1, 3, 96, P=3, rows=96, tiles=3),
            c("f96", "seam", 1, 3, 97, P=3, rows=96, tiles=4), c("f96", "seam", 2, 3, 96, P=4, rows=96, tiles=7), c("p64", "negative", 2, 3, 64, P=4, rows=64, tiles=7)]
    # ---- widths
    for E, NF in ((4, 4), (52, 60), (20, 300), (300, 320)):
        out += [c("p64", "trained", 1, 3, 40, E, NF, rows=64, tiles=3), c("t64", "trained", 1, 3, 40, E, NF, rows=64, tiles=3), c("f96", "trained", 1, 3, 100, E, NF, rows=96, tiles=4)]
    out += [c("p64", "trained", 1, 3, 100, 448, 20, rows=64, tiles=5), c("t64", "trained", 1, 3, 40, 640, 20, sel="planes", rows=64, tiles=3)]
    # ---- the reference's 300 / 300 / 5 once per fused form, and the families on every form
    out += [c("f96", "model", 1, 3, 100, 300, 300, rows=96, tiles=4), c("p64", "model", 1, 3, 40, 300, 300, rows=64, tiles=3), c("t64", "model", 1, 3, 40, 300, 300, rows=64, tiles=3)]
    for form in ("hp", "ch", "ex", "un"):
        out += [c(form, fam, 2, 3, 40) for fam in ("model", "trained", "negative", "seam")] + [c(form, "trained", 1, 3, 30, 300, 300)]
    out += [c("ch", "trained", 1, 3, 40, 52, 60), c("ex", "trained", 1, 3, 40, 52, 60), c("ch", "trained", 1, 3, 20, P=1), c("ch", "trained", 1, 3, 20, P=8, NF=24, E=24)]
    out += [c("p64", "large", 2, 3, 40, rows=64, tiles=6), c("t64", "large", 2, 3, 40, rows=64, tiles=6), c("f96", "large", 1, 3, 100, rows=96, tiles=4), c("ch", "large", 2, 3, 40),
            c("hp", "large", 2, 3, 40)]
    return out


CASES = _cases()
BY_ID = {d["id"]: d for d in CASES}
assert len(BY_ID) == len(CASES)


# ------------------------------------------------------------------ inputs
def family(d):
    """dict of float32 / int64 CPU tensors: table [V,E], d_ids [M,DL], w1 [NF,3,E] (conv_d1 as the pack holds it), b1, w2 [NF,NF], b2, fc2w [PL],
    fc2b [1], qv [B,NF]"""
    fam, B, N, DL, E, NF, P, V = (d[k] for k in ("fam", "B", "N", "DL", "E", "NF", "P", "V"))
    M, PL = B * N, DL - 1 - P
    g = torch.Generator().manual_seed(1000 * DL + 7 * E + 3 * NF + P + 17 * len(fam) + 131 * d["seed"] + M)
    uni = lambda a, *s: (torch.rand(*s, generator=g, dtype=torch.float64) * 2 - 1) * a
    table = uni(0.5, V, E)
    table[PAD] = 0.0
    w1, b1 = uni(2.0 / (3 * E) ** 0.5, NF, 3, E), uni(0.3, NF)
    w2, b2 = uni(2.0 / NF ** 0.5, NF, NF), uni(0.3, NF)
    fc2w, fc2b, qv = uni(2.0 / PL ** 0.5, PL), uni(0.3, 1), uni(1.0, B, NF)
    ids = torch.randint(1, V, (M, DL), generator=g)
    ids[0, DL // 2], ids[0, 0], ids[M - 1, DL - 1] = PAD, V - 1, V - 1           # PAD and the last table row, the latter at both ends of the id array
    if M >= 3 and fam != "seam":
        ids[1] = int(ids[1, 0])                                          # a document of one repeated token: every pooling window is a tie
    if fam in ("trained", "seam"):
        w1, w2, fc2w = w1 * 5.0, w2 * 2.0, fc2w * 2.0
    elif fam == "negative":
        b1 = -2.0 - b1.abs()
    if fam == "seam":
        # heavy fc2 weights on the rows next to every seam; the tokens under those rows come from eight table rows of full-scale entries
        special = torch.arange(V - 9, V - 1)
        table[special] = torch.where(uni(1.0, 8, E) >= 0, 1.0, -1.0).double()
        for n_, t in enumerate(seam_rows(d)):
            fc2w[t] = 1.5 * (1 if n_ % 2 == 0 else -1)
            for m in range(M):
                ids[m, t + (P + 1) // 2] = special[(n_ + 3 * m) % 8]
        taken = {0, DL - 1} | {t + (P + 1) // 2 for t in seam_rows(d)}
        ids[0, min(j for j in range(DL) if j not in taken)] = PAD
    elif fam in ("large", "large_over"):
        # the 2^15 range of the split on both operands of conv_d1 and on conv_d2, with the other operand of every such product small but inside
        # the format's fp32-class range (|x| >= 2^-13, csrc/split2.hpp): table column 0 is small everywhere and filter 1 has its large weights
        # there; four table rows are large in column 1, where every filter's weights are small; filter 0 is dead (c1 = p = 0 exactly), so the
        # large column 0 of conv_d2 multiplies zeros -- a term that overflowed to inf would turn them into NaN
        top = (0.97 if fam == "large" else 1.01) * 32768.0
        small = lambda *s: torch.where(uni(1.0, *s) >= 0, 1.0, -1.0).double() * (2.0 ** -13 + torch.rand(*s, generator=g, dtype=torch.float64) * 2.0 ** -13)
        table[1:, 0], w1[:, :, 1] = small(V - 1), small(NF, 3)
        w1[1, :, 0] = uni(top, 3)
        table[V - 5:V - 1, 1] = uni(top, 4)
        table[V - 2, 1], w1[1, 1, 0] = top, -top
        w1[0], b1[0] = 0.0, 0.0
        w2[:, 0] = uni(top, NF)
        w2[2, 0] = top
    elif fam not in ("model", "trained", "negative"):
        raise ValueError(fam)
    x = dict(table=table, w1=w1, b1=b1, w2=w2, b2=b2, fc2w=fc2w, fc2b=fc2b, qv=qv)
    x = {k: v.float().contiguous() for k, v in x.items()}
    x["d_ids"] = ids.contiguous()
    return x


def bounded(x):
    """`bounded` as rankers.duet.split_bounded decides it for the document side's operands"""
    from context_attentive_ir_amd.rankers.duet import split_bounded
    return split_bounded(x["table"], x["w1"], x["w2"])


# ------------------------------------------------------------------ reference
def _chain(x, dt, N, P):
    """dict(z1 [M,Tc,NF] pre-activations, c1, p [M,PL,NF], dd, m1 [M,NF]) in dtype dt, in the reference's order"""
    t = lambda k: x[k].to(dt)
    emb = F.embedding(x["d_ids"], t("table"))                                         # [M, DL, E]
    z1 = F.conv1d(emb.transpose(1, 2), t("w1").permute(0, 2, 1).contiguous(), t("b1"))   # [M, NF, Tc]
    c1 = torch.tanh(z1)
    p = F.max_pool1d(c1, P, 1)
    dd = torch.tanh(F.conv1d(p, t("w2").unsqueeze(2), t("b2")))                       # [M, NF, PL]
    had = t("qv").repeat_interleave(N, 0).unsqueeze(2) * dd
    m1 = torch.tanh(F.linear(had, t("fc2w").unsqueeze(0), t("fc2b")).squeeze(2))
    return dict(z1=z1.transpose(1, 2), c1=c1.transpose(1, 2), p=p.transpose(1, 2), dd=dd.transpose(1, 2), m1=m1)


def ref64(x, N, P):
    return _chain(x, torch.float64, N, P)["m1"]


def reference(d, x):
    """dict(ref [M, NF] float64, z1, c1, p, dd, e32) of inputs x under the shape of case d"""
    r = _chain(x, torch.float64, d["N"], d["P"])
    r["ref"] = r["m1"]
    r["e32"] = float((_chain(x, torch.float32, d["N"], d["P"])["m1"].double() - r["m1"]).abs().max())
    return r


@functools.lru_cache(maxsize=None)
def _prepared(cid):
    x = family(BY_ID[cid])
    return x, reference(BY_ID[cid], x)


def prepared(d):
    """(inputs, dict(ref, z1, c1, p, dd, e32)) of a case of CASES, computed once and shared by every test that needs it; treat as read-only"""
    return _prepared(d["id"])


def coverage(d, p):
    """what the seam case d does NOT cover, from the tiling restatement and the float64 reference alone: every (tile, slot) that owns pooled rows
    has a heavy first and last own row (so both sides of every tile seam and of every document boundary inside a tile are heavy), both slots
    occur in a flattened tiling, a tile that touches three documents and the last tile of the grid carry a heavy row wherever they own rows,
    and every heavy row reaches HEAVY_SHARE in the reference"""
    M = d["B"] * d["N"]
    tl = case_tiling(d) or tiling(M, d["DL"], d["P"], 64)
    fc2w, dd = p_np(family_cached(d)["fc2w"]), p["dd"].numpy()
    heavy = lambda doc, t: abs(fc2w[t]) >= HEAVY and float(np.abs(fc2w[t] * dd[doc, t]).max()) >= HEAVY_SHARE
    by = {}
    for (doc, t), own in owners(tl, M).items():
        by.setdefault(own[0], []).append((doc, t))
    miss = []
    for key, rows in sorted(by.items()):
        first, last = min(rows), max(rows)
        miss += ["%s first" % (key,)] * (not heavy(*first)) + ["%s last" % (key,)] * (not heavy(*last))
    if tl["flat"] and M > 1 and tl["Tc"] % tl["cap"] and {s for _, s in by} != {0, 1}:       # (Tc == cap: every tile is one document)
        miss.append("slots")
    for b, T in enumerate(tl["tiles"]):
        if (len(T["touches"]) == 3 or b == tl["n"] - 1) and T["ok"].any() and not any(heavy(*dt) for k, v in by.items() if k[0] == b for dt in v):
            miss.append("tile %d" % b)
    return miss


def family_cached(d):
    return prepared(d)[0]


def p_np(t):
    return t.double().numpy()


# ------------------------------------------------------------------ emulation
def _split(a):
    return tuple(t.astype(np.float64) for t in G.split_terms(np.asarray(a, dtype=np.float32), "fp16x2"))


def _f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def _gemm(A, W, blocks, split, cross=True):
    """A W^T with the kernels' fp32 accumulators.  split: the operands as two fp16 terms each, per k-block three products -- h2' h1 and h1 h2' into
    the cross accumulator, h1 h1 into the leading one, h2' h2' dropped (cross = False: the cross accumulator dropped too) -- each MFMA's products
    summed exactly and its addition to the accumulator rounded to fp32, the result acc + 2^-11 acx rounded once.  not split: exact fp32 products."""
    R, Nn = A.shape[0], W.shape[0]
    acc = np.zeros((R, Nn))
    if not split:
        for ks in blocks:
            acc = _f32(acc + A[:, ks] @ W[:, ks].T)
        return acc
    (a1, a2), (w1, w2) = _split(A), _split(W)
    acx = np.zeros((R, Nn))
    for ks in blocks:
        if cross:
            acx = _f32(acx + a2[:, ks] @ w1[:, ks].T)
            acx = _f32(acx + a1[:, ks] @ w2[:, ks].T)
        acc = _f32(acc + a1[:, ks] @ w1[:, ks].T)
    return _f32(acc + acx / 2048.0)


def k_blocks(form, E, drop_tail=False):
    """the k-blocks of conv_d1 in the form's order, as index arrays into the tap-major row (k = tap * E + e).  Plane mode: 32 elements of one tap
    per block, chunk by chunk; fp32 table / ch: 32 consecutive k; hp: 32 consecutive k of the row padded to EP per tap; ex / un: the fp32 MFMA's 4.
    drop_tail (fault 3): what lies past the last whole multiple of 32 (per tap in plane mode) is left out."""
    K = 3 * E
    whole = K // 32 * 32
    if form in PLANE:
        out = [np.arange(u * E + 32 * cc, u * E + min(32 * cc + 32, E)) for cc in range(ept(E) // 32) for u in range(3) if 32 * cc < E]
        return [b for b in out if len(b) == 32] if drop_tail else out
    if form == "hp":
        EP = (E + 7) // 8 * 8
        out = []
        for s in range(0, 3 * EP, 32):
            idx = np.arange(s, min(s + 32, 3 * EP))
            out.append((idx // EP * E + idx % EP)[idx % EP < E])
    else:
        step = 32 if form in SPLIT else 4
        out = [np.arange(s, min(s + step, K)) for s in range(0, K, step)]
    if drop_tail:
        out = [b[b < whole] for b in out]
    return [b for b in out if len(b)]


def _rows_of(x, doc, t, shift=0):
    """the conv_d1 operand rows [len, 3E] of conv rows (doc, t): tokens t, t+1, t+2 of the document (shift: of the flattened id array)"""
    ids, DL = x["d_ids"].numpy(), x["d_ids"].shape[1]
    tab = p_np(x["table"])
    flat = ids.reshape(-1)
    pos = np.clip(doc[:, None] * DL + t[:, None] + np.arange(3)[None] + shift, 0, flat.size - 1)
    return tab[flat[pos]].reshape(len(doc), -1)


def emulate(d, x, fault=None):
    """m1 [M, NF] float64 as the kernel form of case d computes it: the two-term fp16 split with three products per k-block (split forms), fp32
    accumulators in the form's k order, each layer's output rounded to fp32 where the kernels hold it, tanh in float64 (what v_exp / v_rcp add is
    the floor's business); fused forms tile by tile with the kernel's row map, in-tile pooling, row weights, per-tile per-slot fc2 partials summed
    over the four row groups as the kernel does and over the tiles in the finish kernel's order; chain forms layer by layer.  fault: one of
     1  the cross term dropped in GEMM 1                      10  slot-1 partials added to the tile's first document (flattened tilings)
     2  the same in GEMM 2                                    11  the last tile of the grid dropped
     3  the k tail past the last multiple of 32 dropped       12  a third document's token rows read at the second document's offset (plane mode)
     4  taps shifted by one                                   13  fc2_w indexed off by one
     5  pool window P - 1                                     14  the qv row taken as pair % B
     6  the pool's halo rows read as 0 (fused: the tile's rows  15  b1 and b2 swapped
        past its own; chain: past the run of 8 outputs)       16  fc2_b omitted
     7  a row whose window leaves its document keeps a weight  17  the column mask a clamp: columns NF..319 take b2[NF-1] and their fc2 sums land
     8  the last own row of each tile dropped                     on column NF-1 (fused forms)
     9  the first own row of each tile counted twice"""
    form, B, N, DL, E, NF, P = (d[k] for k in ("form", "B", "N", "DL", "E", "NF", "P"))
    M, Tc, PL = B * N, DL - 2, DL - 1 - P
    split = form in SPLIT
    W1, W2 = p_np(x["w1"]).reshape(NF, 3 * E), p_np(x["w2"])
    b1, b2 = (p_np(x["b2"]), p_np(x["b1"])) if fault == 15 else (p_np(x["b1"]), p_np(x["b2"]))
    fc2w, fc2b, qv = p_np(x["fc2w"]), (0.0 if fault == 16 else float(x["fc2b"])), p_np(x["qv"])
    blocks1 = k_blocks(form, E, fault == 3)
    blocks2 = [np.arange(s, min(s + (32 if split else 4), NF)) for s in range(0, NF, 32 if split else 4)]
    conv1 = lambda A: _f32(np.tanh(_f32(_gemm(A, W1, blocks1, split, fault != 1) + b1)))
    conv2 = lambda Pm: _f32(np.tanh(_f32(_gemm(Pm, W2, blocks2, split, fault != 2) + b2)))
    docs, ts = np.repeat(np.arange(M), Tc), np.tile(np.arange(Tc), M)
    if fault == 4:
        ids, tab = x["d_ids"].numpy(), p_np(x["table"])
        A = tab[ids[docs[:, None], np.minimum(ts[:, None] + np.arange(3)[None] + 1, DL - 1)]].reshape(M * Tc, -1)
    else:
        A = _rows_of(x, docs, ts)
    c1 = conv1(A).reshape(M, Tc, NF)
    Pw = P - 1 if fault == 5 else P
    qrow = lambda pair: pair % B if fault == 14 else pair // N
    w_at = lambda t: fc2w[np.minimum(t + 1, PL - 1)] if fault == 13 else fc2w[np.minimum(t, PL - 1)]
    finish = lambda s, pair: _f32(np.tanh(_f32(fc2b + qv[qrow(pair)] * s)))
    out = np.zeros((M, NF))
    if form not in FUSED:
        p = np.full((M, PL, NF), -np.inf)
        tt = np.arange(PL)
        for q in range(Pw):
            v = c1[:, tt + q]
            if fault == 6:
                v = np.where(((tt % 8) + q >= 8)[None, :, None], 0.0, v)
            p = np.maximum(p, v)
        dd = conv2(p.reshape(M * PL, NF)).reshape(M, PL, NF)
        for pair in range(M):
            had = _f32(qv[qrow(pair)][None] * dd[pair])
            out[pair] = _f32(np.tanh(_f32(_f32((w_at(tt)[:, None] * had).sum(0)) + fc2b)))
        return torch.from_numpy(out)
    tl = case_tiling(d)
    rows, own = tl["rows"], tl["own"]
    partial = np.zeros((tl["n"], 2, NF))
    for b, T in enumerate(tl["tiles"]):
        v = c1[T["doc"], T["t"]].copy()
        if fault == 12 and form in PLANE and len(T["touches"]) == 3:
            third = np.nonzero(T["doc"] == T["doc0"] + 2)[0]
            v[third] = conv1(_rows_of(x, T["doc"][third], T["t"][third], shift=-2))
        if fault == 6:
            v[own:] = 0.0
        pr = np.arange(rows)
        pm = v.copy()
        for q in range(1, Pw):
            pm = np.maximum(pm, v[np.minimum(pr + q, rows - 1)])
        d2 = conv2(pm)
        ok = T["ok"] if fault != 7 else (pr < own) & (T["tw"] < Tc) & (T["doc0"] + T["slot"] < M)
        wr = np.where(ok, w_at(T["tw"]), 0.0)
        if fault == 8:
            wr[own - 1] = 0.0
        if fault == 9:
            wr[0] *= 2.0
        for s in (0, 1):
            ws = np.where(T["slot"] == s, wr, 0.0)
            grp = np.zeros((4, NF))
            for r in range(rows):
                g_ = (r % 16) // 4
                grp[g_] = _f32(grp[g_] + ws[r] * d2[r])
            partial[b, s] = _f32(_f32(grp[0] + grp[1]) + _f32(grp[2] + grp[3]))
            if fault == 17 and NF < NFP:
                partial[b, s, NF - 1] = _f32(partial[b, s, NF - 1] + (NFP - NF) * float(ws.sum()) * np.tanh(b2[NF - 1]))
        if fault == 10 and tl["flat"]:
            partial[b, 0], partial[b, 1] = _f32(partial[b, 0] + partial[b, 1]), 0.0
    if fault == 11:
        partial[-1] = 0.0
    for pair in range(M):
        s = np.zeros(NF)
        for b, slot in tl["finish"][pair]:
            if b < tl["n"]:
                s = _f32(s + partial[b, slot])
        out[pair] = finish(s, pair)
    return torch.from_numpy(out)


# ------------------------------------------------------------------ criterion
def _tail(d, x, p):
    """(1 - m1^2) |qv| per (pair, f), and fc2_w^2"""
    m1, qv = p["ref"].numpy(), np.repeat(p_np(x["qv"]), d["N"], 0)
    return (1.0 - m1 ** 2) * np.abs(qv), p_np(x["fc2w"]) ** 2


def fmt_term(d, x, p):
    """the format term of the module docstring (absolute)"""
    if d["form"] not in SPLIT:
        return 0.0
    M, Tc, PL, NF, P = d["B"] * d["N"], d["DL"] - 2, d["DL"] - 1 - d["P"], d["NF"], d["P"]
    W1sq, W2sq = p_np(x["w1"]).reshape(NF, -1) ** 2, p_np(x["w2"]) ** 2
    A = _rows_of(x, np.repeat(np.arange(M), Tc), np.tile(np.arange(Tc), M))
    c1, pp, dd = p["c1"].numpy(), p["p"].numpy(), p["dd"].numpy()
    dc = (1.0 - c1 ** 2) * G16 * np.sqrt((A ** 2) @ W1sq.T).reshape(M, Tc, NF)
    dp = np.max(np.stack([dc[:, q:q + PL] for q in range(P)]), 0)
    dz2 = np.sqrt((dp ** 2) @ W2sq.T + G16 ** 2 * (pp ** 2) @ W2sq.T)
    ddd = (1.0 - dd ** 2) * dz2
    lead, f2 = _tail(d, x, p)
    return float((lead * np.sqrt(np.einsum("t,mtf->mf", f2, ddd ** 2))).max())


def floor_term(d, x, p):
    """the tanh floor of the module docstring (absolute)"""
    dd = p["dd"].numpy()
    live = np.abs(p["c1"].numpy()).max((0, 1)) > 0.0          # a dead filter (z = 0 everywhere) gives tanh(0) = 0 exactly: exp2(0) = 1, rcp(2) = 0.5
    inner = DELTA ** 2 * (1.0 + (1.0 - dd ** 2) ** 2 * ((p_np(x["w2"]) ** 2) * live[None, :]).sum(1)[None, None, :])
    lead, f2 = _tail(d, x, p)
    return float((lead * np.sqrt(np.einsum("t,mtf->mf", f2, inner))).max()) + DELTA


def measure(got, d, x, p):
    """dict(e, e32, fmt, floor, r, ratio) of m1 `got` [M, NF] against the prepared reference p of case d: r = e / max(e32, 2^-23),
    ratio = (e - fmt - floor) / max(e32, 2^-23)"""
    got = torch.as_tensor(np.asarray(got)) if not torch.is_tensor(got) else got.detach().cpu()
    ref = p["ref"]
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "non-finite m1"
    if "fmt" not in p:
        p["fmt"], p["floor"] = fmt_term(d, x, p), floor_term(d, x, p)
    e = float((got.double() - ref).abs().max())
    den = max(p["e32"], EPS)
    return dict(e=e, e32=p["e32"], fmt=p["fmt"], floor=p["floor"], r=e / den, ratio=(e - p["fmt"] - p["floor"]) / den)


def accept(got, d, x, p, margin=None):
    """(ok, figures): the criterion of the module docstring.  margin defaults to MARGIN[form] and may never exceed MARGIN_CAP."""
    margin = MARGIN[d["form"]] if margin is None else margin
    assert margin <= MARGIN_CAP
    r = measure(got, d, x, p)
    r["bound"] = margin * max(r["e32"], EPS) + r["fmt"] + r["floor"]
    return r["e"] <= r["bound"], r
