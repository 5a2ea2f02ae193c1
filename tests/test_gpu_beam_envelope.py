"""GPU (-m gpu): the kernels of the beam search at the C ABI (csrc/beam.hip) on exactly representable inputs.

nir_beam_gen_topk against float64 with planted winners: decode row r is a one-hot vector selecting column c(r) of an integer weight matrix, the
bias holds multiples of 1/8, so every logit is exact in fp32 and in the split-fp16 product and the top-W set, its order and its ties are exact;
lse is compared with the project's bound (n_split = 1 fused, 0 plain).  The plants, by column: all winners inside one 16-row tile (the first
four in one lane's four slots); winners straddling v = 15 / 16 and the last, partial tile; winners spread over the vocabulary (different
waves and workgroup ranges); exact ties inside a tile and across ranges (the smaller index first); a bias-decided row; small random integers
(ties everywhere).  VT = 8 with W = 8 is VT = W.
nir_beam_select directly: step 0, a row with all beams finished, a mix of finished and live beams, ties between a frozen candidate and a live
one in both flat-index orders.  nir_beam_reorder on the reference's recorded shuffle (tests/golden/beam_state.npz), the fp16 term-pair state
against gather-then-pack."""
import pytest
import torch

import beam_ref as R
from conftest import T, load_golden
from context_attentive_ir_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
NEG = float("-inf")


def _bias(VT):
    return ((torch.arange(VT) * 7) % 13).float() / 8


def _positions(p, VT, W):
    """2 W candidate positions of plant p, distinct, inside [0, VT) (padded from the front of the vocabulary)"""
    t0 = (VT // 16 // 2) * 16
    want = {0: [t0 + j for j in range(2 * W)],
            1: [15, 16, VT - 1, VT - 2, 14, 17, VT - 3, 31, 32, VT - 4, 13, 18, 47, 48, 12, 19],
            2: [(j * VT) // (2 * W) + (j % 3) for j in range(2 * W)],
            3: [5, 6, 9, VT // 3, VT // 3 + 1, 2 * VT // 3, VT - 1, VT // 2, 17, 33, VT - 5, 7, 70, 130, 1030, 2050]}[p]
    out = []
    for v in want + list(range(VT)):
        if 0 <= v < VT and v not in out:
            out.append(v)
        if len(out) == 2 * W:
            break
    return out


def _problem(K, VT, rows, W):
    """(x [rows, K] one-hot, weights [VT, K], bias [VT]) with the plants of the module docstring in columns c % 6 = 0 .. 5"""
    g = torch.Generator().manual_seed(K * 7 + VT)
    w = torch.randint(-8, 9, (VT, K), generator=g).float()
    b = _bias(VT)
    cols = (torch.arange(rows) * 211 + 1) % K                                     # spread over [0, K): every k-step and chunk carries a row
    for c in sorted(set(cols.tolist())):                                          # (only the columns a row selects)
        p = c % 6
        if p < 3:
            for j, v in enumerate(_positions(p, VT, W)[:W]):
                w[v, c] = 100 - 4 * ((j * 5) % W if p == 2 else j)               # (p = 2: the order of the values is not the order of the indices)
        elif p == 3:
            for v in _positions(3, VT, W):
                w[v, c] = 64 - b[v]                                               # exactly tied logits: 2 W of them (VT permitting), W kept
        elif p == 4:
            w[:, c] = 0                                                           # the bias alone decides
    x = torch.zeros(rows, K)
    x[torch.arange(rows), cols] = 1
    return x, w, b


def _gen_topk(x, w, b, W, frag):
    L = lib.load()
    rows, K = x.shape
    VT = w.shape[0]
    nb = L.nir_beam_gen_topk_workspace_bytes(rows, K, VT, W, 1 if frag is not None else 0)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    val = torch.empty(rows, W, device=DEV)
    idx = torch.empty(rows, W, dtype=torch.int32, device=DEV)
    lse = torch.empty(rows, device=DEV)
    lib.check(L.nir_beam_gen_topk(lib.ptr(x), rows, K, lib.ptr(w), lib.ptr(b), lib.ptr(frag), VT, W, lib.ptr(ws), nb, lib.ptr(val), lib.ptr(idx),
                                  lib.ptr(lse), lib.stream()), "nir_beam_gen_topk")
    return val.cpu(), idx.cpu().long(), lse.cpu()


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


@pytest.mark.parametrize("K", [32, 48, 96, 512, 1024])
def test_gen_topk_planted_winners_against_fp64(K):
    """K = 48 has the plain form only (48 % 32 != 0); the others run fused and plain.  rows: 65 is one past a 64-row block (NBT = 4), 33 one past a
    32-row block at K = 1024 (NBT = 2)"""
    worst = 0.0
    for VT in (8, 17, 200, 4099):
        for rows in (1, 17, 33, 65, 97):
            for W in (1, 3, 8):
                x, w, b = _problem(K, VT, rows, W)
                logits = x.double() @ w.double().t() + b.double()
                assert torch.equal(logits.float().double(), logits)              # exact in fp32
                sval, sidx = torch.sort(logits, dim=1, descending=True, stable=True)
                lse64 = torch.logsumexp(logits, 1)
                lse32 = torch.logsumexp(logits.float(), 1)
                xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
                frag = _pack(wd)
                assert (frag is None) == (K == 48)
                for form, f in (("fused", frag), ("plain", None)):
                    if form == "fused" and f is None:
                        continue
                    val, idx, lse = _gen_topk(xd, wd, bd, W, f)
                    tag = "K=%d VT=%d rows=%d W=%d %s" % (K, VT, rows, W, form)
                    assert torch.equal(idx, sidx[:, :W]), tag
                    assert torch.equal(val.double(), sval[:, :W]), tag
                    ok, fig = R.accept_scores(lse, lse64, lse32, 1 if form == "fused" else 0)
                    worst = max(worst, fig["ratio"])
                    assert ok, (tag, fig)
    print("beam gen_topk lse K=%d: largest ratio %.3g" % (K, worst))


def _select_ref(val, idx, lse, cum, fin, VT, lut, V):
    """the selection in float32, candidate by candidate -> (cum, finished, backptr, token, next_ids [W B])"""
    B, W = cum.shape
    out = [torch.zeros(B, W), torch.zeros(B, W, dtype=torch.int32), torch.zeros(B, W, dtype=torch.int32), torch.zeros(B, W, dtype=torch.int32),
           torch.zeros(W * B, dtype=torch.int64)]
    for b in range(B):
        cands = []
        for k in range(W):
            if fin[b, k]:
                cands.append((float(cum[b, k]), k * VT + R.EOS))
            else:
                for j in range(W):
                    s = cum[b, k] + (val[k * B + b, j] - lse[k * B + b])          # fp32, this order
                    cands.append((float(s), k * VT + int(idx[k * B + b, j])))
        cands.sort(key=lambda c: (-c[0], c[1]))
        for o, (s, flat) in enumerate(cands[:W]):
            k, v = divmod(flat, VT)
            out[0][b, o], out[1][b, o], out[2][b, o], out[3][b, o] = s, int(v == R.EOS), k, v
            nxt = int(lut[v])
            out[4][o * B + b] = nxt if 0 <= nxt < V else 1
    return out


@pytest.mark.parametrize("W", [1, 3, 8])
def test_select_step0_finished_mixed_and_frozen_live_ties(W):
    VT, V, B = 50, 40, 6
    g = torch.Generator().manual_seed(W)
    R_ = B * W
    val = torch.sort(torch.stack([torch.randperm(80, generator=g)[:W] for _ in range(R_)]).float() / 4 - 10, dim=1, descending=True)[0]
    idx = torch.stack([torch.randperm(VT, generator=g)[:W] for _ in range(R_)]).int()
    lse = val[:, 0] + torch.randint(1, 9, (R_,), generator=g).float() / 4
    lut = (torch.arange(VT) * 3) % 45                                            # some ids land outside [0, V): <unk>
    cum = -torch.rand(B, W, generator=g).float() * 8
    fin = torch.zeros(B, W, dtype=torch.int32)
    cum[0] = NEG                                                                  # row 0: step 0
    cum[0, 0] = 0
    fin[1] = 1                                                                    # row 1: every beam finished
    fin[2, ::2] = 1                                                               # row 2: a mix
    if W > 1:                                                                     # rows 3, 4: a frozen candidate ties with a live one
        for b, (kf, kl) in ((3, (0, 1)), (4, (1, 0))):                            # the frozen beam in front of / behind the live one
            fin[b, kf] = 1
            row = kl * B + b
            val[row] = -30.0 - torch.arange(W)
            val[row, 0], lse[row], cum[b, kl] = 2.0, 3.0, 0.0                     # the live beam's best: 0 + (2 - 3) = -1
            cum[b, kf] = -1.0
            idx[row, 0] = 7
            if W > 2:
                cum[b, 2:] = -50.0
    if R.EOS not in idx[R_ - 1].tolist():
        idx[R_ - 1, 0] = R.EOS                                                    # a live beam that may end now
    want = _select_ref(val, idx, lse, cum, fin, VT, lut, V)
    d = [t.to(DEV).contiguous() for t in (val, idx, lse, lut, cum.clone(), fin.clone())]
    bp, tok = torch.empty(B, W, dtype=torch.int32, device=DEV), torch.empty(B, W, dtype=torch.int32, device=DEV)
    nxt = torch.empty(R_, dtype=torch.int64, device=DEV)
    lib.check(lib.load().nir_beam_select(lib.ptr(d[0]), lib.ptr(d[1]), lib.ptr(d[2]), B, W, VT, lib.ptr(d[3]), V, lib.ptr(d[4]), lib.ptr(d[5]), lib.ptr(bp),
                                         lib.ptr(tok), lib.ptr(nxt), lib.stream()), "nir_beam_select")
    got = [d[4].cpu(), d[5].cpu(), bp.cpu(), tok.cpu(), nxt.cpu()]
    for name, a, b_ in zip(("cum", "finished", "backptr", "token", "next_ids"), got, want):
        assert torch.equal(a, b_), (name, a, b_)
    assert got[3][0].tolist() == idx[0:1, :].reshape(-1).tolist()[:W] and got[2][0].tolist() == [0] * W       # step 0: beam 0's own top-W
    assert got[3][1].tolist() == [R.EOS] * W and torch.equal(got[0][1], torch.sort(cum[1], descending=True)[0])
    if W > 1:
        assert got[2][3, :2].tolist() == [0, 1] and got[3][3, :2].tolist() == [R.EOS, 7]        # flat 3 < VT + 7
        assert got[2][4, :2].tolist() == [0, 1] and got[3][4, :2].tolist() == [7, R.EOS]        # flat 7 < VT + 3
        assert got[0][3, 0] == got[0][3, 1] == -1.0


def _pack16(h):
    """launch_h16_pack on the host: [rows, H] -> [rows][H/8][2 terms][8] fp16 (h1 to nearest, h2' = fp16(2^11 (x - h1)))"""
    hi = h.half()
    lo = ((h - hi.float()) * 2048.0).half()
    return torch.stack([hi.view(h.shape[0], -1, 8), lo.view(h.shape[0], -1, 8)], 2).contiguous()


def test_reorder_is_the_references_beam_update_bit_for_bit():
    g = load_golden("beam_state")
    pos = T(g["positions"]).int()
    B, W = pos.shape
    H = g["lstm_h"].shape[2]
    L = lib.load()
    bp = pos.to(DEV)
    for names in (("lstm_h", "lstm_c"), ("gru_h",)):
        pre = [T(g["pre_" + n])[0].contiguous() for n in names]
        want = [T(g["upd_" + n])[0] for n in names]
        ins = [p.to(DEV) for p in pre] + [_pack16(pre[0]).to(DEV)]
        outs = [torch.zeros_like(t) for t in ins]
        c_in, c_out = (lib.ptr(ins[1]), lib.ptr(outs[1])) if len(names) == 2 else (None, None)
        lib.check(L.nir_beam_reorder(lib.ptr(bp), B, W, H, lib.ptr(ins[0]), lib.ptr(outs[0]), c_in, c_out, lib.ptr(ins[-1]), lib.ptr(outs[-1]),
                                     lib.stream()), "nir_beam_reorder")
        for n, o, w_ in zip(names, outs, want):
            assert torch.equal(o.cpu(), w_), n
        assert torch.equal(outs[-1].cpu().view(torch.int16), _pack16(want[0]).view(torch.int16))          # gather, then pack
        assert not torch.equal(outs[0].cpu(), pre[0])
