"""GPU (-m gpu): the generator + bias + (lse, top-W) kernel on the split state (csrc/beam.hip: beam_gen_topk_kernel on BeamRowsSplit through
nir_beam_hredqs_gen_topk) and the decode entry nir_beam_hredqs_decode at the C ABI, across their envelope.

Shapes of the kernel tests: K in {32, 96, 512, 544, 1024} (one k-step, a chunk that is not full, both row-tile widths on either side of
K = 512, the largest K) x rows in {1, 17, 33, 65} (a partial row tile, one row past a 16-row tile, a second 32-row block at K > 512, a second
64-row block below) x VT in {8, 17, 200, 4099} (VT = W at W = 8, a partial second tile, fewer tiles than the waves of a workgroup can share with
nvr = 1 -- the `nvr % 8` fallback of the grid --, several vocabulary ranges with a zero-padded last tile: nvr a multiple of 8 wherever the device
has >= 8 CUs per row block) x W in {1, 3, 8} (both list widths of the template).

Two input families:
  (a) the exactly representable plants of tests/test_gpu_beam_envelope.py (one-hot rows, integer weights, bias in eighths), split on the host:
      indices and values exact, lse inside the bound with n_split = 1;
  (b) random state rows in (-1, 1) against random weights, so that the LOW term plane carries data: every float64 gap among each row's top
      W + 1 logits is asserted >= 1e-3 before the GPU result is looked at, then indices exact and values and lse inside the bound.  Whether the
      bits equal nir_beam_gen_topk on the fp32 rows is printed, not asserted (that kernel splits with round-toward-zero, the host split here and
      the folded LSTM step round to nearest).
The decode entry runs a decoder without attention at H = 32 (session_beam_ref's restatement of the step, the states paired as the entry pairs
them) at Bd in {1, 17} and, for a pairing that moves rows, B = 3, S = 3, x W in {1, 3, 8} x max_len in {1, 5}, in both forms."""
import pytest
import torch

import beam_ref as BR
import hredqs_beam_ref as R
import session_beam_ref as SR
from context_attentive_ir_amd import lib
from test_gpu_beam_envelope import _gen_topk, _pack, _problem
from test_gpu_hredqs_envelope import _h16

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAD_ARG, WS_ERR = -1, -3
MIN_GAP = 1e-3
KS, ROWS, VTS, WS = (32, 96, 512, 544, 1024), (1, 17, 33, 65), (8, 17, 200, 4099), (1, 3, 8)


def _hq_topk(x, b, frag, VT, W, ws=None):
    """nir_beam_hredqs_gen_topk on the host-split rows of x [rows, K] (CPU fp32) -> (val, idx, lse) on the CPU"""
    L = lib.load()
    rows, K = x.shape
    hd = _h16(x).to(DEV)
    nb = L.nir_beam_hredqs_gen_topk_workspace_bytes(rows, K, VT, W)
    assert nb > 0
    if ws is None:
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    assert ws.numel() >= nb
    val = torch.full((rows, W), -7.0, device=DEV)
    idx = torch.full((rows, W), -7, dtype=torch.int32, device=DEV)
    lse = torch.full((rows,), -7.0, device=DEV)
    lib.check(L.nir_beam_hredqs_gen_topk(lib.ptr(hd), rows, K, lib.ptr(b), lib.ptr(frag), VT, W, lib.ptr(ws), ws.numel(), lib.ptr(val), lib.ptr(idx),
                                         lib.ptr(lse), lib.stream()), "nir_beam_hredqs_gen_topk")
    torch.cuda.synchronize()
    return val.cpu(), idx.cpu().long(), lse.cpu()


@pytest.mark.parametrize("K", KS)
def test_planted_winners_are_exact(K):
    worst = 0.0
    for VT in VTS:
        for rows in ROWS:
            for W in WS:
                x, w, b = _problem(K, VT, rows, W)
                assert torch.equal(_h16(x)[:, :, 0].reshape(rows, K).float(), x) and not bool(_h16(x)[:, :, 1].any())    # one-hot rows split exactly
                logits = x.double() @ w.double().t() + b.double()
                assert torch.equal(logits.float().double(), logits)              # exact in fp32
                sval, sidx = torch.sort(logits, dim=1, descending=True, stable=True)
                wd, bd = w.to(DEV), b.to(DEV)
                val, idx, lse = _hq_topk(x, bd, _pack(wd), VT, W)
                tag = "K=%d VT=%d rows=%d W=%d" % (K, VT, rows, W)
                assert torch.equal(idx, sidx[:, :W]), tag
                assert torch.equal(val.double(), sval[:, :W]), tag
                ok, fig = BR.accept_scores(lse, torch.logsumexp(logits, 1), torch.logsumexp(logits.float(), 1), 1, R.MARGIN)
                worst = max(worst, fig["ratio"])
                assert ok, (tag, fig)
    print("hredqs beam gen_topk planted lse K=%d: largest ratio %.3g" % (K, worst))


def _random_case(seed, rows, K, VT):
    """x [rows, K] in (-1, 1) like an LSTM state, W [VT, K] with rows of norm 64 (logits spread over ~ +-100: the top nine of 4099 lie ~ 1 apart),
    b [VT]; the first of 64 seeds whose float64 logits keep every gap among each row's top min(9, VT) >= 1e-3"""
    for attempt in range(64):
        g = torch.Generator().manual_seed(seed + 7919 * attempt)
        x = torch.rand(rows, K, generator=g) * 2 - 1
        W = torch.randn(VT, K, generator=g)
        W = 64 * W / W.norm(dim=1, keepdim=True)
        b = torch.randn(VT, generator=g) * 0.5
        logits = x.double() @ W.double().t() + b.double()
        top = logits.topk(min(9, VT), 1).values
        if float((top[:, :-1] - top[:, 1:]).min()) >= MIN_GAP:
            return x, W, b, logits
    raise AssertionError("no seed gives top-9 gaps >= %g for rows=%d K=%d VT=%d" % (MIN_GAP, rows, K, VT))


@pytest.mark.parametrize("K", KS)
def test_random_split_rows_against_fp64(K):
    worst, same_bits, total = 0.0, 0, 0
    for VT in VTS:
        for rows in ROWS:
            x, w, b, logits = _random_case(100000 * rows + 7 * K + VT, rows, K, VT)
            assert bool(_h16(x)[:, :, 1].any())                                  # the low term plane carries data
            wd, bd = w.to(DEV), b.to(DEV)
            frag = _pack(wd)
            chain = x @ w.t() + b                                                # the float32 yardstick
            for W in WS:
                sval, sidx = torch.sort(logits, dim=1, descending=True, stable=True)
                top = sval[:, :min(W + 1, VT)]
                assert float((top[:, :-1] - top[:, 1:]).min()) >= MIN_GAP        # asserted before the GPU result is looked at; no row is left out
                val, idx, lse = _hq_topk(x, bd, frag, VT, W)
                tag = "K=%d VT=%d rows=%d W=%d" % (K, VT, rows, W)
                assert torch.equal(idx, sidx[:, :W]), tag
                okv, fv = BR.accept_scores(val, sval[:, :W], chain.gather(1, sidx[:, :W]), 1, R.MARGIN)
                okl, fl = BR.accept_scores(lse, torch.logsumexp(logits, 1), torch.logsumexp(chain, 1), 1, R.MARGIN)
                worst = max(worst, fv["ratio"], fl["ratio"])
                assert okv and okl, (tag, fv, fl)
                v2, i2, l2 = _hq_topk(x, bd, frag, VT, W)
                assert torch.equal(v2, val) and torch.equal(i2, idx) and torch.equal(l2, lse), tag       # the same bits
                fv32, fi32, fl32 = _gen_topk(x.to(DEV), wd, bd, W, frag)
                total += 1
                same_bits += int(torch.equal(fv32, val) and torch.equal(fi32, idx) and torch.equal(fl32, lse))
    print("hredqs beam gen_topk random K=%d: largest ratio %.3g; bits equal to nir_beam_gen_topk on the fp32 rows in %d of %d calls" % (K, worst, same_bits, total))


def test_two_calls_on_one_workspace_do_not_leak_partials():
    L = lib.load()
    rows, K, VT, W = 33, 96, 200, 3
    ws = torch.empty(L.nir_beam_hredqs_gen_topk_workspace_bytes(rows, K, VT, 8), dtype=torch.uint8, device=DEV)
    x, w, b, logits = _random_case(5, rows, K, VT)
    frag = _pack(w.to(DEV))
    loud = b.clone()
    loud[7] = 1000.0                                                        # first call: a candidate far above anything the later calls produce
    val, idx, _ = _hq_topk(x, loud.to(DEV), frag, VT, 8, ws)
    assert bool((idx[:, 0] == 7).all())
    sval, sidx = torch.sort(logits, dim=1, descending=True, stable=True)
    want_lse = torch.logsumexp(logits, 1)
    val, idx, lse = _hq_topk(x, b.to(DEV), frag, VT, W, ws)
    assert torch.equal(idx, sidx[:, :W]) and float((lse.double() - want_lse).abs().max()) <= 1e-4
    val, idx, lse = _hq_topk(x[:5].contiguous(), b.to(DEV), frag, VT, W, ws)       # and fewer rows on the same workspace
    assert torch.equal(idx, sidx[:5, :W]) and float((lse.double() - want_lse[:5]).abs().max()) <= 1e-4
    val, idx, lse = _hq_topk(x, None, frag, VT, W, ws)                      # no bias
    nb_logits = x.double() @ w.double().t()
    assert torch.equal(idx[:, 0], nb_logits.argmax(1))


def test_gen_topk_error_classes_leave_the_outputs_untouched():
    L = lib.load()
    rows, K, VT, W = 5, 64, 40, 3
    x, w, b, _ = _random_case(1, rows, K, VT)
    frag = _pack(w.to(DEV))
    hd, bd = _h16(x).to(DEV), b.to(DEV)
    need = L.nir_beam_hredqs_gen_topk_workspace_bytes(rows, K, VT, W)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    cases = [(dict(K=48), BAD_ARG), (dict(K=1056), BAD_ARG), (dict(VT=0), BAD_ARG), (dict(W=0), BAD_ARG), (dict(W=9), BAD_ARG), (dict(VT=2), BAD_ARG),
             (dict(frag=None), BAD_ARG), (dict(nbytes=need - 64), WS_ERR), (dict(rows=0), 0)]
    for kw, want in cases:
        a = dict(rows=rows, K=K, VT=VT, W=W, frag=frag, nbytes=need)
        a.update(kw)
        val = torch.full((rows, 8), -7.0, device=DEV)
        idx = torch.full((rows, 8), -7, dtype=torch.int32, device=DEV)
        lse = torch.full((rows,), -7.0, device=DEV)
        rc = L.nir_beam_hredqs_gen_topk(lib.ptr(hd), a["rows"], a["K"], lib.ptr(bd), lib.ptr(a["frag"]), a["VT"], a["W"], lib.ptr(ws), a["nbytes"], lib.ptr(val),
                                        lib.ptr(idx), lib.ptr(lse), lib.stream())
        torch.cuda.synchronize()
        assert rc == want and bool((val == -7).all()) and bool((idx == -7).all()) and bool((lse == -7).all()), kw


# ---- the decode entry -------------------------------------------------------------------------------------------------------------------------------
H_ENV, E_ENV, V_ENV = 32, 8, 40


def _problem_states(B, S, seed):
    """a decoder without attention at the smallest dims that reach the fast form (H 32), detinit weights, the generator scaled up so that the
    candidates lie apart; h_steps / c_steps [B, S, H] and, for the restatement, the states as the entry pairs them"""
    from context_attentive_ir_amd.detinit import det_tensor
    d = lambda n, shape, scale=None: det_tensor("hredqs_beam.env." + n, shape, seed, scale)          # noqa: E731
    sd = {SR.TABLE: d("table", (V_ENV, E_ENV), 0.5), "decoder.decoder.rnn.weight_ih_l0": d("wih", (4 * H_ENV, E_ENV)),
          "decoder.decoder.rnn.weight_hh_l0": d("whh", (4 * H_ENV, H_ENV)), "decoder.decoder.rnn.bias_ih_l0": d("bih", (4 * H_ENV,)),
          "decoder.decoder.rnn.bias_hh_l0": d("bhh", (4 * H_ENV,)), "generator.weight": d("gw", (V_ENV, H_ENV), 2.0), "generator.bias": d("gb", (V_ENV,), 1.0)}
    sd["generator.bias"][BR.EOS] += 1.0
    lut = (torch.arange(V_ENV) * 7 + 3) % (V_ENV + 2)                           # two targets map outside the source vocabulary: fed back as <unk>
    hs, cs = d("hs", (B, S, H_ENV), 1.0), d("cs", (B, S, H_ENV), 1.0)
    Bd = B * S
    return dict(kind="plain", sd=sd, hs=hs, cs=cs, dec_h=hs.transpose(0, 1).reshape(Bd, H_ENV), dec_c=cs.transpose(0, 1).reshape(Bd, H_ENV), lut=lut,
                V=V_ENV, B=B, S=S)


def _weights(sd, fast):
    """(struct, tensors kept alive) of nir_hredqs_decoder_weights over the problem's weights on the device"""
    L = lib.load()
    p = {k: sd["decoder.decoder.rnn." + n + "_l0"].to(DEV).contiguous() for k, n in (("rnn_wih", "weight_ih"), ("rnn_whh", "weight_hh"),
                                                                                     ("rnn_bih", "bias_ih"), ("rnn_bhh", "bias_hh"))}
    p.update(gen_w=sd["generator.weight"].to(DEV).contiguous(), gen_b=sd["generator.bias"].to(DEV).contiguous(), table=sd[SR.TABLE].to(DEV).contiguous())
    w = lib.HredqsDecoderWeights()
    for k in ("rnn_wih", "rnn_whh", "rnn_bih", "rnn_bhh", "gen_w", "gen_b"):
        setattr(w, k, p[k].data_ptr())
    w.H, w.VT = H_ENV, V_ENV
    if fast:
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        p["rnn_whh_frag"] = torch.empty(L.nir_lstm_step_whh_frag_bytes(H_ENV), dtype=torch.uint8, device=DEV)
        lib.check(L.nir_lstm_step_pack_whh_frag(lib.ptr(p["rnn_whh"]), H_ENV, lib.ptr(p["rnn_whh_frag"]), lib.ptr(flag), lib.stream()), "pack whh")
        p["gen_frag"] = torch.empty(L.nir_seq2seq_gen_frag_bytes(V_ENV, H_ENV), dtype=torch.uint8, device=DEV)
        lib.check(L.nir_seq2seq_pack_gen_frag(lib.ptr(p["gen_w"]), V_ENV, H_ENV, lib.ptr(p["gen_frag"]), lib.ptr(flag), lib.stream()), "pack gen")
        assert int(flag.item()) == 0
        p["rnn_gate_fold"] = lib.fold_lstm_table(p["table"], p["rnn_wih"], p["rnn_bih"], p["rnn_bhh"], H_ENV, 1, "f32")
        for k in ("rnn_whh_frag", "gen_frag", "rnn_gate_fold"):
            setattr(w, k, p[k].data_ptr())
    return w, p


def _decode_call(cs, W, max_len, fast, B=None, nbytes=None):
    """B: the batch handed to the entry when it is not the buffers' (0: an empty batch over live buffers)"""
    L = lib.load()
    w, p = _weights(cs["sd"], fast)
    Bd = cs["B"] * cs["S"]
    out = {"predictions": torch.full((Bd, W, max_len), -7, dtype=torch.int64, device=DEV), "scores": torch.full((Bd, W), -7.0, device=DEV),
           "lengths": torch.full((Bd, W), -7, dtype=torch.int64, device=DEV), "backptr": torch.full((max_len, Bd, W), -7, dtype=torch.int32, device=DEV)}
    hs, c_, lut = cs["hs"].to(DEV).contiguous(), cs["cs"].to(DEV).contiguous(), cs["lut"].to(DEV)
    nb = L.nir_beam_hredqs_decode_workspace_bytes(cs["B"], cs["S"], W, max_len, lib.C.byref(w))
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    rc = L.nir_beam_hredqs_decode(lib.ptr(hs), lib.ptr(c_), cs["B"] if B is None else B, cs["S"], lib.ptr(p["table"]), V_ENV, E_ENV, lib.ptr(lut), BR.BOS,
                                  max_len, lib.C.byref(w), W, lib.ptr(ws), nb if nbytes is None else nbytes, lib.ptr(out["predictions"]),
                                  lib.ptr(out["scores"]), lib.ptr(out["lengths"]), lib.ptr(out["backptr"]), lib.stream())
    torch.cuda.synchronize()
    return rc, out


def _gapped(B, S, W, max_len, limit=400):
    """the first seed whose float64 decode keeps every gap >= 1e-3 and whose free float32 decode agrees -- decided on the CPU"""
    for seed in range(1, limit):
        cs = dict(_problem_states(B, S, seed), max_len=max_len)
        ref = SR.decode(cs, cs["sd"], W)
        cond = BR.conditions(ref, SR.decode(cs, cs["sd"], W, torch.float32), W)
        if cond["gap"] and cond["f32"]:
            return cs, ref, SR.decode(cs, cs["sd"], W, torch.float32, force=(ref["backptr"], ref["tokens"]))
    raise AssertionError("no gapped seed below %d" % limit)


@pytest.mark.parametrize("B,S", [(1, 1), (17, 1), (1, 17), (3, 3)])
@pytest.mark.parametrize("W", WS)
def test_decode_entry_envelope(B, S, W):
    for max_len in (1, 5):
        cs, ref, chain = _gapped(B, S, W, max_len)
        for fast in (True, False):
            rc, got = _decode_call(cs, W, max_len, fast)
            assert rc == 0
            # the states are given: only the step's and the generator's split products lie on the score's path
            ok, fig = SR.accept_decode(got, ref, chain, SR.n_split(fast, fast, max_len), margin=R.MARGIN)
            print("hredqs beam envelope decode B=%d S=%d W=%d max_len=%d fast=%s: %s" % (B, S, W, max_len, fast, fig))
            assert ok, fig


def test_decode_entry_error_classes_and_empty_batch_on_the_device():
    cs = dict(_problem_states(3, 2, 1), max_len=3)
    for fast in (True, False):
        for kw in (dict(B=0),):
            rc, out = _decode_call(cs, 3, 3, fast, **kw)
            assert rc == 0 and all(bool((v == -7).all()) for v in out.values())  # nothing enqueued: every output as it was
        rc, out = _decode_call(cs, 3, 3, fast, nbytes=64)
        assert rc == WS_ERR and all(bool((v == -7).all()) for v in out.values())
        rc, out = _decode_call(cs, 3, 3, fast, B=-1)
        assert rc == BAD_ARG and all(bool((v == -7).all()) for v in out.values())
        rc, out = _decode_call(cs, 3, 3, fast)
        assert rc == 0 and not any(bool((v == -7).any()) for v in out.values())
