"""GPU (-m gpu): nir_gru_step (csrc/gru_step.hip), ONE GRU decoder step at the C ABI, against float64 over the envelope of its two forms.

Bound, in the project's form (tests/gemm_ref.py): with s = max |ref64|, e = max |got - ref64| / s and e_chain the same figure for the float32
CPU chain,

    e <= MARGIN * max(e_chain, 2^-23) + n_split * FMT["fp16x2"]

n_split = 1 on the fast form (one recurrent product over fp16 term pairs), 0 on the plain form, 6 for six chained fast steps.  Every ratio
(e - fmt) / max(e_chain, 2^-23) is printed (DESIGN.md section 20 has the table).  MARGIN started at 2, the rule's starting value; the largest
ratio measured on the MI355X is 2.780 (plain form, H = 20, B = 5, E = 300; every fast-form ratio is negative, the next plain one 1.047), which
doubled and rounded up to a power of two asks for 8: gemm_ref.MARGIN_CAP holds, so MARGIN = 4 -- the value gemm_ref.MARGIN has for the
fp32-MFMA GEMM the plain form is made of, whose K = 300 products land in one fp32 accumulator (accumulation order, not a lost term; at the
cap every planted fault of the cell is still > 100 bounds away: tests/test_seq2seq_gru_host.py).

Inputs (gru_dec_ref.step_inputs): V = 50, one repeated token id, ids outside [0, V) (the <unk> clamp), a b_hn of order 1 -- a b_hn outside the
reset product is then off by ~0.1, far outside the bound (tests/test_seq2seq_gru_host.py shows that on the CPU).
"""
import pytest
import torch

import gemm_ref
import gru_dec_ref as R
from context_attentive_ir_amd import lib

pytestmark = pytest.mark.gpu
DEV = "cuda"
MARGIN = gemm_ref.MARGIN_CAP
V = 50


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def _pack(whh, H):
    L = lib.load()
    nb = L.nir_gru_step_whh_frag_bytes(H)
    assert nb == 3 * H * H * 4
    frag = torch.empty(nb, dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    lib.check(L.nir_gru_step_pack_whh_frag(lib.ptr(whh), H, lib.ptr(frag), lib.ptr(flag), lib.stream()), "nir_gru_step_pack_whh_frag")
    return frag, int(flag.item())


def _fold(table, wih, bih, bhh, H):
    """gate_fold [V,3H] = table W_ih^T + b_ih + (b_hr, b_hz, 0) through nir_linear_f32, as the host builds it"""
    L = lib.load()
    bias = bih.clone()
    bias[:2 * H] += bhh[:2 * H]
    out = torch.empty(table.shape[0], 3 * H, device=DEV)
    E = table.shape[1]
    lib.check(L.nir_linear_f32(lib.ptr(table), E, None, None, 0, 0, 0, lib.ptr(wih), E, lib.ptr(bias), None, lib.ptr(out), 3 * H, table.shape[0], 3 * H, E, 0,
                               lib.stream()), "nir_linear_f32")
    return out


def _step(ids, table, wih, bih, whh, bhh, h, fold=None, frag=None, h16=None, want16=True):
    L = lib.load()
    B, H = h.shape
    hn = torch.full((B, H), float("nan"), device=DEV)
    h16n = torch.zeros(B, H // 8, 2, 8, dtype=torch.float16, device=DEV) if (want16 and H % 8 == 0) else None
    ws = torch.empty(max(1, L.nir_gru_step_workspace_bytes(B, H)), dtype=torch.uint8, device=DEV)
    lib.check(L.nir_gru_step(lib.ptr(ids), B, lib.ptr(table), table.shape[0], table.shape[1], lib.ptr(wih), lib.ptr(bih), lib.ptr(fold), lib.ptr(whh),
                             lib.ptr(bhh), lib.ptr(frag), H, lib.ptr(h), lib.ptr(h16), lib.ptr(hn), lib.ptr(h16n), lib.ptr(ws), ws.numel(), lib.stream()),
              "nir_gru_step")
    return hn, h16n


def _check(tag, got, x, n_split):
    ref, chain = R.step(*x), R.step(*x, dtype=torch.float32)
    ok, fig = R.accept(got, ref, chain, n_split, margin=MARGIN)
    print("gru_step ratio %s: %.3f  (e %.3g, e_chain %.3g, bound %.3g)" % (tag, fig["ratio"], fig["e"], fig["e_chain"], fig["bound"]))
    assert ok, (tag, fig)


@pytest.mark.parametrize("H", [32, 96, 512, 1024])          # 96: three k-blocks over four waves
@pytest.mark.parametrize("B", [1, 5, 17, 70])               # 17 crosses a 16-row tile edge, 70 a slab edge
def test_fast_form_folded_and_unfolded(H, B):
    x = R.step_inputs(H, B, 20)
    ids, table, wih, bih, whh, bhh, h = _dev(*x)
    frag, bad = _pack(whh, H)
    assert bad == 0
    fold = _fold(table, wih, bih, bhh, H)
    for name, f in (("folded", fold), ("unfolded", None)):
        hn, h16 = _step(ids, table, wih, bih, whh, bhh, h, fold=f, frag=frag)
        _check("fast %s H=%d B=%d" % (name, H, B), hn, x, 1)
        assert torch.equal(h16.cpu(), R.split_pairs(hn.cpu())), "h16_next is the split of h_next, bit for bit"
        again, again16 = _step(ids, table, wih, bih, whh, bhh, h, fold=f, frag=frag)
        assert torch.equal(again, hn) and torch.equal(again16, h16)
        # the state handed over as term pairs gives the same bits as the state split by the call
        hn2, _ = _step(ids, table, wih, bih, whh, bhh, h, fold=f, frag=frag, h16=R.split_pairs(h.cpu()).to(DEV))
        assert torch.equal(hn2, hn)
    # the table is not read when the fold is given
    hn3, _ = _step(ids, torch.full_like(table, float("nan")), wih, bih, whh, bhh, h, fold=fold, frag=frag)
    assert bool(torch.isfinite(hn3).all())


@pytest.mark.parametrize("H", [4, 20, 100])
@pytest.mark.parametrize("B", [1, 5, 17, 70])
@pytest.mark.parametrize("E", [4, 300])
def test_plain_form(H, B, E):
    x = R.step_inputs(H, B, E)
    ids, table, wih, bih, whh, bhh, h = _dev(*x)
    hn, h16 = _step(ids, table, wih, bih, whh, bhh, h)
    _check("plain H=%d B=%d E=%d" % (H, B, E), hn, x, 0)
    if h16 is not None:
        assert torch.equal(h16.cpu(), R.split_pairs(hn.cpu()))
    again, _ = _step(ids, table, wih, bih, whh, bhh, h)
    assert torch.equal(again, hn)


def test_exact_f32_tunable_takes_the_plain_form():
    x = R.step_inputs(64, 17, 20)
    ids, table, wih, bih, whh, bhh, h = _dev(*x)
    frag, _ = _pack(whh, 64)
    with lib.tunable("exact_f32", 1, 0):
        hn, _ = _step(ids, table, wih, bih, whh, bhh, h, fold=_fold(table, wih, bih, bhh, 64), frag=frag)
    _check("exact_f32 H=64 B=17", hn, x, 0)


def test_out_of_range_weight_sets_the_flag_and_the_host_falls_back():
    H = 64
    x = list(R.step_inputs(H, 5, 20))
    x[4] = x[4].clone()
    x[4][2 * H + 3, 7] = 40000.0                                    # |w_hh| >= 2^15
    ids, table, wih, bih, whh, bhh, h = _dev(*x)
    _, bad = _pack(whh, H)
    assert bad == 2
    hn, _ = _step(ids, table, wih, bih, whh, bhh, h)                # what the host does then: no fragment, the plain form
    _check("plain, out-of-range w_hh", hn, x, 0)
    # the host: Seq2seqGRU leaves both packs out
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.recommender import Seq2seqGRU
    net = Seq2seqGRU(default_args("SEQ2SEQ", rnn_type="GRU", nlayers=1, nhid=64, src_vocab_size=60, tgt_vocab_size=40)).to(DEV).eval()
    w = net._decoder_weights().struct
    assert w.rnn_whh_frag and w.rnn_gate_fold
    with torch.no_grad():
        net.decoder.decoder.rnn.weight_hh_l0[5, 5] = 40000.0
    w = net._decoder_weights().struct
    assert not w.rnn_whh_frag and not w.rnn_gate_fold and w.gen_frag


def test_six_chained_steps_carry_the_state():
    H, B, T = 64, 17, 6
    x = R.step_inputs(H, B, 20)
    ids, table, wih, bih, whh, bhh, h = _dev(*x)
    frag, _ = _pack(whh, H)
    fold = _fold(table, wih, bih, bhh, H)
    g = torch.Generator().manual_seed(3)
    toks = [x[0]] + [torch.randint(0, V, (B,), generator=g) for _ in range(T - 1)]
    ref, chain = x[6].double(), x[6].float()
    hd, h16 = h, None
    for t in range(T):
        ref = R.step(toks[t], *x[1:6], ref)
        chain = R.step(toks[t], *x[1:6], chain, dtype=torch.float32)
        hd, h16 = _step(toks[t].to(DEV), table, wih, bih, whh, bhh, hd, fold=fold, frag=frag, h16=h16)
    ok, fig = R.accept(hd, ref, chain, T, margin=MARGIN)
    print("gru_step ratio chained x%d H=%d B=%d: %.3f  (e %.3g, e_chain %.3g)" % (T, H, B, fig["ratio"], fig["e"], fig["e_chain"]))
    assert ok, fig
    # a state that is not carried is far outside
    lost, _ = _step(toks[-1].to(DEV), table, wih, bih, whh, bhh, h, fold=fold, frag=frag)
    assert not R.accept(lost, ref, chain, T, margin=gemm_ref.MARGIN_CAP)[0]


def test_empty_batch_and_bad_arguments_enqueue_nothing():
    L = lib.load()
    x = R.step_inputs(32, 5, 20)
    ids, table, wih, bih, whh, bhh, h = _dev(*x)
    hn = torch.full_like(h, 7.0)
    ws = torch.empty(L.nir_gru_step_workspace_bytes(5, 32), dtype=torch.uint8, device=DEV)
    args = lambda B, H, wsn: (lib.ptr(ids), B, lib.ptr(table), V, 20, lib.ptr(wih), lib.ptr(bih), None, lib.ptr(whh), lib.ptr(bhh), None, H, lib.ptr(h),
                              None, lib.ptr(hn), None, lib.ptr(ws), wsn, lib.stream())          # noqa: E731
    assert L.nir_gru_step(*args(0, 32, ws.numel())) == 0
    assert L.nir_gru_step(*args(5, 30, ws.numel())) == -1
    assert L.nir_gru_step(*args(5, 32, 64)) != 0
    torch.cuda.synchronize()
    assert bool((hn == 7.0).all())
