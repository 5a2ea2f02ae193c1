"""CPU: the restatement and the teeth of the train-mode acceptance criterion (tests/bptt_ref.py), and the reach of the dispatchers it restates.
  * the float64 forward + BPTT equal torch.nn.LSTM / torch.nn.GRU over pack_padded_sequence under float64 autograd, with gradients flowing in through
    h_n / c_n and out through h0 / c0 (and, through a hand-written autograd loop, through the stored cell states); a length-0 row, which torch's
    packed sequences refuse, is checked against the contract directly;
  * at the cap of its margin the criterion accepts the fp32 yardstick in two other summation orders and with activation noise of 1e-7 on EVERY
    input of the GPU tables (tests/test_gpu_bptt_envelope.py) -- an input on which an honest fp32 evaluation fails is replaced there (reseed),
    never the criterion -- and rejects every planted fault, precision faults by at least 1.3 x;
  * every case of the GPU tables lands on the kernel it names, every dispatch threshold is there from both sides."""
import os
import re

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

import bptt_ref as B
import rnn_ref as R
import test_gpu_bptt_envelope as E

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "context_attentive_ir_amd", "csrc")
CAP = B.MARGIN_CAP


def _clean(a):
    """the poison at t >= len taken out (torch multiplies it with the zero padding of its output)"""
    return None if a is None else np.where(np.abs(a) == B.POISON, 0, a).astype(np.float64)


# ------------------------------------------------------------------ the restatement against torch autograd
@pytest.mark.parametrize("ndir", [1, 2])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_restatement_equals_float64_torch_autograd(cell, ndir):
    M, T, H = 6, 7, 9
    NG = 4 if cell == "lstm" else 3
    inp = B.make(cell, "randn", 5 + ndir, M, T, H, ndir, lengths=[T, 3, 1, T, 5, 1], dcst=False)
    gin = torch.tensor(_clean(inp["gin"]), requires_grad=True)
    mod = getattr(torch.nn, cell.upper())(ndir * NG * H, H, 1, bidirectional=ndir == 2, batch_first=True).double()
    sd = {}
    for d, sfx in enumerate(["", "_reverse"][:ndir]):                 # W_ih selects direction d's block of gates_in: x.grad IS the gate gradient
        sel = torch.zeros(NG * H, ndir * NG * H, dtype=torch.float64)
        sel[:, d * NG * H:(d + 1) * NG * H] = torch.eye(NG * H, dtype=torch.float64)
        sd["weight_ih_l0" + sfx], sd["bias_ih_l0" + sfx] = sel, torch.zeros(NG * H, dtype=torch.float64)
        sd["weight_hh_l0" + sfx] = torch.tensor(inp["w_hh"][d].astype(np.float64))
        sd["bias_hh_l0" + sfx] = torch.tensor(inp["b_hh"][d].astype(np.float64)) if cell == "gru" else torch.zeros(NG * H, dtype=torch.float64)
    mod.load_state_dict(sd)
    lens = inp["lens"]
    pk = pack_padded_sequence(gin, lens.tolist(), batch_first=True, enforce_sorted=False)
    dout, dhn = torch.tensor(_clean(inp["dout"])), torch.tensor(inp["dhn"].astype(np.float64))
    if cell == "lstm":
        h0, c0 = (torch.tensor(inp[k].astype(np.float64), requires_grad=True) for k in ("h0", "c0"))
        o, (hn, cn) = mod(pk, (h0, c0))
        loss = (hn * dhn).sum() + (cn * torch.tensor(inp["dcn"].astype(np.float64))).sum()
    else:
        o, hn = mod(pk)
        loss = (hn * dhn).sum()
    out = pad_packed_sequence(o, batch_first=True, total_length=T)[0]
    (loss + (out * dout).sum()).backward()
    fwd, bwd = B.fwd_figures(inp)["ref"], B.bwd_eval(inp, saved=B.fwd_figures(inp)["ref"])
    close = lambda a, b: np.allclose(a, b.detach().numpy(), rtol=0, atol=1e-12)
    assert close(fwd["out"], out) and close(fwd["hn"], hn)
    if cell == "lstm":
        assert close(fwd["cn"], cn) and close(bwd["dgates"], gin.grad) and close(bwd["dh0"], h0.grad) and close(bwd["dc0"], c0.grad)
    else:
        assert close(bwd["dgx"], gin.grad)
        r = fwd["act"][..., :H].reshape(M, T, ndir * H)                # dq = r da_n; db_hn = its sum over the valid positions
        assert np.array_equal(bwd["dq"], bwd["dgx"].reshape(M, T, ndir, 3, H)[:, :, :, 2].reshape(M, T, ndir * H) * r)
        for d, sfx in enumerate(["", "_reverse"][:ndir]):
            assert close(bwd["dq"][:, :, d * H:(d + 1) * H].sum((0, 1)), getattr(mod, "bias_hh_l0" + sfx).grad[2 * H:])


def test_gradient_through_the_stored_cell_states_and_length_zero():
    """dcst (and everything else at once) against a hand-written float64 autograd loop that takes length 0 as well"""
    M, T, H, ndir = 5, 6, 7, 2
    inp = B.make("lstm", "randn", 3, M, T, H, ndir, lengths=[T, 0, 1, 3, -2])
    lens = inp["lens"]
    leaf = lambda k: torch.tensor(_clean(inp[k]), requires_grad=True)
    gin, h0, c0 = leaf("gin"), leaf("h0"), leaf("c0")
    w = torch.tensor(inp["w_hh"].astype(np.float64))
    loss = 0
    for d in range(ndir):
        for m in range(M):
            h, cc = h0[d, m], c0[d, m]
            for step in range(int(lens[m])):
                t = step if d == 0 else int(lens[m]) - 1 - step
                a = gin[m, t, d * 4 * H:(d + 1) * 4 * H] + w[d] @ h
                i, f, g, o = torch.sigmoid(a[:H]), torch.sigmoid(a[H:2 * H]), torch.tanh(a[2 * H:3 * H]), torch.sigmoid(a[3 * H:])
                cc = f * cc + i * g
                h = o * torch.tanh(cc)
                loss = loss + (h * torch.tensor(_clean(inp["dout"])[m, t, d * H:(d + 1) * H])).sum() + (cc * torch.tensor(_clean(inp["dcst"])[m, t, d])).sum()
            loss = loss + (h * torch.tensor(inp["dhn"][d, m].astype(np.float64))).sum() + (cc * torch.tensor(inp["dcn"][d, m].astype(np.float64))).sum()
    loss.backward()
    bwd = B.bwd_eval(inp, saved=B.fwd_figures(inp)["ref"])
    close = lambda a, b: np.allclose(a, b.detach().numpy(), rtol=0, atol=1e-12)
    assert close(bwd["dgates"], gin.grad) and close(bwd["dh0"], h0.grad) and close(bwd["dc0"], c0.grad)
    for m in (1, 4):                                         # the contract of a length-0 row: zero gradients, the final-state gradient handed through
        assert not bwd["dgates"][m].any() and np.array_equal(bwd["dh0"][:, m], inp["dhn"][:, m]) and np.array_equal(bwd["dc0"][:, m], inp["dcn"][:, m])
        fwd = B.fwd_figures(inp)["ref"]
        assert not fwd["out"][m].any() and np.array_equal(fwd["hn"][:, m], inp["h0"][:, m]) and np.array_equal(fwd["cn"][:, m], inp["c0"][:, m])
    g = B.make("gru", "randn", 3, M, T, H, ndir, lengths=[T, 0, 1, 3, -2])
    gb = B.bwd_eval(g, saved=B.fwd_figures(g)["ref"])
    assert not gb["dgx"][1].any() and not gb["dq"][4].any() and gb["dgx"][0].all()


def test_forward_restatement_is_rnn_refs_recurrence():
    for cell in ("lstm", "gru"):
        inp = B.make(cell, "sat", 9, 5, 6, 11, 2, "ends")
        mine, theirs = B.fwd_figures(inp)["ref"], R.evaluate(inp)
        assert all(np.array_equal(mine[k], theirs[k]) for k in ("out", "hn")) and (cell == "gru" or np.array_equal(mine["cn"], theirs["cn"]))
        if cell == "lstm":
            assert np.array_equal(mine["cst"].reshape(theirs["cst"].shape), theirs["cst"])


# ------------------------------------------------------------------ honest fp32 evaluations pass on every input of the GPU tables
def _honest(inp, fwd):
    f = B.fwd_figures(inp) if fwd else B.bwd_figures(inp)
    ev = B.fwd_eval if fwd else B.bwd_eval
    worst = {}
    for name, kw in (("sequential", dict(order="seq")), ("quarters", dict(order="quad")), ("noise 1e-7", dict(noise=np.random.default_rng(inp["H"] + inp["T"])))):
        ok, r = B.accept(ev(inp, np.float32, **kw), f, margin=CAP)
        worst[name] = (ok, r["miss"], r["worst"])
    return worst


GROUPS = {"lstm_fwd": ("lstm_fwd", "lstm_split"), "gru_fwd": ("gru_fwd",), "lstm_bwd": ("lstm_bwd", "lstm_chain"), "gru_bwd": ("gru_bwd", "gru_chain")}


@pytest.mark.parametrize("group", list(GROUPS))
def test_criterion_accepts_honest_fp32_on_every_gpu_input(group):
    """the inputs of the GPU cases themselves (M beyond 40 cut to 33 sequences: the same H, T, family, lengths mode and arguments)"""
    seen, top = set(), (0.0, "")
    for d in E.ALL_CASES + [E.c(cell + "_bwd", E.LBM if cell == "lstm" else E.GBM, 17, 6, h) for cell, h, _ in E.CELL_IO]:
        if d["op"] not in GROUPS[group]:
            continue
        d = dict(d, M=min(d["M"], 33))
        key = (d["op"].split("_")[0], d["M"], d["T"], d["H"], d["fam"], d["ndir"], str(d["lens"]), d["reseed"], tuple(sorted(d["opt"].items())))
        if key in seen:
            continue
        seen.add(key)
        for name, (ok, miss, where) in _honest(E._make(d), "fwd" in group).items():
            assert ok, (d["id"], name, miss, where)
            top = max(top, (miss, "%s %s %s" % (d["id"], name, where)))
    print("%s: %d inputs, the closest honest evaluation is at %.2f of the bound (%s)" % (group, len(seen), top[0], top[1]))


def test_replaced_inputs_are_the_ones_an_honest_evaluation_fails_on():
    """the matrix-core LSTM BPTT sums dgates W_hh over 4H terms in one chain; so does the "sequential" fp32 evaluation, and at 4H >= 256 its dh0 can
    miss the bound at the cap by itself.  Those inputs carry a reseed: the first at which every honest evaluation stays
    within 0.8 of the bound -- decided here, on the CPU, from the fp32 evaluations alone."""
    moved = [d for d in E.ALL_CASES if d["reseed"]]
    assert len(moved) == 6 and all(d["kernel"] == E.LBM and d["H"] >= 64 for d in moved)
    for d in moved:
        for rs in range(d["reseed"] + 1):
            w = _honest(E._make(dict(d, reseed=rs)), False)
            miss = max(m for _, m, _ in w.values())
            print("%s reseed %d: %.2f of the bound" % (d["id"], rs, miss))
            assert (miss <= 0.8) == (rs == d["reseed"]) and (rs > 0 or miss > 1.0), (d["id"], rs, miss)


# ------------------------------------------------------------------ planted faults
FAULT_SHAPES = [(15, 6), (70, 9), (128, 8)]                 # (H, T)


@pytest.mark.parametrize("H,T", FAULT_SHAPES)
@pytest.mark.parametrize("fam", ["randn", "sat"])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_criterion_rejects_every_planted_fault(cell, fam, H, T):
    inp = B.make(cell, fam, H * 1000 + T, 7, T, H, 2, "ends")
    assert {0, 1, T} <= set(inp["lens"].tolist())
    f = B.bwd_figures(inp)
    assert B.accept(f["y32"], f, margin=1.0)[0]
    for mut in (B.LSTM_FAULTS if cell == "lstm" else B.GRU_BWD_FAULTS):
        if mut == "no_hi_units" and H <= 64:
            continue                                         # there are no units >= 64
        ok, r = B.accept(B.bwd_eval(inp, np.float32, mut=mut), f, margin=CAP)
        print("  %s %s H=%d fault %-14s %.3g x bound at %s, tail %d" % (cell, fam, H, mut, r["miss"], r["worst"], r["tail"]))
        assert not ok, (mut, r["miss"])
        if mut in B.PRECISION_FAULTS:
            assert r["miss"] >= 1.3, (mut, r["miss"])         # not a near miss
    if cell == "gru":
        ff = B.fwd_figures(inp)
        ok, r = B.accept(B.fwd_eval(inp, np.float32, mut="bhn_outside"), ff, margin=CAP)
        assert not ok and r["miss"] >= 1.3


def test_faults_show_without_a_length_zero_row_and_in_the_state_carry_families():
    """"last" / "remember" at T = 64: the gradient reaches the early steps through the recurrent path alone; every carry fault is rejected there too"""
    for cell in ("lstm", "gru"):
        for fam in ("last", "remember"):
            inp = B.make(cell, fam, 21, 5, 64, 33, 2, "mixed")
            f = B.bwd_figures(inp)
            faults = ("no_dhn", "dhn_at_T", "idle_overwrite", "b16") + (("no_dcn", "c_cur", "dc_no_f", "early_h0") if cell == "lstm" else ("no_direct", "h_cur", "dq_as_dan"))
            for mut in faults:
                ok, r = B.accept(B.bwd_eval(inp, np.float32, mut=mut), f, margin=CAP)
                print("  %s %s fault %-14s %.3g x bound" % (cell, fam, mut, r["miss"]))
                assert not ok, (cell, fam, mut, r["miss"])


def test_padded_tail_nan_and_the_scale_floor():
    inp = B.make("lstm", "randn", 2, 5, 6, 15, 2, "ends")
    f = B.bwd_figures(inp)
    g = {k: v.copy() for k, v in f["ref"].items()}
    assert B.accept(g, f, margin=1.0)[0]
    m = int(np.flatnonzero(inp["lens"] == 1)[0])
    g["dgates"][m, -1, 0] = 1e-30
    ok, r = B.accept(g, f, margin=CAP)
    assert not ok and r["tail"] == 1 and r["miss"] <= 1.0
    g = {k: v.copy() for k, v in f["ref"].items()}
    g["dh0"][1, 2, 3] = np.nan
    assert not B.accept(g, f, margin=CAP)[0]
    z = B.make("gru", "randn", 2, 5, 6, 15, 2, "ends", dhn=False, dout0=True)      # an all-zero result compares at 2^-23 absolute
    fz = B.bwd_figures(z)
    assert not fz["ref"]["dgx"].any()
    g = {k: v.copy() for k, v in fz["ref"].items()}
    g["dq"][0, 0, 0] = 3 * B.EPS
    assert B.accept(g, fz, margin=CAP)[0]
    g["dq"][0, 0, 0] = 5 * B.EPS
    assert not B.accept(g, fz, margin=CAP)[0]
    with pytest.raises(AssertionError):
        B.accept(g, fz, margin=8.0)


def test_margins_follow_the_rule():
    assert set(B.MARGIN) == set(B.RATIO) and all(1.0 <= m <= CAP == 4.0 for m in B.MARGIN.values())
    assert {B.family_of(d["kernel"]) for d in E.ALL_CASES} | {"cell"} == set(B.MARGIN)
    assert [B.margin_from(r) for r in (-1.0, 0.4, 0.51, 1.0, 1.01, 2.5, 40.0)] == [1.0, 1.0, 2.0, 2.0, 4.0, 4.0, 4.0]
    for fam, ratio in B.RATIO.items():
        assert B.MARGIN[fam] == B.margin_from(ratio), fam


# ------------------------------------------------------------------ the dispatchers
def test_restatement_matches_the_source():
    train, gru = open(os.path.join(CSRC, "train.hip")).read(), open(os.path.join(CSRC, "gru_train.hip")).read()
    cond = "H >= 16 && (hp == 32 || hp == 64 || hp == 72 || hp == 96 || hp == 128)"
    assert cond + " && (H % 2 == 0 || M >= 1024)" in train and cond.replace("H >= 16", "H >= 16 && H <= 128") in gru
    assert "(H % 2 == 0 || M >= 1024)) ? NIR_GRU_FORM_MFMA" in gru and "if (H >= 33) {" in train
    assert sorted(int(a) for a in re.findall(r"gru_bwd_mfma_launch<(\d+)>\(a, st\)", gru)) == sorted(B.BWD_HP)
    assert sorted(re.findall(r"lstm_train_bwd_mfma_kernel<(\d+(?:, 1)?)>", train)) == sorted(["32", "64", "72, 1", "96, 1", "128, 1"])
    assert [B.bwd_mfma_supported(h) for h in (15, 16, 28, 29, 32, 33, 60, 61, 64, 65, 68, 69, 72, 73, 92, 93, 96, 97, 124, 125, 128, 129)] == \
        [False, False, False, True, True, False, False, True, True, False, False, True, True, False, False, True, True, False, False, True, True, False]


def _predict(d):
    op, a = d["op"], (d["M"], d["T"], d["H"], d["ndir"])
    if op == "lstm_fwd":
        return B.predict_lstm_fwd(*a)
    if op == "lstm_split":
        return B.predict_lstm_split(*a)
    if op == "gru_fwd":
        return B.predict_gru_fwd(*a)
    return B.predict_lstm_bwd(*a) if op.startswith("lstm") else B.predict_gru_bwd(*a, form=d["form"])


def test_every_gpu_case_lands_on_the_kernel_it_names_and_every_edge_is_there():
    assert len({d["id"] for d in E.ALL_CASES}) == len(E.ALL_CASES)
    for d in E.ALL_CASES:
        p = _predict(d)
        assert p.kernel == d["kernel"], (d["id"], p)
        assert d["M"] <= 40 or (d["M"] in (1023, 1024) and d["T"] == 2), d["id"]
        assert d["T"] <= 9 or (d["T"] == 64 and d["M"] == 5 and d["fam"] in ("remember", "last")), d["id"]
    has = lambda op, kernel, **kw: any(d["op"] == op and d["kernel"] == kernel and all(d[k] == v for k, v in kw.items()) for d in E.ALL_CASES)
    for op, valu, mfma in (("lstm_bwd", E.LBV, E.LBM), ("gru_bwd", E.GBV, E.GBM)):
        for h in E.MFMA_H:                                   # inside: even H at M = 17, odd H from 1024 sequences on (LSTM: all; GRU: forced at 17 as well)
            assert has(op, mfma, H=h, M=17) or has(op, mfma, H=h, M=1024), (op, h)
            assert h % 2 == 0 or has(op, valu, H=h, M=17), (op, h)
        assert all(has(op, valu, H=h) for h in E.VALU_H)
        assert all(has(op, valu, H=h, M=1023) and has(op, mfma, H=h, M=1024) for h in (31, 127))
        for name in (k for k in E.REPS if k.startswith(op)):
            modes = {str(d["lens"]) for d in E.VARIANTS if name in d["id"].split("-")}
            assert modes >= {"None", "mixed", "ones", "zero", "over", "neg", "wg0", "ends"}, (name, modes)
    assert all(has("gru_bwd", E.GBM, H=h, form=B.GRU_MFMA) and has("gru_bwd", E.GBV, H=h, form=B.GRU_VALU) for h in E.MFMA_H)
    assert all(has("gru_bwd", E.GBM, H=h, fam=f) for h in (69, 70, 71, 72) for f in ("randn", "sat", "remember", "last"))
    assert all(has("lstm_fwd", E.LFV, H=h) for h in (1, 17, 32)) and all(has("lstm_split", E.LSP3 if h <= 96 else E.LSP4, H=h) for h in (65, 70, 96, 97, 128))
    for h in (33, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128):
        both = {d["opt"]["h0"] for d in E.FWD if d["op"] == "lstm_fwd" and d["H"] == h and d["kernel"] == E._g16(h)}
        assert both == {True, False}, h
    assert all(has("gru_fwd", E.GF, H=h) for h in (1, 32, 33, 64, 65, 96, 97, 128))
    for name, S in E.S_OF.items():
        ms = {d["M"] for d in E.VARIANTS if name in d["id"].split("-")}
        assert ms >= ({1, 4, 5} if S == 4 else {1, 15, 16, 17, 33}), (name, ms)
    assert {(cell, h): offs for cell, h, offs in E.CELL_IO} == {(cell, h): ((0, 2, 1) if h != 70 else (0, 1)) for cell in ("lstm", "gru") for h in (32, 64, 70, 128)}
    for fam in ("lstm_bwd_valu", "lstm_bwd_mfma", "gru_bwd_valu", "gru_bwd_mfma"):
        seen = {d["fam"] for d in E.ALL_CASES if B.family_of(d["kernel"]) == fam and d["op"].endswith("bwd")}
        assert {"randn", "sat", "remember", "last"} <= seen, (fam, seen)
