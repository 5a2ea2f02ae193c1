"""The acceptance criterion of the train-mode GRU / stacked encoders (csrc/gru_train.hip, autograd._BiGRU / _GRUSeq, RNNEncoder.forward_train): a
restatement of neuroir/encoders/rnn_encoder.py:62-141 with rnn_type = 'GRU' -- a stack of packed-sequence torch.nn.GRU layers (gate order
r, z, n; b_hn inside the reset product), dropout in front of every layer but the first -- in float64 (the reference) or float32 (the yardstick of
what fp32 arithmetic costs), forward AND a manual backward through time, no autograd:

    r = sigma(gx_r + gh_r)   z = sigma(gx_z + gh_z)   q = gh_n   n = tanh(gx_n + r q)   h_t = (1 - z) n + z h_{t-1}
    dn = dh (1 - z)   dz = dh (h_{t-1} - n)   da_n = dn (1 - n^2)   da_r = da_n q r (1 - r)   da_z = dz z (1 - z)   dq = da_n r
    dgx = (da_r, da_z, da_n)   dgh = (da_r, da_z, dq)   dh_{t-1} = z dh + dgh W_hh

Packed semantics: steps at t >= length do not run, the bank and every gradient are zero there, the reverse direction starts at t = length - 1.

Bars (the project's own, tests/test_gpu_train.py): outputs 2e-5 relative to the largest entry, gradients 1e-4 relative to the largest entry with a
floor of 1e-5 on the scale.

`fault` plants one of six mistakes, to show on the CPU that the bars reject them (tests/test_rnn_train_host.py):
    "bhn_outside"  b_hn added outside the reset product (the LSTM habit: biases summed in front)
    "dq_as_dan"    the n rows of dW_hh / db_hh and of dh_{t-1} taken from da_n instead of r da_n
    "no_direct"    the z dh path into dh_{t-1} dropped
    "h_cur"        dz computed with h_t instead of h_{t-1}
    "past_len"     BPTT runs over t >= length (over the unwritten -- zero -- activations there)
    "rev_start"    the reverse direction starts at T - 1 instead of length - 1
"""
import numpy as np
import torch

FAULTS = ("bhn_outside", "dq_as_dan", "no_direct", "h_cur", "past_len", "rev_start")
OUT_TOL, GRAD_TOL, FLOOR = 2e-5, 1e-4, 1e-5
PNAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

# (H, I, M, T, bidirectional) of tests/test_gpu_rnn_train.py::test_bigru_backward and the streaming form
SHAPES = [(1, 4, 2, 3, True), (15, 40, 7, 6, True), (70, 40, 33, 20, True), (65, 24, 18, 5, True), (128, 64, 3, 64, True),
          (128, 40, 17, 9, False), (96, 132, 300, 30, False)]
SEQ_SHAPES = [(200, 24, 20, 5, True), (256, 16, 37, 6, True)]
FAULT_SHAPE = (15, 40, 7, 6, True)


def rel_err(got, ref, floor=FLOOR):
    a = got.detach().double().cpu().numpy() if torch.is_tensor(got) else np.asarray(got, np.float64)
    b = ref.detach().double().cpu().numpy() if torch.is_tensor(ref) else np.asarray(ref, np.float64)
    return float(np.abs(a - b).max()) / max(float(np.abs(b).max()), floor) if b.size else 0.0


def make_case(H, I, M, T, bi, nlayers=1, seed=0, dtype=torch.float64, gates=3, use_last=True):
    """seeded inputs: per-layer parameters (gates = 3: GRU, 4: LSTM; uniform +-1/sqrt(H), torch's own init range), x, lengths in 1..T with one row
    at T and one at 1, and the bank's incoming gradient"""
    g = torch.Generator().manual_seed(1000 * H + 10 * M + T + seed)
    nd = 2 if bi else 1
    k = 1.0 / max(H, 1) ** 0.5
    layers = []
    for li in range(nlayers):
        isz = I if li == 0 else nd * H
        p = {}
        for sfx in (["", "_reverse"] if bi else [""]):
            for n, shp in zip(PNAMES, ((gates * H, isz), (gates * H, H), (gates * H,), (gates * H,))):
                p[n + sfx] = ((torch.rand(*shp, generator=g, dtype=torch.float64) * 2 - 1) * k).to(dtype)
        layers.append(p)
    x = torch.randn(M, T, I, generator=g, dtype=torch.float64).to(dtype)
    lens = torch.randint(1, T + 1, (M,), generator=g)
    lens[0] = T
    lens[-1] = 1
    dout = torch.randn(M, T, nd * H * (1 if use_last else nlayers), generator=g, dtype=torch.float64).to(dtype)
    return layers, x, lens, dout


def _sig(a):
    return 1.0 / (1.0 + torch.exp(-a))


def _position(lens, T, step, reverse, fault):
    """(position t of recurrence step `step`, clamped; rows that run it in the forward; rows whose step the backward visits)"""
    if not reverse:
        t = torch.full_like(lens, step)
        on = t < lens
        return t, on, (torch.ones_like(on) if fault == "past_len" else on)
    if fault == "rev_start":                       # from T - 1 over the padding: the state is no longer zero at t = length - 1
        t = torch.full_like(lens, T - 1 - step)
        return t, torch.ones_like(t, dtype=torch.bool), t < lens
    t = lens - 1 - step
    return t.clamp(min=0), t >= 0, t >= 0


def _dir_forward(x, lens, wih, whh, bih, bhh, reverse, fault):
    """-> (bank [M,T,H] zero past the length, act [M,T,4H] = (r, z, n, q), h_{t-1} as every step saw it [M,T,H])"""
    M, T, _ = x.shape
    H = whh.shape[1]
    out, act, hprev = x.new_zeros(M, T, H), x.new_zeros(M, T, 4 * H), x.new_zeros(M, T, H)
    gx = x @ wih.t() + bih
    h = x.new_zeros(M, H)
    rows = torch.arange(M)
    outside = fault == "bhn_outside"
    for step in range(T):
        t, on, _ = _position(lens, T, step, reverse, fault)
        g = gx[rows, t]
        gh = h @ whh.t() + bhh
        r, z = _sig(g[:, :H] + gh[:, :H]), _sig(g[:, H:2 * H] + gh[:, H:2 * H])
        q = gh[:, 2 * H:]
        n = torch.tanh(g[:, 2 * H:] + (r * (q - bhh[2 * H:]) + bhh[2 * H:] if outside else r * q))
        h2 = (1 - z) * n + z * h
        out[rows[on], t[on]] = h2[on]
        act[rows[on], t[on]] = torch.cat((r, z, n, q), 1)[on]
        hprev[rows[on], t[on]] = h[on]
        h = torch.where(on.unsqueeze(1), h2, h)
    keep = torch.arange(T).view(1, T) < lens.view(M, 1)
    return out * keep.unsqueeze(2).to(out.dtype), act, hprev


def _dir_backward(dout, x, lens, wih, whh, saved, reverse, fault):
    out, act, hprev = saved
    M, T, H = out.shape
    dgx, dgh = x.new_zeros(M, T, 3 * H), x.new_zeros(M, T, 3 * H)
    dh = x.new_zeros(M, H)
    rows = torch.arange(M)
    for step in range(T - 1, -1, -1):
        t, _, on = _position(lens, T, step, reverse, fault)
        a = act[rows, t]
        r, z, n, q = a[:, :H], a[:, H:2 * H], a[:, 2 * H:3 * H], a[:, 3 * H:]
        hp = out[rows, t] if fault == "h_cur" else hprev[rows, t]
        d = dout[rows, t] + dh
        dan = d * (1 - z) * (1 - n * n)
        da_r = dan * q * r * (1 - r)
        da_z = d * (hp - n) * z * (1 - z)
        dq = dan if fault == "dq_as_dan" else dan * r
        gxs, ghs = torch.cat((da_r, da_z, dan), 1), torch.cat((da_r, da_z, dq), 1)
        dgx[rows[on], t[on]] = gxs[on]
        dgh[rows[on], t[on]] = ghs[on]
        nxt = ghs @ whh + (0.0 if fault == "no_direct" else d * z)
        dh = torch.where(on.unsqueeze(1), nxt, dh)
    g2, h2 = dgx.reshape(M * T, -1), dgh.reshape(M * T, -1)
    grads = dict(weight_ih_l0=g2.t() @ x.reshape(M * T, -1), bias_ih_l0=g2.sum(0), weight_hh_l0=h2.t() @ hprev.reshape(M * T, H), bias_hh_l0=h2.sum(0))
    return dgx @ wih, grads


def gru_stack(layers, x, lens, dout, bi, masks=None, p_drop=0.0, use_last=True, fault=None):
    """Forward and manual backward of the layer stack in x's dtype.  masks: per layer i > 0 a keep mask [M,T,width] (inverted dropout: the layer
    reads bank * keep / (1 - p_drop)); None = no dropout.  dout: gradient of the returned bank.  -> (bank, dx, [per-layer {name: grad}])"""
    sfxs = ["", "_reverse"] if bi else [""]
    saved, banks, inputs = [], [], []
    cur = x
    for li, p in enumerate(layers):
        if li > 0 and masks is not None and masks[li] is not None:
            cur = cur * masks[li].to(cur.dtype) / (1.0 - p_drop)
        inputs.append(cur)
        per_dir = [_dir_forward(cur, lens, *(p[n + s] for n in PNAMES), reverse=bool(s), fault=fault) for s in sfxs]
        saved.append(per_dir)
        cur = torch.cat([d[0] for d in per_dir], 2)
        banks.append(cur)
    bank = banks[-1] if use_last or len(banks) == 1 else torch.cat(banks, 2)
    H = layers[0]["weight_hh_l0"].shape[1]
    W = len(sfxs) * H
    grads = [None] * len(layers)
    d = None
    for li in range(len(layers) - 1, -1, -1):
        dl = dout[:, :, -W:] if li == len(layers) - 1 else (dout[:, :, li * W:(li + 1) * W] if not use_last else None)
        d = dl if d is None else (d if dl is None else d + dl)
        p = layers[li]
        dx = 0
        g = {}
        for di, s in enumerate(sfxs):
            dxi, gi = _dir_backward(d[:, :, di * H:(di + 1) * H], inputs[li], lens, p["weight_ih_l0" + s], p["weight_hh_l0" + s], saved[li][di], bool(s), fault)
            dx = dx + dxi
            g.update({k + s: v for k, v in gi.items()})
        grads[li] = g
        d = dx
        if li > 0 and masks is not None and masks[li] is not None:
            d = d * masks[li].to(d.dtype) / (1.0 - p_drop)
    return bank, d, grads


def torch_stack(layers, x, lens, dout, bi, cell="GRU", masks=None, p_drop=0.0, use_last=True):
    """the same stack as torch.nn.GRU / nn.LSTM modules over pack_padded_sequence under torch autograd, in x's dtype (masks as in gru_stack)
    -> (bank, dx, [per-layer grads])"""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    xr = x.clone().requires_grad_(True)
    mods, banks = [], []
    cur = xr
    for li, p in enumerate(layers):
        if li > 0 and masks is not None and masks[li] is not None:
            cur = cur * masks[li].to(cur.dtype) / (1.0 - p_drop)
        H, isz = p["weight_hh_l0"].shape[1], p["weight_ih_l0"].shape[1]
        m = getattr(torch.nn, cell)(isz, H, 1, bidirectional=bi, batch_first=True).to(x.dtype)
        m.load_state_dict(p)
        mods.append(m)
        pk = pack_padded_sequence(cur, lens.tolist(), batch_first=True, enforce_sorted=False)
        cur = pad_packed_sequence(m(pk)[0], batch_first=True, total_length=x.shape[1])[0]
        banks.append(cur)
    bank = banks[-1] if use_last or len(banks) == 1 else torch.cat(banks, 2)
    bank.backward(dout)
    return bank.detach(), xr.grad, [{k: v.grad for k, v in m.named_parameters()} for m in mods]


def figures(got, ref):
    """(bank error, dx error, worst parameter-gradient error) of a (bank, dx, grads) triple against another"""
    worst = max(rel_err(got[2][li][k], ref[2][li][k]) for li in range(len(ref[2])) for k in ref[2][li])
    return rel_err(got[0], ref[0]), rel_err(got[1], ref[1]), worst


def accept(got, ref):
    fo, fx, fp = figures(got, ref)
    return fo <= OUT_TOL and fx <= GRAD_TOL and fp <= GRAD_TOL, (fo, fx, fp)
