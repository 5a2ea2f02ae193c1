"""The acceptance criterion of the CARS session tail (csrc/cars_session.hip: nir_cars_rank_session and its _shard / _rows / _pre /
query_side forms, nir_cars_click_max): a restatement of neuroir/multitask/cars.py:262-520 -- encode_clicks with the batch-wide mask
quirk, the two session LSTM chains, the cross attention over the session states keyed by the query, the maxout ranker, the inner pools
and the decoder-initialisation states -- the float64 reference, the fp32 yardstick, the bound and the case table the CPU and the GPU
test files share (tests/test_cars_session_host.py, tests/test_gpu_cars_session_envelope.py).

Reference and yardstick: oracle.neuroir_cpu.cars_encode_clicks / cars_session_full, called with float64 inputs (the reference) and
with float32 inputs (e_chain).  Two call forms live here and not in the oracle: m_groups (the B sessions are blocks with an m of their
own: the oracle is called per block with a one-row label matrix of m ones as labels_all) and the candidate slice (the ranker scores a
candidate against the session state alone, so the slice's scores are the matching columns of the full result).
`restate` is the same computation written out once more so that a mistake can be planted in it (fault=), its products can be summed
in another order (order="chunk": K in chunks of 8, one accumulator) and every tanh / sigmoid output can be shifted (shift=); with
none of the three it equals the oracle (asserted on the CPU).

Bound, per output (clicks, scores, dec_h, dec_c, inner_q, inner_d): the NaN pattern of `got` equals the reference's exactly, and on the
other entries, with s = max |ref64|, e = max |got - ref64| / s and e_chain the same figure for the float32 oracle,

    e <= MARGIN * max(e_chain, 2^-23) + n_split * FMT["fp16x2"] + act_term

n_split (n_split() below, derived from the dispatch code for the flags, fragments and sizes of the case): the products formed on
fp16 term pairs on the longest path to the output.
    click0   click_attn.0 GEMM [B S N, D] x [D, D]        rank_bounded bit 2, and the GEMM large enough for the split kernel
    wih      the hoisted x W_ih^T GEMM [B S, D] x [D, 4 HS]   bit 3, likewise (one per chain; the chains run side by side: counted once)
    rec      h W_hh^T of one session step                 both chains' fragments given, HS % 32 == 0, tunable exact_f32 off;
                                                          step 0 has no previous state: a path over states 1..k holds k - 1 of them
    mo0/mo1  ranknet layers 0 / 1 [B S NR, 4 D] / [., 256]    bits 0 / 1, likewise
  The U GEMM, the rank projection, ranknet layer 2, the inner-attention GEMMs and transform_hid / transform_cell never carry the
  bounded flag: never counted.  A GEMM takes a split kernel only when ceil(M / 128) ceil(N / 128) >= 96, N >= 96 and K >= 32
  (launch_linear_ex, csrc/gemm.hip); below that it runs on the fp32 MFMA whatever the bit says, and is not counted.
    clicks                      click0
    scores                      click0 [d_on] + wih + (S - 2) rec + mo0 + mo1       (step S-1 attends over states 0..S-1)
    dec_h, dec_c                click0 [d_on] + wih + (S - 2) rec                   (states 1..S-1)
    inner_q                     wih + (S - 1) rec                                   (states 1..S)
    inner_d                     click0 + wih + (S - 1) rec
act_term: the fast_tanh / fast_sigmoid evaluations, priced the way tests/rnn_ref.py and gemm_ref.act_term do: the larger deviation of
  the float64 restatement from itself under +DELTA and under -DELTA, divided by s, DELTA = 2e-7 (twice the ~1e-7 csrc/common.hpp
  documents).  Under DELTA every sigmoid and tanh output of the LSTM cells is shifted by DELTA (rnn_ref), and every logit of the three
  tanh-rowdot attention heads (click_attn, session_*_inner_attn: the tanh sits in the GEMM epilogue) by DELTA * sum |w3| (gemm_ref's
  figure for a row-dot output), with alternating sign along the softmax axis -- a shift common to all logits cancels in the softmax.
MARGIN: the rule's starting value is 2; then the largest (e - fmt - act_term) / max(e_chain, 2^-23) the GPU tests print on the MI355X,
  doubled, rounded up to a power of two, never above gemm_ref.MARGIN_CAP = 4.  Measured (DESIGN.md section 22 has the figures per
  output and kernel form): 2.31 on the scores of rows_all1_n3 (B = S = 1, three scores, e_chain below 2^-23: the three maxout GEMMs
  add all K products of an output into one fp32 accumulator, as gemm_ref's docstring describes for the fp32-MFMA kernels) -> the rule
  asks for 8, the cap holds: 4.  Every other output stays below 1.

`fault` plants one of ten mistakes (tests/test_cars_session_host.py shows which case rejects which):
    "clicked_only"              attend over the clicked candidates only (rank >= m dropped)
    "m_own_rows"                m from the call's own rows where labels_all / m_groups supply it
    "ties_reversed"             equal labels ranked by descending index
    "cross_no_zero_state"       the cross attention without the zero state's logit
    "doc_attn_keyed_by_click"   the document-session attention keyed by the click vector instead of the query
    "inner_with_zero_state"     the inner pools include the zero state
    "dec_session_major"         dec_h / dec_c rows in (session, step) order
    "no_priv1"                  W_priv1 left out of the rank projection
    "doc_chain_first_candidate" the document chain fed the first pooled candidate instead of the click pool
    "split_drop_cross"          h W_hh^T on fp16 term pairs with the h2' w1 cross term dropped (gemm_ref.emulate)
"""
import collections
import functools

import numpy as np
import torch
import torch.nn.functional as F

import gemm_ref
from oracle import neuroir_cpu as O

MARGIN = 4.0
EPS = gemm_ref.EPS
DELTA = 2e-7
OUTPUTS = ("clicks", "scores", "dec_h", "dec_c", "inner_q", "inner_d")
FAULTS = ("clicked_only", "m_own_rows", "ties_reversed", "cross_no_zero_state", "doc_attn_keyed_by_click", "inner_with_zero_state",
          "dec_session_major", "no_priv1", "doc_chain_first_candidate", "split_drop_cross")
SQ, SD = "session_query_encoder.encoder.rnns.0", "session_doc_encoder.encoder.rnns.0"
BIG = 40000.0
# rank_bounded bit -> the state-dict weights whose GEMM it switches
BIT_WEIGHTS = {0: ("ranknet._linear_layers.0.weight",), 1: ("ranknet._linear_layers.1.weight",), 2: ("click_attn.0.weight",),
               3: (SQ + ".weight_ih_l0", SD + ".weight_ih_l0")}


# ------------------------------------------------------------------ weights
def make_sd(D, HS, HDEC, seed, q_on=True, d_on=True):
    """a seeded float32 state dict under the reference's key names for free D / HS / HDEC; the ranknet stays 4D -> 512/2 -> 256/2 -> 2/2.
    The attention heads are scaled up so that no softmax is near-uniform: a wrong mask or key moves the result far beyond the bound."""
    g = torch.Generator().manual_seed(seed)
    nch = int(q_on) + int(d_on)

    def w(o, i, scale=1.0):
        return (torch.randn(o, i, generator=g, dtype=torch.float64) * scale / i ** 0.5).float()

    def b(o, scale=0.1):
        return (torch.randn(o, generator=g, dtype=torch.float64) * scale).float()

    sd = collections.OrderedDict()

    def mlp(p, n, head):
        sd[p + ".0.weight"], sd[p + ".0.bias"] = w(n, n, 2.0), b(n)
        sd[p + ".3.weight"], sd[p + ".3.bias"] = w(1, n, head), b(1)

    def lstm(p, i):
        sd[p + ".weight_ih_l0"], sd[p + ".weight_hh_l0"] = w(4 * HS, i), w(4 * HS, HS)
        sd[p + ".bias_ih_l0"], sd[p + ".bias_hh_l0"] = b(4 * HS), b(4 * HS)

    if d_on:
        mlp("click_attn", D, 6.0)
        sd["session_doc_attn.weight"], sd["session_doc_attn.bias"] = w(D, HS, 3.0), b(D)
        lstm(SD, D)
        mlp("session_doc_inner_attn", HS, 6.0)
    if q_on:
        sd["session_query_attn.weight"], sd["session_query_attn.bias"] = w(D, HS, 3.0), b(D)
        lstm(SQ, D)
        mlp("session_query_inner_attn", HS, 6.0)
    sd["q_projection.linear.weight"], sd["q_projection.linear.bias"] = w(D, D), b(D)
    if nch:
        sd["shared_session_projector.linear.weight"] = w(D, nch * HS)
        sd["private_session_projector1.linear.weight"] = w(D, nch * HS)
        sd["transform_hid.linear.weight"], sd["transform_hid.linear.bias"] = w(HDEC, nch * HS), b(HDEC)
        sd["transform_cell.linear.weight"], sd["transform_cell.linear.bias"] = w(HDEC, nch * HS), b(HDEC)
    for i, (o, k) in enumerate(((512, 4 * D), (256, 256), (2, 128))):
        sd["ranknet._linear_layers.%d.weight" % i], sd["ranknet._linear_layers.%d.bias" % i] = w(o, k), b(o)
    return sd


def _cast(sd, dt):
    return {k: v.to(dt) for k, v in sd.items()}


# ------------------------------------------------------------------ the restatement
def _m_rows(labels, labels_all, m_groups, spg, own):
    """the click count m of every (session, step) row of the call"""
    B, S, N = labels.shape
    count = (labels.reshape(B * S, N) != 0).sum(1)
    if m_groups is not None and not own:
        return torch.as_tensor(list(m_groups), dtype=torch.long).repeat_interleave(spg * S)
    if labels_all is not None and not own:
        return torch.full((B * S,), int((labels_all.reshape(-1, N) != 0).sum(1).max()), dtype=torch.long)
    return torch.full((B * S,), int(count.max()), dtype=torch.long)


@torch.no_grad()
def restate(sd, pooled_q, pooled_docs, labels, q_on=True, d_on=True, rank_on=True, labels_all=None, m_groups=None, spg=0, cols=None,
            dtype=torch.float64, fault=None, order="blas", shift=0.0):
    """-> dict over OUTPUTS (None where the switches leave an output out); cols = (n0, NR): the ranked candidate slice"""
    assert fault is None or fault in FAULTS, fault
    sd = _cast(sd, dtype)
    pq = pooled_q.to(dtype)
    docs = pooled_docs.to(dtype) if pooled_docs is not None else None
    B, S, D = pq.shape

    def lin(x, p, bias=True):
        w = sd[p + ".weight"] if p + ".weight" in sd else sd[p]
        if order == "blas":
            y = x @ w.t()
        else:
            y = torch.zeros(x.shape[:-1] + (w.shape[0],), dtype=dtype)
            for k in range(0, w.shape[1], 8):
                y = y + x[..., k:k + 8] @ w[:, k:k + 8].t()
        bb = sd.get(p + ".bias") if bias else None
        return y if bb is None else y + bb

    tanh = lambda x: torch.tanh(x) + shift
    sig = lambda x: torch.sigmoid(x) + shift

    def head(x, p):
        """Linear(n, 1) over tanh(Linear(n, n)) -> the logits of a softmax over dim 1.  The tanh runs in the GEMM epilogue (fast_tanh): a logit is
        priced like gemm_ref.act_term prices a row-dot output, shift * sum |w3|, with alternating sign along the softmax axis (a shift common
        to all logits would cancel in the softmax)"""
        lg = lin(torch.tanh(lin(x, p + ".0")), p + ".3").squeeze(2)
        if shift:
            sgn = 1.0 - 2.0 * (torch.arange(lg.shape[1]) % 2).to(dtype)
            lg = lg + shift * float(sd[p + ".3.weight"].abs().sum()) * sgn.unsqueeze(0)
        return lg
    out = dict.fromkeys(OUTPUTS)
    clicks = None
    if d_on:
        N = docs.shape[2]
        lab = labels.reshape(B * S, N)
        if fault == "ties_reversed":
            perm = (N - 1) - lab.flip(1).sort(dim=1, descending=True, stable=True)[1]
        else:
            perm = lab.sort(dim=1, descending=True, stable=True)[1]
        sdocs = torch.gather(docs.reshape(B * S, N, D), 1, perm.unsqueeze(2).expand(-1, -1, D))
        count = (lab != 0).sum(1)
        m = _m_rows(labels, labels_all, m_groups, spg, fault == "m_own_rows")
        rank = torch.arange(N).unsqueeze(0)
        keep = rank < count.unsqueeze(1)
        if fault != "clicked_only":
            keep = keep | (rank >= m.unsqueeze(1))
        a = head(sdocs, "click_attn")
        a = F.softmax(a.masked_fill(~keep, float("-inf")), 1)
        clicks = (sdocs * a.unsqueeze(2)).sum(1).view(B, S, D)
        out["clicks"] = clicks
    nch = int(q_on) + int(d_on)
    if not nch and not rank_on:
        return out

    def step(p, x, state):
        h, c = state
        if fault == "split_drop_cross":
            rec = torch.from_numpy(gemm_ref.emulate(h.float().numpy(), sd[p + ".weight_hh_l0"].float().numpy(), "fp16x2", drop="a2w1")).to(dtype)
        else:
            rec = lin(h, p + ".weight_hh_l0")
        g = lin(x, p + ".weight_ih_l0") + sd[p + ".bias_ih_l0"] + rec + sd[p + ".bias_hh_l0"]
        i, f, gg, o = g.chunk(4, 1)
        c = sig(f) * c + sig(i) * tanh(gg)
        return sig(o) * tanh(c), c

    def inner(p, states):
        st = torch.stack(states if fault == "inner_with_zero_state" else states[1:], 1)
        w = F.softmax(head(st, p), 1)
        return (st * w.unsqueeze(2)).sum(1)

    HS = sd[(SQ if q_on else SD) + ".weight_hh_l0"].shape[1] if nch else 0
    z = pq.new_zeros(B, HS)
    qs, ds, qstate, dstate = [z], [z], (z, z), (z, z)
    scores, hid, cell, inner_q, inner_d = [], [], [], [], []
    for t in range(S):
        qv = pq[:, t]

        def attend(states, p, key):
            st = torch.stack(states, 1)
            lg = (lin(st, p) * key.unsqueeze(1)).sum(2)
            if fault == "cross_no_zero_state":
                if t == 0:
                    return torch.zeros_like(z)
                st, lg = st[:, 1:], lg[:, 1:]
            return (st * F.softmax(lg, 1).unsqueeze(2)).sum(1)

        if rank_on:
            parts = []
            if q_on:
                parts.append(attend(qs, "session_query_attn", qv))
            if d_on:
                parts.append(attend(ds, "session_doc_attn", clicks[:, t] if fault == "doc_attn_keyed_by_click" else qv))
            qp = lin(qv, "q_projection.linear")
            if parts:
                sess = torch.cat(parts, 1)
                qp = qp + lin(sess, "shared_session_projector.linear")
                if fault != "no_priv1":
                    qp = qp + lin(sess, "private_session_projector1.linear")
            dx = docs[:, t] if cols is None else docs[:, t, cols[0]:cols[0] + cols[1]]
            qx = qp.unsqueeze(1).expand_as(dx)
            x = torch.cat((qx, dx, (qx - dx).abs(), qx * dx), 2)
            for i in range(3):
                x = lin(x, "ranknet._linear_layers.%d" % i)
                x = x.view(x.shape[:-1] + (x.shape[-1] // 2, 2)).max(-1)[0]
            scores.append(x.squeeze(2))
        hp, cp = [], []
        if q_on:
            qstate = step(SQ, qv, qstate)
            qs.append(qstate[0]); hp.append(qstate[0]); cp.append(qstate[1])
            inner_q.append(inner("session_query_inner_attn", qs))
        if d_on:
            dstate = step(SD, docs[:, t, 0] if fault == "doc_chain_first_candidate" else clicks[:, t], dstate)
            ds.append(dstate[0]); hp.append(dstate[0]); cp.append(dstate[1])
            inner_d.append(inner("session_doc_inner_attn", ds))
        if hp:
            hid.append(torch.cat(hp, 1)); cell.append(torch.cat(cp, 1))
    if scores:
        out["scores"] = torch.stack(scores, 1)
    if hid and S > 1:
        if fault == "dec_session_major":
            rows = lambda xs: torch.stack(xs[:-1], 1).reshape((S - 1) * B, -1)
        else:
            rows = lambda xs: torch.cat(xs[:-1], 0)
        out["dec_h"] = lin(rows(hid), "transform_hid.linear")
        out["dec_c"] = lin(rows(cell), "transform_cell.linear")
    if inner_q:
        out["inner_q"] = torch.stack(inner_q, 1)
    if inner_d:
        out["inner_d"] = torch.stack(inner_d, 1)
    return out


@torch.no_grad()
def oracle(sd, pooled_q, pooled_docs, labels, q_on=True, d_on=True, rank_on=True, labels_all=None, m_groups=None, spg=0, cols=None,
           dtype=torch.float64):
    """the same dict from oracle.neuroir_cpu in `dtype`: the float64 reference, the float32 yardstick"""
    sd = _cast(sd, dtype)
    pq = pooled_q.to(dtype)
    docs = pooled_docs.to(dtype) if pooled_docs is not None else None
    B, S, _ = pq.shape
    out = dict.fromkeys(OUTPUTS)
    clicks = None
    if d_on:
        if m_groups is not None:
            N = labels.shape[2]
            blocks = []
            for g, m in enumerate(m_groups):
                sl = slice(g * spg, (g + 1) * spg)
                one = torch.zeros(1, N)
                one[0, :m] = 1.0
                blocks.append(O.cars_encode_clicks(sd, docs[sl], labels[sl], one))
            clicks = torch.cat(blocks, 0)
        else:
            clicks = O.cars_encode_clicks(sd, docs, labels, labels_all)
        out["clicks"] = clicks
    if not (q_on or d_on or rank_on):
        return out
    scores, states, attns = O.cars_session_full(sd, pq, docs, clicks, q_on, d_on, rank_on, True)
    if scores is not None:
        out["scores"] = scores if cols is None else scores[:, :, cols[0]:cols[0] + cols[1]]
    if states is not None:
        out["dec_h"], out["dec_c"] = states[0].squeeze(0), states[1].squeeze(0)
    out["inner_q"], out["inner_d"] = attns
    return out


# ------------------------------------------------------------------ which products are split (csrc/gemm.hip, csrc/cars_session.hip)
def gemm_is_split(M, N, K, bounded, exact=False):
    """launch_linear_ex on a dense fp32 A: the fp16 two-term kernel runs iff the bounded flag is set and the GEMM takes the large-tile path"""
    return bool(bounded and not exact and K % 4 == 0 and N >= 96 and K >= 32 and -(-M // 128) * -(-N // 128) >= 96)


def steps_are_f16(c):
    """launch_lstm_step: the fp16-term form needs HS % 32 == 0, exact_f32 off and the fragment of EVERY chain that runs"""
    return c["HS"] % 32 == 0 and not c["exact"] and all(f for f, on in ((c["frag_q"], c["q_on"]), (c["frag_d"], c["d_on"])) if on)


def step_kernel(c):
    """the instantiation launch_lstm_step picks for the case, by name"""
    B, HS = c["B"], c["HS"]
    if steps_are_f16(c):
        return "lstm_step16_kernel<%s>" % ("4,4,2" if B >= 256 else "4,1,4" if B > 32 else "2,1,8" if B > 16 else "1,1,8")
    return "lstm_step_kernel<%s>" % ("4,2" if B >= 256 and HS % 8 == 0 else "4" if B > 32 else "2" if B > 16 else "1")


def products(c):
    """name -> 1 if that product of the case runs on fp16 term pairs else 0 (rec: per step with a previous state)"""
    B, S, N, D, HS = c["B"], c["S"], c["N"], c["D"], c["HS"]
    NR = c["cols"][1] if c["cols"] else N
    bits, ex = c["bits"], c["exact"]
    nch = int(c["q_on"]) + int(c["d_on"])
    return dict(click0=int(c["d_on"] and gemm_is_split(B * S * N, D, D, bits & 4, ex)),
                wih=int(nch > 0 and gemm_is_split(B * S, 4 * HS, D, bits & 8, ex)),
                rec=int(nch > 0 and steps_are_f16(c)),
                mo0=int(c["rank_on"] and gemm_is_split(B * S * NR, 512, 4 * D, bits & 1, ex)),
                mo1=int(c["rank_on"] and gemm_is_split(B * S * NR, 256, 256, bits & 2, ex)))


def n_split(c):
    """output -> the split products on its longest path (the table of the module docstring)"""
    p, S = products(c), c["S"]
    chain = p["click0"] + p["wih"]
    return dict(clicks=p["click0"], scores=chain + max(S - 2, 0) * p["rec"] + p["mo0"] + p["mo1"], dec_h=chain + max(S - 2, 0) * p["rec"],
                dec_c=chain + max(S - 2, 0) * p["rec"], inner_q=p["wih"] + (S - 1) * p["rec"], inner_d=chain + (S - 1) * p["rec"])


# ------------------------------------------------------------------ the criterion
def figures(got, ref, chain, nsplit, act):
    """dict(e, e_chain, s, extra, ratio, nan_equal) on the entries where the reference is not NaN"""
    got = got.detach().cpu().double() if torch.is_tensor(got) else torch.as_tensor(np.asarray(got)).double()
    ref, chain = ref.double(), chain.double()
    assert tuple(got.shape) == tuple(ref.shape), (tuple(got.shape), tuple(ref.shape))
    nan = torch.isnan(ref)
    same = bool(torch.equal(torch.isnan(got), nan)) and bool(torch.equal(torch.isnan(chain), nan))
    ok = ~nan & ~torch.isnan(got)
    s = float(ref[~nan].abs().max()) if bool((~nan).any()) else 1.0
    assert s > 0
    e = float((got - ref)[ok].abs().max()) / s if bool(ok.any()) else 0.0
    if not bool(torch.isfinite(got[ok]).all()):
        e = float("inf")
    e_chain = float((chain - ref)[~nan].abs().max()) / s if bool((~nan).any()) else 0.0
    extra = nsplit * gemm_ref.FMT["fp16x2"] + act
    return dict(e=e, e_chain=e_chain, s=s, extra=extra, ratio=(e - extra) / max(e_chain, EPS), nan_equal=same)


def accept(got, ref, chain, nsplit, act, margin=None):
    """(ok, figures): the criterion of the module docstring on one output"""
    margin = MARGIN if margin is None else margin
    assert margin <= gemm_ref.MARGIN_CAP
    r = figures(got, ref, chain, nsplit, act)
    r["bound"] = margin * max(r["e_chain"], EPS) + r["extra"]
    return r["nan_equal"] and r["e"] <= r["bound"], r


def accept_all(got, data, margin=None):
    """every output the case produces -> (ok, {output: figures}); got: dict over OUTPUTS"""
    ok, figs = True, {}
    for k in OUTPUTS:
        if data["ref"][k] is None:
            continue
        assert got.get(k) is not None, k
        o, figs[k] = accept(got[k], data["ref"][k], data["chain"][k], data["n_split"][k], data["act"][k], margin)
        ok = ok and o
    return ok, figs


# ------------------------------------------------------------------ the cases
def _case(name, B, S, N, D=64, HS=32, HDEC=32, q_on=True, d_on=True, rank_on=True, bits=15, frag_q=True, frag_d=True, exact=False,
          labels="graded", rows_all=0, m_groups=None, spg=0, cols=None, big=None, nan=False, seed=None):
    frag_q, frag_d = frag_q and HS % 32 == 0, frag_d and HS % 32 == 0         # no fragment exists for another HS
    return dict(name=name, B=B, S=S, N=N, D=D, HS=HS, HDEC=HDEC, q_on=q_on, d_on=d_on, rank_on=rank_on, bits=bits, frag_q=frag_q,
                frag_d=frag_d, exact=exact, labels=labels, rows_all=rows_all, m_groups=m_groups, spg=spg, cols=cols, big=big, nan=nan,
                seed=seed)


def _build_cases():
    cs = []
    # step dispatch: one case per instantiation and per side of every batch boundary, S = 3 so that two steps have a previous state
    for B, HS in ((1, 32), (16, 160), (16, 1056), (17, 160), (32, 1056), (33, 512), (65, 544), (255, 32), (256, 288), (257, 32)):
        cs.append(_case("step16_b%d_h%d" % (B, HS), B, 3, 3, HS=HS))
    for B, HS in ((1, 16), (16, 784), (17, 48), (32, 528), (33, 48), (255, 400), (256, 272), (257, 16)):
        cs.append(_case("step32_b%d_h%d" % (B, HS), B, 3, 3, HS=HS))
    cs.append(_case("step32_nofrag_b33_h64", 33, 3, 3, HS=64, frag_q=False, frag_d=False))
    cs.append(_case("step32_exact_b257_h64", 257, 3, 3, HS=64, exact=True))
    cs.append(_case("step32_mixed_b16_h64", 16, 3, 3, HS=64, frag_d=False))
    # operand formats: the one shape at which all four switched GEMMs take the split kernel
    opf = dict(D=128, HS=512, B=161, S=4, N=19)
    cs.append(_case("opf_all_bits", **opf))
    # (bit 1 promises that layer 0's OUTPUTS stay below 2^15, which a layer-0 weight of 40000 breaks: the bit-0 case clears both, as
    # the wrapper's host check does)
    for bit in range(4):
        cs.append(_case("opf_bit%d_clear_big" % bit, bits=15 & ~((1 << bit) | (2 if bit == 0 else 0)), big=bit, **opf))
    cs.append(_case("whh_out_of_range", 5, 3, 4, HS=64, frag_q=False, big="whh"))
    # click pooling: N on both sides of the two kernels' and of the 64-candidate rounds' boundaries
    for N in (1, 2, 63, 64, 65, 128, 129):
        cs.append(_case("pool_n%d" % N, 3, 2, N, labels="all" if N == 1 else "graded"))
    cs.append(_case("pool_n2048", 1, 2, 2048))
    for ra, (B, S) in ((1, (1, 1)), (63, (2, 2)), (64, (2, 2)), (65, (2, 2)), (129, (2, 2))):
        cs.append(_case("rows_all%d_n3" % ra, B, S, 3, rows_all=ra))
    cs.append(_case("rows_all65_n70", 2, 2, 70, rows_all=65))
    cs.append(_case("mgroups3", 3, 2, 5, m_groups=(1, 4, 2), spg=1))
    cs.append(_case("mgroups1", 3, 2, 5, m_groups=(3,), spg=3))
    cs.append(_case("mgroups2_n70", 4, 2, 70, m_groups=(9, 33), spg=2))
    for pat in ("none", "all", "graded"):
        cs.append(_case("labels_%s" % pat, 3, 3, 5, labels=pat))
    cs.append(_case("labels_nan_planted", 4, 3, 5, labels="nan", nan=True))
    cs.append(_case("labels_nan_planted_n70", 3, 2, 70, labels="nan", nan=True))
    # switches
    for q in (0, 1):
        for d in (0, 1):
            for r in (0, 1):
                if q or d or r:
                    cs.append(_case("switch_q%dd%dr%d" % (q, d, r), 3, 3, 4, q_on=bool(q), d_on=bool(d), rank_on=bool(r)))
    cs.append(_case("s1", 3, 1, 4))
    cs.append(_case("slice_nr1", 3, 3, 5, cols=(2, 1)))
    cs.append(_case("slice_nr5", 3, 3, 5, cols=(0, 5)))
    for i, c in enumerate(cs):
        if c["seed"] is None:
            c["seed"] = 1000 + 17 * i
    return collections.OrderedDict((c["name"], c) for c in cs)


CASES = _build_cases()


def make_labels(c, g):
    """labels [B,S,N] (and labels_all for a rows_all case).  No pattern but "nan" has a row without a click while m = N: "graded" leaves the
    last candidate of every row unclicked, so m <= N - 1."""
    B, S, N = c["B"], c["S"], c["N"]
    pat = "sparse" if (c["rows_all"] or c["m_groups"]) else c["labels"]
    if pat == "none":
        lab = torch.zeros(B, S, N)
    elif pat == "all":
        lab = torch.randint(1, 3, (B, S, N), generator=g).float()
    elif pat == "sparse":                                                  # at most one click a row: the batch-wide m comes from elsewhere
        lab = torch.zeros(B, S, N)
        for b in range(B):
            for s_ in range(S):
                if (b + s_) % 2 == 0:
                    lab[b, s_, (b + 2 * s_) % N] = 1.0 + (b % 2)
    else:
        lab = torch.randint(0, 4, (B, S, N), generator=g).float()          # graded 0..3 with ties
        if N > 1:
            lab[:, :, -1] = 0.0
        lab[0, 0, : max(N - 1, 1)] = torch.arange(max(N - 1, 1)).float() % 3 + 1.0          # m = N - 1 (1 at N = 1)
        if B * S > 1:
            lab[B - 1, S - 1] = 0.0                                        # a row without a click: only rank N - 1 is attended, a tie decides which
    if pat == "nan":
        lab[0, 0] = torch.arange(N).float() % 2 + 1.0                      # every candidate clicked: m = N
        lab[1] = torch.randint(0, 3, (S, N), generator=g).float()
        lab[1, :, 0] = 1.0
        lab[1, 0] = 0.0                                                    # session 1, step 0: no click -> all masked, NaN from there on
        lab[B - 1, :, 1] = 3.0
    lab_all = None
    if c["rows_all"]:
        extra = c["rows_all"] - B * S
        lab_all = lab.reshape(B * S, N)
        if extra > 0:
            more = torch.zeros(extra, N)
            more[-1, : N - 1 if N > 1 else 1] = 1.0                          # the batch-wide m sits in the LAST row of the wider matrix
            lab_all = torch.cat((lab_all, more), 0)
    return lab, lab_all


@functools.lru_cache(maxsize=None)
def build(name):
    """the inputs, the float64 reference, the float32 yardstick, act_term and n_split of a case; computed once per process, shared by every test"""
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    B, S, N, D = c["B"], c["S"], c["N"], c["D"]
    sd = make_sd(D, c["HS"], c["HDEC"], c["seed"] + 1, c["q_on"], c["d_on"])
    if c["big"] == "whh":
        sd[SQ + ".weight_hh_l0"][7, 3] = 32768.0
    elif c["big"] is not None:
        for i, k in enumerate(BIT_WEIGHTS[c["big"]]):
            sd[k][3 + i, 5] = BIG * (-1.0) ** i
    pq = (torch.rand(B, S, D, generator=g) * 2 - 1) * 0.95
    docs = (torch.rand(B, S, N, D, generator=g) * 2 - 1) * 0.95
    lab, lab_all = make_labels(c, g)
    kw = dict(q_on=c["q_on"], d_on=c["d_on"], rank_on=c["rank_on"], labels_all=lab_all, m_groups=c["m_groups"], spg=c["spg"], cols=c["cols"])
    ref = oracle(sd, pq, docs, lab, dtype=torch.float64, **kw)
    chain = oracle(sd, pq, docs, lab, dtype=torch.float32, **kw)
    r0 = restate(sd, pq, docs, lab, **kw)
    rp, rm = restate(sd, pq, docs, lab, shift=DELTA, **kw), restate(sd, pq, docs, lab, shift=-DELTA, **kw)
    act = {}
    for k in OUTPUTS:
        if ref[k] is None:
            act[k] = 0.0
            continue
        ok = ~torch.isnan(ref[k])
        s = float(ref[k][ok].abs().max())
        act[k] = max(float((rp[k] - r0[k])[ok].abs().max()), float((rm[k] - r0[k])[ok].abs().max())) / s
    return dict(case=c, sd=sd, pooled_q=pq, pooled_docs=docs, labels=lab, labels_all=lab_all, kw=kw, ref=ref, chain=chain, restated=r0,
                act=act, n_split=n_split(c))


# ------------------------------------------------------------------ the weights struct at the C ABI (GPU tests)
_FIELDS = dict(click0_w="click_attn.0.weight", click0_b="click_attn.0.bias", click3_w="click_attn.3.weight", click3_b="click_attn.3.bias",
               sq_attn_w="session_query_attn.weight", sq_attn_b="session_query_attn.bias", sd_attn_w="session_doc_attn.weight",
               sd_attn_b="session_doc_attn.bias", sq_wih=SQ + ".weight_ih_l0", sq_whh=SQ + ".weight_hh_l0", sq_bih=SQ + ".bias_ih_l0",
               sq_bhh=SQ + ".bias_hh_l0", sd_wih=SD + ".weight_ih_l0", sd_whh=SD + ".weight_hh_l0", sd_bih=SD + ".bias_ih_l0",
               sd_bhh=SD + ".bias_hh_l0", qproj_w="q_projection.linear.weight", qproj_b="q_projection.linear.bias",
               shared_w="shared_session_projector.linear.weight", priv1_w="private_session_projector1.linear.weight",
               mo0_w="ranknet._linear_layers.0.weight", mo0_b="ranknet._linear_layers.0.bias", mo1_w="ranknet._linear_layers.1.weight",
               mo1_b="ranknet._linear_layers.1.bias", mo2_w="ranknet._linear_layers.2.weight", mo2_b="ranknet._linear_layers.2.bias",
               sq_inner0_w="session_query_inner_attn.0.weight", sq_inner0_b="session_query_inner_attn.0.bias",
               sq_inner3_w="session_query_inner_attn.3.weight", sq_inner3_b="session_query_inner_attn.3.bias",
               sd_inner0_w="session_doc_inner_attn.0.weight", sd_inner0_b="session_doc_inner_attn.0.bias",
               sd_inner3_w="session_doc_inner_attn.3.weight", sd_inner3_b="session_doc_inner_attn.3.bias",
               th_w="transform_hid.linear.weight", th_b="transform_hid.linear.bias", tc_w="transform_cell.linear.weight",
               tc_b="transform_cell.linear.bias")


def pack_whh_frag(whh_dev, HS):
    """nir_lstm_step_pack_whh_frag -> (fragment tensor, flag word)"""
    from context_attentive_ir_amd import lib
    L = lib.load()
    nb = L.nir_lstm_step_whh_frag_bytes(HS)
    assert nb
    frag = torch.empty(nb, dtype=torch.uint8, device=whh_dev.device)
    flag = torch.zeros(1, dtype=torch.int32, device=whh_dev.device)
    lib.check(L.nir_lstm_step_pack_whh_frag(lib.ptr(whh_dev), HS, lib.ptr(frag), lib.ptr(flag), lib.stream()), "nir_lstm_step_pack_whh_frag")
    return frag, int(flag.item())


def device_weights(sd, c, device="cuda", q_on=None, d_on=None, rank_on=None, bits=None, frag_q=None, frag_d=None, pack=True):
    """(lib.CarsSessionWeights, the tensors it points into): every switch, every rank_bounded bit and either fragment under the caller's control
    (defaults: the case's); pack: run nir_cars_session_pack and set wrank / attn_ut"""
    from context_attentive_ir_amd import lib
    L = lib.load()
    pick = lambda v, k: c[k] if v is None else v
    q_on, d_on, rank_on, bits = pick(q_on, "q_on"), pick(d_on, "d_on"), pick(rank_on, "rank_on"), pick(bits, "bits")
    frag_q, frag_d = pick(frag_q, "frag_q"), pick(frag_d, "frag_d")
    keep = {f: sd[k].to(device).contiguous() for f, k in _FIELDS.items() if k in sd}
    w = lib.CarsSessionWeights()
    for f, t in keep.items():
        setattr(w, f, t.data_ptr())
    w.D, w.HS, w.HDEC = c["D"], c["HS"], c["HDEC"]
    w.q_on, w.d_on, w.rank_on, w.rank_bounded = int(q_on), int(d_on), int(rank_on), int(bits)
    for key, want, on in (("sq", frag_q, q_on), ("sd", frag_d, d_on)):
        if want and on:
            frag, flag = pack_whh_frag(keep[key + "_whh"], c["HS"])
            assert flag == 0, "W_hh outside the fp16 split's range"
            keep[key + "_whh_frag"] = frag
            setattr(w, key + "_whh_frag", frag.data_ptr())
    if pack and rank_on:
        na, nb = lib.C.c_size_t(0), lib.C.c_size_t(0)
        L.nir_cars_session_pack_floats(lib.C.byref(w), lib.C.byref(na), lib.C.byref(nb))
        keep["wrank"] = torch.empty(max(na.value, 1), device=device)
        keep["attn_ut"] = torch.empty(max(nb.value, 1), device=device)
        lib.check(L.nir_cars_session_pack(lib.C.byref(w), lib.ptr(keep["wrank"]), lib.ptr(keep["attn_ut"]), lib.stream()), "nir_cars_session_pack")
        w.wrank = keep["wrank"].data_ptr()
        w.attn_ut = keep["attn_ut"].data_ptr()
    return w, keep
