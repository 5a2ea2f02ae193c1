"""The acceptance criterion of the session models' beam search (csrc/beam.hip: nir_beam_cars_decode / nir_beam_plain_decode, CARS /
M_MATCH_TENSOR / MNSRF .decode_beam): the two decoders' steps restated in float64 (the reference) and float32 (the yardstick of what fp32
arithmetic costs), driven by beam_ref.search unchanged.  The semantics are those of DESIGN.md sections 21 and 23 (include/neuroir_beam.h,
include/neuroir_session_beam.h) with "source row" read as "decode row of the greedy decode":

    rows      Bd = B (S-1) source rows, R = Bd W beam rows, row = k Bd + i
    CARS      beam row r attends the memory bank and length of source row rowmap[r % Bd] and adds the session term of decode row r % Bd

The mathematics are oracle/neuroir_cpu.py's cars_decode and plain_greedy_decode, restated here for any dtype (the oracle's helpers go through
float32 state dicts and its own row bookkeeping).  `aux` of a step is a one-column dummy: these decoders export no attention.

Bound on the scores (beam_ref's): with s = max |ref64|, e = max |got - ref64| / s and e_chain the same figure for the float32 chain FORCED along
the float64 choices,

    e <= MARGIN * max(e_chain, 2^-23) + n_split * FMT["fp16x2"]

n_split = the split-fp16 products on the score's path per step, times max_len: 2 with the folded step and the fused generator, 1 with one of
them, 0 with neither.  MARGIN started at beam_ref.MARGIN (2) and moves only by the house rule (the largest ratio measured on the MI355X doubled,
rounded up to a power of two, never above gemm_ref.MARGIN_CAP): it is 4; the measured ratios are in DESIGN.md section 23.

`fault` plants beam_ref's model-independent mistakes (passed through to the search) or one that only the session layout can make:
    "wrong_source_row"  beam rows k > 0 attend the memory bank and length of source row r instead of rowmap[r % Bd]       (CARS)
    "sess_dropped"      the session term is added for beam 0 only                                                          (CARS, KS > 0)
"""
import functools
import json
import os

import torch

import beam_ref as BR
from conftest import GOLDEN, T, load_golden
from helpers import build_model, cpu_state_dict
from oracle import neuroir_cpu as O

EOS, BOS = BR.EOS, BR.BOS
# beam_ref.MARGIN (2) moved by the house rule: the largest ratios measured on the MI355X are 2.434 (the envelope's plain decoder, Bd 9 and 17,
# W = 1, max_len 1, both plain forms) and, on the fixtures, 1.377 (M_MATCH_TENSOR, W = 1) and 1.294 (CARS qoff), both plain forms -- doubled and
# rounded up to a power of two, never above gemm_ref.MARGIN_CAP: 4
MARGIN = 4.0
SESSION_FAULTS = ("wrong_source_row", "sess_dropped")
CARS_CFG = {"full": {}, "qoff": dict(query_session_off=True), "doff": dict(doc_session_off=True)}
CASES = [("cars", "full"), ("cars", "qoff"), ("cars", "doff"), ("mmt", ""), ("mnsrf", "")]
WIDE_CASES = [("cars", "full"), ("mnsrf", "")]                                          # the cases that also run W = 3 and W = 8
TABLE = "embedder.word_embeddings.make_embedding.emb_luts.0.weight"
PRED2 = "token_prob_predictor2.weight"
# the perturbation of the fixtures (tests/golden/generate_session_beam.py): the golden weights give flat token distributions
BIAS_NOISE = 0.5                                                                          # beam_ref.noisy_bias's, on generator.bias
CARS_NOISE = 1.5                 # on token_prob_predictor2.weight (no bias to add noise to): a logit spread (~2.8) at which the top 9 of 1600
CARS_EOS_LIFT = 4.0              # candidates keep gaps >= 1e-3 over 45 (row, step) pairs; the mean lift of the EOS logit that goes with it


def widths(kind, tag):
    return (1, 3, 4, 8) if (kind, tag) in WIDE_CASES else (1, 4)


def name(kind, tag):
    return kind + ("_" + tag if tag else "")


def seeds():
    """{"<case>": {"<W>": [seed, smallest gap]}}: tests/golden/session_beam_seeds.json"""
    return json.loads(open(os.path.join(GOLDEN, "session_beam_seeds.json")).read())


# ------------------------------------------------------------------ the cases: golden weights, states and greedy tokens
@functools.lru_cache(maxsize=None)
def load_case(kind, tag):
    """dict(kind, sd (float32 state dict, unmodified), dec_h, dec_c [Bd, H], lut, max_len, B, SD, V, greedy [Bd, max_len] and for CARS enc
    [rows_src, QL, DQ], lens [rows_src], session_cat [rows_src, KS] or None) -- read-only, shared"""
    if kind == "cars":
        g = load_golden("cars_decode")
        model = build_model("CARS", tgt_vocab_size=int(g["meta_vocab"]), **CARS_CFG[tag])
        sd = cpu_state_dict(model)
        q, ql = T(g["source_words"]), T(g["source_lens"])
        B, S, _ = q.shape
        _, enc = O.cars_encode(sd, q, ql)
        attns = [T(g[tag + "_" + n]) if (tag + "_" + n) in g else None for n in ("inner_q", "inner_d")]
        cat = [a for a in attns if a is not None]
        return dict(kind=kind, tag=tag, sd=sd, dec_h=T(g[tag + "_dec_h"])[0], dec_c=T(g[tag + "_dec_c"])[0], lut=T(g["tgt2src"]), max_len=int(g["max_len"]),
                    B=B, SD=S - 1, V=sd[TABLE].shape[0], greedy=T(g[tag + "_predictions"]).reshape(B * (S - 1), -1), enc=enc.float(), lens=ql.reshape(-1),
                    attns=attns, session_cat=torch.cat(cat, 2).reshape(B * S, -1) if cat else None, cfg=CARS_CFG[tag])
    g = load_golden("m_match_tensor" if kind == "mmt" else "mnsrf")
    sd = cpu_state_dict(build_model("M_MATCH_TENSOR" if kind == "mmt" else "MNSRF", tgt_vocab_size=int(g["tgt_vocab_size"])))
    B, S = g["source_words"].shape[:2]
    return dict(kind=kind, tag=tag, sd=sd, dec_h=T(g["dec_h"])[0], dec_c=T(g["dec_c"])[0], lut=T(g["tgt2src"]), max_len=int(g["max_len"]), B=B, SD=S - 1,
                V=sd[TABLE].shape[0], greedy=T(g["predictions"]).reshape(B * (S - 1), -1))


def _cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    g = x @ w_ih.t() + b_ih + h @ w_hh.t() + b_hh
    i, f, gg, o = g.chunk(4, 1)
    c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(gg)
    return torch.sigmoid(o) * torch.tanh(c), c


def model_step(cs, sd, dtype, fault=None, record=None):
    """(state0, step_fn) of a case with the state dict `sd` (the case's own or a perturbed copy); record: a list that collects every step's
    generator input (p1 for CARS, h for the plain decoders)"""
    sd = {k: v.to(dtype) for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
    table = sd[TABLE]
    p = [sd["decoder.decoder.rnn." + n + "_l0"] for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")]
    state0 = (cs["dec_h"].to(dtype), cs["dec_c"].to(dtype))
    Bd = state0[0].shape[0]
    if cs["kind"] != "cars":
        def step(state, tok):
            h, c = _cell(table[tok], state[0], state[1], *p)
            if record is not None:
                record.append(h)
            return (h, c), h @ sd["generator.weight"].t() + sd["generator.bias"], torch.zeros(tok.shape[0], 1, dtype=dtype)
        return state0, step
    B, SD = cs["B"], cs["SD"]
    rows_src = B * (SD + 1)
    i = torch.arange(Bd)
    rowmap = (i // SD) * (SD + 1) + i % SD                                              # the reference's [:, :-1] selection
    mem_all = cs["enc"].to(dtype) @ sd["dec_attn.weight"].t()                          # [rows_src, QL, HD]
    QL = mem_all.shape[1]
    sess = None
    if cs["session_cat"] is not None:
        wsum = sd["shared_session_projector.linear.weight"] + sd["private_session_projector2.linear.weight"]
        sess = cs["session_cat"].to(dtype)[rowmap] @ wsum.t()                          # [Bd, P]

    def step(state, tok):
        R = tok.shape[0]
        r = torch.arange(R)
        k = r // Bd
        src = rowmap[r % Bd]
        if fault == "wrong_source_row":
            src = torch.where(k > 0, r % rows_src, src)
        h, c = _cell(table[tok], state[0], state[1], *p)
        mem = mem_all[src]
        mask = torch.arange(QL).unsqueeze(0) < cs["lens"][src].unsqueeze(1)
        qv = h @ sd["decoder.decoder.attn.linear_in.weight"].t()
        align = torch.bmm(mem, qv.unsqueeze(2)).squeeze(2).masked_fill(~mask, float("-inf"))
        ctx = torch.bmm(torch.softmax(align, 1).unsqueeze(1), mem).squeeze(1)
        out = torch.tanh(torch.cat((ctx, h), 1) @ sd["decoder.decoder.attn.linear_out.weight"].t())
        p1 = out @ sd["token_prob_predictor1.weight"].t()
        if sess is not None:
            add = sess[r % Bd]
            if fault == "sess_dropped":
                add = torch.where((k == 0).unsqueeze(1), add, torch.zeros_like(add))
            p1 = p1 + add
        if record is not None:
            record.append(p1)
        return (h, c), p1 @ sd[PRED2].t(), torch.zeros(R, 1, dtype=dtype)
    return state0, step


@torch.no_grad()
def decode(cs, sd, W, dtype=torch.float64, fault=None, force=None, record=None):
    """beam-search decode of a case -> beam_ref.search's dict (predictions [Bd, W, max_len], scores, lengths, backptr, tokens, gaps, finished)"""
    state0, step = model_step(cs, sd, dtype, fault if fault in SESSION_FAULTS else None, record)
    out = BR.search(step, state0, state0[0].shape[0], W, cs["max_len"], cs["lut"], cs["V"], None if fault in SESSION_FAULTS else fault, force)
    out.pop("aux")
    return out


# ------------------------------------------------------------------ the perturbed fixtures
@functools.lru_cache(maxsize=None)
def eos_direction(kind, tag):
    """CARS: the float64 mean of p1 over the greedy fixture's rows and steps, scaled so that adding it to the EOS row of token_prob_predictor2
    lifts the mean EOS logit by 1"""
    cs = load_case(kind, tag)
    rec = []
    decode(cs, cs["sd"], 1, record=rec)
    m = torch.stack(rec).mean((0, 1))
    return m / float(m @ m)


def perturbed(kind, tag, W, seed=None):
    """the case's state dict with the fixture noise of width W (W = 1 shares the seed of W = 4): generator.bias as beam_ref.noisy_bias for the
    plain decoders; for CARS token_prob_predictor2.weight + CARS_NOISE noise(seed) and CARS_EOS_LIFT along eos_direction on the EOS row.  The same
    values on every machine (detinit, not torch.randn)."""
    from context_attentive_ir_amd.detinit import det_tensor
    cs = load_case(kind, tag)
    if seed is None:
        seed = seeds()[name(kind, tag)][str(4 if W == 1 else W)][0]
    sd = dict(cs["sd"])
    if kind == "cars":
        w = sd[PRED2].clone() + CARS_NOISE * det_tensor("session_beam.noise", sd[PRED2].shape, seed, scale=1.0)
        w[EOS] += (CARS_EOS_LIFT * eos_direction(kind, tag)).float()
        sd[PRED2] = w
    else:
        sd["generator.bias"] = BR.noisy_bias(sd["generator.bias"], seed)
    return sd


def conditions(cs, sd, ref, free, W):
    """beam_ref.conditions of a (case, W), plus -- where they apply -- that the fixture separates the two session faults at the margin's cap"""
    cond = BR.conditions(ref, free, W)
    if W == 4 and cs["kind"] == "cars":
        chain = decode(cs, sd, W, torch.float32, force=(ref["backptr"], ref["tokens"]))
        for f in SESSION_FAULTS:
            if f == "sess_dropped" and cs["session_cat"] is None:
                continue
            if f == "wrong_source_row" and cs["tag"] != "full":
                continue
            cond[f] = not accept_decode(decode(cs, sd, W, fault=f), ref, chain, 2 * cs["max_len"], margin=4.0)[0]
    return cond


def conditions_ok(cond, W):
    keys = ("gap", "f32") if W == 1 else ("gap", "f32", "eos", "mixed", "moved")
    return all(cond[k] for k in keys) and all(cond[f] for f in SESSION_FAULTS if f in cond)


# ------------------------------------------------------------------ the bound
def n_split(folded, fused, max_len):
    return (int(bool(folded)) + int(bool(fused))) * max_len


def accept_decode(got, ref, chain, nsplit, margin=None):
    """tokens, back-pointers (when given) and lengths exactly the float64 restatement's; scores inside the bound -> (ok, figures)"""
    cpu = lambda x: torch.as_tensor(x.cpu() if torch.is_tensor(x) else x)                  # noqa: E731
    shape = ref["predictions"].shape
    same = bool(torch.equal(cpu(got["predictions"]).long().reshape(shape), ref["predictions"]))
    same = same and bool(torch.equal(cpu(got["lengths"]).long().reshape(shape[:2]), ref["lengths"]))
    if got.get("backptr") is not None:
        same = same and bool(torch.equal(cpu(got["backptr"]).long(), ref["backptr"]))
    sc = cpu(got["scores"]).reshape(shape[:2])
    if not bool(torch.isfinite(sc).all()):
        return False, dict(same=same, scores="non-finite")
    ok, fig = BR.accept_scores(sc, ref["scores"], chain["scores"], nsplit, MARGIN if margin is None else margin)
    return same and ok, dict(same=same, scores=fig)
