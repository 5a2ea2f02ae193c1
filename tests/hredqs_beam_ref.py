"""The acceptance criterion of the HredQS beam search (csrc/beam.hip: nir_beam_hredqs_decode, HredQS.decode_beam): the decoder step of
tests/hredqs_ref.py -- an LSTM without attention, then the generator with bias -- restated as a step function in float64 (the reference) and
float32 (the yardstick of what fp32 arithmetic costs) and driven by beam_ref.search unchanged.  The semantics are those of DESIGN.md sections
21, 23 and 25 (include/neuroir_hredqs_beam.h) with "source row" read as "decode row of the HredQS greedy decode":

    rows      Bd = B S source rows, one per session prefix, in (b, s) order; R = Bd W beam rows, row = k Bd + i
    pairing   source row i starts from the state of session step i // B of session i % B (hredqs_ref.paired), every beam of it alike

`aux` of a step is a one-column dummy: HredQS exports no attention.

Bound on the scores (beam_ref's): with s = max |ref64|, e = max |got - ref64| / s and e_chain the same figure for the float32 chain FORCED along
the float64 choices,

    e <= MARGIN * max(e_chain, 2^-23) + n_split * FMT["fp16x2"]

n_split = hredqs_ref.n_split(QL, S) (the split products on the path of the initial states: the query encoder and the session LSTM) plus, in the
fast form, 2 max_len (one recurrent and one generator split product per step).  MARGIN started at beam_ref.MARGIN (2) and moves only by the house
rule (the largest ratio measured on the MI355X doubled, rounded up to a power of two, never above gemm_ref.MARGIN_CAP): it is 4; the measured
ratios are in DESIGN.md section 25.

`fault` plants beam_ref's model-independent mistakes (passed through to the search) or the one only HredQS can make:
    "natural_pairing"   source row (b, s) starts from the state of step s of session b
"""
import functools
import json
import os

import torch

import beam_ref as BR
import hredqs_ref as H
from conftest import GOLDEN, T

EOS, BOS = BR.EOS, BR.BOS
# beam_ref.MARGIN (2) moved by the house rule: the largest ratios measured on the MI355X are 1.409 and 1.382 (the envelope's decode entry, B = S = 1,
# W = 8 and 3, max_len 1, plain form) and 1.170 (B = S = 3, W = 8, max_len 5, plain form); every fast-form and every fixture ratio is below zero --
# doubled and rounded up to a power of two, never above gemm_ref.MARGIN_CAP: 4
MARGIN = 4.0
CASES = H.CASES
WIDE_CASES = ("h64", "h1024")                    # the cases that also run W = 3 and W = 8
HREDQS_FAULTS = ("natural_pairing",)
SHORT_MAX_LEN = 4                                # the horizon of a (case, W) without a seed at the goldens' max_len


def widths(tag):
    return (1, 3, 4, 8) if tag in WIDE_CASES else (1, 4)


def seeds():
    """{"<case>": {"<W>": [seed, smallest gap, max_len]}}: tests/golden/hredqs_beam_seeds.json"""
    return json.loads(open(os.path.join(GOLDEN, "hredqs_beam_seeds.json")).read())


def case_w(all_seeds=None):
    """every (case, W) the fixtures hold: widths() without the pairs the seed search found nothing for (recorded as null)"""
    s = seeds() if all_seeds is None else all_seeds
    return [(t, W) for t in CASES for W in widths(t) if s[t].get(str(4 if W == 1 else W)) is not None]


@functools.lru_cache(maxsize=None)
def load_case(tag):
    """dict(tag, cfg, sd (float32 state dict, unmodified), src [B,S,QL], lens [B,S], lut, max_len, B, S, QL, V, VT, greedy [B,S,max_len]) --
    read-only, shared"""
    net, c, g = H.case(tag)
    sd = {k: v.detach().clone() for k, v in net.state_dict().items()}
    src = g["source_words"]
    return dict(tag=tag, cfg=c, sd=sd, src=src, lens=g["source_lens"], lut=T(g["tgt2src"]), max_len=int(g["max_len"]), B=c["B"], S=c["S"],
                QL=src.shape[2], V=sd[H.EMB].shape[0], VT=sd["generator.weight"].shape[0], greedy=T(g["predictions"]))


@functools.lru_cache(maxsize=None)
def _session_states(tag, dtype):
    """(h, c) of every session step of a case, [B, S, HS] each: they do not depend on the generator bias, the one tensor a fixture perturbs"""
    cs = load_case(tag)
    return H.session_steps(H._cast(cs["sd"], dtype), cs["src"], cs["lens"])


def model_step(cs, sd, dtype, fault=None):
    """(state0, step_fn) of a case with the state dict `sd` (the case's own or a copy with another generator.bias)"""
    sd = H._cast(sd, dtype)
    table = sd[H.EMB]
    p = H._lstm(sd, H.DEC)
    steps = _session_states(cs["tag"], dtype) if cs.get("whole", True) else H.session_steps(sd, cs["src"], cs["lens"])
    state0 = H.paired(*steps, fault="natural_pairing" if fault == "natural_pairing" else None)

    def step(state, tok):
        h, c = H._cell(table[tok], state[0], state[1], *p)
        return (h, c), h @ sd["generator.weight"].t() + sd["generator.bias"], torch.zeros(tok.shape[0], 1, dtype=dtype)
    return state0, step


@torch.no_grad()
def decode(cs, sd, W, dtype=torch.float64, fault=None, force=None, max_len=None):
    """beam-search decode of a case -> beam_ref.search's dict (predictions [Bd, W, max_len], scores, lengths, backptr, tokens, gaps, finished)"""
    state0, step = model_step(cs, sd, dtype, fault if fault in HREDQS_FAULTS else None)
    out = BR.search(step, state0, state0[0].shape[0], W, cs["max_len"] if max_len is None else max_len, cs["lut"], cs["V"],
                    None if fault in HREDQS_FAULTS else fault, force)
    out.pop("aux")
    return out


def perturbed(tag, W, seed=None):
    """the case's state dict with generator.bias = beam_ref.noisy_bias(bias, seed) of width W (W = 1 shares the seed of W = 4)"""
    cs = load_case(tag)
    if seed is None:
        seed = seeds()[tag][str(4 if W == 1 else W)][0]
    sd = dict(cs["sd"])
    sd["generator.bias"] = BR.noisy_bias(sd["generator.bias"], seed)
    return sd


def sub_case(tag, b=None, s=None):
    """the case cut down to session b (B = 1) and / or query s (S = 1): a batch of its own, with its own session states and pairing"""
    cs = dict(load_case(tag), whole=False)
    src, lens = cs["src"], cs["lens"]
    if b is not None:
        src, lens = src[b:b + 1], lens[b:b + 1]
    if s is not None:
        src, lens = src[:, s:s + 1], lens[:, s:s + 1]
    cs.update(src=src.contiguous(), lens=lens.contiguous(), B=src.shape[0], S=src.shape[1])
    return cs


def fixture_max_len(tag, W):
    return int(seeds()[tag][str(4 if W == 1 else W)][2])


def conditions_ok(cond, W):
    keys = ("gap", "f32") if W == 1 else ("gap", "f32", "eos", "mixed", "moved")
    return all(cond[k] for k in keys)


# ------------------------------------------------------------------ the bound
def n_split(QL, S, fast, max_len):
    return H.n_split(QL, S) + (2 * max_len if fast else 0)


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
