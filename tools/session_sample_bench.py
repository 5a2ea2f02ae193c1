"""decode_sample of HredQS and the session models (csrc/session_sample.hip): the fused form against the entry's own plain
form, against decode_beam and against the greedy decode of the same rows.

Shapes: HredQS at tools/hredqs_bench.py's -- nhid_session 1024, emsize 300, vocabularies of 30 000, max_len 10, S = 4, --hq_batch sessions
(16: Bd = 64 prefixes), random states in (-1, 1), the C entries driven directly as there; CARS and MNSRF at tools/session_beam_bench.py's --
16 sessions of 7 queries (Bd = 96 decode rows), q_len 4, a source vocabulary of 100 000, the default target vocabulary and max_query_len --
with the decoder's inputs taken once from the wrapper's ranking pass, so that the timed region is the decode alone.
N in --N samples per decode row, top_k in {0, --top_k}.  Per (model, N, top_k):

    fused    decode_sample with the fused generator forced on at every row count (`fuse_sample_max_rows` lifted; HredQS: the fast form, which
             draws on the split state)
    plain    the entry's own plain form (`fuse_generator_argmax` / `fuse_generator_topk` = False; HredQS: the weights without packs)
    beam     decode_beam at W = min(N, 8)
    greedy   the greedy decode of the same R = Bd N rows: the greedy entry handed R rows (the batch repeated N times)
Device events around one whole call, eager; --warmup calls, then the median of --iters, in --rounds alternating rounds; the medians of the
rounds and their spread are reported, and whether the faster of fused / plain wins by more than both spreads.

    python tools/session_sample_bench.py [--models HREDQS,CARS,MNSRF] [--N 4,8,12] [--top_k 4] [--iters 10] [--warmup 3] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from dssm_bench import timed  # noqa: E402


def report(model, shape, N, top_k, t, toks):
    med = {k: float(np.median(v)) for k, v in t.items()}
    best, other = ("fused", "plain") if med["fused"] <= med["plain"] else ("plain", "fused")
    return dict(model=model, N=N, top_k=top_k, beam_width=min(N, 8), **shape, ms={k: round(v, 4) for k, v in med.items()},
                spread_ms={k: round(float(max(v) - min(v)), 4) for k, v in t.items()}, ms_rounds={k: [round(x, 4) for x in v] for k, v in t.items()},
                faster_form=best, faster_wins_outside_spread=bool(max(t[best]) < min(t[other])),
                tokens_equal_fused_plain=float((toks["fused"] == toks["plain"]).float().mean()))


def hredqs(a, emit):
    from context_attentive_ir_amd import lib
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.constants import BOS
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.multitask import suggest
    from context_attentive_ir_amd.recommender import HredQS
    L, dev = lib.load(), "cuda"
    H, VT, E, V, S, ml = 1024, 30000, 300, 30000, 4, 10
    net = HredQS(default_args("HREDQS", emsize=E, nhid=64, nhid_session=H, bidirection=False, src_vocab_size=V, tgt_vocab_size=VT))
    fill_module_(net, 1013)
    net = net.to(dev).eval()
    w = net._decoder_weights()
    assert w.struct.gen_frag and w.struct.rnn_whh_frag and w.struct.rnn_gate_fold, "the fast form's packs were not built"
    net.fast_decode = False
    wp = net._decoder_weights()                                         # the same weights without packs: the entry's plain form
    table = net.embedder.word_embeddings.table.detach().float().contiguous()
    g = torch.Generator().manual_seed(7)
    lut = torch.randint(4, V, (VT,), generator=g).to(dev)
    B = a.hq_batch
    Bd = B * S
    for N in a.Ns:
        R, W = Bd * N, min(N, 8)
        hs, cs = ((torch.rand(B * N, S, H, generator=g) * 2 - 1).to(dev) for _ in range(2))      # B N sessions: the greedy decode's R rows
        for top_k in (0, a.top_k):
            out = suggest.sample_outputs(Bd, N, ml, dev)
            bout = suggest.beam_outputs(Bd, W, ml, dev, False)
            gpred = torch.empty(R, ml, dtype=torch.int64, device=dev)
            ws = {f: torch.empty(L.nir_sample_hredqs_decode_workspace_bytes(B, S, N, top_k, ml, x.ref()), dtype=torch.uint8, device=dev)
                  for f, x in (("fused", w), ("plain", wp))}
            ws_b = torch.empty(L.nir_beam_hredqs_decode_workspace_bytes(B, S, W, ml, w.ref()), dtype=torch.uint8, device=dev)
            ws_g = torch.empty(L.nir_hredqs_decode_workspace_bytes(B * N, S, ml, w.ref()), dtype=torch.uint8, device=dev)

            def sample(form):
                x = w if form == "fused" else wp
                lib.check(L.nir_sample_hredqs_decode(lib.ptr(hs), lib.ptr(cs), B, S, lib.ptr(table), V, E, lib.ptr(lut), BOS, ml, x.ref(), N, top_k, 1.0, 7,
                                                     lib.ptr(ws[form]), ws[form].numel(), lib.ptr(out["predictions"]), lib.ptr(out["token_logprobs"]),
                                                     lib.ptr(out["scores"]), lib.ptr(out["lengths"]), lib.stream()), "nir_sample_hredqs_decode")
                return out["predictions"]

            def beam():
                lib.check(L.nir_beam_hredqs_decode(lib.ptr(hs), lib.ptr(cs), B, S, lib.ptr(table), V, E, lib.ptr(lut), BOS, ml, w.ref(), W, lib.ptr(ws_b),
                                                   ws_b.numel(), lib.ptr(bout["predictions"]), lib.ptr(bout["scores"]), lib.ptr(bout["lengths"]), None,
                                                   lib.stream()), "nir_beam_hredqs_decode")

            def greedy():
                lib.check(L.nir_hredqs_decode_greedy(lib.ptr(hs), lib.ptr(cs), B * N, S, lib.ptr(table), V, E, lib.ptr(lut), BOS, ml, w.ref(), lib.ptr(ws_g),
                                                     ws_g.numel(), lib.ptr(gpred), lib.stream()), "nir_hredqs_decode_greedy")

            t = {k: [] for k in ("fused", "plain", "beam", "greedy")}
            toks = {}
            for _ in range(max(1, a.rounds)):                    # the paths alternate, so that drift of the machine meets all of them
                t["fused"].append(timed(lambda: sample("fused"), a.iters, a.warmup))
                toks["fused"] = sample("fused").clone()
                t["beam"].append(timed(beam, a.iters, a.warmup))
                t["greedy"].append(timed(greedy, a.iters, a.warmup))
                t["plain"].append(timed(lambda: sample("plain"), a.iters, a.warmup))
                toks["plain"] = sample("plain").clone()
            emit(report("hredqs_sample", dict(decode_rows=Bd, rows=R, H=H, VT=VT, max_len=ml), N, top_k, t, toks))


def session(kind, a, emit):
    from context_attentive_ir_amd import synth
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import Multitask
    batch, sess = 16, 7
    ex = {k: v.cuda() for k, v in synth.session_batch(batch, sess, 10, 4, 64, 100000, 1013).items()}
    w = Multitask(default_args(kind, src_vocab_size=100000))
    fill_module_(w.network, 1013)
    w.cuda()
    w.id_check_interval = 0
    net = w.network.eval()
    net.fuse_sample_max_rows = net.fuse_topk_max_rows = 1 << 30          # `fused` is the fused form at every row count: the cap is what is being measured
    ml, SD = int(w.args.max_query_len), sess - 1
    with torch.no_grad():
        _, states, attns, enc = w._rank(ex, True)
    kw = dict(states=states, max_len=ml, src_dict=None, tgt_dict=None, batch_size=batch, session_len=SD, encoded_source=enc[0], source_len=enc[1],
              session_attns=attns)
    for N in a.Ns:
        W = min(N, 8)
        rep = dict(kw, states=tuple(s.reshape(-1, s.shape[-1]).repeat(N, 1).unsqueeze(0) for s in states), batch_size=batch * N)
        if enc[0] is not None:
            rep.update(encoded_source=enc[0].repeat(N, 1, 1), source_len=enc[1].reshape(-1).repeat(N),
                       session_attns=tuple(x.repeat(N, 1, 1) if x is not None else None for x in attns))
        for top_k in (0, a.top_k):
            sample = lambda: net.decode_sample(num_samples=N, temperature=1.0, top_k=top_k, seed=7, **kw)["predictions"]      # noqa: E731
            beam = lambda: net.decode_beam(beam_size=W, **kw)["predictions"]                                                  # noqa: E731
            greedy = lambda: net.decode(use_cuda=True, **rep)["predictions"]                                                           # noqa: E731
            t = {k: [] for k in ("fused", "plain", "beam", "greedy")}
            toks = {}
            with torch.no_grad():
                for _ in range(max(1, a.rounds)):
                    net.fuse_generator_argmax = net.fuse_generator_topk = True
                    t["fused"].append(timed(sample, a.iters, a.warmup))
                    toks["fused"] = sample().clone()
                    t["beam"].append(timed(beam, a.iters, a.warmup))
                    t["greedy"].append(timed(greedy, a.iters, a.warmup))
                    net.fuse_generator_argmax = net.fuse_generator_topk = False
                    t["plain"].append(timed(sample, a.iters, a.warmup))
                    toks["plain"] = sample().clone()
                net.fuse_generator_argmax = net.fuse_generator_topk = True
            emit(report(kind.lower() + "_sample", dict(decode_rows=batch * SD, rows=batch * SD * N, VT=int(w.args.tgt_vocab_size), max_len=ml), N, top_k, t,
                        toks))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="HREDQS,CARS,MNSRF")
    ap.add_argument("--N", default="4,8,12")
    ap.add_argument("--top_k", type=int, default=4)
    ap.add_argument("--hq_batch", type=int, default=16)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("session_sample_bench needs a GPU: a CPU run gives no time")
    a.Ns = [int(v) for v in a.N.split(",")]
    results = []

    def emit(r):
        print(json.dumps(r), flush=True)
        results.append(r)
    for kind in a.models.split(","):
        if kind == "HREDQS":
            hredqs(a, emit)
        else:
            session(kind, a, emit)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
