"""HredQS decode: `nir_hredqs_decode_greedy` in its fast form (csrc/hredqs.hip: the folded LSTM step reading arg-max keys + the keyed
generator / arg-max kernel, two launches per step) against `nir_decode_greedy_plain_folded` (the attention-free decoder the library had
before: folded step, fp32 generator GEMM into an [R, VT] logits tensor, arg-max kernel) on IDENTICAL paired initial states, weights and
packs, and against the entry's own plain form.

Shape: hyparam.HREDQS -- nhid_session 1024, emsize 300, tgt_vocab_size 30000, max_len = max_query_len's default (10); R = B S decode rows
in {128, 256, 768} (S = 4).  States are random in (-1, 1) like LSTM states; weights come from detinit.

Per R: --rounds alternating rounds of (baseline, fast, plain); in a round each path is warmed up --warmup times and timed --iters times
with device events around ONE whole decode; a round's figure is the median.  Reported: the median over the rounds, the per-round figures
and the spread (max - min over the rounds) of every path, whether the fast form beats the baseline by more than the baseline's spread, the
share of tokens on which the paths agree (random states and weights give some near-ties, so less than 1.0 is expected between a split and
an fp32 product), and the device's name and current clock as torch reports them.

    python tools/hredqs_bench.py [--rows 128,256,768] [--iters 30] [--warmup 5] [--rounds 5] [--json out.json]

--beam_size W (1 .. 8) times the beam search instead; --rows are then BEAM rows R = B S W (default 128,256,512,768):
`nir_beam_hredqs_decode` in its fast form (`fast`: the folded step + the top-W kernel on the split state), `nir_beam_plain_decode` with all
three packs on host-paired states (`base`: the best path the library had before -- folded step, beam_gen_topk_kernel on fp32 rows), the
entry's plain form (`plain`: fp32 step, fp32 GEMM, row top-k) and, next to them, the greedy decode of the same B S prefixes (`greedy`).
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="")
    ap.add_argument("--beam_size", type=int, default=0)
    ap.add_argument("--S", type=int, default=4)
    ap.add_argument("--V", type=int, default=30000, help="source vocabulary (the folded gate table is V x 4H floats)")
    ap.add_argument("--VT", type=int, default=30000)
    ap.add_argument("--emsize", type=int, default=300)
    ap.add_argument("--nhid_session", type=int, default=1024)
    ap.add_argument("--max_len", type=int, default=10)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    W = a.beam_size
    a.rows = a.rows or ("128,256,512,768" if W else "128,256,768")
    if not torch.cuda.is_available():
        raise SystemExit("hredqs_bench needs a GPU: a CPU run gives no time")
    from context_attentive_ir_amd import lib
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.recommender import HredQS
    L = lib.load()
    dev = "cuda"
    H, VT, E = a.nhid_session, a.VT, a.emsize
    # (the encoder's width does not matter here: the decode starts from given states)
    net = HredQS(default_args("HREDQS", emsize=E, nhid=64, nhid_session=H, bidirection=False, src_vocab_size=a.V, tgt_vocab_size=VT))
    fill_module_(net, 1013)
    net = net.to(dev).eval()
    w = net._decoder_weights()
    assert w.struct.gen_frag and w.struct.rnn_whh_frag and w.struct.rnn_gate_fold, "the fast form's packs were not built"
    net.fast_decode = False
    wp = net._decoder_weights()                                         # the same weights without packs: the entry's plain form
    k = w.keep
    table = net.embedder.word_embeddings.table.detach().float().contiguous()
    g = torch.Generator().manual_seed(7)
    lut = torch.randint(4, a.V, (VT,), generator=g).to(dev)
    props = torch.cuda.get_device_properties(0)
    try:
        clock = torch.cuda.clock_rate()
    except Exception:  # noqa: BLE001  (not every build exposes it)
        clock = None
    out = dict(model="hredqs_beam_decode" if W else "hredqs_decode", beam_size=W, H=H, emsize=E, V=a.V, VT=VT, max_len=a.max_len, S=a.S, iters=a.iters, warmup=a.warmup, rounds=a.rounds,
               device=props.name, cus=props.multi_processor_count, clock_mhz=clock, shapes=[])
    for R in [int(x) for x in a.rows.split(",")]:
        S = a.S
        if W:
            out["shapes"].append(beam_shape(a, L, lib, R, W, w, wp, k, table, lut, g, dev))
            continue
        B = R // S
        assert B * S == R, "rows must be a multiple of S"
        hs = (torch.rand(B, S, H, generator=g) * 2 - 1).to(dev)
        cs = (torch.rand(B, S, H, generator=g) * 2 - 1).to(dev)
        ph, pc = (t.transpose(0, 1).reshape(R, H).contiguous() for t in (hs, cs))          # the pairing, done on the host for the baseline
        preds = {n: torch.empty(R, a.max_len, dtype=torch.int64, device=dev) for n in ("base", "fast", "plain")}
        ws_b = torch.empty(L.nir_decode_greedy_plain_workspace_bytes(R, H, VT), dtype=torch.uint8, device=dev)
        ws_f = torch.empty(L.nir_hredqs_decode_workspace_bytes(B, S, a.max_len, w.ref()), dtype=torch.uint8, device=dev)
        ws_p = torch.empty(L.nir_hredqs_decode_workspace_bytes(B, S, a.max_len, wp.ref()), dtype=torch.uint8, device=dev)

        def base():
            lib.check(L.nir_decode_greedy_plain_folded(lib.ptr(ph), lib.ptr(pc), R, H, lib.ptr(table), table.shape[0], E, lib.ptr(k["rnn_wih"]),
                                                       lib.ptr(k["rnn_whh"]), lib.ptr(k["rnn_bih"]), lib.ptr(k["rnn_bhh"]), lib.ptr(k["gen_w"]),
                                                       lib.ptr(k["gen_b"]), VT, lib.ptr(lut), 2, a.max_len, lib.ptr(k["rnn_gate_fold"]),
                                                       lib.ptr(k["rnn_whh_frag"]), lib.ptr(ws_b), ws_b.numel(), lib.ptr(preds["base"]), lib.stream()),
                      "nir_decode_greedy_plain_folded")

        def entry(pk, ws, name):
            def run():
                lib.check(L.nir_hredqs_decode_greedy(lib.ptr(hs), lib.ptr(cs), B, S, lib.ptr(table), table.shape[0], E, lib.ptr(lut), 2, a.max_len,
                                                     pk.ref(), lib.ptr(ws), ws.numel(), lib.ptr(preds[name]), lib.stream()), "nir_hredqs_decode_greedy")
            return run
        paths = dict(base=base, fast=entry(w, ws_f, "fast"), plain=entry(wp, ws_p, "plain"))
        rounds = {n: [] for n in paths}
        for _ in range(max(1, a.rounds)):                                # the paths alternate, so that drift of the machine meets all of them
            for n, fn in paths.items():
                rounds[n].append(timed(fn, a.iters, a.warmup))
        torch.cuda.synchronize()
        med = {n: float(np.median(v)) for n, v in rounds.items()}
        spread = {n: float(max(v) - min(v)) for n, v in rounds.items()}
        rec = dict(R=R, B=B, S=S)
        for n in paths:
            rec[n + "_ms"] = round(med[n], 4)
            rec[n + "_ms_rounds"] = [round(v, 4) for v in rounds[n]]
            rec[n + "_spread_ms"] = round(spread[n], 4)
            rec[n + "_us_per_step"] = round(1000.0 * med[n] / a.max_len, 2)
        rec["fast_beats_base_by_more_than_its_spread"] = bool(med["base"] - med["fast"] > spread["base"])
        rec["speedup_fast_over_base"] = round(med["base"] / med["fast"], 3)
        rec["tokens_equal_fast_base"] = float((preds["fast"] == preds["base"]).float().mean())
        rec["tokens_equal_fast_plain"] = float((preds["fast"] == preds["plain"]).float().mean())
        rec["first_tokens_equal_fast_base"] = float((preds["fast"][:, 0] == preds["base"][:, 0]).float().mean())
        out["shapes"].append(rec)
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


def beam_shape(a, L, lib, R, W, w, wp, k, table, lut, g, dev):
    """one shape of the beam comparison: R = B S W beam rows"""
    S, H, VT, E, ml = a.S, a.nhid_session, a.VT, a.emsize, a.max_len
    Bd = R // W
    B = Bd // S
    assert B * S * W == R, "rows must be a multiple of S * beam_size"
    hs = (torch.rand(B, S, H, generator=g) * 2 - 1).to(dev)
    cs = (torch.rand(B, S, H, generator=g) * 2 - 1).to(dev)
    ph, pc = (t.transpose(0, 1).reshape(Bd, H).contiguous() for t in (hs, cs))              # the pairing, done on the host for the baseline
    outs = {n: dict(pred=torch.empty(Bd, W, ml, dtype=torch.int64, device=dev), sc=torch.empty(Bd, W, device=dev),
                    ln=torch.empty(Bd, W, dtype=torch.int64, device=dev)) for n in ("base", "fast", "plain")}
    greedy_pred = torch.empty(Bd, ml, dtype=torch.int64, device=dev)
    ws_b = torch.empty(L.nir_beam_plain_decode_workspace_bytes(Bd, H, VT, W, ml, 1, 1), dtype=torch.uint8, device=dev)
    ws_f = torch.empty(L.nir_beam_hredqs_decode_workspace_bytes(B, S, W, ml, w.ref()), dtype=torch.uint8, device=dev)
    ws_p = torch.empty(L.nir_beam_hredqs_decode_workspace_bytes(B, S, W, ml, wp.ref()), dtype=torch.uint8, device=dev)
    ws_g = torch.empty(L.nir_hredqs_decode_workspace_bytes(B, S, ml, w.ref()), dtype=torch.uint8, device=dev)

    def base():
        o = outs["base"]
        lib.check(L.nir_beam_plain_decode(lib.ptr(ph), lib.ptr(pc), Bd, H, lib.ptr(table), table.shape[0], E, lib.ptr(k["rnn_wih"]), lib.ptr(k["rnn_whh"]),
                                          lib.ptr(k["rnn_bih"]), lib.ptr(k["rnn_bhh"]), lib.ptr(k["gen_w"]), lib.ptr(k["gen_b"]), VT, lib.ptr(lut), 2, ml,
                                          lib.ptr(k["rnn_gate_fold"]), lib.ptr(k["rnn_whh_frag"]), lib.ptr(k["gen_frag"]), W, lib.ptr(ws_b), ws_b.numel(),
                                          lib.ptr(o["pred"]), lib.ptr(o["sc"]), lib.ptr(o["ln"]), None, lib.stream()), "nir_beam_plain_decode")

    def entry(pk, ws, name):
        o = outs[name]

        def run():
            lib.check(L.nir_beam_hredqs_decode(lib.ptr(hs), lib.ptr(cs), B, S, lib.ptr(table), table.shape[0], E, lib.ptr(lut), 2, ml, pk.ref(), W,
                                               lib.ptr(ws), ws.numel(), lib.ptr(o["pred"]), lib.ptr(o["sc"]), lib.ptr(o["ln"]), None, lib.stream()),
                      "nir_beam_hredqs_decode")
        return run

    def greedy():
        lib.check(L.nir_hredqs_decode_greedy(lib.ptr(hs), lib.ptr(cs), B, S, lib.ptr(table), table.shape[0], E, lib.ptr(lut), 2, ml, w.ref(),
                                             lib.ptr(ws_g), ws_g.numel(), lib.ptr(greedy_pred), lib.stream()), "nir_hredqs_decode_greedy")
    paths = dict(base=base, fast=entry(w, ws_f, "fast"), plain=entry(wp, ws_p, "plain"), greedy=greedy)
    rounds = {n: [] for n in paths}
    for _ in range(max(1, a.rounds)):                                    # the paths alternate, so that drift of the machine meets all of them
        for n, fn in paths.items():
            rounds[n].append(timed(fn, a.iters, a.warmup))
    torch.cuda.synchronize()
    med = {n: float(np.median(v)) for n, v in rounds.items()}
    spread = {n: float(max(v) - min(v)) for n, v in rounds.items()}
    rec = dict(R=R, B=B, S=S, W=W, Bd=Bd)
    for n in paths:
        rec[n + "_ms"] = round(med[n], 4)
        rec[n + "_ms_rounds"] = [round(v, 4) for v in rounds[n]]
        rec[n + "_spread_ms"] = round(spread[n], 4)
    for other in ("base", "plain"):
        rec["fast_beats_%s_outside_the_spread" % other] = bool(med[other] - med["fast"] > max(spread[other], spread["fast"]))
        rec["fast_loses_to_%s_outside_the_spread" % other] = bool(med["fast"] - med[other] > max(spread[other], spread["fast"]))
        rec["speedup_fast_over_" + other] = round(med[other] / med["fast"], 3)
        rec["tokens_equal_fast_" + other] = float((outs["fast"]["pred"] == outs[other]["pred"]).float().mean())
    rec["best_first_tokens_equal_fast_greedy"] = float((outs["fast"]["pred"][:, 0, 0] == greedy_pred[:, 0]).float().mean())
    return rec


if __name__ == "__main__":
    main()
