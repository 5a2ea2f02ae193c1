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
    ap.add_argument("--rows", default="128,256,768")
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
    out = dict(model="hredqs_decode", H=H, emsize=E, V=a.V, VT=VT, max_len=a.max_len, S=a.S, iters=a.iters, warmup=a.warmup, rounds=a.rounds,
               device=props.name, cus=props.multi_processor_count, clock_mhz=clock, shapes=[])
    for R in [int(x) for x in a.rows.split(",")]:
        S = a.S
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


if __name__ == "__main__":
    main()
