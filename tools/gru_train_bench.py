"""One graphed `Ranker.update` of MATCH_TENSOR at the shape of bench.py's `train_C2_match_tensor_update` (config C2_match_tensor, read from bench.py;
the reference's default dropouts) with three encoder configurations in ONE process: the hyparam 1-layer LSTM (the yardstick: the path bench.py
times), `gru1` (rnn_type GRU, 1 layer) and `gru2` (GRU, 2 layers).  Blocks of graphed steps alternate over the configurations for several rounds;
reported is the median ms per step of each with its spread, and -- from the library's launch profiler over four eager steps -- the recurrence
kernels of the document encoder: microseconds per launch and per time step.

    python tools/gru_train_bench.py [--rounds 7] [--steps 20]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (CONFIGS, make_batches: the benchmark's own shape and batches)
from context_attentive_ir_amd import lib  # noqa: E402
from context_attentive_ir_amd.config import default_args  # noqa: E402
from context_attentive_ir_amd.detinit import fill_module_  # noqa: E402
from context_attentive_ir_amd.wrappers import GraphedUpdate, Ranker  # noqa: E402

CONFIGS = (("lstm1", dict()), ("gru1", dict(rnn_type="GRU", nlayers=1)), ("gru2", dict(rnn_type="GRU", nlayers=2)))
RECURRENCES = ("gru_train", "lstm")       # labels of the recurrence launches (forward and BPTT) in the library's profile report


def kernel_times(w, batches, L):
    """{kernel label: (launches, microseconds per launch)} of the recurrence kernels over four eager updates"""
    L.nir_profile_enable(1)
    for i in range(4):
        w.update(batches[i % 4])
    torch.cuda.synchronize()
    L.nir_profile_enable(0)
    buf = ctypes.create_string_buffer(1 << 17)
    L.nir_profile_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().strip().splitlines():
        name, cnt, ms = line.rsplit(",", 2)
        if any(r in name.split("[")[0] for r in RECURRENCES):
            m = bench._SHAPE.match(name)
            T = int(m.group(3)) if m else 0
            us = float(ms) * 1e3 / max(int(cnt), 1)
            out[name] = dict(launches=int(cnt), us_per_launch=round(us, 1), us_per_step=round(us / T, 2) if T else None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    L = lib.load()
    c = dict(bench.CONFIGS["C2_match_tensor"])
    dev = torch.device("cuda", 0)
    batches = bench.make_batches(c, 4, 0, dev)
    extra = dict(optimizer="adam", learning_rate=0.001, weight_decay=0, momentum=0, grad_clipping=10.0, fix_embeddings=True)
    steps, kernels = {}, {}
    for tag, kw in CONFIGS:
        w = Ranker(default_args("MATCH_TENSOR", src_vocab_size=c["vocab"], **extra, **kw))
        fill_module_(w.network, 1013)
        w.cuda()
        w.init_optimizer()
        w.id_check_interval = 0
        kernels[tag] = kernel_times(w, batches, L)
        step = GraphedUpdate(w)
        for i in range(4):                                    # first call per shape: eager step + capture
            step(batches[i % 4])
        steps[tag] = step
    torch.cuda.synchronize()
    ms = {tag: [] for tag, _ in CONFIGS}
    for _ in range(a.rounds):
        for tag, _kw in CONFIGS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(a.steps):
                steps[tag](batches[i % 4])
            torch.cuda.synchronize()
            ms[tag].append((time.perf_counter() - t0) / a.steps * 1e3)
    rec = {"shape": {k: c[k] for k in ("batch", "cands", "qlen", "dlen", "vocab")}, "rounds": a.rounds, "steps_per_block": a.steps,
           "graphed_update_ms": {tag: dict(median=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4)) for tag, v in ms.items()},
           "recurrence_kernels": kernels}
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
