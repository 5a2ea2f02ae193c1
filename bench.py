#!/usr/bin/env python
"""bench.py -- ranked (query,doc) pairs/sec of the encode-and-rank hot path on N MI355X.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR] [--full]

A plain run does what the headline figure needs and nothing else: set-up, warm-up, the timed steps, --dump-outputs, the line.  --full adds
everything else this file measures: the headline's roofline, power, one-batch latency, precompute, H2D-inclusive, wrapper-default and CPU
baseline figures, the sub-records (--sub picks among them) and at N > 1 the weak-scaling figure.  Without --full those entries of the line
are null (`sub` is empty) and `full` is false.

N > 1: launched by torch.distributed.run (one rank per GPU; RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* from the environment) -- or plainly, in
which case bench.py starts the N ranks itself.  A world that is not --gpus is refused; n_gpus of the line = an all-reduce of ones.

OUTPUT.  The LAST line of stdout is ONE compact JSON object (~2.5 KB): metric / value / unit / n_gpus / steps / warmup / reps / ms_per_step /
scaling / dtype / data, `config`, `roofline`, `cpu_baseline` and one four-scalar entry per sub-record in `sub`.  The full records (every
sub-record's roofline block, per-kernel microseconds, precompute, H2D stream) go to bench_detail.json (`config.detail`).  stderr of a successful
run is EMPTY: file descriptor 2 points at bench_stderr.<rank>.log for the length of the run and is replayed only on failure.  Both files are
written in the repository root (BENCH_LOG_DIR overrides it), or, where the running user cannot write there, in a per-user directory under the
system temporary directory (log_path).  At N > 1 with --full the headline is printed as a complete record before the sub-records run; the
final line supersedes it.

HEADLINE: BASELINE.json configs[2], the largest configuration BASELINE marks 1 x MI355X -- CARS multitask, 16 sessions x session_len 7 x 10
candidates, q_len 4, doc_len 64, emb_dim 300, fp32, synthetic MSMARCO-shaped ids (Zipf over a 100 000 x 300 table, seed 1013), full-length
sequences.  A "step" = Multitask.predict's ranking path on one batch already resident in HBM: encode + rank_document + softmax over the
candidates (the suggestion decoder is not a ranking step; sub-record C3_cars_with_decode times the full predict).  Steps are replayed as
hipGraphs over resident macro-batches (8 batches per replay at C3, 4 lanes); EXACTLY --steps steps are timed between barrier + synchronize,
max over ranks; a region shorter than 0.25 s is repeated and the median reported (`reps`).  --dump-outputs DIR: after the timed region, the
probabilities of the last timed step are written to DIR/click_scores.npy (session models, [B,S,N]) or DIR/scores.npy (rankers, [B,N]), float32;
the inputs and weights are seeded, so two builds run with the same arguments can be compared output for output.

SUB-RECORDS (--full, N = 1): C1 ESM 8x5, C2 MatchTensor 32x10, the north-star 32x50 MatchTensor shape, C4 DUET and DRMM 64x50xdoc_len 290 (DRMM / ESM
with uniform ids over a 1M-row table so the gather really comes from HBM; DRMM with its histogram gap on overlapping ids), the C5 shape (CARS
64x7x50) in bf16, the two other session rankers (M_MATCH_TENSOR, MNSRF) at the configs[2] shape, C3 without folded tables, C3 with decode, the C5 session stream (ids from the host), the CARS / MatchTensor training steps.

N > 1 (strong scaling): every rank holds the SAME global batch.  Rankers: its slice of the candidate axis (ceil(N_cand / N),
padded), all-gather of the score shards over RCCL.  CARS: the (session, candidate) pair axis in whole sessions per rank when B % N == 0 (no exchange
of pooled vectors, all-gather of the probabilities), else the candidate axis with an all-to-all.  value = global pairs / max-rank time.
Sub-records (--full): C4 DUET / DRMM, the C5 shape, the headline on the other CARS axis, the C5 stream in both stream modes, and
`config.weak_scaling_pairs_per_s` (labelled, secondary: every rank scoring its own full batch with no collective).

roofline (--full): the dominant kernel (largest summed duration), timed with HIP events on its launch stream in a profiled pass over the same launches
right after the timed region; algorithmic flops / bytes per launch are priced from the launch's own shape.  Peaks: HBM
8 TB/s; fp32 MFMA 157.3 TFLOP/s; fp16 / bf16 MFMA 2500 TFLOP/s (a two-term fp16 split executes 3 MFMAs per product, a three-term bf16 split 6).
cpu_baseline (--full): the pinned CPU oracle (oracle/neuroir_cpu.py) on the host cores, bounded sample, rank 0 at N = 1 only.
"""
import os
os.environ.setdefault("NIR_DEBUG_TUNABLES", "1")      # the isolated-kernel profile pass switches the library's internal fork off (nir_debug_set_tunable)
import argparse
import ctypes
import json
import os
import re
import sys
import time

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from context_attentive_ir_amd import lib, sharding, synth  # noqa: E402
from context_attentive_ir_amd.config import default_args  # noqa: E402
from context_attentive_ir_amd.detinit import fill_module_  # noqa: E402
from context_attentive_ir_amd.wrappers import Multitask, Ranker  # noqa: E402

PEAK_HBM_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
PEAK_FP32_TFLOPS = 157.3     # fp32 vector == fp32 MFMA peak
PEAK_BF16_TFLOPS = 2500.0    # dense bf16 MFMA
PEAK_BF16X3_TFLOPS = PEAK_BF16_TFLOPS / 6.0

SESSION_MODELS = ("cars", "m_match_tensor", "mnsrf")
MIN_REGION_S = 0.25          # a timed region shorter than this is repeated (median reported)
MAX_REPS = 41

# name -> workload (BASELINE.json configs; SURVEY.md section 8d shapes)
CONFIGS = {
    "C3_cars": dict(model="cars", batch=16, session=7, cands=10, qlen=4, dlen=64, vocab=100000, uniform=False, dtype="f32",
                    baseline="configs[2]: CARS multitask, session_len=7, batch=16 sessions x 10 candidates, 1xMI355X"),
    "C1_esm": dict(model="esm", batch=8, cands=5, qlen=4, dlen=64, vocab=100000, uniform=False, dtype="f32",
                   baseline="configs[0]: ESM ranker, batch=8 queries x 5 candidates, q_len=4/doc_len=64"),
    "C2_match_tensor": dict(model="match_tensor", batch=32, cands=10, qlen=4, dlen=64, vocab=100000, uniform=False, dtype="f32",
                            baseline="configs[1]: match_tensor ranker, batch=32 x 10 candidates, emb_dim=300, fp32"),
    "NS_match_tensor_50": dict(model="match_tensor", batch=32, cands=50, qlen=4, dlen=64, vocab=100000, uniform=False, dtype="f32",
                               baseline="north_star shape: q_len 4, doc_len 64, 50 candidates"),
    # north_star's OWN throughput workload -- sessions, q_len 4, doc_len 64, 50 candidates -- at the reference's fp32
    # (neuroir/config.py:42 --num_candidates, multitask/cars.py:522-540); the record carries max_abs_diff_vs_oracle_softmax on a 4-session slice
    "NS_cars_50": dict(model="cars", batch=16, session=7, cands=50, qlen=4, dlen=64, vocab=100000, uniform=False, dtype="f32", oracle_slice=4,
                       baseline="north_star shape: CARS sessions (session_len 7), q_len 4, doc_len 64, 50 candidates, fp32"),
    "C4_duet": dict(model="duet", batch=64, cands=50, qlen=4, dlen=290, vocab=100000, uniform=False, dtype="f32",
                    baseline="configs[3]: DUET, batch=64 x 50 candidates, doc_len=290"),
    "C4_drmm": dict(model="drmm", batch=64, cands=50, qlen=4, dlen=290, vocab=1000000, uniform=True, dtype="f32",
                    baseline="configs[3]: DRMM, batch=64 x 50 candidates, doc_len=290 (uniform ids, 1M-row table: HBM-resident gather)"),
    "C4_esm_hbm": dict(model="esm", batch=64, cands=50, qlen=4, dlen=290, vocab=1000000, uniform=True, dtype="f32",
                       baseline="ESM at the C4 shape (uniform ids, 1M-row table): the pure gather-reduce HBM roofline"),
    "C5_cars_bf16": dict(model="cars", batch=64, session=7, cands=50, qlen=4, dlen=64, vocab=100000, uniform=False, dtype="bf16",
                         baseline="configs[4] shape on one GPU: CARS, 50 candidates/query, bf16 folded tables + bf16 MFMA recurrence"),
    # the other two session rankers main/multitask.py can select, at the configs[2] shape (not BASELINE configurations)
    "X3_m_match_tensor": dict(model="m_match_tensor", batch=16, session=7, cands=10, qlen=4, dlen=64, vocab=100000, uniform=False, dtype="f32",
                              baseline="SURVEY 8(f) rank 3: M_MATCH_TENSOR at the configs[2] shape"),
    "X3_mnsrf": dict(model="mnsrf", batch=16, session=7, cands=10, qlen=4, dlen=64, vocab=100000, uniform=False, dtype="f32",
                     baseline="SURVEY 8(f) rank 3: MNSRF at the configs[2] shape (256-unit encoders on the four-CU cluster recurrence, csrc/lstm_cluster.hip)"),
    # the opt-in 2-MFMA precision tier of the fp32-table recurrence as a LABELLED sub-record (never the headline): W_hh as two fp16
    # terms x h as ONE fp16 term in the recurrent product and the attention GEMM (NIR_DTYPE_F32_SPLIT2), the headline's shape
    "C3_cars_split2": dict(model="cars", batch=16, session=7, cands=10, qlen=4, dlen=64, vocab=100000, uniform=False, dtype="f32_split2",
                           baseline="the configs[2] shape on the opt-in precision tier (fp32 folded tables; fp16x2 W_hh x fp16 h recurrence, fp16 rows into the "
                                    "attention pipeline): NOT the parity path -- its own error figure rides in the record"),
}
HEADLINE = "C3_cars"
SUB_STEPS = {"NS_cars_50": 60, "C3_cars_split2": 200, "C1_esm": 400, "C2_match_tensor": 400, "NS_match_tensor_50": 200, "C4_duet": 24, "C4_drmm": 60, "C4_esm_hbm": 60,
             "C5_cars_bf16": 24, "X3_m_match_tensor": 100, "X3_mnsrf": 100}


def algorithmic_bytes_per_pair(N, QL, DL, E=300, table_bytes=4):
    """every token occurrence gathers its row once + int64 id, + 4 B score."""
    return DL * (table_bytes * E + 8) + QL * (table_bytes * E + 8) / N + 4


def flops_per_pair(model, qlen, dlen):
    named = {("match_tensor", 4, 64): 1.76e7, ("cars", 4, 64): 6.72e7, ("duet", 4, 290): 2.08e8, ("drmm", 4, 290): 8.7e5,
             ("esm", 4, 64): 2.1e4}
    return named.get((model, qlen, dlen))


_SHAPE = re.compile(r"^(.*)\[M=(\d+),N=(\d+),K=(\d+)\]$")


def kernel_work(name, c, pairs_per_launch=None):
    """Work of ONE launch, priced from the launch's own shape label:
      flops  algorithmic (fp32-equivalent) FLOPs of the op the kernel implements
      terms  MFMAs EXECUTED per algorithmic product block (fp16 two-term split 3, bf16 three-term split 6, single fp16/bf16/f32 term 1)
      pipe   dense peak of the executed MFMA type (2500 TF f16/bf16, 157.3 TF f32-input)
      bytes  the kernel's own minimal traffic model (its operands once) -- informational; the HBM figures of the line use SURVEY 8(d)
    Returns None for kernels without a model."""
    m = _SHAPE.match(name)
    base, M, N, K = (m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4))) if m else (name, 0, 0, 0)
    B, NC, QL, DL, E = c["batch"], c["cands"], c["qlen"], c["dlen"], 300
    pairs = B * NC * (c.get("session", 1) if c["model"] in SESSION_MODELS else 1)
    if pairs_per_launch:                      # a macro-batched launch covers several batches
        pairs = pairs_per_launch
    F16, F32 = PEAK_BF16_TFLOPS, PEAK_FP32_TFLOPS
    if base.startswith("gemm3h_kernel") or base.startswith("gemm_h2p_kernel"):     # fp16 two-term split: 3 MFMAs per product block
        gathered = "[gather]" in base
        return dict(flops=2.0 * M * N * K, bytes=4.0 * (M * K + N * K + M * N) + (8.0 * M * max(1, K // E) if gathered else 0), terms=3, pipe=F16)
    if base.startswith("duet_doc_kernel"):
        # fused DUET document branch (csrc/duet_fused.hip): the algorithmic work of the pairs it covers -- conv_d1 (K = 3E) and conv_d2
        # (K = NF) per pooled position -- not the padded tile work in the label (M = tiles x 64 rows, N = NF, K = 3E)
        Tc, Tp = DL - 2, DL - 6
        return dict(flops=pairs * 2.0 * N * (Tc * K + Tp * N), bytes=pairs * DL * (4.0 * E + 8), terms=3, pipe=F16)
    if base.startswith("attn_pool_fused_kernel") or base.startswith("attn_pool_pipe_kernel"):
        # fused attention pooling (csrc/cars_attn.hip): M rows of D = N = K = 256.  Pipeline template arguments <ONE, IN>: ONE = single fp16 terms
        # (bf16 encoders), IN = 1 fp16 rows / 2 the recurrence's term pairs (4 B per element, like fp32 rows)
        one = "<true" in base                           # (the single-role kernel always runs the three-MFMA form)
        in16 = "<true,1>" in base
        in16 = in16 or "<false,1>" in base                 # fp16 rows with a two-term W0 (the split2 tier): 2 MFMAs per fragment pair
        return dict(flops=2.0 * M * N * K + 4.0 * M * N, bytes=(2.0 if in16 else 4.0) * M * K + 4.0 * N * K, terms=1 if one else (2 if "<false,1>" in base else 3), pipe=F16)
    if base.startswith("pred_argmax_kernel"):      # csrc/cars_decode.hip: [M decode rows] x [N = V_tgt, K = 256] projection + arg-max, fp16 two-term split, no logits
        return dict(flops=2.0 * M * N * K, bytes=4.0 * N * K + 4.0 * M * K + 8.0 * M * max(1, N // 960), terms=3, pipe=F16)
    if base.startswith("gemm3_kernel"):
        gathered = "[gather]" in base
        return dict(flops=2.0 * M * N * K, bytes=4.0 * (M * K + N * K + M * N) + (8.0 * M * max(1, K // E) if gathered else 0), terms=6, pipe=F16)
    if base.startswith("gemm_kernel") or base.startswith("gemm16_kernel") or base.startswith("gemm32_kernel") or base.startswith("gemm_skinny_kernel"):
        return dict(flops=2.0 * M * N * K, bytes=4.0 * (M * K + N * K + M * N), terms=1, pipe=F32)
    if base.startswith("lstm16_pt_bf16_kernel") or base.startswith("lstm16_pt_bf16w8_kernel"):      # M sequences, N = T steps, K = H; both directions in one launch; bf16 table rows,
        # fp16 MFMA operands; the states leave as fp16 when they feed the pipelined attention kernel of the same encode call
        out_b = 2.0 if M * N >= 2 * 256 * 64 else 4.0
        return dict(flops=M * N * 2 * 2.0 * 4 * K * K, bytes=M * N * (8.0 + 2 * 4 * K * 2 + 2 * K * out_b), terms=1, pipe=F16)
    if base.startswith("lstm16_pt_h2_kernel"):        # fp32-accurate two-term fp16 split: 3 fp16 MFMAs per k-block (",true" = H1: the one-term-h tier, 2 MFMAs, fp16 rows out)
        h1 = ",true>" in base
        return dict(flops=M * N * 2 * 2.0 * 4 * K * K, bytes=M * N * (8.0 + 2 * 4 * K * 4 + 2 * K * (2 if h1 else 4)), terms=2 if h1 else 3, pipe=F16)
    if base.startswith("lstm_cluster_kernel"):       # csrc/lstm_cluster.hip: M sequences x N steps x 2 directions, K = 256 units, W_hh resident on 4-CU clusters
        # bytes: one 4 KB folded gate row per (token, direction) + the ids (+ the bank, unless the max over time is fused: [maxpool])
        out_b = 0.0 if "[maxpool]" in base else 2 * K * 4.0
        return dict(flops=M * N * 2 * 2.0 * 4 * K * K, bytes=M * N * (8.0 + 2 * 4 * K * 4 + out_b) + (M * 2 * K * 4.0 if "[maxpool]" in base else 0.0), terms=3, pipe=F16)
    if base.startswith("lstm16_pt_kernel"):
        return dict(flops=M * N * 2 * 2.0 * 4 * K * K, bytes=M * N * (8.0 + 2 * 4 * K * 4 + 2 * K * 4), terms=1, pipe=F32)
    if base.startswith("lstm_mfma16_gin_kernel") or base.startswith("lstm_mfma_gin_kernel") or base.startswith("lstm_rec_kernel<"):
        return dict(flops=M * N * 2 * 2.0 * 4 * K * K, bytes=M * N * (2 * 4 * K * 4 + 2 * K * 4.0), terms=1, pipe=F32)
    if base.startswith("lstm_mfma_kernel") or base.startswith("lstm_mfma16_kernel") or base.startswith("lstm_rec_kernel[fused]"):
        F = 40                                         # MatchTensor: input projection fused (I = featsize 40)
        return dict(flops=M * N * 2 * 2.0 * 4 * K * (K + F), bytes=M * N * (2 * F + 2 * K) * 4.0, terms=1, pipe=F32)
    if base == "mt_head_kernel":
        C = 50
        return dict(flops=pairs * QL * DL * 2.0 * (15 * C * 6 + 45 * 6 + 18 * 20), bytes=pairs * DL * (C * 4 + 8.0) + pairs * 4, terms=3, pipe=F16)
    if base.startswith("wgrad_kernel") or base.startswith("wgrad_lds_kernel"):     # dW = dY^T X on the f32 MFMA (csrc/train.hip): M rows reduced, [N, K] output
        return dict(flops=2.0 * M * N * K, bytes=4.0 * (M * N + M * K + N * K), terms=1, pipe=F32)
    if base.startswith("lstm_train_fwd_kernel") or base.startswith("lstm_train_bwd_kernel") or base.startswith("lstm_train_bwd_mfma_kernel"):
        # M sequences, N = T steps, K = H units, both directions: the recurrent product h W_hh^T (forward) / W_hh^T dg (BPTT), f32 MFMA
        return dict(flops=M * N * 2 * 2.0 * 4 * K * K, bytes=M * N * 2 * (4 * K + 2 * K) * 4.0, terms=1, pipe=F32)
    if base.startswith("lstm256_bptt_steps"):
        # csrc/lstm256_bptt.hip: ONE label for the T step launches of a BPTT (both directions): dg W_hh on the f32 MFMA; bytes per step and direction:
        # activations + gate gradients (2 x 4K), cell states x 2, dout, dc in / out, eight dh partials written and read (16K)
        return dict(flops=M * N * 2 * 2.0 * 4 * K * K, bytes=M * N * 2 * (8 * K + 5 * K + 16 * K) * 4.0, terms=1, pipe=F32)
    if base in ("esm16_kernel", "esm_kernel", "drmm_kernel"):
        fl = flops_per_pair(c["model"], QL, DL) or (2.0 * DL * E if base != "drmm_kernel" else 2.0 * QL * DL * E)
        return dict(flops=fl * pairs, bytes=algorithmic_bytes_per_pair(NC, QL, DL) * pairs, terms=0, pipe=F32)   # VALU kernels: no MFMA
    return None


def pmc_entry(name, prof_name):
    """profiles/pmc_summary.json (tools/derive_profiles.py: rocprofv3 --pmc passes of this same workload, separate FETCH_SIZE / WRITE_SIZE /
    SQ passes, gfx950 x2 FETCH correction): {bytes_per_launch, mfma_busy} of the kernel behind the library's profile label, or None."""
    for fn in ("pmc_summary.json",):
        try:
            tj = json.load(open(os.path.join(ROOT, "profiles", fn)))
            ent = traffic_entry(tj.get("configs", {}).get(name, {}), prof_name)
            if ent:
                return ent
        except (OSError, ValueError, KeyError, AttributeError):
            pass
    return None


def traffic_entry(kernels, prof_name):
    """profiles/traffic.json is keyed by rocprofv3's kernel names (template arguments, no shape label); match the library's
    profile label: exact template name first, then the family (a "[gather]" label = the gathering instantiation <1>/<2>)."""
    m = _SHAPE.match(prof_name)
    base = m.group(1) if m else prof_name
    gather = "[gather]" in base
    fam = base.replace("[gather]", "").replace("[fused]", "")
    if fam in kernels:
        return kernels[fam]
    cands = [k for k in kernels if k.split("<")[0] == fam.split("<")[0]]
    if fam.split("<")[0] == "gemm3_kernel":
        cands = [k for k in cands if (k != "gemm3_kernel<0>") == gather]
    return kernels[max(cands, key=lambda k: kernels[k]["bytes_per_launch"])] if cands else None


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--config", default=HEADLINE, choices=sorted(CONFIGS) + ["C5_stream"],
                    help="headline workload (default: C3 CARS); C5_stream = the whole 223 876-session bf16 stream, ids from the host (prints its own record)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline's timed steps: its roofline, power, one-batch latency, H2D, wrapper-default "
                    "and CPU-baseline figures, the sub-records and (N > 1) the weak-scaling figure; off: setup, warm-up, the timed steps, "
                    "--dump-outputs and the line")
    ap.add_argument("--sub", default=None, help="--full: comma-separated sub-records to measure (default: all; 'none' to skip)")
    # ad-hoc shapes (tools/, profiling): override fields of --config
    ap.add_argument("--model", default=None, choices=["match_tensor", "esm", "drmm", "duet", "cars", "m_match_tensor", "mnsrf"])
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--cands", type=int, default=None)
    ap.add_argument("--qlen", type=int, default=None)
    ap.add_argument("--dlen", type=int, default=None)
    ap.add_argument("--session", type=int, default=None)
    ap.add_argument("--vocab", type=int, default=None)
    ap.add_argument("--uniform", action="store_true", default=None, help="uniform token ids (worst case for the gather) instead of Zipf")
    ap.add_argument("--dtype", default=None, choices=["f32", "bf16"], help="CARS: bf16 = bf16 folded tables + bf16 MFMA recurrence")
    ap.add_argument("--no-fold", action="store_true", help="CARS: per-batch gather-GEMM instead of the folded embedding table")
    ap.add_argument("--nbatches", type=int, default=12, help="distinct resident batches cycled through")
    ap.add_argument("--streams", type=int, default=4, help="batches in flight: step i runs on HIP stream i %% streams")
    ap.add_argument("--in-flight-hint", type=int, default=0, help="library batches-in-flight hint (default: --streams); profiling runs pass the timed run's "
                    "lane count with --streams 1 so that the serial capture launches the SAME kernel instantiations the timed run does")
    ap.add_argument("--no-graph", action="store_true", help="do not replay the step from a captured hipGraph")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full: no CPU baseline and no checker legs against the CPU oracle")
    ap.add_argument("--cpu-seconds", type=float, default=10.0, help="--full: seconds of the CPU baseline's timed sample")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps of the headline, write the probabilities its LAST timed step computed to DIR/<name>.npy (float32): "
                    "click_scores [B,S,N] for the session models, scores [B,N] for the rankers")
    return ap.parse_args()


def build_model(c, args):
    kind = c["model"].upper()
    extra = dict(max_query_len=c["qlen"], max_doc_len=c["dlen"]) if kind == "DUET" else {}
    margs = default_args(kind, src_vocab_size=c["vocab"], **extra)
    wrapper = Multitask(margs) if c["model"] in SESSION_MODELS else Ranker(margs)
    fill_module_(wrapper.network, 1013)
    if kind == "CARS":
        wrapper.network.compute_dtype = c.get("dtype", "f32")
        wrapper.network.fold_embeddings = not (args.no_fold or c.get("nofold"))
    elif kind in ("MATCH_TENSOR", "MNSRF") and (args.no_fold or c.get("nofold")):
        wrapper.network.fold_embeddings = False
    wrapper.cuda()
    wrapper.network.eval()
    wrapper.id_check_interval = 0        # synthetic ids are valid by construction: no per-call flag work inside the tuned timed loops
    wrapper.args.predict_graphs = False  # the tuned records capture their own graphs over predict(); the wrapper's own cache is timed by dropin_record
    return wrapper


def precompute_info(wrapper, c):
    """Inference-time precompute behind the folded recurrences (csrc/lstm_fold.hip): emb(id) W_ih^T + b folded into one [V, ndir*4H] gate table
    per encoder and weight version, built OUTSIDE the timed region.  Reported so the line says what it costs: build time (cold, measured
    here by forcing a rebuild), resident bytes, and the vocabulary it scales with.  None when the model runs without folded tables."""
    net = wrapper.network
    kind = c["model"]
    if kind == "cars" and net.fold_embeddings and net._use_fold(net.embedder.word_embeddings.table, net._enc_weights("d").struct.H):
        def build():
            return [net._folded_table(w, net._enc_weights(w)) for w in ("q", "d")]
        caches = (net._fq, net._fd)
    elif kind == "match_tensor" and getattr(net, "fold_embeddings", False):
        def build():
            return list(net._folded_tables(net._weights()))
        caches = (net._fold,)
    elif kind == "duet" and getattr(net, "table_planes", False) and getattr(net, "fuse_document_branch", False):
        # fused DUET document kernel in plane mode (csrc/duet_fused.hip): the embedding table as fp16 term planes [V, 2, E -> 64k], built with the
        # rest of the weight pack, once per weight version
        def build():
            pk = net._weights()
            return [pk.keep[k] for k in ("ftable", "fw1c") if k in pk.keep]
        caches = (net._pack,)
    else:
        return None
    build()
    torch.cuda.synchronize()
    for ch in caches:
        ch.invalidate()
    t0 = time.perf_counter()
    tabs = build()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    return {"fold_ms": round(ms, 3), "fold_bytes": int(sum(t.numel() * t.element_size() for t in tabs)), "vocab": int(c["vocab"]),
            "tables": len(tabs), "rebuilt": "once per weight version (PackCache); not part of a step"}


def macro_batch(c, env_key="BENCH_MACRO_BATCH", share=1):
    """batches merged into one macro-batch per graph replay (Multitask.predict_many): ONE policy at every N -- a rank's launch sequence is
    filled to ~8 960 documents, at most 8 steps per replay (and per gather).  Small batches (C3: 1 120 documents) are merged eight at a time at
    N = 1 -- a lone C3 batch fills 140 of 256 CUs with recurrence workgroups and pays 76 MB of session-weight traffic whatever its size; a
    recurrence workgroup (16 sequences, one direction) occupies a whole CU for the 64 steps, so the launch runs in ROUNDS of 256 workgroups:
    4 batches = 560 workgroups = 3 rounds (the last 19 % full), 8 batches = 1 120 = 5 rounds (measured, 504 steps: KG 4 / 6 / 7 / 8 / 9 = 8.15 / 8.28 /
    8.51 / 8.64 / 8.50 M pairs/s) -- large ones (C5: 22 400 documents) are not merged (no gain measured, 4x the scratch).  share > 1: the rank holds
    1/share of every batch (sharded CARS step), so the same target merges as many steps (cap 8).  The environment variable overrides; the
    `*_kg_matched` sub-record of an N > 1 run repeats the headline with the N = 1 count."""
    if os.environ.get(env_key):
        return max(1, int(os.environ[env_key]))
    tokens = c["batch"] * c.get("session", 1) * c["cands"] * c["dlen"] // max(1, share)      # 8 960 documents of 64 tokens
    return max(1, min(8, 8960 * 64 // max(1, tokens)))


def make_batches(c, nbatches, rank_seed, dev):
    out = []
    for i in range(nbatches):
        seed = 1013 + 7919 * i + 104729 * rank_seed
        if c["model"] in SESSION_MODELS:
            b = synth.session_batch(c["batch"], c["session"], c["cands"], c["qlen"], c["dlen"], c["vocab"], seed)
        else:
            b = synth.ranker_batch(c["batch"], c["cands"], c["qlen"], c["dlen"], c["vocab"], seed, uniform=c["uniform"])
        out.append({k: v.to(dev) for k, v in b.items()})
    return out


class Env(object):
    def __init__(self, gpus=None):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        # --gpus N and the launched world must agree (main() re-launches itself under torch.distributed.run when WORLD_SIZE is unset):
        # a run that says N and measures something else is refused here, before anything is timed
        if gpus is not None and self.world != gpus and not (self.world == 1 and gpus == 1):
            raise SystemExit("bench.py: --gpus %d but WORLD_SIZE=%d -- refusing to measure a world that is not the one asked for" % (gpus, self.world))
        self.rank = int(os.environ.get("RANK", "0"))
        local = int(os.environ.get("LOCAL_RANK", "0")) % torch.cuda.device_count()   # (N ranks on a 1-GPU box share device 0)
        torch.cuda.set_device(local)
        self.dev = torch.device("cuda", local)
        self.backend = os.environ.get("BENCH_BACKEND", "nccl")   # "gloo": flow test without RCCL (gathers through the host)
        self.dist = None
        self.multi = self.world > 1 or bool(os.environ.get("BENCH_FORCE_DIST"))
        if self.multi:
            import torch.distributed as dist
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("MASTER_PORT", "29511")
            if self.backend == "nccl":
                import datetime      # (a rank that died takes the others down after 5 minutes, not after the default 10 + the driver's own limit)
                dist.init_process_group("nccl", rank=self.rank, world_size=self.world, device_id=self.dev,
                                        timeout=datetime.timedelta(seconds=int(os.environ.get("BENCH_PG_TIMEOUT_S", "300"))))
            else:
                dist.init_process_group(self.backend, rank=self.rank, world_size=self.world)
            self.dist = dist
            # n_gpus of the line = the ranks the process group really has: an all-reduce of ones, not an environment variable
            one = torch.ones(1, device=self.dev if self.backend == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(one)
            self.seen = int(round(float(one.item())))
            if self.seen != self.world or dist.get_world_size() != self.world:
                raise SystemExit("bench.py: process group has %d ranks (all-reduce of ones: %d), WORLD_SIZE=%d" % (dist.get_world_size(), self.seen, self.world))
        else:
            self.seen = 1

    def barrier(self):
        if self.dist:
            self.dist.barrier()

    def max_over_ranks(self, x):
        if not self.dist:
            return x
        t = torch.tensor([x], device=self.dev if self.backend == "nccl" else "cpu", dtype=torch.float64)
        self.dist.all_reduce(t, op=self.dist.ReduceOp.MAX)
        return float(t.item())


# hipGraph captures are thread-local: the ProcessGroupNCCL watchdog thread polls hipEventQuery on the warm-up collectives while the
# main thread captures, and in the default (global) mode that query invalidates the capture and aborts the process (seen 1 run in 6).
CAPTURE_MODE = "thread_local"


def sample_power(keep_busy, seconds=2.5):
    """Package power and shader clock while `keep_busy()` (one untimed call = `steps` steps of the timed workload, synchronised) loops: an
    UNTIMED leg after the timed repetitions.  The headline kernels run at the package power cap (1.35 kW of 1.40 kW during
    the recurrence, shader clock 1.8-2.2 GHz instead of 2.4), so `roofline.frac` is read next to these two numbers.  None when rocm-smi is
    absent, fails or BENCH_NO_POWER is set."""
    import re
    import shutil
    import subprocess
    import threading
    smi = shutil.which("rocm-smi") or "/opt/rocm/bin/rocm-smi"
    if os.environ.get("BENCH_NO_POWER") or not os.path.exists(smi):
        return None
    dev = os.environ.get("LOCAL_RANK", "0")
    got, stop = [], threading.Event()

    def ask(*flags):
        return subprocess.run([smi, "-d", dev] + list(flags), capture_output=True, text=True, timeout=20).stdout

    def poll():
        while not stop.is_set():
            try:
                out = ask("--showpower", "--showclocks")
                w = re.search(r"Power \(W\):\s*([0-9.]+)", out)
                f = re.search(r"sclk clock level:[^(]*\(([0-9.]+)Mhz\)", out)
                if w:
                    got.append((float(w.group(1)), float(f.group(1)) if f else None))
            except Exception:
                return
    try:
        th = threading.Thread(target=poll, daemon=True)
        t0 = time.perf_counter()
        keep_busy()
        th.start()
        while time.perf_counter() - t0 < seconds or len(got) < 2:
            keep_busy()
            if time.perf_counter() - t0 > 4 * seconds + 10:
                break
        stop.set()
        th.join(timeout=25)
        cap = re.search(r"Max Graphics Package Power \(W\):\s*([0-9.]+)", ask("--showmaxpower"))
    except Exception:
        stop.set()
        return None
    if not got:
        return None
    ws = sorted(w for w, _ in got)
    fs = sorted(f for _, f in got if f)
    return {"package_w": ws[len(ws) // 2], "package_w_max": ws[-1], "cap_w": float(cap.group(1)) if cap else None,
            "sclk_mhz": fs[len(fs) // 2] if fs else None, "samples": len(got),
            "leg": "untimed: the timed region replayed for %.1f s after the timed repetitions, rocm-smi polled beside it" % (time.perf_counter() - t0)}


def _phase(name, what):
    """BENCH_PHASES=<file>: append "record: phase" lines (synchronised) -- locates a device fault, which arrives asynchronously and without a Python trace"""
    path = os.environ.get("BENCH_PHASES")
    if path:
        torch.cuda.synchronize()
        with open(path, "a") as f:
            f.write("%s: %s\n" % (name, what))


def run_config(name, c, args, env, steps, warmup, shard, want_cpu=False, with_h2d=False, axis=None, kg=None, dump=None, lean=False):
    """Time one workload; returns the record dict (rank 0) or None.  dump: directory for the outputs of the last timed step (write_outputs).
    lean: set-up, warm-up and the timed steps only -- no precompute, power, one-batch / overlap, profile or checker legs (their fields are None)."""
    _phase(name, "start")
    L = lib.load()
    dev, world, rank = env.dev, env.world, env.rank
    adhoc_power_off = bool(os.environ.get("BENCH_NO_POWER"))
    is_sess = c["model"] in SESSION_MODELS
    sharded = shard and env.multi
    # lane-count tuning aid (never set by the driver): BENCH_FORCE_DIST=1 BENCH_EMULATE_WORLD=W on ONE GPU gives this process rank 0's
    # 1/W candidate shard and a W-shard gather buffer (the other shards stay zero), so the per-rank GPU work of an N=W run can be
    # timed here; the scores are meaningless and the cross-GPU latency of the collective is not included.
    wsh = world
    if world == 1 and env.multi and os.environ.get("BENCH_EMULATE_WORLD"):
        wsh = int(os.environ["BENCH_EMULATE_WORLD"])
    emu = wsh != world
    model = build_model(c, args)
    pre = precompute_info(model, c) if rank == 0 and not lean else None
    # batches in flight: --streams lanes (BENCH_SHARD_LANES overrides it for the sharded CARS step)
    nlanes = max(1, args.streams)
    if sharded and c["model"] == "cars" and wsh > 1 and env.backend == "nccl":
        nlanes = int(os.environ.get("BENCH_SHARD_LANES", nlanes))       # (8 lanes measured SLOWER than 4 in the 8-rank emulation: C3 0.111 vs 0.097 ms)
    nbatches = (max(args.nbatches, nlanes) + nlanes - 1) // nlanes * nlanes
    if c["model"] == "cars" or not env.multi:       # macro-batched paths: every lane gets whole groups of KG batches
        kg = kg or macro_batch(c, "BENCH_GATHER_EVERY" if env.multi else "BENCH_MACRO_BATCH", wsh if (env.multi and sharded and c["model"] == "cars") else 1)
        nbatches = (max(args.nbatches, kg * nlanes) + kg * nlanes - 1) // (kg * nlanes) * (kg * nlanes)
    # strong scaling: identical global batches on every rank; weak (shard=False at N>1): independent per-rank batches
    batches = make_batches(c, nbatches, 0 if sharded or not env.multi else rank, dev)
    pairs_global = c["batch"] * c["cands"] * (c["session"] if is_sess else 1)
    ncand = c["cands"]
    plan = None
    if sharded and c["model"] == "cars":
        # round 3: candidate-sharded encode -> all-to-all -> session-sharded tail -> all-gather of the probabilities (sharding.SessionShardPlan);
        # every per-rank input slice is resident in HBM like the full batch would be
        # BENCH_SHARD_AXIS: "auto" (default) = the flattened (session, candidate) pair axis in contiguous chunks when B % world == 0 -- each rank
        # then encodes ALL candidates of B/world whole sessions: no padding of the candidate axis, no exchange of pooled vectors, only the
        # all-gather of the probabilities -- else the candidate axis with the all-to-all exchange; "candidate" / "pair" force one of them
        plan = sharding.SessionShardPlan(c["batch"], c["session"], ncand, wsh, rank, axis=axis or os.environ.get("BENCH_SHARD_AXIS", "auto"))
        for b in batches:
            b["_q_own"], b["_ql_own"] = plan.own(b["source_words"]), plan.own(b["source_lens"])
            b["_doc_shard"], b["_len_shard"] = plan.doc_shard(b["document_words"], b["document_lens"])
            b["_lab_own"] = plan.own(b["document_labels"])
    elif sharded and is_sess:
        model.parallelize()
    if sharded and not is_sess:       # pre-slice this rank's candidate shard (resident in HBM like the full batch would be)
        for b in batches:
            b["doc_rep"], b["doc_len"] = sharding.shard_candidates(b["doc_rep"], b["doc_len"], wsh, rank)

    coll = {}       # per (batch slot) exchange / gather buffers of the sharded CARS step

    def cars_bufs(key, D=256):
        if key not in coll:
            G, bper, S_, per = plan.world, plan.bper, plan.S, plan.per
            coll[key] = (torch.zeros(G, bper, S_, per, D, device=dev), torch.zeros(bper, S_, ncand, device=dev),
                         torch.zeros(G * bper, S_, ncand, device=dev))
        return coll[key]

    # one candidate-/session-sharded CARS ranking step in four pieces (eager or under capture): encode | exchange | tail | gather.
    # via_gather: the exchange as all_gather_into_tensor (every slice to every rank, own sessions' chunk kept) -- the form RCCL can replay
    # from a captured hipGraph; else all_to_all_single (1/G of the bytes, eager only).
    def cars_encode(ex):
        return model.shard_encode(ex["_q_own"], ex["_ql_own"], ex["_doc_shard"], ex["_len_shard"])

    def cars_exchange(key, pl, via_gather):
        if plan.aligned:                                     # pair axis: this rank encoded all candidates of its own sessions
            return pl.view(1, *pl.shape)
        recv = cars_bufs(key)[0]
        if via_gather:
            if (key, "g") not in coll:
                coll[(key, "g")] = torch.zeros(plan.world, plan.world * plan.bper, plan.S, plan.per, pl.shape[-1], device=dev)
            big = coll[(key, "g")]
            # (emulated world: the 1-rank group fills chunk 0 only; the tail reads rank 0's session block of every chunk all the same)
            env.dist.all_gather_into_tensor(big[:1].view(pl.shape) if emu else big.view(-1, *pl.shape[1:]), pl)
            return big[:, rank * plan.bper:(rank + 1) * plan.bper]
        if env.backend == "nccl":
            # (emulated world: the 1-rank group copies the whole buffer -- the bytes a real exchange moves, meaningless scores)
            env.dist.all_to_all_single(recv.view(pl.shape), pl)
        else:
            h = torch.empty(pl.shape)
            env.dist.all_to_all_single(h, pl.cpu())
            recv.view(pl.shape).copy_(h)
        return recv

    def cars_tail(ex, key, pq, recv):
        return model.shard_tail(pq, recv, ex["_lab_own"], ex["document_labels"], ncand, cars_bufs(key)[1])

    def cars_gather(key, probs_own):
        allp = cars_bufs(key)[2]
        if env.backend == "nccl":
            env.dist.all_gather_into_tensor(allp[:plan.bper] if emu else allp, probs_own)
        else:
            h = torch.empty(allp.shape)
            env.dist.all_gather_into_tensor(h, probs_own.cpu())
            allp.copy_(h)
        return allp[:c["batch"]]

    def sharded_cars_step(ex, key, via_gather=False):
        pq, pl = cars_encode(ex)
        return cars_gather(key, cars_tail(ex, key, pq, cars_exchange(key, pl, via_gather)))

    def forward(i):
        ex = batches[i % len(batches)]
        if plan is not None:
            return sharded_cars_step(ex, ("eager", i % len(batches)))
        if is_sess:
            return model.predict(ex, suggest=False)["click_scores"]
        s = model.network(ex["que_rep"], ex["que_len"], ex["doc_rep"], ex["doc_len"])
        if sharded:
            return s
        out = torch.empty_like(s)
        lib.check(L.nir_softmax_rows(lib.ptr(s), lib.ptr(out), s.shape[0], s.shape[1], lib.stream()), "softmax")
        return out

    lanes = [torch.cuda.Stream() for _ in range(nlanes)]
    fbufs = [None] * len(lanes)
    # Candidate-/session-sharded CARS over RCCL.  Default: PIPELINED -- per lane and step ONE hipGraph replay ( tail of the lane's previous
    # step ; encode of this step ) and ONE eager all_to_all_single that carries this step's pooled candidate slices out and the previous
    # step's click probabilities to everybody (sharding.SessionShardPipeline): 2 host calls per step, collectives of all lanes in issue
    # order on the process group's communication stream (identical on every rank).  Opt-in (BENCH_FUSED_GRAPH=1): FUSED graphs -- KSTEP
    # whole steps, kernels and collectives, captured into one hipGraph as parallel branches (measured slower: the runtime runs the branches
    # of one graph with far less overlap than separate streams get).  Fallback: eager.
    fused_ok = plan is not None and env.backend == "nccl" and not args.no_graph and bool(os.environ.get("BENCH_FUSED_GRAPH"))
    staged = plan is not None and env.backend == "nccl" and not args.no_graph
    KSTEP = max(1, int(os.environ.get("BENCH_KSTEP", "8")))
    def finish(s):
        """cross-rank part of a ranker step (eager): one all-gather of the score shards, softmax over all candidates."""
        if not sharded or is_sess:
            return s
        if env.backend == "nccl":
            cur = torch.cuda.current_stream()
            ln = lanes.index(cur) if cur in lanes else 0
            if fbufs[ln] is None:
                fbufs[ln] = (torch.zeros(wsh * s.shape[0], s.shape[1], device=dev), torch.empty(s.shape[0], ncand, device=dev))
            gbuf, probs = fbufs[ln]
            env.dist.all_gather_into_tensor(gbuf[:s.shape[0]] if emu else gbuf, s.contiguous())
            lib.check(L.nir_softmax_gathered(lib.ptr(gbuf), lib.ptr(probs), None, wsh, s.shape[0], s.shape[1], ncand, lib.stream()),
                      "nir_softmax_gathered")
            return probs
        full = sharding.gather_scores(s.cpu(), ncand).to(dev)
        out = torch.empty_like(full)
        lib.check(L.nir_softmax_rows(lib.ptr(full), lib.ptr(out), full.shape[0], full.shape[1], lib.stream()), "softmax")
        return out

    # several batches in flight: the library drops its own query/document fork and packs fuller workgroups
    hint = args.in_flight_hint or len(lanes)
    lib.set_batches_in_flight(hint, lanes)             # per stream: the hint travels with the lane, nothing process-wide is mutated
    lane_of = lambda i: (i % len(batches)) % len(lanes)   # noqa: E731
    torch.cuda.set_stream(lanes[0])
    for i in range(max(2, min(warmup, 3)) * len(lanes)):
        with torch.cuda.stream(lanes[lane_of(i)]):
            finish(forward(i))
    torch.cuda.synchronize()
    graphs = None
    stages = None
    if env.multi:
        time.sleep(0.3)      # let the RCCL watchdog (100 ms poll) retire the finished warm-up collectives before any capture starts
    fused = None
    if fused_ok:
        try:
            probe_a = torch.zeros(1, 8, device=dev); probe_b = torch.zeros(world, 8, device=dev)
            env.dist.all_gather_into_tensor(probe_b, probe_a)
            torch.cuda.synchronize()
            time.sleep(0.3)
            pg = torch.cuda.CUDAGraph()                       # does this build capture a collective at all?
            with torch.cuda.graph(pg, stream=lanes[0], capture_error_mode=CAPTURE_MODE):
                env.dist.all_gather_into_tensor(probe_b, probe_a)
            pg.replay()
            torch.cuda.synchronize()
            branches = [torch.cuda.Stream() for _ in range(KSTEP)]
            lib.set_batches_in_flight(KSTEP, branches + lanes)

            def capture_group(first, n):
                """n consecutive steps (batches first .. first+n-1) as parallel branches of ONE graph; returns (graph, outputs)."""
                keys = [("fused", first, j) for j in range(n)]
                for j in range(n):                               # warm: packs, workspaces, collective buffers
                    with torch.cuda.stream(branches[j]):
                        sharded_cars_step(batches[(first + j) % len(batches)], keys[j], via_gather=True)
                torch.cuda.synchronize()
                time.sleep(0.3)
                g, outs = torch.cuda.CUDAGraph(), []
                exs = [batches[(first + j) % len(batches)] for j in range(n)]
                with torch.cuda.graph(g, stream=lanes[0], capture_error_mode=CAPTURE_MODE):
                    main = torch.cuda.current_stream()
                    # captured PHASE by phase, not step by step: the process group runs its collectives in issue order on ONE
                    # communication stream, so "exchange_1 after gather_0" would chain the branches end to end (measured: 8 branches took
                    # 8 x the one-in-flight latency).  Issue order on that stream here: exchange_0 .. exchange_n-1, gather_0 .. gather_n-1.
                    enc, rcv, prb = [None] * n, [None] * n, [None] * n
                    for j in range(n):
                        branches[j].wait_stream(main)
                        with torch.cuda.stream(branches[j]):
                            enc[j] = cars_encode(exs[j])
                    for j in range(n):
                        with torch.cuda.stream(branches[j]):
                            rcv[j] = cars_exchange(keys[j], enc[j][1], True)
                    for j in range(n):
                        with torch.cuda.stream(branches[j]):
                            prb[j] = cars_tail(exs[j], keys[j], enc[j][0], rcv[j])
                    for j in range(n):
                        with torch.cuda.stream(branches[j]):
                            outs.append(cars_gather(keys[j], prb[j]))
                    for j in range(n):
                        main.wait_stream(branches[j])
                return g, outs
            fused = {"full": [capture_group(0, KSTEP), capture_group(KSTEP, KSTEP)], "rem": {}, "capture": capture_group}
            staged = False
        except Exception as e:  # pragma: no cover - falls back to staged graphs around eager collectives
            print("[bench] collectives could not be captured for %s (%s: %s); staged graphs" % (name, type(e).__name__, e), file=sys.stderr)
            fused = None
            try:
                torch.cuda.synchronize()
            except Exception:
                pass
            lib.set_batches_in_flight(hint, lanes)
    _phase(name, "setup done, capturing")
    macro_single = (plan is None and (not env.multi or not sharded) and macro_batch(c) > 1
                    and c["model"] in ("cars", "m_match_tensor", "mnsrf", "match_tensor", "esm", "drmm", "duet"))
    if (staged and plan.aligned) or macro_single:
        try:
            # pair axis: a lane's hipGraph holds KG whole steps ( encode own sessions -> tail -> probabilities ) merged into one macro-batch,
            # followed by ONE eager all-gather of the KG probability blocks.  Results lag by at most KG - 1 steps.
            KG = kg or macro_batch(c, "BENCH_MACRO_BATCH" if macro_single else "BENCH_GATHER_EVERY", 1 if macro_single else wsh)
            nl, nb = len(lanes), len(batches)
            agroups = {}
            gbuf = {}
            macro_inputs, eager_fns = {}, {}
            bper_, S_ = (c["batch"], c.get("session", 1) if is_sess else 1) if macro_single else (plan.bper, plan.S)

            def group_bufs(gb, k):
                if (gb, k) not in gbuf:
                    gbuf[(gb, k)] = (torch.zeros(k, bper_, S_, ncand, device=dev),
                                     None if macro_single else torch.zeros(plan.world, k, bper_, S_, ncand, device=dev))
                return gbuf[(gb, k)]

            def capture_aligned(gb, k):
                """steps on batches KG*gb .. KG*gb + k - 1 (mod nb), lane gb % nl"""
                ln = lanes[gb % nl]
                mine, allg = group_bufs(gb, k)
                if macro_single:
                    # single GPU: the k batches are resident as ONE macro-batch (concatenated once, here, outside the graph -- exactly what the
                    # host-fed stream's collator produces): the replayed graph holds the library's kernels only, no torch.cat / copy launches
                    exs = [batches[(KG * gb + j) % nb] for j in range(k)]
                    keys = ("source_words", "source_lens", "document_words", "document_lens", "document_labels") if is_sess else ("que_rep", "que_len", "doc_rep", "doc_len")
                    with torch.cuda.stream(ln):               # (on the lane that reads it: a remainder group is built while other lanes' graphs run)
                        mb = {key: (torch.cat([e[key] for e in exs]).contiguous() if k > 1 else exs[0][key]) for key in keys}
                    ln.synchronize()
                    macro_inputs[(gb, k)] = mb

                    def body1():
                        if is_sess:       # Multitask.predict_groups: every batch of the macro-batch keeps its own click count
                            model.predict_groups(mb, k, out=mine.view(k * bper_, S_, ncand))
                        else:             # rankers: every (query, candidate) pair is independent of the rest of its batch
                            s_ = model.network(mb["que_rep"], mb["que_len"], mb["doc_rep"], mb["doc_len"]).contiguous()
                            lib.check(L.nir_softmax_rows(lib.ptr(s_), lib.ptr(mine), s_.shape[0], s_.shape[1], lib.stream()), "softmax")
                    eager_fns[(gb, k)] = body1
                    with torch.cuda.stream(ln):
                        body1()
                    torch.cuda.synchronize()
                    if args.no_graph:                         # (profiling runs: the same macro-batched launches, eagerly)
                        return type("Eager", (), {"replay": staticmethod(body1)})(), mine, None
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=ln, capture_error_mode=CAPTURE_MODE):
                        body1()
                    return g, mine, None

                # the k blocks (this rank's sessions of k consecutive batches) run as ONE macro-batch: one encode over k x the sequences, one
                # tail over k x bper sessions -- the session LSTM / ranknet weights (76 MB of L2 traffic per tail at C3, whatever the number
                # of sessions) are streamed once for all k; every block keeps the click count m of ITS OWN batch (labels_groups)
                exs = [batches[(KG * gb + j) % nb] for j in range(k)]
                with torch.cuda.stream(ln):                   # (built on the lane that reads it, like the single-GPU macro-batches)
                    mq, mql = torch.cat([e["_q_own"] for e in exs]), torch.cat([e["_ql_own"] for e in exs])
                    md, ml = torch.cat([e["_doc_shard"] for e in exs]), torch.cat([e["_len_shard"] for e in exs])
                    mlab, mall = torch.cat([e["_lab_own"] for e in exs]), torch.stack([e["document_labels"] for e in exs])
                ln.synchronize()

                # (the graph below reads these tensors on every replay: they must outlive this function -- until round 6 they did not, and a later
                # group's inputs could be allocated over them; with the allocator handing the segment back, a replay faulted)
                macro_inputs[(gb, k)] = (mq, mql, md, ml, mlab, mall)

                def body():
                    pq, pl = model.shard_encode(mq, mql, md, ml)
                    model.tail_probs(pq, pl, mlab, None, probs=mine.view(k * plan.bper, plan.S, ncand), labels_groups=mall)
                eager_fns[(gb, k)] = body
                with torch.cuda.stream(ln):
                    body()
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=ln, capture_error_mode=CAPTURE_MODE):
                    body()
                return g, mine, (allg[:1] if emu else allg)      # noqa: E501

            ngroups = (nb + KG - 1) // KG
            for gb in range(ngroups):
                agroups[(gb, KG)] = capture_aligned(gb, KG)
            stages = {"aligned": agroups, "capture": capture_aligned, "KG": KG, "ngroups": ngroups, "nl": nl, "pos": 0, "graphed": not args.no_graph, "eager": eager_fns}
        except Exception as e:  # pragma: no cover
            print("[bench] graph capture unavailable for %s (%s: %s); eager sharded steps" % (name, type(e).__name__, e), file=sys.stderr)
            stages = None
            torch.cuda.synchronize()
    elif staged:
        try:
            nl, nb = len(lanes), len(batches)
            pipes = [sharding.SessionShardPipeline(plan, 256, dev) for _ in lanes]
            pq_buf = [torch.zeros(plan.bper, plan.S, 256, device=dev) for _ in batches]      # pooled queries of a step, kept for its tail

            def segment(b, do_tail, do_encode):
                """compute segment of batch b on its lane: tail of the lane's PREVIOUS batch (its pooled documents arrived with the last
                exchange), then encode of b."""
                pp, pb = pipes[b % nl], (b - nl) % nb
                if do_tail:
                    pp.put_probs(model.shard_tail(pq_buf[pb], pp.got_pooled(), batches[pb]["_lab_own"], batches[pb]["document_labels"], ncand))
                if do_encode:
                    pq, pl = cars_encode(batches[b])
                    pq_buf[b].copy_(pq)
                    pp.put_pooled(pl)

            def exchange(ln):       # (emulated world: the 1-rank group copies the whole buffer -- the bytes a real exchange moves)
                env.dist.all_to_all_single(pipes[ln].recv, pipes[ln].send)

            for b in range(nb):                                 # warm: packs, workspaces, communicator
                with torch.cuda.stream(lanes[b % nl]):
                    segment(b, True, True)
                    exchange(b % nl)
            torch.cuda.synchronize()
            time.sleep(0.3)
            seg_graphs = {}
            for b in range(nb):     # "full" = steady state; "first" = encode only (pipeline start); "flush" = tail only (delivers the last step)
                for kind, (dt, de) in (("full", (True, True)), ("first", (False, True)), ("flush", (True, False))):
                    g = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(g, stream=lanes[b % nl], capture_error_mode=CAPTURE_MODE):
                        segment(b, dt, de)
                    seg_graphs[(b, kind)] = g
            stages = {"graphs": seg_graphs, "exchange": exchange, "pipes": pipes, "pos": 0, "nl": nl, "nb": nb}
        except Exception as e:  # pragma: no cover - falls back to the eager sharded step
            print("[bench] pipelined graph capture unavailable for %s (%s: %s); eager sharded steps" % (name, type(e).__name__, e), file=sys.stderr)
            stages = None
            torch.cuda.synchronize()
    # the sharded CARS step contains a collective (all-gather of the pooled documents) between its kernels: staged graphs above, else eager
    use_graph = not args.no_graph and not (sharded and is_sess) and not (env.backend != "nccl" and env.multi) and fused is None and stages is None
    if use_graph:
        try:
            graphs = []
            for i in range(len(batches)):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=lanes[lane_of(i)], capture_error_mode=CAPTURE_MODE):
                    out = forward(i)
                graphs.append((g, out))
        except Exception as e:  # pragma: no cover - graph capture is an optimisation only
            print("[bench] graph capture unavailable for %s (%s); timing eager launches" % (name, e), file=sys.stderr)
            graphs = None
            torch.cuda.synchronize()

    _phase(name, "graphs captured")
    def run(i, only_lane=None):
        ln = lane_of(i) if only_lane is None else only_lane
        with torch.cuda.stream(lanes[ln]):
            if graphs is not None:
                g, out = graphs[i % len(graphs)]
                g.replay()
            else:
                out = forward(i)
            return finish(out)

    final = {"step": None}     # -> the output tensor of the last step run_steps issued (what a caller of that step receives; --dump-outputs)

    def run_steps(n):
        """exactly n steps: pipelined segments (sharded CARS), fused groups of KSTEP (+ one remainder group) on one stream, else one
        replay / eager call per step."""
        if stages is not None and "aligned" in stages:
            KG, gi, left = stages["KG"], stages["pos"], n
            while left > 0:
                k = min(KG, left)
                gb = gi % stages["ngroups"]
                if (gb, k) not in stages["aligned"]:           # remainder group (captured before the timed region, see below)
                    stages["aligned"][(gb, k)] = stages["capture"](gb, k)
                g, mine, allg = stages["aligned"][(gb, k)]
                with torch.cuda.stream(lanes[gb % stages["nl"]]):
                    g.replay()
                    if allg is not None:
                        env.dist.all_gather_into_tensor(allg.view(-1, *mine.shape[1:]), mine)     # [G*k, bper, S, N] <- [k, bper, S, N]
                # step k-1 of the group: this rank's block of the macro-batch, or every rank's sessions of it from the all-gather
                final["step"] = (lambda m=mine, a=allg, j=k - 1: m[j] if a is None else a[:, j].reshape(-1, *m.shape[2:])[:c["batch"]])
                gi += 1
                left -= k
            stages["pos"] = gi
            return
        if stages is not None:
            # n encodes + n tails: every lane starts with an encode-only segment, runs full segments, and ends with a tail-only segment +
            # exchange that delivers the probabilities of its last step (the results of step k arrive with the exchange of step k + lanes)
            nl, nb, G = stages["nl"], stages["nb"], stages["graphs"]
            start, last = stages["pos"], {}
            for i in range(start, start + n):
                b = i % nb
                ln = b % nl
                with torch.cuda.stream(lanes[ln]):
                    G[(b, "full" if ln in last else "first")].replay()
                    stages["exchange"](ln)
                last[ln] = b
            for ln, b in last.items():
                with torch.cuda.stream(lanes[ln]):
                    G[((b + nl) % nb, "flush")].replay()
                    stages["exchange"](ln)
            stages["pos"] = start + n
            final["step"] = None      # (the probabilities live in the pipelines' exchange buffers: not dumped)
            return
        if fused is None:
            out = None
            for i in range(n):
                out = run(i)
            final["step"] = lambda o=out: o
            return
        with torch.cuda.stream(lanes[0]):
            for k in range(n // KSTEP):
                fused["full"][k % 2][0].replay()
                final["step"] = lambda o=fused["full"][k % 2][1][-1]: o
            rem = n % KSTEP
            if rem:
                if rem not in fused["rem"]:
                    fused["rem"][rem] = fused["capture"](2 * KSTEP, rem)
                fused["rem"][rem][0].replay()
                final["step"] = lambda o=fused["rem"][rem][1][-1]: o

    def rewind():
        """every call pattern starts from the same group position: the remainder groups captured in the dry run are the ones the timed
        repetitions replay (no capture inside a timed region)"""
        if stages is not None:
            stages["pos"] = 0

    patterns = (max(warmup, 1), steps) + (() if lean else (max(6, min(steps, 60)),))      # (the last: the one-batch / overlap check's)
    if stages is not None and "aligned" in stages:      # dry run of every call pattern below: remainder groups get captured now
        for n in patterns:
            rewind()
            run_steps(n)
        torch.cuda.synchronize()
    if fused is not None:                    # remainder groups are captured before the timed region
        for n in {p % KSTEP for p in patterns} - {0}:
            fused["rem"][n] = fused["capture"](2 * KSTEP, n)
    rewind()
    run_steps(max(warmup, 1))

    if dump and stages is not None and "aligned" not in stages:      # (every rank takes this exit: the arguments are the same on all of them)
        raise SystemExit("bench.py: --dump-outputs is not available on the software-pipelined candidate-axis path of %s" % name)

    _phase(name, "timed region")
    def timed_region():
        """EXACTLY `steps` steps between barrier + synchronize on both sides; returns (max-over-ranks seconds, host enqueue seconds)"""
        rewind()
        torch.cuda.synchronize()
        env.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run_steps(steps)
        host = time.perf_counter() - t0
        torch.cuda.synchronize()
        env.barrier()
        torch.cuda.synchronize()
        return env.max_over_ranks(time.perf_counter() - t0), host

    # A short region (the driver's --steps 20 is ~3 ms of GPU time here) is one sample of launch jitter: when steps x ms_per_step < 0.25 s the
    # SAME `steps`-step region is repeated and the MEDIAN repetition is the one reported (`reps`; `steps` stays the argument).  The count
    # follows from the first repetition's max-over-ranks time, so every rank repeats equally often.
    first, host_s = timed_region()
    reps = 1
    if first < MIN_REGION_S:
        reps = int(min(MAX_REPS, max(3, np.ceil(MIN_REGION_S / max(first, 1e-6))))) | 1
    samples = [first] + [timed_region()[0] for _ in range(reps - 1)]
    elapsed = float(np.median(samples))
    host_ms = host_s / steps * 1e3
    per_step_pairs = pairs_global if (sharded or not env.multi) else pairs_global * world
    value = per_step_pairs * steps / elapsed
    ms_per_step = elapsed / steps * 1e3
    spread = (round(min(samples) / steps * 1e3, 5), round(max(samples) / steps * 1e3, 5))
    if dump and rank == 0:           # every repetition replays the same steps: the buffers hold the last timed step's result
        probs = final["step"]().reshape(c["batch"], *((c["session"],) if is_sess else ()), ncand)
        write_outputs(dump, {"click_scores" if is_sess else "scores": probs})
    power = None
    if rank == 0 and not env.multi and not adhoc_power_off and not lean:        # every N = 1 record: which configurations run at the package power cap
        def busy():
            rewind()
            run_steps(steps)
            torch.cuda.synchronize()
        power = sample_power(busy, 2.5 if want_cpu else 1.5)

    _phase(name, "single / overlap check")
    single_ms, overlap_diff = (None if lean else ms_per_step), None
    if len(lanes) > 1 and not lean:
        if graphs is not None and not sharded:
            # concurrent-vs-serial check of EVERY captured graph.  (Round 4 cloned the outputs the timed region happened to leave behind: with
            # more resident batches than steps + warm-up -- X3_mnsrf: 32 graphs, 30 steps, 8 warm-up replays -- the last graphs had never
            # been replayed, and their never-written output buffers were compared with a real result: the 0.2068 of r04_bench_detail.json
            # was max(probability) of batch 31, not a race.)  Now: two rounds of all graphs with every lane in flight, then each alone.
            for _ in range(2):
                for j, (g, _) in enumerate(graphs):
                    with torch.cuda.stream(lanes[lane_of(j)]):
                        g.replay()
            torch.cuda.synchronize()
            conc = [out.clone() for _, out in graphs]
            torch.cuda.synchronize()
            overlap_diff = 0.0
            for j, (g, out) in enumerate(graphs):
                with torch.cuda.stream(lanes[lane_of(j)]):
                    g.replay()
                torch.cuda.synchronize()
                overlap_diff = max(overlap_diff, float((out - conc[j]).abs().max()))
            if not (overlap_diff <= OVERLAP_TOL):          # also catches NaN
                raise RuntimeError("%s: %d lanes in flight change the result of the same captured graphs by %.3g (> %.0e)" % (
                    name, len(lanes), overlap_diff, OVERLAP_TOL))
        ns = max(6, min(steps, 60))
        torch.cuda.synchronize()
        env.barrier()
        ts = time.perf_counter()
        if macro_single and stages is not None and stages["graphed"]:
            # macro-batched single-GPU path: the latency figure is ONE batch through its own hipGraph, nothing else in flight; and the
            # macro-batched probabilities are checked against that single-batch path
            g1 = torch.cuda.CUDAGraph()
            lib.set_batches_in_flight(1, lanes[:1])        # a lone batch: the library forks its query / document chains onto two streams
            with torch.cuda.stream(lanes[0]):
                forward(0)
            torch.cuda.synchronize()
            with torch.cuda.graph(g1, stream=lanes[0], capture_error_mode=CAPTURE_MODE):
                o1 = forward(0)
            torch.cuda.synchronize()
            ts = time.perf_counter()
            with torch.cuda.stream(lanes[0]):
                for i in range(ns):
                    g1.replay()
            torch.cuda.synchronize()
            single_ms = (time.perf_counter() - ts) / ns * 1e3
            lib.set_batches_in_flight(hint, lanes[:1])
            mg_, mine_, _ = stages["aligned"][(0, stages["KG"])]
            with torch.cuda.stream(lanes[0]):
                mg_.replay()
            torch.cuda.synchronize()
            overlap_diff = float((mine_[0].reshape(o1.shape) - o1).abs().max())
            ts = None
        elif fused is not None or stages is not None:   # (fused / pipelined steps: "one in flight" has no separate meaning there)
            rewind()
            run_steps(ns)
        else:
            for i in range(ns):
                run(i, only_lane=0)
        torch.cuda.synchronize()
        if ts is not None:
            single_ms = (time.perf_counter() - ts) / ns * 1e3
        env.barrier()

    # ---- H2D-inclusive figure: ids arrive from the HOST for every batch (collate into pinned staging -> H2D -> replay -> D2H of the
    # probabilities), sustained over >= 5 s regardless of --steps.  CARS: graph_runner.StreamingSessionPredictor (int32 wire format,
    # 2 staging slots per lane, producer thread); rankers: GraphedPredictor fed from packed pinned batches.
    h2d_value, h2d_info, sustained = None, None, None
    if with_h2d and world == 1 and not env.multi and not os.environ.get("BENCH_NO_H2D"):
        try:
            secs = float(os.environ.get("BENCH_H2D_SECONDS", "5"))
            # the RESIDENT loop over the same protocol as the H2D-inclusive figure below (sustained for the same seconds, one synchronise at the
            # end): the ratio of the two is then an H2D cost, not a difference between a 3 ms median region and a 5 s window
            rewind()
            torch.cuda.synchronize()
            ts_, ns_ = time.perf_counter(), 0
            while time.perf_counter() - ts_ < secs:
                run_steps(steps)
                ns_ += steps
                if ns_ % (8 * steps) == 0:
                    torch.cuda.synchronize()              # (bounded queue depth, like the streaming path's slots)
            torch.cuda.synchronize()
            sustained = per_step_pairs * ns_ / (time.perf_counter() - ts_)
            if c["model"] == "cars":
                from context_attentive_ir_amd.graph_runner import StreamingSessionPredictor
                from context_attentive_ir_amd.inputters import SyntheticSessionCorpus
                corpus = SyntheticSessionCorpus(n_sessions=64 * c["batch"], n_cands=c["cands"], qlen=c["qlen"], dlen=c["dlen"], vocab=c["vocab"],
                                                fixed_len=c["session"], pool=64)
                mk = macro_batch(c)
                sp = StreamingSessionPredictor(model, c["cands"], c["qlen"], c["dlen"], mk * c["batch"], max_session_len=c["session"],
                                               lanes=len(lanes), slots=2, macro=mk)
                bl, _ = sp.merge_batches(corpus, corpus.batches(c["batch"]), mk)
                sp.prepare([c["session"]], example=(corpus, bl[0]))
                sp.run(corpus, bl, max_batches=8 * len(lanes))
                h2d_info = sp.run(corpus, bl, min_seconds=secs)
                h2d_value = h2d_info["pairs_per_s"]
                h2d_info = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in h2d_info.items()}
                h2d_info["wire"] = "int32 ids/lengths + float32 labels, widened on device (nir_widen_ids_i32)"
                h2d_info["macro_batch"] = mk
                del sp
            else:
                from context_attentive_ir_amd.graph_runner import GraphedPredictor
                gps = [GraphedPredictor(model, batches[0], queue_ahead=len(lanes) == 1) for _ in lanes]
                host = [gps[0].pack({k: v.cpu() for k, v in b.items()}) for b in batches]
                for i in range(3 * len(gps)):
                    gps[i % len(gps)].predict(host[i % len(host)], clone=False)
                torch.cuda.synchronize()
                th, nh = time.perf_counter(), 0
                while time.perf_counter() - th < secs:
                    for _ in range(16):
                        gps[nh % len(gps)].predict(host[nh % len(host)], clone=False)
                        nh += 1
                torch.cuda.synchronize()
                h2d_value = pairs_global * nh / (time.perf_counter() - th)
                h2d_info = {"batches": nh, "seconds": round(time.perf_counter() - th, 3), "wire": "int64 (the reference's LongTensor batch), one pinned buffer per batch"}
            lib.set_batches_in_flight(hint, lanes)
        except Exception as e:  # pragma: no cover - secondary figure only
            print("[bench] H2D-inclusive figure unavailable: %s: %s" % (type(e).__name__, e), file=sys.stderr)

    roofline = None
    if not lean:
        _phase(name, "profile pass")
        # ---- profiled pass: HIP events around every kernel of the library, same workload, serial -------------------
        torch.cuda.set_stream(lanes[0])
        lib.set_batches_in_flight(hint, lanes)
        nprof = max(4, min(steps, 30))
        L.nir_debug_set_tunable(b"no_fork", 1)          # time every kernel in isolation (no query/document stream overlap)
        if rank == 0:
            L.nir_profile_enable(1)
        prof_div = nprof
        if macro_single and stages is not None:        # the launches of the timed region: macro-batches of KG batches
            KGp = stages["KG"]
            for i in range(max(2, nprof // KGp)):
                stages["eager"][(i % stages["ngroups"], KGp)]()
            prof_div = max(2, nprof // KGp) * KGp
        else:
            for i in range(nprof):
                finish(forward(i))
        torch.cuda.synchronize()
        L.nir_profile_enable(0)
        L.nir_debug_set_tunable(b"no_fork", 0)
    if rank == 0 and not lean:
        buf = ctypes.create_string_buffer(1 << 17)
        L.nir_profile_report(buf, len(buf))
        kern = {}
        for line in buf.value.decode().strip().splitlines():
            kname, cnt, ms = line.rsplit(",", 2)
            kern[kname] = (int(cnt), float(ms))
        if kern:
            dom = max(kern, key=lambda k: kern[k][1])
            cnt, ms = kern[dom]
            avg_us = ms / cnt * 1e3
            roofline = {"kernel": dom, "avg_us": round(avg_us, 3), "launches_per_step": cnt / prof_div,
                        "kernels_us_per_step": {k: round(v[1] / prof_div * 1e3, 2) for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1])}}
            cc = dict(c)
            if sharded and not is_sess:
                cc["cands"] = batches[0]["doc_rep"].shape[1]
            bpp = algorithmic_bytes_per_pair(c["cands"], c["qlen"], c["dlen"], table_bytes=2 if c.get("dtype") == "bf16" else 4)
            step_pairs_rank = pairs_global / (wsh if sharded else 1)
            work = kernel_work(dom, cc, pairs_per_launch=step_pairs_rank / (cnt / prof_div))
            # SURVEY 8(d) bytes of the pairs ONE launch of the dominant kernel covers (a macro-batched launch covers KG steps)
            bytes_8d = bpp * step_pairs_rank / (cnt / prof_div)
            t = avg_us * 1e-6
            if work:
                alg_tf = work["flops"] / t / 1e12
                exe_tf = alg_tf * work["terms"]
                gbs8 = bytes_8d / t / 1e9
                ridge = work["pipe"] * 1e12 / (PEAK_HBM_GBS * 1e9)
                # `frac` of an MFMA-bound kernel = EXECUTED matrix-pipe FLOP/s (algorithmic FLOPs x split terms) / the dense peak of the
                # executed MFMA type: what SQ_VALU_MFMA_BUSY_CYCLES measures; of an HBM-bound kernel = SURVEY 8(d) bytes/s / 8 TB/s
                if work["terms"] and work["flops"] * work["terms"] / bytes_8d > ridge:
                    roofline.update(bound="mfma", achieved=round(exe_tf, 3), peak=round(work["pipe"], 1), unit="TFLOP/s", frac=round(exe_tf / work["pipe"], 5))
                else:
                    roofline.update(bound="hbm", achieved=round(gbs8, 2), peak=PEAK_HBM_GBS, unit="GB/s", frac=round(gbs8 / PEAK_HBM_GBS, 5))
                roofline.update(alg_flops_per_launch=work["flops"], mfma_terms_per_product=work["terms"], alg_TFLOPs_fp32_equiv=round(alg_tf, 3),
                                executed_mfma_TFLOPs=round(exe_tf, 3), mfma_frac=round(exe_tf / work["pipe"], 5) if work["terms"] else 0.0,
                                bytes_8d_per_launch=round(bytes_8d), hbm_GBps_8d=round(gbs8, 2), hbm_frac_8d=round(gbs8 / PEAK_HBM_GBS, 5),
                                kernel_model_bytes_per_launch=work["bytes"])
            # HBM bytes per launch and matrix-pipe busy fraction from the committed PMC capture of this same workload
            roofline["traffic"] = roofline["traffic_ratio"] = roofline["mfma_busy_pmc"] = None
            ent = pmc_entry(name, dom)
            if ent and not sharded:
                roofline["traffic"] = ent["bytes_per_launch"]
                roofline["traffic_ratio"] = round(ent["bytes_per_launch"] / bytes_8d, 3)
                roofline["mfma_busy_pmc"] = ent.get("mfma_busy")
            roofline["step_hbm_GBps_8d"] = round(value * bpp / 1e9 / (1 if sharded or not env.multi else world), 2)
            roofline["step_hbm_frac_8d"] = round(roofline["step_hbm_GBps_8d"] / PEAK_HBM_GBS, 5)
            if roofline["step_hbm_GBps_8d"] > 6300.0:
                # above what MI355X_MICROARCH.md measures as achievable from HBM (6.3 TB/s): part of the 8(d) bytes is served by the 256 MB Infinity Cache
                # (uniform ids over a 1.2 GB table re-hit ~20 % of their rows there) -- the figure is algorithmic bytes per second, not HBM traffic
                roofline["step_hbm_source"] = "HBM + Infinity Cache (above the 6.3 TB/s achievable from HBM alone)"
            fpp = flops_per_pair(c["model"], c["qlen"], c["dlen"])
            if fpp:
                roofline["step_alg_TFLOPs_ref_ops"] = round(value * fpp / 1e12 / (world if env.multi and not sharded else 1), 2)

    # the wrapper's DEFAULT settings next to the tuned ones: Multitask.predict / Ranker.predict on one stream, resident
    # inputs, calls issued back to back (the per-batch-synchronised loop of the reference's drivers is the `dropin_loop_C3` sub-record):
    #   default          round 6: deferred id check (pinned error word, no read-back) + the shape-keyed hipGraph cache inside predict()
    #   deferred_eager   the deferred id check, eager launches
    #   blocking_eager   round 5's defaults: two blocking flag read-backs per call (the reference's IndexError at the offending call), eager
    eager_default = None
    if want_cpu and rank == 0 and not env.multi:
        eager_default = {}
        lib.set_batches_in_flight(1, lanes[:1])
        for mode in ("blocking_eager", "deferred_eager", "default"):
            model.id_check_interval = 1
            model.id_check = "blocking" if mode == "blocking_eager" else "deferred"
            model.args.predict_graphs = mode == "default"
            call = (lambda: model.predict(batches[0], suggest=False)) if is_sess else (lambda: model.predict(batches[0]))
            for _ in range(12):                         # (past predict_graph_min_calls = 8: the "default" mode is timed on its replays)
                call()
            torch.cuda.synchronize()
            te = time.perf_counter()
            for _ in range(40):
                call()
            torch.cuda.synchronize()
            eager_default["%s_ms_per_call" % mode] = round((time.perf_counter() - te) / 40 * 1e3, 4)
        model.check_ids()
        model.id_check_interval, model.id_check = 0, "deferred"
        model.args.predict_graphs = False
        model.clear_predict_graphs()
        lib.set_batches_in_flight(hint, lanes[:1])
        # what a caller who changes NOTHING gets from back-to-back predict() calls
        eager_default["default_settings_pairs_per_s"] = round(pairs_global / eager_default["default_ms_per_call"] * 1e3, 1)
        eager_default["deferred_eager_pairs_per_s"] = round(pairs_global / eager_default["deferred_eager_ms_per_call"] * 1e3, 1)
        eager_default["r5_defaults_pairs_per_s"] = round(pairs_global / eager_default["blocking_eager_ms_per_call"] * 1e3, 1)
    cpu = None
    if want_cpu and rank == 0 and not env.multi and not args.no_cpu_baseline:
        cpu = cpu_baseline(c, model, batches, lambda: finish(forward(0)), pairs_global, args)
    _phase(name, "checker legs")
    tier_err = None
    if (c.get("dtype") == "f32_split2" or c.get("oracle_slice")) and rank == 0 and not env.multi and not args.no_cpu_baseline and not lean:
        # the record's own error figure (checker leg, the oracle as the checker only): click probabilities of two resident batches against the oracle
        # (oracle_slice = n: the first n sessions of each -- the synthetic labels hold exactly one click per query, so the batch-wide click count
        # of cars.py:285-289 is 1 for the slice as for the batch)
        from oracle import neuroir_cpu as O
        sd_ = {k: v.detach().cpu().float() for k, v in model.network.state_dict().items()}
        tier_err = 0.0
        for bi in range(min(2, len(batches))):
            ex_ = {k: v.cpu() for k, v in batches[bi].items() if torch.is_tensor(v)}
            if c.get("oracle_slice"):
                ex_ = {k: v[:c["oracle_slice"]].contiguous() for k, v in ex_.items()}
                got_ = model.predict({k: v.to(dev) for k, v in ex_.items()}, suggest=False)["click_scores"].cpu()
                ref_ = O.predict_softmax(O.cars_scores(sd_, ex_["source_words"], ex_["source_lens"], ex_["document_words"], ex_["document_lens"], ex_["document_labels"]))
                tier_err = max(tier_err, float((got_ - ref_.view_as(got_)).abs().max()))
                continue
            ref_ = O.predict_softmax(O.cars_scores(sd_, ex_["source_words"], ex_["source_lens"], ex_["document_words"], ex_["document_lens"], ex_["document_labels"]))
            got_ = model.predict(batches[bi], suggest=False)["click_scores"].cpu()
            tier_err = max(tier_err, float((got_ - ref_.view_as(got_)).abs().max()))
    _phase(name, "end")
    lib.set_batches_in_flight(0, lanes)
    if rank != 0:
        return None
    tag = "%s, batch=%d%s x %d candidates, q_len=%d, doc_len=%d, emb_dim=300, vocab=%d, %s, full-length %s ids" % (
        c["model"], c["batch"], (" sessions x session_len %d" % c["session"]) if is_sess else " queries", c["cands"], c["qlen"], c["dlen"],
        c["vocab"], c.get("dtype", "f32"), "uniform" if c["uniform"] else "Zipf")
    par = "single GPU"
    if env.multi:
        if not sharded:
            par = "x%d independent per-rank batches, no collective (weak scaling)" % world
        elif plan is not None and plan.aligned:
            par = ("strong: (session, candidate) pair axis in %d contiguous chunks = %d whole sessions x all %d candidates per rank (candidate documents "
                   "sharded, no padding, no exchange of pooled vectors) -> session tail on the owning rank -> %s all-gather of probabilities; %s" % (
                       wsh, plan.bper, ncand, "RCCL" if env.backend == "nccl" else env.backend,
                       ("%d steps per hipGraph replay + one collective, %d lanes" % (stages["KG"], len(lanes))) if stages is not None else "eager"))
            if emu:
                par += " [EMULATED on one GPU: rank 0's 1/%d share of the work, loop-back collectives, no xGMI latency]" % wsh
        elif plan is not None:
            par = "strong: candidate-sharded encode x%d -> %s %s (%d B out per rank and step) -> session-sharded tail -> all-gather of probabilities; %s" % (
                wsh, "RCCL" if env.backend == "nccl" else env.backend, "all-gather exchange" if fused is not None else "all-to-all",
                plan.world * plan.bper * plan.S * plan.per * 256 * 4 if fused is not None else plan.exchange_bytes(256),
                ("%d steps + collectives per hipGraph" % KSTEP) if fused is not None else
                ("software-pipelined: one hipGraph replay + ONE collective per step (probabilities of step k-1 ride with the slices of step k), %d lanes" % len(lanes)
                 if stages is not None else "eager"))
            if emu:
                par += " [EMULATED on one GPU: rank 0's 1/%d share of the work, loop-back collectives, no xGMI latency]" % wsh
        elif is_sess:
            par = "strong: candidate-sharded document encoding x%d (Multitask.parallelize) + %s all-gather of pooled documents, session part replicated" % (
                world, "RCCL" if env.backend == "nccl" else env.backend)
        else:
            par = "strong: candidate-sharded x%d (%d per rank) + %s all-gather of scores" % (
                world, batches[0]["doc_rep"].shape[1], "RCCL" if env.backend == "nccl" else env.backend)
    shard_axis = None if not sharded else ("pair" if plan is not None and plan.aligned else "candidate")
    return {"name": name, "baseline_config": c.get("baseline"), "workload": tag, "shard_axis": shard_axis,
            # machine-readable marker of the lane-count tuning aid (BENCH_EMULATE_WORLD): `pairs_per_s` is then rank 0's 1/W share x W on ONE GPU
            "emulated": bool(emu), "emulated_world": wsh if emu else None,
            "kg": (stages["KG"] if (stages is not None and "aligned" in stages) else 1), "pairs_per_s": round(value, 1), "ms_per_step": round(ms_per_step, 5),
            "ms_per_step_one_batch_in_flight": None if single_ms is None else round(single_ms, 5), "global_batch_pairs": per_step_pairs, "parallelism": par, "world_size": world,
            "steps": steps, "reps": reps, "ms_per_step_min_max": spread, "hipgraph": (graphs is not None) or (stages is not None and stages.get("graphed", True)) or (fused is not None),
            "batches_in_flight": len(lanes) * (stages["KG"] if (stages is not None and "aligned" in stages) else 1),
            "macro_batch": (stages["KG"] if (stages is not None and "aligned" in stages) else 1), "lanes": len(lanes), "host_enqueue_ms_per_step": round(host_ms, 5),
            "overlapped_vs_serial_max_abs_diff": overlap_diff, "pairs_per_s_with_host_ids_h2d": None if h2d_value is None else round(h2d_value, 1),
            "resident_sustained_pairs_per_s": None if sustained is None else round(sustained, 1),
            "h2d_inclusive_over_resident": None if (h2d_value is None or not sustained) else round(h2d_value / sustained, 4), "h2d_stream": h2d_info,
            "dtype": c.get("dtype", "f32") if c.get("dtype") != "f32_split2" else "f32 table, fp16x2 W_hh x fp16 h recurrence and attention rows (opt-in tier)",
            "max_abs_diff_vs_oracle_softmax": tier_err, "precompute": pre, "wrapper_predict_eager_one_stream": eager_default, "roofline": roofline, "cpu_baseline": cpu, "power": power}


def cpu_baseline(c, model, batches, gpu_step, pairs, args):
    from oracle import neuroir_cpu as O
    sd = {k: v.detach().cpu().float() for k, v in model.network.state_dict().items()}
    ex = {k: v.cpu() for k, v in batches[0].items()}
    ncores = torch.get_num_threads()
    m = c["model"]
    if m == "mnsrf":
        fn = lambda: torch.softmax(O.mnsrf_scores(sd, ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"]), -1)  # noqa: E731
    elif m == "m_match_tensor":
        fn = lambda: torch.softmax(O.m_match_tensor_scores(sd, ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"]), -1)  # noqa: E731
    elif m == "cars":
        fn = lambda: O.predict_softmax(O.cars_scores(sd, ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"], ex["document_labels"]))  # noqa: E731
    else:
        f = O.MODEL_FNS[m.upper()]
        fn = lambda: O.predict_softmax(f(sd, ex["que_rep"], ex["que_len"], ex["doc_rep"], ex["doc_len"]))  # noqa: E731
    ref = fn()
    gpu = gpu_step().cpu()
    maxdiff = float((gpu - ref.view_as(gpu)).abs().max())
    avail = os.cpu_count() or ncores
    try:
        import psutil
        phys = psutil.cpu_count(logical=False) or avail
    except Exception:
        phys = avail
    best_t, best_rate, by_threads = ncores, 0.0, {}
    # k = 8 AND all physical cores, stated; the counts between are probed because tiny per-op tensors oversubscribe a big host
    for t in sorted({min(avail, k) for k in (8, 16, 32, 64, phys)}):
        torch.set_num_threads(t)
        fn()
        n0, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < 0.75:
            fn(); n0 += 1
        rate = n0 / (time.perf_counter() - t0)
        by_threads[str(t)] = round(rate * pairs, 1)               # (SURVEY 8d asks for k = 8 next to the best count: kept in the detail record)
        if rate > best_rate:
            best_t, best_rate = t, rate
    torch.set_num_threads(best_t)
    n, t1 = 0, time.perf_counter()
    while True:
        fn()
        n += 1
        dt = time.perf_counter() - t1
        if dt > args.cpu_seconds or n >= 5000:
            break
    cpu_model = "unknown"
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                cpu_model = ln.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    return {"value": round(n * pairs / dt, 1), "unit": "pairs/s", "cores": best_t, "kind": "port", "cpu_model": cpu_model,
            "host_logical_cores": avail, "host_physical_cores": phys, "value_8_threads": by_threads.get(str(min(avail, 8))),
            "value_all_physical_cores": by_threads.get(str(min(avail, phys))), "threads_pinned": "torch.set_num_threads(%d)" % best_t, "probe_pairs_per_s_by_threads": by_threads,
            "sample": "%d batches of the same %s workload in %.1f s (oracle/neuroir_cpu.py = pinned port of the reference, torch %s CPU, "
                      "best of {8,16,32,64} threads = %d; host has %d logical cores)" % (n, m, dt, torch.__version__, best_t, avail),
            "max_abs_diff_vs_gpu_softmax": maxdiff}


class QuietStderr(object):
    """The driver reads the record from the tail of stdout FOLLOWED by stderr, so whatever a successful run writes to stderr lands behind the
    JSON line (round 3: a torch warning did, and the record could not be parsed).  File descriptor 2 is pointed at a log file for the length
    of the run -- C-level writers (RCCL, the HIP runtime) included -- and is replayed to the real stderr only when the run fails."""

    def __init__(self, path):
        self.path, self.saved = path, None

    def __enter__(self):
        if os.environ.get("BENCH_KEEP_STDERR"):
            return self
        sys.stderr.flush()
        self.saved = os.dup(2)
        fd = os.open(self.path, os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
        os.dup2(fd, 2)
        os.close(fd)
        return self

    def __exit__(self, et, ev, tb):
        if self.saved is None:
            return False
        sys.stderr.flush()
        ctypes.CDLL(None).fflush(None)
        os.dup2(self.saved, 2)
        os.close(self.saved)
        if et is not None and not (et is SystemExit and not ev.code):
            try:
                sys.stderr.write(open(self.path, errors="replace").read()[-6000:])
            except OSError:
                pass
        return False


def self_launch(args):
    """`python bench.py --gpus N` with N > 1 and no launcher around it: start the N ranks here (torch.distributed.run, one process per GPU,
    rendezvous on 127.0.0.1) and hand their stdout through.  The launcher's own chatter goes to the log unless the run fails."""
    import socket
    import subprocess
    ndev = torch.cuda.device_count()
    if ndev < args.gpus and os.environ.get("BENCH_BACKEND", "nccl") == "nccl":
        raise SystemExit("bench.py: --gpus %d asked for, %d visible -- RCCL needs one device per rank (BENCH_BACKEND=gloo runs the flow on fewer)" % (args.gpus, ndev))
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    env.setdefault("OMP_NUM_THREADS", "8")
    p = subprocess.run(cmd, env=env, stderr=subprocess.PIPE)
    if p.returncode != 0:
        sys.stderr.write(p.stderr.decode(errors="replace")[-6000:])
    else:
        try:
            open(log_path("bench_launcher.log"), "wb").write(p.stderr)
        except OSError:
            pass
    raise SystemExit(p.returncode)


LOG_DIR = os.environ.get("BENCH_LOG_DIR", ROOT)


def log_path(name):
    """<LOG_DIR>/<name> when the running user may write it there, else <name> in a per-user directory under the system temporary directory
    (the same path for the launcher and every rank): a checkout that is read-only for the user, or holds another user's file of an earlier
    run, is still benchmarked."""
    path = os.path.join(LOG_DIR, name)
    if os.access(path, os.W_OK) if os.path.exists(path) else os.access(LOG_DIR, os.W_OK):
        return path
    import tempfile
    d = os.path.join(tempfile.gettempdir(), "context_attentive_ir_bench.%d" % os.getuid())
    os.makedirs(d, exist_ok=True)
    return os.path.join(d, name)


OVERLAP_TOL = 1e-5      # max |concurrent - serial| of one captured graph's output above which a record FAILS
ROOF_KEYS = ("kernel", "avg_us", "launches_per_step", "bound", "achieved", "peak", "unit", "frac", "hbm_frac_8d", "traffic", "traffic_ratio",
             "mfma_busy_pmc", "step_hbm_GBps_8d")


def short_sub(n, r):
    rf = r.get("roofline") or {}
    e = {"name": n, "pairs_per_s": r.get("pairs_per_s"), "frac": rf.get("frac"), "bound": rf.get("bound")}
    if r.get("world_size", 1) > 1 or r.get("shard_axis"):
        e["axis"] = r.get("shard_axis")
    if r.get("error"):
        e["error"] = str(r["error"])[:80]
    if r.get("emulated"):                     # BENCH_EMULATE_WORLD: one GPU's 1/W share extrapolated x W -- never a measured multi-GPU figure
        e["emulated_world"] = r.get("emulated_world")
    if r.get("overlapped_vs_serial_max_abs_diff") is not None:       # lanes in flight vs the same graphs alone (a record above OVERLAP_TOL fails)
        e["ovl"] = float("%.2g" % r["overlapped_vs_serial_max_abs_diff"])
    for k in ("hist_rows_differ", "pairs_differ", "map_delta_vs_oracle", "max_abs_diff_vs_oracle", "prob_max_abs_diff", "map10_equal", "max_abs_diff_vs_oracle_softmax", "kg"):
        if k in r and r[k] is not None:
            e[k] = r[k]
    if r.get("power"):
        e["w"] = r["power"].get("package_w")
    if n.startswith("train_") or r.get("pairs_per_s") is None:
        e["ms_per_step"] = r.get("ms_per_step")
    # the line stays under 4 KB: no null entries, error figures to three significant digits
    if e.get("kg") == 1:
        del e["kg"]
    if isinstance(e.get("pairs_per_s"), float):
        e["pairs_per_s"] = int(round(e["pairs_per_s"]))
    if isinstance(e.get("frac"), float):
        e["frac"] = round(e["frac"], 4)
    return {k: (float("%.3g" % v) if isinstance(v, float) and k not in ("pairs_per_s", "ms_per_step", "frac") else v) for k, v in e.items() if v is not None}


def main():
    args = parse()
    if args.sub not in (None, "none") and not args.full:
        raise SystemExit("bench.py: --sub %s names sub-records: they run with --full only" % args.sub)
    launcher = args.gpus > 1 and "WORLD_SIZE" not in os.environ
    # (the redirect starts BEFORE the HIP runtime initialises: libdrm's "amdgpu.ids: No such file" line is stderr noise of every run on this image)
    with QuietStderr(log_path("bench_stderr.%s.log" % ("launcher" if launcher else "rank%d" % int(os.environ.get("RANK", "0"))))):
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a ROCm GPU (the HIP path has no CPU fallback)")
        if launcher:
            self_launch(args)
        result_line = run_all(args)
    if result_line is not None:
        sys.stderr.flush()
        print(result_line, flush=True)


def run_all(args):
    env = Env(args.gpus)
    try:
        return run_records(args, env)
    finally:
        if env.dist:
            try:
                env.dist.destroy_process_group()
            except Exception:
                pass
        # RCCL writes its version banner through C stdio (buffered when stdout is a pipe): flush it out first so that the
        # JSON line is the LAST line of rank 0's stdout
        ctypes.CDLL(None).fflush(None)


def run_records(args, env):
    for kv in filter(None, os.environ.get("NIR_TUNE", "").split(",")):     # kernel-variant A/B runs: NIR_TUNE=name=value,...
        k, v = kv.split("=")
        lib.check(lib.load().nir_debug_set_tunable(k.encode(), int(v)), "nir_debug_set_tunable")
    if args.config == "C5_stream":
        if args.dump_outputs:
            raise SystemExit("bench.py: --dump-outputs is not available for --config C5_stream")
        r = stream_record(args, env, seconds=None)
        if env.rank != 0:
            return None
        write_detail({"C5_stream": r})
        keep = ("name", "pairs_per_s", "sessions_per_s", "batches", "seconds", "h2d_GBps", "lanes", "macro_batch", "parallelism", "world_size", "whole_stream", "error")
        line = {"metric": "ranked (query,doc) pairs/sec", "value": r.get("pairs_per_s"), "unit": "pairs/s", "n_gpus": env.seen, "steps": r.get("batches"), "warmup": 0,
                "ms_per_step": r.get("ms_per_step"), "higher_is_better": True, "scaling": "strong", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
                "config": {k: r.get(k) for k in keep if k in r}}
        return json.dumps(line)
    head = dict(CONFIGS[args.config])
    adhoc = False
    for k in ("model", "batch", "cands", "qlen", "dlen", "session", "vocab", "uniform", "dtype"):
        v = getattr(args, k)
        if v is not None:
            head[k] = v
            adhoc = True
    if head["model"] in SESSION_MODELS:
        head.setdefault("session", 7)
    hname = args.config if not adhoc else "adhoc_" + head["model"]
    rec = run_config(hname, head, args, env, args.steps, args.warmup, shard=True, want_cpu=args.full, with_h2d=args.full, dump=args.dump_outputs,
                     lean=not args.full)
    if not args.full:                   # a plain run: the headline's timed steps and nothing else
        return compose_line(args, env, rec, {}, None) if env.rank == 0 else None
    if env.multi and env.world > 1 and env.rank == 0:
        # N > 1: a rank that fails inside a sub-record must take the job down (the others would hang in its collectives) -- so the headline is
        # printed NOW as a complete record of its own; the final line (with the sub-records) supersedes it as the last line of stdout
        print(compose_line(args, env, rec, {}, None), flush=True)

    sub = {}

    def attempt(n, fn):
        try:
            r = fn()
        except Exception as e:  # a sub-record must never take the headline down
            if env.multi and env.world > 1:
                raise      # (but a rank that leaves a collective sequence must take the JOB down, not hang the other ranks)
            r = {"name": n, "error": "%s: %s" % (type(e).__name__, e)} if env.rank == 0 else None
            torch.cuda.synchronize()
        if r is not None:
            sub[n] = r
        torch.cuda.empty_cache()

    # N = 1: every single-GPU BASELINE configuration.  N > 1: the configurations BASELINE shards (configs[3] DUET / DRMM candidate-sharded,
    # configs[4] shape) next to the headline, the headline on the OTHER CARS shard axis and with the N = 1 macro-batch (KG-matched)
    names = [] if adhoc else ([n for n in CONFIGS if n != args.config] if not env.multi else
                              [n for n in ("C4_duet", "C4_drmm", "C5_cars_bf16") if n != args.config])
    if args.sub is not None:
        names = [] if args.sub == "none" else [n for n in args.sub.split(",") if n in CONFIGS]
    for n in names:
        attempt(n, lambda n=n: run_config(n, dict(CONFIGS[n]), args, env, SUB_STEPS.get(n, 100), min(args.warmup, 8), shard=True))
        if n == "C4_drmm" and not env.multi and env.rank == 0 and "error" not in sub.get(n, {"error": 1}) and not args.no_cpu_baseline:
            try:
                gap = drmm_parity_gap(args)
                sub[n]["parity_gap_on_overlapping_ids"] = gap
                sub[n].update({k: gap["reference"][k] for k in ("hist_rows_differ", "pairs_differ", "map_delta_vs_oracle")})       # the default policy
            except Exception as e:
                sub[n]["parity_gap_on_overlapping_ids"] = {"error": "%s: %s" % (type(e).__name__, e)}
        if n == "C5_cars_bf16" and not env.multi and env.rank == 0 and "error" not in sub.get(n, {"error": 1}) and not args.no_cpu_baseline:
            try:
                gap = bf16_parity_gap(args)
                sub[n]["bf16_error_vs_oracle"] = gap
                sub[n].update({k: gap[k] for k in ("max_abs_diff_vs_oracle", "prob_max_abs_diff", "map_delta_vs_oracle", "map10_equal")})
            except Exception as e:
                sub[n]["bf16_error_vs_oracle"] = {"error": "%s: %s" % (type(e).__name__, e)}
            torch.cuda.empty_cache()
    full = not adhoc and args.sub is None
    if head["model"] == "cars" and full and not env.multi:
        # the same workload WITHOUT the folded gate tables: per-batch gather-GEMM for the LSTM input projection
        attempt(hname + "_nofold", lambda: run_config(hname + "_nofold", dict(head, nofold=True), args, env, max(40, args.steps // 4), min(args.warmup, 8), shard=True))
        sub["C3_cars_with_decode"] = decode_record(head, args, env)
        torch.cuda.empty_cache()
        sub["dropin_loop_C3"] = dropin_record(head, args, env)
        torch.cuda.empty_cache()
        sub["train_C3_cars_update"] = train_record("CARS", dict(head), args, env)
        sub["train_C2_match_tensor_update"] = train_record("MATCH_TENSOR", dict(CONFIGS["C2_match_tensor"]), args, env)
        # the other two session models on the same session shape (Multitask.update of M_MATCH_TENSOR / MNSRF: models/multitask.py:161-223)
        sub["train_X3_m_match_tensor_update"] = train_record("M_MATCH_TENSOR", dict(CONFIGS["X3_m_match_tensor"]), args, env, steps=8)
        sub["train_X3_mnsrf_update"] = train_record("MNSRF", dict(CONFIGS["X3_mnsrf"]), args, env, steps=8)
    elif args.sub is not None and not env.multi:
        # --sub train_<...>_update[,..]: the named training records alone (iteration on one training step without the whole line)
        trains = {"train_C3_cars_update": ("CARS", HEADLINE, 12), "train_C2_match_tensor_update": ("MATCH_TENSOR", "C2_match_tensor", 12),
                  "train_X3_m_match_tensor_update": ("M_MATCH_TENSOR", "X3_m_match_tensor", 8), "train_X3_mnsrf_update": ("MNSRF", "X3_mnsrf", 8)}
        for n in args.sub.split(","):
            if n in trains:
                sub[n] = train_record(trains[n][0], dict(CONFIGS[trains[n][1]]), args, env, steps=trains[n][2])
    eff_world = int(os.environ.get("BENCH_EMULATE_WORLD", env.world)) if env.multi else 1      # (emulation: one process times rank 0's share of W)
    if head["model"] == "cars" and full and env.multi and eff_world > 1:
        # the SAME record on the other CARS shard axis (rank 0 holds its own axis name, every rank takes part) and -- when the per-rank macro-batch policy
        # gives another count than N = 1 gets -- with the N = 1 count (KG-matched)
        ax = "pair" if (os.environ.get("BENCH_SHARD_AXIS", "auto") in ("auto", "pair") and head["batch"] % eff_world == 0) else "candidate"
        other = "candidate" if ax == "pair" else "pair"
        if other == "candidate" or head["batch"] % eff_world == 0:
            attempt(hname + "_axis_" + other, lambda: run_config(hname + "_axis_" + other, head, args, env, args.steps, min(args.warmup, 8), shard=True, axis=other))
        if macro_batch(head) != macro_batch(head, "BENCH_GATHER_EVERY", eff_world):
            attempt(hname + "_kg_matched", lambda: run_config(hname + "_kg_matched", head, args, env, args.steps, min(args.warmup, 8), shard=True, kg=macro_batch(head)))
    if head["model"] == "cars" and full and not os.environ.get("BENCH_NO_STREAM"):
        secs = float(os.environ.get("BENCH_H2D_SECONDS", "5"))
        attempt("C5_stream", lambda: stream_record(args, env, seconds=secs, mode="batch" if env.multi else None))
        if not env.multi and env.rank == 0 and "error" not in sub.get("C5_stream", {"error": 1}) and not args.no_cpu_baseline:
            try:
                gap = bf16_parity_gap(args, stream=True)
                sub["C5_stream"]["bf16_error_vs_oracle"] = gap
                sub["C5_stream"].update({k: gap[k] for k in ("prob_max_abs_diff", "map_delta_vs_oracle")})
            except Exception as e:
                sub["C5_stream"]["bf16_error_vs_oracle"] = {"error": "%s: %s" % (type(e).__name__, e)}
            torch.cuda.empty_cache()
        if env.multi and CONFIGS["C5_cars_bf16"]["batch"] % int(os.environ.get("BENCH_EMULATE_WORLD", env.world)) == 0:
            attempt("C5_stream_pair", lambda: stream_record(args, env, seconds=secs, mode="pair"))
    weak = None
    if env.multi and not os.environ.get("BENCH_NO_WEAK"):           # labelled secondary number: every rank scores its own full batch, no collective
        r = run_config(hname + "_weak", head, args, env, max(20, args.steps // 4), min(args.warmup, 8), shard=False)
        weak = r["pairs_per_s"] if r else None

    return compose_line(args, env, rec, sub, weak) if env.rank == 0 else None


def compose_line(args, env, rec, sub, weak):
    """detail file + the ONE compact line the driver parses (every sub-record once, four scalars each; the full records are in `detail`)"""
    rec = dict(rec)
    roof = rec.pop("roofline") or {}
    cpu = rec.pop("cpu_baseline")
    pre = rec.get("precompute") or {}
    detail = {"headline": dict(rec, roofline=roof, cpu_baseline=cpu), "sub": sub, "weak_scaling_pairs_per_s": weak,
              "hw_queues": int(os.environ.get("GPU_MAX_HW_QUEUES", "4")), "argv": sys.argv[1:]}
    where = write_detail(detail)
    cfg = {"name": rec["name"], "workload": rec["workload"], "macro_batch": rec["macro_batch"], "lanes": rec["lanes"],
           "batches_in_flight": rec["batches_in_flight"], "ms_per_step_one_batch_in_flight": rec["ms_per_step_one_batch_in_flight"],
           "hipgraph": rec["hipgraph"], "parallelism": rec["parallelism"][:400], "shard_axis": rec.get("shard_axis"), "world_size": rec["world_size"],
           "pairs_per_s_with_host_ids_h2d": rec["pairs_per_s_with_host_ids_h2d"], "weak_scaling_pairs_per_s": weak, "detail": where,
           # `value` runs hipGraph replays, several lanes, macro-batches and no per-call id check (id_check_interval = 0); next to it what the wrapper's
           # defaults give for back-to-back predict() calls on one stream (round 6: deferred id check + the hipGraph cache inside predict())
           "default_settings_pairs_per_s": (rec.get("wrapper_predict_eager_one_stream") or {}).get("default_settings_pairs_per_s"),
           # the reference's own per-batch loop (predict -> .cpu() -> metrics, one batch in flight) on the wrapper's defaults, at the headline batch
           # size and at --test_batch_size 128, ranking only and with the decode the reference's predict always runs (sub-record dropin_loop_C3)
           "dropin_loop_pairs_per_s": {k: v.get("pairs_per_s") for k, v in (sub.get("dropin_loop_C3") or {}).items() if isinstance(v, dict)} or None,
           "resident_sustained_pairs_per_s": rec.get("resident_sustained_pairs_per_s"),
           "h2d_inclusive_over_resident_sustained": rec.get("h2d_inclusive_over_resident")}
    pw = rec.get("power")
    pw = {k: pw.get(k) for k in ("package_w", "cap_w", "sclk_mhz")} if pw else None
    small = {k: roof.get(k) for k in ROOF_KEYS}
    small["precompute_fold_ms"], small["precompute_fold_bytes"] = pre.get("fold_ms"), pre.get("fold_bytes")
    if cpu:
        cpu = {k: cpu.get(k) for k in ("value", "unit", "cores", "kind", "cpu_model", "host_logical_cores", "host_physical_cores", "value_8_threads",
                                       "value_all_physical_cores", "max_abs_diff_vs_gpu_softmax")}
        cpu["sample"] = "%.0f s of the same workload through oracle/neuroir_cpu.py (torch CPU) at the best thread count (cores); k = 8 / all physical cores beside it" % args.cpu_seconds
    line = {"metric": "ranked (query,doc) pairs/sec", "value": rec["pairs_per_s"], "unit": "pairs/s", "n_gpus": env.seen,
            "steps": args.steps, "warmup": args.warmup, "reps": rec["reps"], "ms_per_step": rec["ms_per_step"], "higher_is_better": True,
            # the global batch is FIXED as N grows (every rank scores its share of the same batch): strong scaling at every N
            "scaling": "strong", "vs_baseline": None, "dtype": rec["dtype"], "data": "synthetic", "full": args.full,
            "config": cfg, "roofline": small if args.full else None, "power": pw, "cpu_baseline": cpu, "sub": [short_sub(n, r) for n, r in sub.items()]}
    if rec.get("emulated"):
        # BENCH_EMULATE_WORLD (tuning aid, never set by the driver): `value` is ONE GPU's 1/W share of the work extrapolated x W, not a measured
        # multi-GPU figure -- flagged at the top level so that a tool reading value / n_gpus cannot take it for one
        line["emulated"], line["emulated_world"] = True, rec.get("emulated_world")
        line["value_measured_one_gpu_share"] = round(rec["pairs_per_s"] / max(1, rec.get("emulated_world") or 1), 1)
    return json.dumps(line, separators=(",", ":"))


DUMP_MAX_BYTES = 64 << 20


def write_outputs(path, arrays):
    """--dump-outputs: every tensor as <path>/<name>.npy, float32 (float64 stays float64), at most DUMP_MAX_BYTES in all.  An array larger
    than its share of that is written as a fixed sample: the elements at the first n positions of a seed-0 permutation of its flattened
    index, in that order (the same positions for every build of the same shape)."""
    os.makedirs(path, exist_ok=True)
    share = DUMP_MAX_BYTES // max(1, len(arrays))
    for name, t in arrays.items():
        t = t.detach()
        a = (t.double() if t.dtype == torch.float64 else t.float()).cpu().numpy()
        if a.nbytes > share:
            a = a.reshape(-1)[np.random.default_rng(0).permutation(a.size)[:share // a.itemsize]]
        np.save(os.path.join(path, name + ".npy"), np.ascontiguousarray(a))


def write_detail(obj):
    """the full records (every sub-record with its roofline block, per-kernel microseconds, precompute, H2D stream) -> bench_detail.json"""
    path = os.environ.get("BENCH_DETAIL") or log_path("bench_detail.json")
    try:
        with open(path, "w") as f:
            json.dump(obj, f, indent=1, default=str)
        rel = os.path.relpath(path, ROOT)
        return path if rel.startswith("..") else rel          # (outside the checkout: the absolute path)
    except OSError:
        return None


def drmm_parity_gap(args):
    """Checker leg (rank 0, N = 1; the oracle is used as the checker only): DRMM on Zipf ids, where queries and documents SHARE tokens and the
    exact-match bins carry signal.  At an exact overlap the cosine is 1 +- 1 ulp by reduction order (reference
    rankers/drmm.py:66-78).  Policy "reference" (the default since round 5): the bin the reference's host path gives cos(row, row) is looked up
    per embedding row -> the integer histograms are the reference's; "numpy" (rounds 1-4: the kernel's own cosine) and the opt-in "snap" rule
    ride along.  Per policy: (pair, query term) rows and pairs whose histogram differs from the oracle's, and the MAP delta on this slice."""
    from oracle import neuroir_cpu as O
    from context_attentive_ir_amd.eval import ltorank
    V, B, N, QL, DL = 100000, 16, 50, 4, 290
    ex = synth.ranker_batch(B, N, QL, DL, V, seed=1013, full_length=False)
    m = build_model(dict(CONFIGS["C4_drmm"], vocab=V), args).network
    sd = {k: v.detach().cpu().float() for k, v in m.state_dict().items()}
    q, ql, d, dl, lab = (ex[k] for k in ("que_rep", "que_len", "doc_rep", "doc_len", "label"))
    gate, _, hist_ref = O.drmm_parts(sd, q, d)
    s_ref = O.drmm_scores_from_hist(sd, gate, hist_ref, B, N)
    overlaps = int(((q[:, None, :, None] == d[:, :, None, :]) & (q[:, None, :, None] != 0)).sum())
    a_ref = np.argsort(-s_ref.numpy(), 1, kind="stable")
    out = {"slice": "%dx%dx%dx%d Zipf ids, V=%d" % (B, N, QL, DL, V), "exact_overlaps": overlaps, "hist_rows": B * N * QL}
    for policy in ("reference", "numpy", "snap"):
        m.exact_match_policy = policy
        s, h = m(q.cuda(), ql.cuda(), d.cuda(), dl.cuda(), return_hist=True)
        h, hr = h.cpu().numpy(), hist_ref.numpy()
        rows = (h != hr).any(-1)
        a_got = np.argsort(-s.cpu().numpy(), 1, kind="stable")
        out[policy] = {"hist_rows_differ": int(rows.sum()), "pairs_differ": int(rows.any(-1).sum()), "lower_bins_differ": int((h[..., :3] != hr[..., :3]).sum()),
                       "map_delta_vs_oracle": round(ltorank.MAP(a_got, lab.numpy()) - ltorank.MAP(a_ref, lab.numpy()), 5)}
    m.exact_match_policy = "reference"
    return out


def bf16_parity_gap(args, stream=False):
    """Checker leg (rank 0, N = 1; the oracle is used as the checker only): the ACHIEVED error of the bf16 path (BASELINE configs[4]) against the
    fp32 oracle on slices the oracle finishes in seconds -- (a) a configs[4]-shaped slice (4 sessions x 7 queries x 50 candidates, q_len 4,
    doc_len 64, V = 100 000), (b) a 10-candidate slice for MAP@10 (BASELINE's "MAP@10 parity" = equality here); stream=True: the same model
    through graph_runner.StreamingSessionPredictor on a 24-session stream.  Rides in the C5_cars_bf16 / C5_stream records."""
    from oracle import neuroir_cpu as O
    from context_attentive_ir_amd.eval import ltorank
    c = dict(CONFIGS["C5_cars_bf16"])
    model = build_model(c, args)
    sd = {k: v.detach().cpu().float() for k, v in model.network.state_dict().items()}

    def oracle(ex):
        return O.cars_scores(sd, ex["source_words"], ex["source_lens"], ex["document_words"], ex["document_lens"], ex["document_labels"])
    out = {}
    if not stream:
        worst_s, worst_p = 0.0, 0.0
        for tag, (B, S, N) in (("c5_slice", (4, 7, 50)), ("map10_slice", (8, 7, 10))):
            ex = synth.session_batch(B, S, N, c["qlen"], c["dlen"], c["vocab"], seed=17 + N, full_length=False)
            ref = oracle(ex)
            got = model.scores(ex).cpu()
            lab = ex["document_labels"].reshape(-1, N).numpy().astype(int)
            a_ref, a_got = (np.argsort(-t.reshape(-1, N).numpy(), 1, kind="stable") for t in (ref, got))
            ds, dp = float((got - ref).abs().max()), float((torch.softmax(got, -1) - torch.softmax(ref, -1)).abs().max())
            worst_s, worst_p = max(worst_s, ds), max(worst_p, dp)
            out[tag] = {"shape": [B, S, N, c["qlen"], c["dlen"]], "max_abs_diff_vs_oracle": ds, "prob_max_abs_diff": dp,
                        "map_delta_vs_oracle": ltorank.MAP(a_got, lab) - ltorank.MAP(a_ref, lab), "rows_reordered": int((a_ref != a_got).any(1).sum())}
        out.update({"max_abs_diff_vs_oracle": float("%.3g" % worst_s), "prob_max_abs_diff": float("%.3g" % worst_p),
                    "map_delta_vs_oracle": out["c5_slice"]["map_delta_vs_oracle"], "map10_equal": out["map10_slice"]["map_delta_vs_oracle"] == 0.0})
        return out
    from context_attentive_ir_amd.graph_runner import StreamingSessionPredictor
    from context_attentive_ir_amd.inputters import SyntheticSessionCorpus
    B, N = 4, c["cands"]
    corpus = SyntheticSessionCorpus(n_sessions=24, n_cands=N, qlen=c["qlen"], dlen=c["dlen"], vocab=c["vocab"], seed=9, pool=4, full_length=False, s_max=7)
    batches = corpus.batches(B, seed=1)
    sp = StreamingSessionPredictor(model, N, c["qlen"], c["dlen"], B, max_session_len=7, lanes=2, slots=2)
    got = {}
    sp.run(corpus, batches, on_result=lambda k, idx, probs: got.__setitem__(k, probs.clone()))
    worst_p, maps = 0.0, [[], []]
    for k, idx in enumerate(batches):
        ex = corpus.batch_tensors(idx)
        ref = torch.softmax(oracle(ex), -1)
        worst_p = max(worst_p, float((got[k] - ref).abs().max()))
        lab = ex["document_labels"].reshape(-1, N).numpy().astype(int)
        maps[0].append(ltorank.MAP(np.argsort(-got[k].reshape(-1, N).numpy(), 1, kind="stable"), lab))
        maps[1].append(ltorank.MAP(np.argsort(-ref.reshape(-1, N).numpy(), 1, kind="stable"), lab))
    del sp
    return {"stream_slice": "%d sessions in %d batches of %d, %d candidates" % (len(corpus), len(batches), B, N), "prob_max_abs_diff": float("%.3g" % worst_p),
            "map_delta_vs_oracle": float(np.mean(maps[0]) - np.mean(maps[1]))}


def stream_record(args, env, seconds=None, n_sessions=None, mode=None):
    """BASELINE.json configs[4]: CARS at MSMARCO scale as a STREAM -- 223 876 synthetic sessions with
    S ~ clip(Poisson(4.84) + 2, 2, 16) queries, batched exactly as the reference sampler does (equal-length sessions per
    batch, full batches, shuffled; neuroir/inputters/multitask/data.py:42-72), 64 sessions x 50 candidates per batch, bf16 folded tables.
    Ids arrive from the host for every batch (int32 wire block collated into pinned staging by a producer thread), one captured hipGraph
    per session length and lane; value = pairs of the batches submitted / wall seconds, H2D and D2H of the probabilities included.
    N > 1 (sharding.StreamShardPlan): mode "batch" = rank r scores batches r, r+N, .. whole; "pair" = every batch cut into N blocks of whole
    sessions; either way the probabilities of every batch are all-gathered to every rank on the lanes' communication streams while the
    next batch is encoded.  Every rank runs the same number of rounds; value = pairs scored by all ranks / max-over-ranks seconds.
    seconds=None: the WHOLE stream once; else sustained for about that long (batches cycled)."""
    try:
        from context_attentive_ir_amd.graph_runner import StreamingSessionPredictor
        from context_attentive_ir_amd.inputters import SyntheticSessionCorpus
        c = dict(CONFIGS["C5_cars_bf16"])
        model = build_model(c, args)
        n_sessions = n_sessions or int(os.environ.get("BENCH_STREAM_SESSIONS", "223876"))
        t0 = time.perf_counter()
        corpus = SyntheticSessionCorpus(n_sessions=n_sessions, n_cands=c["cands"], qlen=c["qlen"], dlen=c["dlen"], vocab=c["vocab"], pool=96)
        bl = corpus.batches(c["batch"])
        t_corpus = time.perf_counter() - t0
        lengths = sorted({int(corpus.lengths[b[0]]) for b in bl})
        nl = max(2, min(args.streams, 4))
        mk = max(1, int(os.environ.get("BENCH_STREAM_MACRO", "1")))       # (64 x S x 50 per batch: macro 2 measured +1 %, macro 4 runs out of HBM)
        plan, W = None, env.world
        if env.multi:
            mode = mode or os.environ.get("BENCH_STREAM_MODE", "batch")
            if env.world == 1 and os.environ.get("BENCH_EMULATE_WORLD"):
                W = int(os.environ["BENCH_EMULATE_WORLD"])
            plan = sharding.StreamShardPlan(W, env.rank, mode, batch_size=c["batch"])
        sp = StreamingSessionPredictor(model, c["cands"], c["qlen"], c["dlen"], mk * c["batch"], max_session_len=max(lengths), lanes=nl, slots=2, macro=mk,
                                       plan=plan)
        n_sampler_batches = len(bl)
        # mk sampler batches of one session length per wire block / graph replay; the < mk left-over batches per length are not part of this
        # measurement (`left_over_batches_not_timed`; a full run scores them through a macro = 1 predictor)
        bl, rest = sp.merge_batches(corpus, bl, mk)
        lengths = sorted({int(corpus.lengths[b[0]]) for b in bl})
        t0 = time.perf_counter()
        sp.prepare(lengths, example=(corpus, bl[0]))
        torch.cuda.synchronize()
        t_capture = time.perf_counter() - t0
        prod = 2 if (nl * 2) % 2 == 0 else 1
        # RCCL: the all-gather and the D2H of the gathered block are part of submit() (device side), like the single-GPU record nothing is
        # unpacked on the host; gloo (flow tests): the gather itself happens at hand-over, so a consumer is needed
        sink = (lambda *a: None) if (plan is not None and sp.gather == "host") else None
        sp.run(corpus, bl, max_batches=4 * nl, on_result=sink)                                     # warm the pipeline
        if plan is None:
            r = sp.run(corpus, bl, min_seconds=seconds, producers=prod)
            elapsed, pairs_all, rounds = r["seconds"], r["pairs"], r["batches"]
        else:
            rounds = plan.rounds(len(bl))
            if seconds is not None:       # a fixed round count every rank agrees on (a round is a collective): calibrated on rank-local time, MIN over ranks
                probe = sp.run(corpus, bl, max_batches=8 * nl, cycle=True, on_result=sink, producers=prod)
                want = torch.tensor([max(4 * nl, seconds / (probe["seconds"] / probe["batches"]))], dtype=torch.float64,
                                    device=env.dev if env.backend == "nccl" else "cpu")
                env.dist.all_reduce(want, op=env.dist.ReduceOp.MIN)
                rounds = int(want.item())
            torch.cuda.synchronize()
            env.barrier()
            t1 = time.perf_counter()
            r = sp.run(corpus, bl, max_batches=rounds, cycle=True, on_result=sink, producers=prod)
            torch.cuda.synchronize()
            env.barrier()
            elapsed = env.max_over_ranks(time.perf_counter() - t1)
            tot = torch.tensor([float(r["pairs"])], dtype=torch.float64, device=env.dev if env.backend == "nccl" else "cpu")
            env.dist.all_reduce(tot)
            pairs_all = float(tot.item()) * (W if sp.emulated else 1)        # (emulated world: every other rank would have scored the same share)
        if env.rank != 0:
            return None
        hist = {int(k): int(v) for k, v in zip(*np.unique(corpus.lengths, return_counts=True))}
        per_round_batches = mk * (1 if plan is None or plan.mode == "pair" else W)
        par = "single GPU"
        if plan is not None:
            par = ("stream over %d ranks, mode '%s' (%s), all-gather of the click probabilities of every batch to every rank (%s) overlapped with the next "
                   "batch's H2D / widen / encode; %d rounds on every rank" % (
                       W, plan.mode, "rank r scores sampler batches r, r+%d, .. whole" % W if plan.mode == "batch" else
                       "every batch cut into %d blocks of %d whole sessions, the batch's click count shipped with the block" % (W, plan.bper),
                       {"device": "RCCL on the lane's communication stream", "host": "gloo through the host", "none": "none"}[sp.gather], rounds))
            if sp.emulated:
                par += " [EMULATED on one GPU: rank 0's share, loop-back collective, no xGMI latency; value = %d x this rank's pairs]" % W
        return {"name": "C5_stream", "baseline_config": "configs[4]: CARS at MSMARCO scale: ~224k-session stream, 50 candidates/query, bf16",
                "emulated": bool(plan is not None and sp.emulated), "emulated_world": W if (plan is not None and sp.emulated) else None,
                "workload": "cars bf16, %d sessions, S ~ clip(Poisson(4.84)+2,2,16) (mean %.2f), %d candidates, q_len %d, doc_len %d, batches of %d equal-length "
                            "sessions (reference sampler), ids from the host per batch" % (len(corpus), float(corpus.lengths.mean()), c["cands"], c["qlen"], c["dlen"], c["batch"]),
                "pairs_per_s": round(pairs_all / elapsed, 1), "sessions_per_s": round(pairs_all / c["cands"] / float(corpus.lengths.mean()) / elapsed, 1),
                "batches": int(rounds * per_round_batches), "rounds": int(rounds), "world_size": env.world, "shard_axis": None if plan is None else plan.mode,
                "parallelism": par, "macro_batch": mk, "sampler_batches": n_sampler_batches, "left_over_batches_not_timed": len(rest),
                "whole_stream": seconds is None, "seconds": round(elapsed, 3), "h2d_GBps": round(r["h2d_GBps"], 3), "lanes": r["lanes"],
                "slots_per_lane": r["slots_per_lane"], "producer_threads": r["producers"], "session_lengths": lengths, "length_histogram": hist,
                "graphs": len(lengths) * nl, "graph_capture_s": round(t_capture, 2), "corpus_build_s": round(t_corpus, 2), "dtype": "bf16",
                "wire": "int32 ids/lengths + float32 labels (nir_widen_ids_i32 on device); D2H of the click probabilities included",
                "ms_per_step": round(elapsed / max(1, rounds * per_round_batches) * 1e3, 5)}
    except Exception as e:  # pragma: no cover
        if env.multi:
            raise          # (a rank that drops out of a collective sequence must take the job down, not hang the others)
        return {"name": "C5_stream", "error": "%s: %s" % (type(e).__name__, e)}


def train_record(kind, c, args, env, steps=12):
    """Training step throughput: Ranker.update / Multitask.update (models/ranker.py:192-230, models/multitask.py:161-223)
    = train-mode forward with the reference's default dropouts, loss, backward, clip_grad_norm, Adam -- on the config's batch shape, batches
    resident in HBM, eager (torch.autograd over the HIP operators of autograd.py).  Dominant kernel from the library profiler."""
    try:
        L = lib.load()
        V = c["vocab"]
        extra = dict(optimizer="adam", learning_rate=0.001, weight_decay=0, momentum=0, grad_clipping=10.0, fix_embeddings=True)
        if kind in ("CARS", "MNSRF", "M_MATCH_TENSOR"):
            w = Multitask(default_args(kind, src_vocab_size=V, tgt_vocab_size=30000, **extra))
        else:
            w = Ranker(default_args(kind, src_vocab_size=V, **extra))
        fill_module_(w.network, 1013)
        w.cuda()
        w.init_optimizer()
        w.id_check_interval = 0
        batches = make_batches(c, 4, 0, env.dev)
        if kind in ("CARS", "MNSRF", "M_MATCH_TENSOR"):     # teacher-forcing targets: the next query of the session, [BOS w.. EOS] (multitask/vector.py:82-149)
            for b in batches:
                src = b["source_words"][:, 1:]                                                     # [B,S-1,QL]
                B_, S1, QL = src.shape
                tw = torch.zeros(B_, S1, QL + 2, dtype=torch.int64, device=env.dev)
                tw[..., 0] = 2
                tw[..., 1:QL + 1] = src
                tw[..., QL + 1] = 3
                b["target_words"], b["target_seq"] = tw, tw % 30000
                b["target_lens"] = torch.full((B_, S1), QL + 2, dtype=torch.int64, device=env.dev)
        for i in range(3):
            w.update(batches[i % 4])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            w.update(batches[i % 4])
        torch.cuda.synchronize()
        dt_eager = (time.perf_counter() - t0) / steps
        # the same step as ONE hipGraph (wrappers.GraphedUpdate: static batch buffers, device-resident dropout seed, capturable Adam)
        dt, graphed = dt_eager, False
        try:
            from context_attentive_ir_amd.wrappers import GraphedUpdate
            step = GraphedUpdate(w)
            for i in range(3):                    # first call per shape: eager step + capture (all four batches share one shape)
                step(batches[i % 4])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                step(batches[i % 4])
            torch.cuda.synchronize()
            dt, graphed = (time.perf_counter() - t0) / steps, True
        except Exception as e:  # pragma: no cover
            sys.stderr.write("[bench] graphed update unavailable (%s: %s); eager figure reported\n" % (type(e).__name__, e))
        L.nir_profile_enable(1)
        for i in range(4):
            w.update(batches[i % 4])
        torch.cuda.synchronize()
        L.nir_profile_enable(0)
        buf = ctypes.create_string_buffer(1 << 17)
        L.nir_profile_report(buf, len(buf))
        kern = {}
        for line in buf.value.decode().strip().splitlines():
            kname, cnt, ms = line.rsplit(",", 2)
            kern[kname] = (int(cnt), float(ms))
        pairs = c["batch"] * c["cands"] * (c.get("session", 1) if kind in ("CARS", "MNSRF", "M_MATCH_TENSOR") else 1)
        rec = {"workload": "%s.update on the %s batch shape (train-mode forward + loss + backward + clip + Adam, default dropouts), %s" % (
                   "Multitask" if kind in ("CARS", "MNSRF", "M_MATCH_TENSOR") else "Ranker", c.get("baseline", "")[:11],
                   "one hipGraph per step (wrappers.GraphedUpdate)" if graphed else "eager"),
               "ms_per_step": round(dt * 1e3, 4), "updates_per_s": round(1.0 / dt, 2), "pairs_per_s": round(pairs / dt, 1), "dtype": "f32",
               "hipgraph": graphed, "eager_ms_per_step": round(dt_eager * 1e3, 4),
               "hip_kernel_ms_per_step": round(sum(v[1] for v in kern.values()) / 4, 4)}
        if kern:
            dom = max(kern, key=lambda k: kern[k][1])
            cnt, ms = kern[dom]
            avg_us = ms / cnt * 1e3
            rf = {"kernel": dom, "avg_us": round(avg_us, 3), "launches_per_step": cnt / 4.0, "share_of_hip_kernel_time": round(ms / sum(v[1] for v in kern.values()), 4)}
            work = kernel_work(dom, c)
            if work:
                tf = work["flops"] * max(1, work["terms"]) / (avg_us * 1e-6) / 1e12
                rf.update(bound="mfma", achieved=round(tf, 3), peak=round(work["pipe"], 1), unit="TFLOP/s", frac=round(tf / work["pipe"], 5),
                          mfma_frac=round(tf / work["pipe"], 5))
            rec["roofline"] = rf
            rec["top_kernels_ms_per_step"] = {k: round(v[1] / 4, 4) for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1])[:6]}
            if os.environ.get("BENCH_TRAIN_ALL_KERNELS"):          # every library launch label of the step: [launches per step, ms per step]
                rec["hip_kernels_per_step"] = {k: [round(v[0] / 4, 2), round(v[1] / 4, 4)] for k, v in sorted(kern.items(), key=lambda kv: -kv[1][1])}
        return rec
    except Exception as e:  # pragma: no cover
        return {"error": "%s: %s" % (type(e).__name__, e)}


def dropin_record(c, args, env):
    """The reference's OWN evaluation loop on the wrapper's DEFAULT settings: `eval.validate.reference_loop` = main/multitask.py:280-290
    as written -- one `model.predict(ex)` per batch on pinned host batches (DataLoader(pin_memory=True)), `scores.cpu().numpy()`, argsort,
    MAP / MRR / P@1,3,5 per batch, nothing else in flight -- at the headline's batch size and at the reference's default `--test_batch_size 128`
    (main/multitask.py:61), ranking only (`suggest=False`) and with the greedy decode the reference's predict always runs.  Defaults = the
    deferred id check (pinned error word) + the shape-keyed hipGraph cache inside predict(); next to each figure the same loop on round 5's
    defaults (blocking flag read-back per call, eager launches)."""
    from context_attentive_ir_amd.eval.validate import reference_loop
    try:
        kind = c["model"].upper()
        model = Multitask(default_args(kind, src_vocab_size=c["vocab"]))
        fill_module_(model.network, 1013)
        model.cuda()
        out = {"workload": "%s reference loop (predict -> .cpu().numpy() -> argsort -> MAP/MRR/P@k per batch, one batch in flight), session_len %d x %d "
                           "candidates, q_len %d, doc_len %d, vocab %d, fp32, pinned host batches" % (kind, c["session"], c["cands"], c["qlen"], c["dlen"], c["vocab"]),
               "settings": "wrapper defaults: id_check 'deferred' (interval 1), predict_graphs on"}
        for B in (c["batch"], 128):
            batches = [{k: v.pin_memory() for k, v in synth.session_batch(B, c["session"], c["cands"], c["qlen"], c["dlen"], c["vocab"], seed=50 + i).items()}
                       for i in range(8)]
            pairs = B * c["session"] * c["cands"]
            for dec in (False, True):
                ent, ref = {}, None
                for mode in ("default", "r5"):
                    model.id_check_interval = 1
                    model.id_check = "blocking" if mode == "r5" else "deferred"
                    model.args.predict_graphs = mode == "default"
                    model.clear_predict_graphs()
                    reference_loop(batches, model, 16, suggest=dec)
                    torch.cuda.synchronize()
                    iters = 150 if mode == "default" else 40
                    best = None
                    for _ in range(3):
                        t0 = time.perf_counter()
                        maps = reference_loop(batches, model, iters, suggest=dec)
                        dt = (time.perf_counter() - t0) / iters
                        best = dt if best is None else min(best, dt)
                    if ref is None:
                        ref = maps[:8]
                    ent["ms_per_call" if mode == "default" else "r5_defaults_ms_per_call"] = round(best * 1e3, 4)
                    ent["pairs_per_s" if mode == "default" else "r5_defaults_pairs_per_s"] = round(pairs / best, 1)
                    ent["map_equal_across_modes"] = maps[:8] == ref
                model.check_ids()
                out["b%d%s" % (B, "_decode" if dec else "")] = ent
        model.clear_predict_graphs()
        out["pairs_per_s"] = out["b%d" % c["batch"]]["pairs_per_s"]
        out["ms_per_step"] = out["b%d" % c["batch"]]["ms_per_call"]
        return out
    except Exception as e:  # pragma: no cover
        return {"error": "%s: %s" % (type(e).__name__, e)}


def decode_record(c, args, env):
    """Full Multitask.predict (ranking + greedy suggestion decode, models/multitask.py:229-317) on the headline workload: the whole predict
    -- encoders, session part, 10 greedy decoding steps with the 256 -> 30 000 projection -- captured into one hipGraph per resident batch,
    replayed with --streams batches in flight like the headline (eager single-stream figure reported beside it)."""
    try:
        model = build_model(c, args)
        nl = max(1, args.streams)
        batches = make_batches(c, 2 * nl, 0, env.dev)
        lanes = [torch.cuda.Stream() for _ in range(nl)]
        lib.set_batches_in_flight(nl, lanes)
        for i in range(2 * nl):
            with torch.cuda.stream(lanes[i % nl]):
                model.predict(batches[i])
        torch.cuda.synchronize()
        pairs = c["batch"] * c["session"] * c["cands"]
        n, t0 = 12, time.perf_counter()
        for i in range(n):
            model.predict(batches[i % len(batches)])
        torch.cuda.synchronize()
        eager = (time.perf_counter() - t0) / n
        mk = macro_batch(c)                                  # macro-batches of mk resident batches per graph (predict_many with decode)
        batches = make_batches(c, mk * nl * 2, 0, env.dev)
        groups = [batches[i:i + mk] for i in range(0, len(batches), mk)]
        for gi, gr in enumerate(groups):
            with torch.cuda.stream(lanes[gi % nl]):
                model.predict_many(gr, suggest=True)
        torch.cuda.synchronize()
        graphs = []
        for gi, gr in enumerate(groups):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=lanes[gi % nl], capture_error_mode=CAPTURE_MODE):
                out = model.predict_many(gr, suggest=True)
            graphs.append((g, out))
        ref = model.predict(groups[0][mk - 1])
        graphs[0][0].replay()
        torch.cuda.synchronize()
        same = bool(torch.equal(ref["predictions"], graphs[0][1]["predictions"][mk - 1])) and \
            float((ref["click_scores"] - graphs[0][1]["click_scores"][mk - 1]).abs().max()) < 1e-6
        for i in range(2 * len(graphs)):
            with torch.cuda.stream(lanes[i % nl]):
                graphs[i % len(graphs)][0].replay()
        torch.cuda.synchronize()
        n, t0 = 40 * nl, time.perf_counter()
        for i in range(n):
            with torch.cuda.stream(lanes[i % nl]):
                graphs[i % len(graphs)][0].replay()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / (n * mk)
        # roofline block (VERDICT r5 #7c): HIP events around every kernel of one macro-batched full predict, eagerly on one stream; the dominant
        # kernel priced by its own shape label (pred_argmax_kernel: executed MFMA FLOPs = 3 x 2 M N K)
        roofline = None
        try:
            torch.cuda.set_stream(lanes[0])
            lib.load().nir_profile_enable(1)
            nrep = 3
            for i in range(nrep):
                model.predict_many(groups[i % len(groups)], suggest=True)
            torch.cuda.synchronize()
            lib.load().nir_profile_enable(0)
            buf = ctypes.create_string_buffer(1 << 17)
            lib.load().nir_profile_report(buf, len(buf))
            kern = {}
            for line in buf.value.decode().strip().splitlines():
                kname, cnt, ms = line.rsplit(",", 2)
                kern[kname] = (int(cnt), float(ms))
            if kern:
                dom = max(kern, key=lambda k_: kern[k_][1])
                cnt, ms = kern[dom]
                avg_us = ms / cnt * 1e3
                roofline = {"kernel": dom, "avg_us": round(avg_us, 3), "launches_per_step": round(cnt / (nrep * mk), 4),
                            "kernels_us_per_step": {k_: round(v[1] / (nrep * mk) * 1e3, 2) for k_, v in sorted(kern.items(), key=lambda kv: -kv[1][1])[:14]}}
                work = kernel_work(dom, c)
                if work and work["terms"]:
                    exe_tf = work["flops"] * work["terms"] / (avg_us * 1e-6) / 1e12
                    roofline.update(bound="mfma", achieved=round(exe_tf, 3), peak=round(work["pipe"], 1), unit="TFLOP/s", frac=round(exe_tf / work["pipe"], 5),
                                    alg_flops_per_launch=work["flops"], mfma_terms_per_product=work["terms"], traffic=None)
        except Exception as e:  # pragma: no cover - the record stands without it
            roofline = {"error": "%s: %s" % (type(e).__name__, e)}
            lib.load().nir_profile_enable(0)
        torch.cuda.set_stream(torch.cuda.default_stream())
        lib.set_batches_in_flight(0, lanes)
        return {"roofline": roofline, "workload": "headline batch through the full predict: ranking + greedy decode of max_query_len tokens; macro-batches of %d batches "
                            "(Multitask.predict_many(suggest=True)), one hipGraph each, %d in flight" % (mk, nl), "macro_batch": mk,
                "ms_per_step": round(dt * 1e3, 4), "pairs_per_s": round(pairs / dt, 1), "suggested_queries_per_s": round(c["batch"] * (c["session"] - 1) / dt, 1),
                "hipgraph": True, "batches_in_flight": nl, "graph_predictions_equal_eager": same,
                "eager_one_in_flight_ms_per_step": round(eager * 1e3, 4), "eager_one_in_flight_pairs_per_s": round(pairs / eager, 1)}
    except Exception as e:  # pragma: no cover
        return {"error": "%s: %s" % (type(e).__name__, e)}


if __name__ == "__main__":
    main()
