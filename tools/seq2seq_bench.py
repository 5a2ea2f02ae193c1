"""Seq2seq: `Recommender.predict` (csrc/seq2seq.hip) against the reference's greedy decode written as stock torch ops on the same GPU and
weights.

Shape: scripts/recommender.sh of the reference -- batch 64, max_query_len 20, emsize 300, nhid 512, nlayers 1, general attention, a source
vocabulary of 100 000, tgt_vocab_size 30 000, max_len 20.  The torch composition is seq2seq.py:118-195 as its users run it today
(embedding, packed nn.LSTM encoder, the length-sorted initial state, per step nn.LSTM -> GlobalAttention -> generator -> softmax -> max)
with two things in its favour: the source lengths are handed over as a host list (the reference's `lengths.tolist()` synchronises), and
the token map is a device lookup table (the reference loops over `.item()` and two Python dicts on the host every step).

Prints one JSON line: ms per batch (median of --iters, CUDA events, after --warmup) of predict() with the fused generator + arg-max kernel,
of predict() with the unfused generator (fp32 GEMM + arg-max kernel), of predict() with the plain decoder step (fold_decoder_step off) and
of the torch composition, each per round of --rounds alternating rounds, the medians over the rounds, the speed-up, and whether the tokens
of the paths agree.  --rnn_type GRU times Seq2seqGRU (csrc/gru_step.hip) against nn.GRU the same way.

--beam_size W times `Recommender.predict_beam` (csrc/beam.hip) instead: the fused generator + top-k kernel against the plain form (fp32 GEMM into
[B W, VT] logits + one workgroup per row), graph replay, the same protocol; the greedy predict() of the same batch is timed next to them.

    python tools/seq2seq_bench.py [--rnn_type LSTM|GRU] [--beam_size W] [--iters 20] [--warmup 5] [--rounds 3] [--json out.json]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]
from dssm_bench import timed  # noqa: E402


def torch_decode(net, src, lens, lens_host, lut, max_len):
    """the reference's maths (seq2seq.py:118-195, general attention) as stock torch ops (fp32), written for this tool"""
    table = net.embedder.word_embeddings.table
    att = net.decoder.decoder.attn
    order = torch.sort(lens, 0, True)[1]
    packed = pack_padded_sequence(torch.nn.functional.embedding(src, table)[order], sorted(lens_host, reverse=True), batch_first=True)
    out, final = net.encoder.encoder.rnns[0](packed)
    bank = pad_packed_sequence(out, batch_first=True)[0][torch.sort(order, 0)[1]]           # un-sorted; the states stay sorted (rnn_encoder.py:104-113)
    halves = lambda s: torch.cat([s[0:s.size(0):2], s[1:s.size(0):2]], 2)                    # noqa: E731  (decoders/decoder.py:163-177)
    state = tuple(halves(s) for s in final) if isinstance(final, tuple) else halves(final)
    mask = torch.arange(bank.shape[1], device=src.device).unsqueeze(0) < lens.unsqueeze(1)
    tok = torch.full((src.shape[0], 1), 2, dtype=torch.long, device=src.device)
    preds = []
    for _ in range(max_len):
        h, state = net.decoder.decoder.rnn(torch.nn.functional.embedding(tok, table), state)
        align = torch.bmm(att.linear_in(h), bank.transpose(1, 2)).masked_fill(~mask.unsqueeze(1), float("-inf"))
        a = torch.softmax(align, -1)
        o = torch.tanh(att.linear_out(torch.cat([torch.bmm(a, bank), h], 2)))
        p = torch.softmax(net.generator(o.squeeze(1)), 1).max(1, keepdim=True)[1]
        preds.append(p.squeeze(1))
        tok = lut[p]
    return torch.stack(preds, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=64)
    ap.add_argument("--ql", type=int, default=20)
    ap.add_argument("--qmean", type=float, default=8)
    ap.add_argument("--V", type=int, default=100000)
    ap.add_argument("--VT", type=int, default=30000)
    ap.add_argument("--emsize", type=int, default=300)
    ap.add_argument("--nhid", type=int, default=512)
    ap.add_argument("--max_len", type=int, default=20)
    ap.add_argument("--rnn_type", default="LSTM", choices=["LSTM", "GRU"])
    ap.add_argument("--beam_size", type=int, default=0, help="> 0: time predict_beam of this width (fused against plain generator top-k)")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3, help="alternating repeats of the timings; the spread of their medians is reported")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.detinit import fill_module_
    from context_attentive_ir_amd.wrappers import Recommender
    rng = np.random.default_rng(1)
    # src_dict[tgt_dict[i]]: tgt_dict = identity, src_dict = a random map into the source vocabulary (its first VT entries are the ones looked up)
    src_dict = [int(x) for x in rng.integers(4, a.V, size=a.V)]
    r = Recommender(default_args("SEQ2SEQ", emsize=a.emsize, nhid=a.nhid, nlayers=1, max_query_len=a.max_len, rnn_type=a.rnn_type), src_dict, list(range(a.VT)))
    fill_module_(r.network, 1013)
    r.cuda()
    r.predict_graph_min_calls = 2          # the timed calls replay the captured graph (the default captures at the eighth sighting of a shape)
    net = r.network.eval()
    lens = np.clip(rng.poisson(a.qmean, size=a.B), 1, a.ql).astype(np.int64)
    lens[0] = a.ql
    src = rng.integers(4, a.V, size=(a.B, a.ql), dtype=np.int64)
    src[np.arange(a.ql)[None] >= lens[:, None]] = 0
    ex = dict(source_words=torch.from_numpy(src).unsqueeze(1).cuda(), source_lens=torch.from_numpy(lens).unsqueeze(1).cuda())
    lut = torch.tensor(src_dict[:a.VT], dtype=torch.int64).cuda()
    srcd, lensd, lens_host = ex["source_words"].squeeze(1), ex["source_lens"].squeeze(1), lens.tolist()

    def ours():
        return r.predict(ex)["prediction_ids"]

    def flavour(fuse, fold=True):
        net.fuse_generator_argmax, net.fold_decoder_step = fuse, fold             # (part of the pack's key: the next call captures the other path)

    if a.beam_size > 0:
        def beam():
            return r.predict_beam(ex, a.beam_size)["prediction_ids"]
        fused_r, plain_r, greedy_r = [], [], []
        with torch.no_grad():
            for _ in range(max(1, a.rounds)):
                net.fuse_generator_topk = True
                fused_r.append(timed(beam, a.iters, a.warmup))
                p_fused = beam().clone()
                net.fuse_generator_topk = False
                plain_r.append(timed(beam, a.iters, a.warmup))
                p_plain = beam().clone()
                greedy_r.append(timed(ours, a.iters, a.warmup))
            net.fuse_generator_topk = True
        fused, plain, greedy = (float(np.median(v)) for v in (fused_r, plain_r, greedy_r))
        out = dict(model="seq2seq_beam", rnn_type=a.rnn_type, beam_size=a.beam_size, B=a.B, QL=a.ql, emsize=a.emsize, nhid=a.nhid, V=a.V, VT=a.VT,
                   max_len=a.max_len, ms_per_decode=round(fused, 4), plain_topk_ms_per_decode=round(plain, 4), greedy_ms_per_decode=round(greedy, 4),
                   ms_rounds=[round(v, 4) for v in fused_r], plain_topk_ms_rounds=[round(v, 4) for v in plain_r],
                   greedy_ms_rounds=[round(v, 4) for v in greedy_r], fused_wins_outside_spread=bool(max(fused_r) < min(plain_r)),
                   tokens_equal_fused_plain=float((p_fused == p_plain).float().mean()))
        print(json.dumps(out))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(out, f, indent=1)
        return

    with torch.no_grad():
        fused_r, plain_r, step_r, ref_r = [], [], [], []
        for _ in range(max(1, a.rounds)):                    # the paths alternate, so that drift of the machine meets all of them
            flavour(True)
            fused_r.append(timed(ours, a.iters, a.warmup))
            p_fused = ours().clone()
            flavour(False)
            plain_r.append(timed(ours, a.iters, a.warmup))
            p_plain = ours().clone()
            flavour(True, False)
            step_r.append(timed(ours, a.iters, a.warmup))
            p_step = ours().clone()
            ref_r.append(timed(lambda: torch_decode(net, srcd, lensd, lens_host, lut, a.max_len), a.iters, a.warmup))
        p_ref = torch_decode(net, srcd, lensd, lens_host, lut, a.max_len)
    fused, plain, step, ref = (float(np.median(v)) for v in (fused_r, plain_r, step_r, ref_r))
    out = dict(model="seq2seq", rnn_type=a.rnn_type, B=a.B, QL=a.ql, emsize=a.emsize, nhid=a.nhid, V=a.V, VT=a.VT, max_len=a.max_len,
               ms_per_batch=round(fused, 4), unfused_ms_per_batch=round(plain, 4), torch_ms_per_batch=round(ref, 4),
               plain_step_ms_per_batch=round(step, 4), plain_step_ms_rounds=[round(v, 4) for v in step_r],
               tokens_equal_plain_step=float((p_fused == p_step).float().mean()),
               ms_rounds=[round(v, 4) for v in fused_r], unfused_ms_rounds=[round(v, 4) for v in plain_r], torch_ms_rounds=[round(v, 4) for v in ref_r],
               speedup=round(ref / fused, 2), unfused_speedup=round(ref / plain, 2),
               tokens_equal_fused_unfused=float((p_fused == p_plain).float().mean()), tokens_equal_torch=float((p_fused == p_ref).float().mean()))
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
