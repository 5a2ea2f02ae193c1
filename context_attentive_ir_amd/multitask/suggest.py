"""Suggestion side shared by M_MATCH_TENSOR and MNSRF (the reference's two session models whose decoder has no attention):

* session_states: the unidirectional session LSTM over the S pooled queries of every session -> the session bank AND the decoder's
  initial states, i.e. the LSTM state after every query but the last, concatenated along the batch axis in STEP-major order
  (/root/reference/neuroir/multitask/mmtensor.py:94-124, mnsrf.py:88-112);
* greedy_decode: embedding -> Decoder(attn_type='none') LSTM step -> generator -> arg-max -> target id mapped to its source id and
  fed back (mmtensor.py:281-325, mnsrf.py:251-296) -- nir_decode_greedy_plain, no host synchronisation.
"""
import math

import torch

from .. import autograd as A
from .. import lib
from ..constants import BOS, EOS, PAD, UNK


def session_states(x, lstm):
    """x [B,S,I] pooled queries, lstm = the session encoder's single-layer unidirectional nn.LSTM (parameter container)
    -> (session_bank [B,S,HS], (h [1,(S-1)*B,HS], c [1,(S-1)*B,HS]))."""
    L, st = lib.load(), lib.stream()
    B, S, I = x.shape
    HS = lstm.hidden_size
    dev = x.device
    wih, whh = lstm.weight_ih_l0.detach().float().contiguous(), lstm.weight_hh_l0.detach().float().contiguous().view(1, 4 * HS, HS)
    bih, bhh = lstm.bias_ih_l0.detach().float().contiguous(), lstm.bias_hh_l0.detach().float().contiguous()
    xf = x.float().contiguous()
    gates = torch.empty(B * S, 4 * HS, device=dev, dtype=torch.float32)
    lib.check(L.nir_linear_f32(lib.ptr(xf), I, None, None, 0, 0, 0, lib.ptr(wih), I, lib.ptr(bih), lib.ptr(bhh), lib.ptr(gates), 4 * HS,
                               B * S, 4 * HS, I, 0, st), "nir_linear_f32")
    bank = torch.empty(B, S, HS, device=dev, dtype=torch.float32)
    cst = torch.empty(B, S, HS, device=dev, dtype=torch.float32)
    ws = lib.workspace(L.nir_bilstm_steps_workspace_bytes(B, HS), dev)
    lib.check(L.nir_birnn_steps_fwd(0, lib.ptr(gates), None, lib.ptr(whh), None, None, None, lib.ptr(bank), lib.ptr(cst), None, None, B, S, HS, 1,
                                    lib.ptr(ws), ws.numel(), st), "nir_birnn_steps_fwd")
    # states after queries 0 .. S-2, step-major along the batch axis (torch.cat(states[:-1], dim=1) of the reference)
    h = bank[:, :S - 1].transpose(0, 1).reshape(1, (S - 1) * B, HS).contiguous()
    c = cst[:, :S - 1].transpose(0, 1).reshape(1, (S - 1) * B, HS).contiguous()
    return bank, (h, c)


def tgt2src_lut(owner, src_dict, tgt_dict, n, dev):
    """[V_tgt] device lookup table target id -> source id (the reference maps every predicted token through tgt_dict[idx] -> word ->
    src_dict[word] on the host); cached on `owner`; None (identity) without dictionaries."""
    if src_dict is None or tgt_dict is None:
        return None
    key = (id(src_dict), id(tgt_dict), len(src_dict), len(tgt_dict), str(dev))
    if getattr(owner, "_lut_key", None) != key:
        lut = [int(src_dict[tgt_dict[i]]) if i < len(tgt_dict) else 0 for i in range(n)]
        owner._lut, owner._lut_key = torch.tensor(lut, dtype=torch.int64, device=dev), key
    return owner._lut


def candidate_inputs(owner, candidate_seq, candidate_rep, src_dict, tgt_dict, tgt2src, VT, V):
    """the embedder ids a teacher-forced scorer feeds for candidate_seq [..., TL] (target-vocabulary ids, BOS first): candidate_rep through the
    model's id check where given, else what the decodes feed -- the first token as it is (they start from BOS itself, an id both vocabularies
    share), tgt2src[token] behind it (the token itself without a table), <unk> outside the source vocabulary"""
    if candidate_rep is not None:
        return owner._clean_ids(candidate_rep.reshape(candidate_seq.shape), None, V)[0]
    if tgt2src is None:
        tgt2src = tgt2src_lut(owner, src_dict, tgt_dict, VT, candidate_seq.device)
    rep = candidate_seq if tgt2src is None else torch.cat((candidate_seq[..., :1], tgt2src[candidate_seq[..., 1:].clamp(0, VT - 1)]), -1)
    return torch.where((rep >= 0) & (rep < V), rep, torch.full_like(rep, UNK))


def score_rows(owner, dec_out, candidate_seq, gen_w, gen_b, gen_frag):
    """The tail of every score_candidates (include/neuroir_score.h).  dec_out [..., TL - 1, K]: the decoder outputs of the
    teacher-forced steps, rows in candidate_seq's order; candidate_seq [..., TL].  ONE nir_score_gen_target over all rows -- step t against token
    t + 1; gen_frag (a uint8 tensor, or None: the plain form) -- and one nir_score_sequences -> {'token_logprobs': [..., TL - 1], 'scores':
    [...], 'lengths': LongTensor [...]}.  An id outside the target vocabulary sets the device's id flag (owner.check_ids())."""
    L = lib.load()
    lead, TL = tuple(candidate_seq.shape[:-1]), int(candidate_seq.shape[-1])
    T, K, VT = TL - 1, int(dec_out.shape[-1]), int(gen_w.shape[0])
    x = dec_out.reshape(-1, K).float().contiguous()
    dev = x.device
    R = x.shape[0]
    nseq = R // T
    target = candidate_seq[..., 1:].reshape(-1).contiguous()
    logp = torch.empty(R, dtype=torch.float32, device=dev)
    scores = torch.empty(nseq, dtype=torch.float32, device=dev)
    lengths = torch.empty(nseq, dtype=torch.int64, device=dev)
    if R > 0:
        ws = lib.workspace(L.nir_score_gen_target_workspace_bytes(R, K, VT, 1 if gen_frag is not None else 0), dev)
        lib.check(L.nir_score_gen_target(lib.ptr(x), R, K, lib.ptr(gen_w), lib.ptr(gen_b), lib.ptr(gen_frag), VT, lib.ptr(target), PAD, lib.ptr(ws),
                                         ws.numel(), lib.ptr(logp), None, lib.ptr(owner._flag_word(dev)), lib.stream()), "nir_score_gen_target")
        lib.check(L.nir_score_sequences(lib.ptr(logp), lib.ptr(target), nseq, T, PAD, EOS, lib.ptr(scores), lib.ptr(lengths), lib.stream()),
                  "nir_score_sequences")
    return {"token_logprobs": logp.view(lead + (T,)), "scores": scores.view(lead), "lengths": lengths.view(lead)}


def candidate_front(owner, states, candidate_seq, candidate_rep, src_dict, tgt_dict, tgt2src, batch_size, session_len, table, dec_rnn, VT):
    """The front every session model's score_candidates shares: the shape checks, candidate_inputs, the embedding, ONE
    GEMM for the input gates of all teacher-forced steps and ONE nir_birnn_steps_fwd over the Bd N sequences of TL - 1 steps, each started from
    the state of its decode row -> (h_all [Bd N, TL - 1, H], candidate_seq as int64 [B, S-1, N, TL]).  Candidate row (i, n), i = b (S-1) + j,
    starts from row i of `states` -- the pairing of decode() and decode_beam()."""
    name = type(owner).__name__
    if owner.training:
        raise NotImplementedError("HIP %s.score_candidates runs in eval mode" % name)
    B, SD = int(batch_size), int(session_len)
    cand = lib.ids64(candidate_seq)
    if cand.dim() != 4 or tuple(cand.shape[:2]) != (B, SD) or cand.shape[3] < 2:
        raise ValueError("score_candidates: candidate_seq must be [B, S-1, N, TL] = [%d, %d, N, TL] with TL >= 2 (got %s)" % (B, SD, tuple(cand.shape)))
    if candidate_rep is not None and candidate_rep.numel() != cand.numel():
        raise ValueError("score_candidates: candidate_rep %s does not match candidate_seq %s" % (tuple(candidate_rep.shape), tuple(cand.shape)))
    lib.require_device(*states, cand, candidate_rep, table)
    L, st = lib.load(), lib.stream()
    dec_h, dec_c = (s.reshape(-1, s.shape[-1]).float().contiguous() for s in states)
    Bd, H = dec_h.shape
    if Bd != B * SD:
        raise RuntimeError("score_candidates: %d initial states for %d x %d decode rows" % (Bd, B, SD))
    dev = dec_h.device
    N, T = int(cand.shape[2]), int(cand.shape[3]) - 1
    rep = candidate_inputs(owner, cand, candidate_rep, src_dict, tgt_dict, tgt2src, int(VT), table.shape[0])
    M = Bd * N
    h_all = torch.empty(M, T, H, device=dev, dtype=torch.float32)
    if M == 0:
        return h_all, cand
    t = table.detach().float().contiguous()
    emb = A.embed(rep[..., :-1].reshape(M, T), t).reshape(M * T, -1).contiguous()
    wih, whh, bih, bhh = (getattr(dec_rnn, n).detach().float().contiguous() for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"))
    E = emb.shape[1]
    gates = torch.empty(M * T, 4 * H, device=dev, dtype=torch.float32)
    lib.check(L.nir_linear_f32(lib.ptr(emb), E, None, None, 0, 0, 0, lib.ptr(wih), E, lib.ptr(bih), lib.ptr(bhh), lib.ptr(gates), 4 * H, M * T, 4 * H, E,
                               0, st), "nir_linear_f32")
    h0, c0 = dec_h.repeat_interleave(N, 0).contiguous(), dec_c.repeat_interleave(N, 0).contiguous()          # rows (i, n)
    ws = lib.workspace(L.nir_bilstm_steps_workspace_bytes(M, H), dev)
    lib.check(L.nir_birnn_steps_fwd(0, lib.ptr(gates), None, lib.ptr(whh), None, lib.ptr(h0), lib.ptr(c0), lib.ptr(h_all), None, None, None, M, T, H, 1,
                                    lib.ptr(ws), ws.numel(), st), "nir_birnn_steps_fwd")
    return h_all, cand


def plain_candidate_rows(owner, states, candidate_seq, candidate_rep, src_dict, tgt_dict, batch_size, session_len, table, dec_rnn, generator,
                         tgt2src=None):
    """score_candidates of the two decoders without attention (M_MATCH_TENSOR, MNSRF): candidate_front, then score_rows on
    the LSTM outputs with the generator's weight and bias.  The generator fragments are a pack of their own (`_pgen_score`): the beam's row cap
    does not apply -- the score kernel stages a row block once per vocabulary range, not once per step -- and `fuse_generator_topk = False`
    selects the plain generator form here as it does in the beam."""
    VT = generator.weight.shape[0]
    h_all, cand = candidate_front(owner, states, candidate_seq, candidate_rep, src_dict, tgt_dict, tgt2src, batch_size, session_len, table, dec_rnn, VT)
    frag = gen_frag_pack(owner, generator.weight, 0, attr="_pgen_score")
    gw, gb = generator.weight.detach().float().contiguous(), generator.bias.detach().float().contiguous()
    return score_rows(owner, h_all.view(tuple(cand.shape[:3]) + h_all.shape[1:]), cand, gw, gb, frag)


def plain_fold(owner, table, dec_rnn, t, p, H, dev):
    """(folded gate table, W_hh fragments) of a decoder without attention, or None -- shared by greedy_decode and beam_decode, cached on `owner`.
    The decoder LSTM's input is the previous token's embedding alone: gate rows folded per token + W_hh as fp16 term fragments, once per weight
    version (a weight outside the split's range, H % 32 != 0 or `fold_decoder_step = False` on the model keep the fp32 step)."""
    L = lib.load()

    def build():
        nb = L.nir_lstm_step_whh_frag_bytes(H)
        if not (getattr(owner, "fold_decoder_step", True) and nb and t.is_cuda and t.shape[0] * 4 * H * 4 <= getattr(owner, "fold_budget_bytes", 64 << 30)):
            return None
        frag, flag = torch.empty(nb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        lib.check(L.nir_lstm_step_pack_whh_frag(lib.ptr(p[1]), H, lib.ptr(frag), lib.ptr(flag), lib.stream()), "nir_lstm_step_pack_whh_frag")
        if int(flag.item()) != 0:
            return None
        return lib.fold_lstm_table(t, p[0], p[2], p[3], H, 1, "f32"), frag
    cache = getattr(owner, "_pdec_plain", None)
    if cache is None:
        cache = owner._pdec_plain = lib.PackCache(retain=1)
    return cache.get([table] + [getattr(dec_rnn, n) for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
                     + [getattr(owner, "fold_decoder_step", True)], build)


class PlainInputs(object):
    """What greedy_decode, beam_decode and sample_decode prepare alike for a decoder without attention: the initial states as [Bd, H] rows (Bd =
    batch_size x session_len, else the row-count error), the generator's weight and bias, the target -> source table (given, or tgt2src_lut),
    the embedding table as fp32, the four LSTM tensors and plain_fold's pair (or None).  The tensors stay alive with the record."""

    def __init__(self, owner, states, src_dict, tgt_dict, batch_size, session_len, table, dec_rnn, generator, tgt2src):
        self.dec_h, self.dec_c = (s.reshape(-1, s.shape[-1]).float().contiguous() for s in states)
        self.B, self.SD = int(batch_size), int(session_len)
        self.Bd, self.H = self.dec_h.shape
        if self.Bd != self.B * self.SD:
            raise RuntimeError("decode: %d initial states for %d x %d decode rows" % (self.Bd, batch_size, session_len))
        self.dev = self.dec_h.device
        self.gw, self.gb = generator.weight.detach().float().contiguous(), generator.bias.detach().float().contiguous()
        self.VT = self.gw.shape[0]
        self.tgt2src = tgt2src_lut(owner, src_dict, tgt_dict, self.VT, self.dev) if tgt2src is None else tgt2src
        self.t = table.detach().float().contiguous()
        self.p = [getattr(dec_rnn, n).detach().float().contiguous() for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
        self.fold = plain_fold(owner, table, dec_rnn, self.t, self.p, self.H, self.dev)

    def c_args(self, max_len):
        """the arguments the three plain entries share, states to fold pointers"""
        t, fold = self.t, self.fold
        return [lib.ptr(self.dec_h), lib.ptr(self.dec_c), self.Bd, self.H, lib.ptr(t), t.shape[0], t.shape[1]] + [lib.ptr(x) for x in self.p] + [
            lib.ptr(self.gw), lib.ptr(self.gb), self.VT, lib.ptr(self.tgt2src), BOS, max_len, lib.ptr(fold[0]) if fold else None,
            lib.ptr(fold[1]) if fold else None]


def greedy_decode(owner, states, max_len, src_dict, tgt_dict, batch_size, session_len, table, dec_rnn, generator, tgt2src=None):
    """-> {'predictions': LongTensor [batch_size, session_len, max_len]} in target-vocabulary ids; `session_len` = decoded queries per
    session (the caller passes S-1, models/multitask.py:286)."""
    L = lib.load()
    c = PlainInputs(owner, states, src_dict, tgt_dict, batch_size, session_len, table, dec_rnn, generator, tgt2src)
    max_len = int(max_len)
    ws = lib.workspace(L.nir_decode_greedy_plain_workspace_bytes(c.Bd, c.H, c.VT), c.dev)
    preds = torch.empty(c.Bd, max_len, dtype=torch.int64, device=c.dev)
    lib.check(L.nir_decode_greedy_plain_folded(*c.c_args(max_len), lib.ptr(ws), ws.numel(), lib.ptr(preds), lib.stream()),
              "nir_decode_greedy_plain_folded")
    return {"predictions": preds.view(c.B, c.SD, max_len)}


FUSE_TOPK_MAX_ROWS = 384     # beam rows up to which the fused generator + top-k is the default (it wins at 384, loses at 768)
FUSE_SAMPLE_MAX_ROWS = 512   # decode rows up to which the fused generator + Gumbel arg-max is the default (it wins at 512, not at 768)


def gen_frag_pack(owner, weight, rows, attr="_pgen_beam", wanted=None):
    """nir_seq2seq_pack_gen_frag of a generator weight [VT, K] (the fused generator + top-W kernel of the beam reads it), once per weight version,
    cached on `owner`; None when K has no fragment form, the weight lies outside the split's range, the model says `fuse_generator_topk = False`
    or the decode has more than `fuse_topk_max_rows` (default FUSE_TOPK_MAX_ROWS) beam rows: the fused kernel re-reads the fragments once per
    64-row block, and from there on the fp32 GEMM + row top-k was measured faster.  wanted (a bool): the caller's own switch and cap in the
    place of those two (sample_fused below)."""
    if (not getattr(owner, "fuse_generator_topk", True) or rows > getattr(owner, "fuse_topk_max_rows", FUSE_TOPK_MAX_ROWS)) if wanted is None else not wanted:
        return None
    L = lib.load()

    def build():
        w = weight.detach().float().contiguous()
        VT, K = w.shape
        nb = L.nir_seq2seq_gen_frag_bytes(VT, K)
        if not (nb and w.is_cuda):
            return None
        frag, flag = torch.empty(nb, dtype=torch.uint8, device=w.device), torch.zeros(1, dtype=torch.int32, device=w.device)
        lib.check(L.nir_seq2seq_pack_gen_frag(lib.ptr(w), VT, K, lib.ptr(frag), lib.ptr(flag), lib.stream()), "nir_seq2seq_pack_gen_frag")
        return frag if int(flag.item()) == 0 else None
    cache = getattr(owner, attr, None)
    if cache is None:
        cache = lib.PackCache(retain=1)
        setattr(owner, attr, cache)
    return cache.get([weight], build)


def beam_outputs(Bd, W, max_len, dev, return_backptr, QL=None):
    """the output tensors of a beam entry over Bd decode rows; QL: the attention decoders' 'attentions' [Bd, W, max_len, QL] with them"""
    out = {"predictions": torch.empty(Bd, W, max_len, dtype=torch.int64, device=dev), "scores": torch.empty(Bd, W, dtype=torch.float32, device=dev),
           "lengths": torch.empty(Bd, W, dtype=torch.int64, device=dev)}
    if QL is not None:
        out["attentions"] = torch.empty(Bd, W, max_len, QL, dtype=torch.float32, device=dev)
    if return_backptr:
        out["backptr"] = torch.empty(max_len, Bd, W, dtype=torch.int32, device=dev)
    return out


def beam_view(out, B, SD):
    """predictions, scores and lengths of a beam entry, [Bd, W, ...], viewed [B, SD, W, ...] in place ('backptr' stays [max_len, Bd, W])"""
    for k in ("predictions", "scores", "lengths"):
        out[k] = out[k].view((B, SD) + tuple(out[k].shape[1:]))
    return out


def check_beam_size(W, VT):
    if not 1 <= W <= lib.BEAM_MAX_W or W > VT:
        raise ValueError("decode_beam: beam_size %d outside [1, %d] or above the target vocabulary (%d)" % (W, lib.BEAM_MAX_W, VT))


def beam_decode(owner, states, max_len, beam_size, src_dict, tgt_dict, batch_size, session_len, table, dec_rnn, generator, tgt2src=None,
                return_backptr=False):
    """Beam search next to greedy_decode (include/neuroir_session_beam.h) -> {'predictions': LongTensor [batch_size,
    session_len, W, max_len] (best beam first, EOS repeated behind the first EOS), 'scores': [batch_size, session_len, W], 'lengths': LongTensor
    [batch_size, session_len, W]} (+ 'backptr': IntTensor [max_len, Bd, W] on request).  The same fold cache as greedy_decode plus a cached
    generator fragment pack; the initial states are not repeated here -- nir_beam_plain_decode does that."""
    if owner.training:
        raise NotImplementedError("HIP %s.decode_beam runs in eval mode" % type(owner).__name__)
    lib.require_device(*states)
    L = lib.load()
    c = PlainInputs(owner, states, src_dict, tgt_dict, batch_size, session_len, table, dec_rnn, generator, tgt2src)
    W, max_len = int(beam_size), int(max_len)
    check_beam_size(W, c.VT)
    frag = gen_frag_pack(owner, generator.weight, c.Bd * W)
    out = beam_outputs(c.Bd, W, max_len, c.dev, return_backptr)
    if c.Bd > 0 and max_len > 0:
        ws = lib.workspace(L.nir_beam_plain_decode_workspace_bytes(c.Bd, c.H, c.VT, W, max_len, int(c.fold is not None), int(frag is not None)), c.dev)
        lib.check(L.nir_beam_plain_decode(*c.c_args(max_len), lib.ptr(frag), W, lib.ptr(ws), ws.numel(), lib.ptr(out["predictions"]),
                                          lib.ptr(out["scores"]), lib.ptr(out["lengths"]), lib.ptr(out.get("backptr")), lib.stream()),
                  "nir_beam_plain_decode")
    return beam_view(out, c.B, c.SD)


def check_sample_args(owner, num_samples, temperature, top_k, seed, VT):
    """the argument checks of every decode_sample (Seq2seq.decode_sample's) -> (N, top_k, temperature, seed)"""
    if owner.training:
        raise NotImplementedError("HIP %s.decode_sample runs in eval mode" % type(owner).__name__)
    N, K, tau, seed = int(num_samples), int(top_k), float(temperature), int(seed)
    if N < 1:
        raise ValueError("decode_sample: num_samples %d < 1" % N)
    if not (math.isfinite(tau) and tau > 0.0 and 1e-38 < 1.0 / tau < 3e38):      # (1 / tau travels as an fp32)
        raise ValueError("decode_sample: temperature %r is not finite and > 0" % (temperature,))
    if not 0 <= seed < (1 << 64):
        raise ValueError("decode_sample: seed %d outside [0, 2^64)" % seed)
    VT = int(VT)
    if not 0 <= K <= min(lib.BEAM_MAX_W, VT):
        raise ValueError("decode_sample: top_k %d outside {0} and [1, %d] (at most %d, and the target vocabulary's %d)"
                         % (K, min(lib.BEAM_MAX_W, VT), lib.BEAM_MAX_W, VT))
    return N, K, tau, seed


def sample_fused(owner, rows, top_k):
    """whether a decode_sample of the session models over `rows` sample rows runs its fused generator form: `fuse_generator_argmax` (top_k = 0)
    or `fuse_generator_topk` (top_k > 0) on the model, up to `fuse_sample_max_rows` sample rows in either case (None: no cap).  Measured at 384,
    768 and 1152 rows (profiles/session_sample_bench_mi355x.json): CARS' fused form wins at all three in both settings --
    the model sets no cap --; MNSRF's wins at 384 and loses at 768 in both settings, which the cap inherited from section 28
    (FUSE_SAMPLE_MAX_ROWS = 512, between the last measured win and the first loss) already separates, so it stays."""
    cap = getattr(owner, "fuse_sample_max_rows", FUSE_SAMPLE_MAX_ROWS)
    on = getattr(owner, "fuse_generator_topk", True) if top_k > 0 else getattr(owner, "fuse_generator_argmax", True)
    return bool(on) and (cap is None or rows <= cap)


def sample_outputs(Bd, N, max_len, dev, QL=None):
    """the output tensors of a sampling entry over Bd decode rows; QL: the attention decoders' 'attentions' [Bd, N, max_len, QL] with them"""
    out = {"predictions": torch.empty(Bd, N, max_len, dtype=torch.int64, device=dev),
           "token_logprobs": torch.empty(Bd, N, max_len, dtype=torch.float32, device=dev),
           "scores": torch.empty(Bd, N, dtype=torch.float32, device=dev), "lengths": torch.empty(Bd, N, dtype=torch.int64, device=dev)}
    if QL is not None:
        out["attentions"] = torch.empty(Bd, N, max_len, QL, dtype=torch.float32, device=dev)
    return out


def sample_view(out, B, SD):
    """the four outputs of a sampling entry, [Bd, N, ...], viewed [B, SD, N, ...]"""
    return {k: v.view((B, SD) + tuple(v.shape[1:])) for k, v in out.items()}


def sample_decode(owner, states, max_len, num_samples, temperature, top_k, seed, src_dict, tgt_dict, batch_size, session_len, table, dec_rnn, generator,
                  tgt2src=None):
    """Sampling next to greedy_decode and beam_decode (include/neuroir_session_sample.h) -> {'predictions': LongTensor
    [batch_size, session_len, N, max_len] (in sample order, EOS repeated behind the first EOS), 'token_logprobs': [batch_size, session_len, N,
    max_len], 'scores': [batch_size, session_len, N], 'lengths': LongTensor [batch_size, session_len, N]}.  The same fold cache as greedy_decode,
    a cached generator fragment pack of its own (`_pgen_sample`) under sample_fused's switches; the initial states are not repeated here --
    nir_sample_plain_decode does that."""
    N, K, tau, seed = check_sample_args(owner, num_samples, temperature, top_k, seed, generator.weight.shape[0])
    lib.require_device(*states)
    L = lib.load()
    c = PlainInputs(owner, states, src_dict, tgt_dict, batch_size, session_len, table, dec_rnn, generator, tgt2src)
    max_len = int(max_len)
    frag = gen_frag_pack(owner, generator.weight, c.Bd * N, attr="_pgen_sample", wanted=sample_fused(owner, c.Bd * N, K))
    out = sample_outputs(c.Bd, N, max_len, c.dev)
    if c.Bd > 0 and max_len > 0:
        nb = L.nir_sample_plain_decode_workspace_bytes(c.Bd, c.H, c.VT, N, K, max_len, int(c.fold is not None), int(frag is not None))
        if nb == 0:
            raise ValueError("%s.decode_sample: the shapes are outside the entry's range (nir_sample_plain_decode)" % type(owner).__name__)
        ws = lib.workspace(nb, c.dev)
        lib.check(L.nir_sample_plain_decode(*c.c_args(max_len), lib.ptr(frag), N, K, 1.0 / tau, seed, lib.ptr(ws), ws.numel(),
                                            lib.ptr(out["predictions"]), lib.ptr(out["token_logprobs"]), lib.ptr(out["scores"]),
                                            lib.ptr(out["lengths"]), lib.stream()), "nir_sample_plain_decode")
    return sample_view(out, c.B, c.SD)


class PlainSuggestions(object):
    """decode / decode_beam / decode_sample / score_candidates of the two session models whose decoder has no attention (M_MATCH_TENSOR:
    mmtensor.py:281-325; MNSRF: mnsrf.py:251-296): the class supplies `embedder`, `decoder.decoder.rnn`, `generator` and its own _check_eval."""

    fuse_generator_topk = True               # decode_beam: generator + bias + (lse, top-W) in one kernel (no [Bd W, VT] logits)

    def _plain_modules(self):
        return self.embedder.word_embeddings.table, self.decoder.decoder.rnn, self.generator

    def decode(self, states, max_len, src_dict, tgt_dict, batch_size, session_len, use_cuda=True, tgt2src=None, **kwargs):
        """greedy, decoder without attention -> {'predictions': LongTensor [batch_size, session_len, max_len]}."""
        self._check_eval()
        return greedy_decode(self, states, max_len, src_dict, tgt_dict, batch_size, session_len, *self._plain_modules(), tgt2src)

    def decode_beam(self, states, max_len, beam_size, src_dict, tgt_dict, batch_size, session_len, use_cuda=True, tgt2src=None, return_backptr=False,
                    **kwargs):
        """Beam search of width `beam_size` with the arguments of decode() (include/neuroir_session_beam.h) ->
        {'predictions': LongTensor [batch_size, session_len, W, max_len], 'scores': [batch_size, session_len, W], 'lengths': LongTensor
        [batch_size, session_len, W]}, best beam first."""
        self._check_eval()
        return beam_decode(self, states, max_len, beam_size, src_dict, tgt_dict, batch_size, session_len, *self._plain_modules(), tgt2src,
                           return_backptr)

    @torch.no_grad()
    def decode_sample(self, states, max_len, num_samples, src_dict, tgt_dict, batch_size, session_len, temperature=1.0, top_k=0, seed=0, use_cuda=True,
                      tgt2src=None, **kwargs):
        """`num_samples` i.i.d. draws per decode row with the arguments of decode() (include/neuroir_session_sample.h; the
        rules are Seq2seq.decode_sample's) -> {'predictions': LongTensor [batch_size, session_len, N, max_len], 'token_logprobs': [batch_size,
        session_len, N, max_len], 'scores': [batch_size, session_len, N], 'lengths': LongTensor [batch_size, session_len, N]}, in sample order."""
        return sample_decode(self, states, max_len, num_samples, temperature, top_k, seed, src_dict, tgt_dict, batch_size, session_len,
                             *self._plain_modules(), tgt2src)

    @torch.no_grad()
    def score_candidates(self, states, candidate_seq, src_dict, tgt_dict, batch_size, session_len, candidate_rep=None, tgt2src=None):
        """log P(candidate | session prefix) for N candidate next queries per decode row, with the states of decode():
        candidate_seq [B, S-1, N, TL] target-vocabulary ids, BOS first, PAD behind the end; candidate_rep: the embedder ids fed to the decoder
        (default: what decode() feeds back) -> {'token_logprobs': [B, S-1, N, TL-1], 'scores': [B, S-1, N], 'lengths': LongTensor [B, S-1, N]}
        by section 26's rules.  Candidate row b (S-1) + j starts from row b (S-1) + j of `states`, like decode()'s output rows."""
        return plain_candidate_rows(self, states, candidate_seq, candidate_rep, src_dict, tgt_dict, batch_size, session_len,
                                    *self._plain_modules(), tgt2src)


def bilstm_train(x, lens, lstm):
    """Train-mode BiLSTM memory bank [M,T,2H] for any hidden size (autograd.bilstm holds the wide-H form since round 4)."""
    return A.bilstm(x, lens, lstm)


def suggestion_loss(model, h_steps, c_steps, target_rep, target_seq):
    """Teacher-forced decoding loss shared by M_MATCH_TENSOR and MNSRF (mmtensor.py:224-254, mnsrf.py:198-228): the decoder without
    attention starts from the session state after queries 0 .. S-2 (rows step-major: torch.cat(states[:-1], 1), paired with the
    batch-major target rows exactly as the reference pairs them), generator, masked NLL summed over time and averaged over rows, plus the
    entropy regulariser.  h_steps / c_steps [B,S,HS] differentiable session states."""
    B, S, HS = h_steps.shape
    Bd = B * (S - 1)
    dec_h = h_steps[:, :S - 1].transpose(0, 1).reshape(Bd, HS)
    dec_c = c_steps[:, :S - 1].transpose(0, 1).reshape(Bd, HS)
    tgt = lib.ids64(target_rep.reshape(Bd, -1))
    seq = lib.ids64(target_seq.reshape(Bd, -1))
    emb = A.dropout(A.embed(tgt, model.embedder.word_embeddings.table), model.embedder.dropout.p, True)
    h_all, _ = A.lstm_seq(emb, model.decoder.decoder.rnn, dec_h, dec_c)                  # [Bd,TL,HS]
    h_all = A.dropout(h_all, model.dec_dropout_p, True)                                   # RNNDecoder's own dropout (dropout_rnn)
    # (the last step's logits feed nothing: sliced off in front of the generator)
    logits = A.linear(h_all[:, :-1], model.generator.weight, model.generator.bias)
    return A.suggestion_loss(logits, seq[:, 1:], PAD, model.regularize_coeff)
