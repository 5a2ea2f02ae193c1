"""HredQS -- the hierarchical recurrent encoder-decoder for context-aware query suggestion (drop-in for neuroir.recommender.hredqs.HredQS,
neuroir/recommender/hredqs.py:9-230 of the reference).

encode():  RNNEncoder over every query -> max over ALL QL positions of the zero-padded memory bank -> the unidirectional session LSTM, one step
           per query, the (h, c) of EVERY step -> [1, S B, nhid_session] in step-major order.
decode():  ONE C-ABI call for the whole greedy decode of all B S session prefixes (nir_hredqs_decode_greedy, csrc/hredqs.hip): the folded LSTM
           step and the generator + bias + arg-max kernel, two launches per step; the winner travels as an arg-max key.
decode_beam(): ONE C-ABI call for the beam search over the same prefixes (nir_beam_hredqs_decode, csrc/beam.hip): n-best suggestions with scores.
forward(): the teacher-forced loss on the differentiable HIP operators of autograd.py.
score_candidates(): log P(candidate | session prefix) of given next queries: the session states and pairing of decode(), the teacher-forced
           decoder pass, ONE generator call over the rows of all time steps that keeps the logits on chip (nir_score_gen_target, csrc/score.hip).

Kept quirks of the reference:
  * the pairing: the decoder's rows are in (b, s) order (source_rep.view(B S, -1)), the session states in (s, b) order (torch.cat over the
    steps, hredqs.py:79-83), and nothing transposes them -- decode row r = b S + s, i.e. predictions[b, s], starts from the state of STEP
    r // B of SESSION r % B.  With B = 1 or S = 1 that is the natural pairing; with B = 3, S = 4 ten of twelve rows are moved.  decode()
    and forward() both keep it (the C entry applies it itself; forward() as a differentiable transpose).
  * the max pooling runs over the padded width QL, padding zeros included: a query shorter than QL has a pooled vector >= 0.
  * bidirection = True (hyparam.HREDQS's own value) constructs, and fails in forward / decode like the reference: decoders/decoder.py:163-169
    halves the session states, which have one direction.
  * nlayers != 1 constructs, and fails in forward / decode like the reference (IndexError in its session loop).
"""
import torch
import torch.nn as nn

from .. import autograd as A
from .. import lib
from ..constants import BOS, PAD
from ..multitask import suggest
from .layers import Decoder, Embedder, Encoder, encode_train

BIDIRECTION_ERROR = "Sizes of tensors must match except in dimension 2. Expected size 1 but got size 0 for tensor number 1 in the list."
NLAYERS_ERROR = "tuple index out of range"


class HredQS(nn.Module, lib.IdCheck):
    def __init__(self, args):
        super().__init__()
        if args.rnn_type != "LSTM":
            raise NotImplementedError("HIP HredQS implements rnn_type 'LSTM' (got %r); the reference's own encode fails for GRU" % (args.rnn_type,))
        self.embedder = Embedder(args.emsize, args.src_vocab_size, args.dropout_emb)
        self.encoder = Encoder(args.rnn_type, args.emsize, args.bidirection, args.nlayers, args.nhid, args.dropout_rnn)
        self.session_encoder = Encoder(args.rnn_type, args.nhid, False, args.nlayers, args.nhid_session, args.dropout_rnn)
        self.decoder = Decoder(args.emsize, args.nlayers, args.nhid_session, "none", args.dropout_rnn)
        self.dropout = nn.Dropout(args.dropout)
        self.generator = nn.Linear(args.nhid_session, args.tgt_vocab_size)
        self.nlayers, self.nhid, self.nhid_session = int(args.nlayers), int(args.nhid), int(args.nhid_session)
        self.bidirection = bool(args.bidirection)
        self.dec_dropout_p = float(args.dropout_rnn)        # RNNDecoder.dropout (decoders/decoder.py:87)
        self.fast_decode = True                  # decode: the folded step + the keyed generator / arg-max kernel (False: the entry's plain form)
        self.fold_budget_bytes = 64 << 30
        self._pdec = lib.PackCache(retain=1)

    # ---- shared checks -----------------------------------------------------------------------------------------------------------
    def _check_config(self):
        """(before any launch, like the reference's failures)"""
        if self.nlayers != 1:
            raise IndexError(NLAYERS_ERROR)
        if self.bidirection:
            raise RuntimeError(BIDIRECTION_ERROR)

    def _decoder_weights(self):
        rnn = self.decoder.decoder.rnn
        table = self.embedder.word_embeddings.table

        def build():
            L = lib.load()
            t = dict(rnn_wih=rnn.weight_ih_l0, rnn_whh=rnn.weight_hh_l0, rnn_bih=rnn.bias_ih_l0, rnn_bhh=rnn.bias_hh_l0,
                     gen_w=self.generator.weight, gen_b=self.generator.bias)
            H, VT = int(rnn.hidden_size), int(self.generator.weight.shape[0])
            pk = lib.Packed(lib.HredqsDecoderWeights, t, dict(H=H, VT=VT))
            dev = pk.keep["gen_w"].device
            nbg, nbw = L.nir_seq2seq_gen_frag_bytes(VT, H), L.nir_lstm_step_whh_frag_bytes(H)
            if not (self.fast_decode and dev.type == "cuda" and nbg and nbw and table.is_cuda and table.shape[1] == rnn.input_size
                    and table.shape[0] * 4 * H * 4 <= self.fold_budget_bytes):
                return pk
            # the fast form needs all three packs: one blocking flag read per weight version says whether a weight lies outside the fp16
            # range of the split
            flag = torch.zeros(1, dtype=torch.int32, device=dev)
            gfrag = torch.empty(nbg, dtype=torch.uint8, device=dev)
            wfrag = torch.empty(nbw, dtype=torch.uint8, device=dev)
            lib.check(L.nir_seq2seq_pack_gen_frag(lib.ptr(pk.keep["gen_w"]), VT, H, lib.ptr(gfrag), lib.ptr(flag), lib.stream()),
                      "nir_seq2seq_pack_gen_frag")
            lib.check(L.nir_lstm_step_pack_whh_frag(lib.ptr(pk.keep["rnn_whh"]), H, lib.ptr(wfrag), lib.ptr(flag), lib.stream()),
                      "nir_lstm_step_pack_whh_frag")
            if int(flag.item()) != 0:
                return pk
            pk.keep.update(gen_frag=gfrag, rnn_whh_frag=wfrag,
                           rnn_gate_fold=lib.fold_lstm_table(table, pk.keep["rnn_wih"], pk.keep["rnn_bih"], pk.keep["rnn_bhh"], H, 1, "f32"))
            for k in ("gen_frag", "rnn_whh_frag", "rnn_gate_fold"):
                setattr(pk.struct, k, pk.keep[k].data_ptr())
            return pk
        params = list(self.decoder.parameters()) + list(self.generator.parameters())
        return self._pdec.get(params + [table, self.fast_decode, self.fold_budget_bytes], build)

    # ---- eval: encode, greedy decode -------------------------------------------------------------------------------------------------
    def _session_steps(self, src, lens, B, S):
        """ids [B S, QL] (rows in (b, s) order), lengths [B S] -> (h, c) of every session step, [B, S, nhid_session] each (eval mode)"""
        L, st = lib.load(), lib.stream()
        table = self.embedder.word_embeddings.table
        R, QL = src.shape
        _, bank = self.encoder.encoder(A.embed(src, table), lens)
        bank = bank.float().contiguous()                                  # [R, QL, nhid], zero beyond each length (dropout: eval identity)
        dev = bank.device
        nh = bank.shape[2]
        mem = torch.empty(R, nh, device=dev, dtype=torch.float32)
        lib.check(L.nir_maxpool_time_f32(lib.ptr(bank), R, QL, nh, lib.ptr(mem), st), "nir_maxpool_time_f32")
        wih, whh, bih, bhh = self.session_encoder.encoder.packed(0)       # [4HS, nhid], [1, 4HS, HS], [4HS], [4HS]
        HS = whh.shape[2]
        gates = torch.empty(R, 4 * HS, device=dev, dtype=torch.float32)
        lib.check(L.nir_linear_f32(lib.ptr(mem), nh, None, None, 0, 0, 0, lib.ptr(wih), nh, lib.ptr(bih), lib.ptr(bhh), lib.ptr(gates), 4 * HS,
                                   R, 4 * HS, nh, 0, st), "nir_linear_f32")
        hs = torch.empty(B, S, HS, device=dev, dtype=torch.float32)
        cs = torch.empty(B, S, HS, device=dev, dtype=torch.float32)
        ws = lib.workspace(L.nir_bilstm_steps_workspace_bytes(B, HS), dev)
        lib.check(L.nir_birnn_steps_fwd(0, lib.ptr(gates), None, lib.ptr(whh), None, None, None, lib.ptr(hs), lib.ptr(cs), None, None, B, S, HS, 1,
                                        lib.ptr(ws), ws.numel(), st), "nir_birnn_steps_fwd")
        return hs, cs

    def _session_steps_train(self, src, lens, B, S):
        """the same on the differentiable operators (dropout active in train mode only)"""
        tr = self.training
        table = self.embedder.word_embeddings.table
        mem, _, _ = encode_train(self.encoder.encoder.rnns[0], A.dropout(A.embed(src, table), self.embedder.dropout.p, tr), lens)
        pooled = A.max_pool(A.dropout(mem, self.dropout.p, tr))            # over the zero-padded bank: all QL positions
        return A.lstm_seq(pooled.view(B, S, -1), self.session_encoder.encoder.rnns[0])

    def encode(self, source_rep, source_len, batch_size, session_len):
        """hredqs.py:46-87: source_rep [B S, QL] with rows in (b, s) order -> (h, c), [1, S B, nhid_session] each, in STEP-major order
        (index s B + b)."""
        self._check_config()
        table = self.embedder.word_embeddings.table
        lib.require_device(source_rep, source_len, table)
        B, S = int(batch_size), int(session_len)
        src, _ = self._clean_ids(source_rep.reshape(B * S, -1), None, table.shape[0])
        lens = lib.ids64(source_len.reshape(-1))
        hs, cs = (self._session_steps_train if self.training else self._session_steps)(src, lens, B, S)
        return tuple(s.transpose(0, 1).reshape(1, S * B, -1) for s in (hs, cs))

    def _source_rows(self, source_rep, source_len, *more):
        """source_rep [B, S, QL] -> (B, S, QL, the embedding table), all tensors of the call on the device"""
        B, S, QL = source_rep.shape
        table = self.embedder.word_embeddings.table
        lib.require_device(source_rep, source_len, table, *more)
        return B, S, QL, table

    def _decode_inputs(self, source_rep, source_len, B, S, table, src_dict, tgt_dict, tgt2src):
        """what every decode and score_candidates feed their entry: the checked ids through _session_steps -> ((h, c) of every session step, the
        packed decoder weights, the target -> source table (given, or suggest.tgt2src_lut), the embedding table as fp32)"""
        src, _ = self._clean_ids(source_rep.reshape(B * S, source_rep.shape[2]), None, table.shape[0])
        hs, cs = self._session_steps(src, lib.ids64(source_len.reshape(-1)), B, S)
        w = self._decoder_weights()
        if tgt2src is None:
            tgt2src = suggest.tgt2src_lut(self, src_dict, tgt_dict, int(w.struct.VT), table.device)
        return hs, cs, w, tgt2src, table.detach().float().contiguous()

    @torch.no_grad()
    def decode(self, source_rep, source_len, max_len, src_dict, tgt_dict, src_map=None, alignment=None, blank=None, fill=None,
               source_vocabs=None, tgt2src=None):
        """hredqs.py:169-230 (greedy) -> {'predictions': LongTensor [B, S, max_len] (target-vocabulary ids)}; there are no attentions.
        source_rep [B, S, QL], source_len [B, S].  The reference maps each predicted token back to a source id on the host
        (tgt_dict[idx] -> word -> src_dict[word]); here that is one device lookup table (identity without dictionaries)."""
        if self.training:
            raise NotImplementedError("HIP HredQS.decode runs in eval mode")
        self._check_config()
        B, S, _, table = self._source_rows(source_rep, source_len)
        L = lib.load()
        max_len = int(max_len)
        dev = table.device
        preds = torch.empty(B, S, max_len, dtype=torch.int64, device=dev)
        if B * S == 0 or max_len == 0:
            return {"predictions": preds}
        hs, cs, w, tgt2src, t = self._decode_inputs(source_rep, source_len, B, S, table, src_dict, tgt_dict, tgt2src)
        ws = lib.workspace(L.nir_hredqs_decode_workspace_bytes(B, S, max_len, w.ref()), dev)
        lib.check(L.nir_hredqs_decode_greedy(lib.ptr(hs), lib.ptr(cs), B, S, lib.ptr(t), t.shape[0], t.shape[1], lib.ptr(tgt2src), BOS, max_len,
                                             w.ref(), lib.ptr(ws), ws.numel(), lib.ptr(preds), lib.stream()), "nir_hredqs_decode_greedy")
        return {"predictions": preds}

    @torch.no_grad()
    def decode_beam(self, source_rep, source_len, max_len, beam_size, src_dict=None, tgt_dict=None, tgt2src=None, return_backptr=False):
        """Beam search next to decode() (include/neuroir_hredqs_beam.h; the reference has no counterpart) ->
        {'predictions': LongTensor [B, S, W, max_len] (best beam first, EOS repeated behind the first EOS), 'scores': [B, S, W], 'lengths':
        LongTensor [B, S, W]} (+ 'backptr': IntTensor [max_len, B S, W] on request); there are no attentions.  One C-ABI call
        (nir_beam_hredqs_decode) over the same session states, pack cache and target -> source table as decode(); the entry pairs and repeats
        the states itself.  `fast_decode = False` forces its plain form."""
        if self.training:
            raise NotImplementedError("HIP HredQS.decode_beam runs in eval mode")
        self._check_config()
        max_len, W = int(max_len), int(beam_size)
        suggest.check_beam_size(W, int(self.generator.weight.shape[0]))
        if max_len < 1:
            raise ValueError("decode_beam: max_len must be positive")
        B, S, _, table = self._source_rows(source_rep, source_len)
        L = lib.load()
        dev = table.device
        out = suggest.beam_outputs(B * S, W, max_len, dev, return_backptr)
        if B * S > 0:
            hs, cs, w, tgt2src, t = self._decode_inputs(source_rep, source_len, B, S, table, src_dict, tgt_dict, tgt2src)
            ws = lib.workspace(L.nir_beam_hredqs_decode_workspace_bytes(B, S, W, max_len, w.ref()), dev)
            lib.check(L.nir_beam_hredqs_decode(lib.ptr(hs), lib.ptr(cs), B, S, lib.ptr(t), t.shape[0], t.shape[1], lib.ptr(tgt2src), BOS, max_len,
                                               w.ref(), W, lib.ptr(ws), ws.numel(), lib.ptr(out["predictions"]), lib.ptr(out["scores"]),
                                               lib.ptr(out["lengths"]), lib.ptr(out.get("backptr")), lib.stream()), "nir_beam_hredqs_decode")
        return suggest.beam_view(out, B, S)

    # ---- eval: sampling ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode_sample(self, source_rep, source_len, max_len, num_samples, temperature=1.0, top_k=0, seed=0, src_dict=None, tgt_dict=None,
                      tgt2src=None):
        """`num_samples` i.i.d. draws per session prefix next to decode() and decode_beam() (include/neuroir_session_sample.h, DESIGN.md section
        29; the rules are Seq2seq.decode_sample's, section 28) -> {'predictions': LongTensor [B, S, N, max_len] (in sample order, EOS repeated
        behind the first EOS), 'token_logprobs': [B, S, N, max_len], 'scores': [B, S, N], 'lengths': LongTensor [B, S, N]}; there are no
        attentions.  One C-ABI call (nir_sample_hredqs_decode) over the same session states, pack cache and target -> source table as decode();
        the entry pairs and repeats the states itself, and in its fast form draws on the split state the folded step leaves: no [R, VT] logits.
        `fast_decode = False` forces its plain form, as does a `fuse_sample_max_rows` set on the model for more sample rows than that (none by
        default: DESIGN.md section 29)."""
        N, K, tau, seed = suggest.check_sample_args(self, num_samples, temperature, top_k, seed, self.generator.weight.shape[0])
        self._check_config()
        max_len = int(max_len)
        if max_len < 1:
            raise ValueError("decode_sample: max_len must be positive")
        B, S, _, table = self._source_rows(source_rep, source_len)
        L = lib.load()
        dev = table.device
        out = suggest.sample_outputs(B * S, N, max_len, dev)
        if B * S > 0:
            hs, cs, w, tgt2src, t = self._decode_inputs(source_rep, source_len, B, S, table, src_dict, tgt_dict, tgt2src)
            ref = w.ref()
            cap = getattr(self, "fuse_sample_max_rows", None)
            if cap is not None and K == 0 and B * S * N > cap and w.struct.gen_frag:
                ref = lib.C.byref(w.without("rnn_gate_fold", "rnn_whh_frag", "gen_frag"))      # without the three packs: the entry's plain form
            nb = L.nir_sample_hredqs_decode_workspace_bytes(B, S, N, K, max_len, ref)
            if nb == 0:
                raise ValueError("HredQS.decode_sample: the shapes are outside the entry's range (nir_sample_hredqs_decode)")
            ws = lib.workspace(nb, dev)
            lib.check(L.nir_sample_hredqs_decode(lib.ptr(hs), lib.ptr(cs), B, S, lib.ptr(t), t.shape[0], t.shape[1], lib.ptr(tgt2src), BOS, max_len,
                                                 ref, N, K, 1.0 / tau, seed, lib.ptr(ws), ws.numel(), lib.ptr(out["predictions"]),
                                                 lib.ptr(out["token_logprobs"]), lib.ptr(out["scores"]), lib.ptr(out["lengths"]), lib.stream()),
                      "nir_sample_hredqs_decode")
        return suggest.sample_view(out, B, S)

    # ---- eval: teacher-forced scoring of given candidates ---------------------------------------------------------------------------------
    @torch.no_grad()
    def score_candidates(self, source_rep, source_len, candidate_seq, candidate_rep=None, src_dict=None, tgt_dict=None, tgt2src=None):
        """log P(candidate | session prefix) for N candidate next queries per prefix (include/neuroir_score.h).
        source_rep [B, S, QL], source_len [B, S]; candidate_seq [B, S, N, TL]: target-vocabulary ids, BOS first, PAD behind the end; candidate_rep
        [B, S, N, TL]: the embedder ids fed to the decoder (default: what decode() feeds -- the first token as it is, tgt2src[token] behind it, <unk> outside the source
        vocabulary) -> {'token_logprobs': [B, S, N, TL - 1], 'scores': [B, S, N], 'lengths': LongTensor [B, S, N]}.  The session states and
        their pairing are decode()'s (row b S + s starts from step (b S + s) // B of session (b S + s) % B); the teacher-forced decoder pass
        is forward()'s without dropout; ONE generator call over all rows that keeps the logits on chip (`fast_decode = False`: its plain form)."""
        dec_out, cand, w = self._candidate_rows(source_rep, source_len, candidate_seq, candidate_rep, src_dict, tgt_dict, tgt2src)
        return suggest.score_rows(self, dec_out, cand, w.keep["gen_w"], w.keep["gen_b"], w.keep.get("gen_frag"))

    def _candidate_rows(self, source_rep, source_len, candidate_seq, candidate_rep, src_dict, tgt_dict, tgt2src):
        """score_candidates in front of the generator -> (the decoder outputs of the teacher-forced steps [B, S, N, TL - 1, nhid_session],
        candidate_seq as int64, the packed decoder weights)"""
        if self.training:
            raise NotImplementedError("HIP HredQS.score_candidates runs in eval mode")
        self._check_config()
        B, S, _ = source_rep.shape
        cand = lib.ids64(candidate_seq)
        if cand.dim() != 4 or tuple(cand.shape[:2]) != (B, S) or cand.shape[3] < 2:
            raise ValueError("score_candidates: candidate_seq must be [B, S, N, TL] with TL >= 2 (got %s)" % (tuple(cand.shape),))
        table = self._source_rows(source_rep, source_len, cand, candidate_rep)[3]
        R, N, T = B * S, int(cand.shape[2]), int(cand.shape[3]) - 1
        hs, cs, w, tgt2src, _ = self._decode_inputs(source_rep, source_len, B, S, table, src_dict, tgt_dict, tgt2src)
        rep = suggest.candidate_inputs(self, cand, candidate_rep, src_dict, tgt_dict, tgt2src, int(w.struct.VT), table.shape[0])
        # the reference's pairing (see the module docstring), then every row's state once per candidate: rows (b, s, n)
        dec_h, dec_c = (s.transpose(0, 1).reshape(R, -1).repeat_interleave(N, 0).contiguous() for s in (hs, cs))
        h_all, _ = A.lstm_seq(A.embed(rep[..., :-1].reshape(R * N, T), table), self.decoder.decoder.rnn, dec_h, dec_c)
        return h_all.view(B, S, N, T, -1), cand, w

    # ---- train: teacher-forced loss ---------------------------------------------------------------------------------------------------
    def forward(self, source_rep, source_len, target_rep, target_len, target_seq, source_map=None, alignment=None):
        """hredqs.py:89-143 -> scalar loss over the R = B S rows: logits of steps [:-1] against target_seq[:, 1:], NLL masked at PAD, summed
        over time, averaged over rows.  Differentiable through the HIP operators of autograd.py; dropout is active in train mode only."""
        self._check_config()
        B, S, QL = source_rep.shape
        R = B * S
        table = self.embedder.word_embeddings.table
        lib.require_device(source_rep, source_len, target_rep, target_seq, table)
        tr = self.training
        src, tgt = self._clean_ids(source_rep.reshape(R, QL), target_rep.reshape(R, -1), table.shape[0])
        hs, cs = self._session_steps_train(src, lib.ids64(source_len.reshape(-1)), B, S)       # [B, S, HS]; gradient flows into both
        # the reference's pairing (see the module docstring): decode row r takes the state at step-major index r
        dec_h, dec_c = (s.transpose(0, 1).reshape(R, -1) for s in (hs, cs))
        temb = A.dropout(A.embed(tgt, table), self.embedder.dropout.p, tr)
        h_all, _ = A.lstm_seq(temb, self.decoder.decoder.rnn, dec_h, dec_c)                   # [R, TL, HS]
        h_all = A.dropout(h_all, self.dec_dropout_p, tr)[:, :-1]
        logits = A.linear(h_all, self.generator.weight, self.generator.bias)
        return A.suggestion_loss(logits, lib.ids64(target_seq.reshape(R, -1))[:, 1:], PAD, 0.0)
