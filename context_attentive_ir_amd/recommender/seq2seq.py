"""Seq2seq -- the attention encoder-decoder of the recommender driver (drop-in for neuroir.recommender.seq2seq.Seq2seq,
/root/reference/neuroir/recommender/seq2seq.py:13-195; ACG is the same network with a copy generator on top).

decode():  RNNEncoder over the source query -> the decoder's initial state (the encoder's final state of source row order[b], see below)
           -> ONE C-ABI call for the whole greedy decode (nir_seq2seq_decode_greedy, csrc/seq2seq.hip): LSTM step, Luong attention
           ('general' / 'dot' / 'mlp'), linear_out, generator + arg-max, the token fed back through a device lookup table.
forward(): the teacher-forced loss on the differentiable HIP operators of autograd.py.
score_candidates(): log P(candidate | source) of given next queries -- decode()'s encoder and initial state, the teacher-forced decoder pass,
           then ONE generator call over the rows of all time steps that keeps the logits on chip (nir_score_gen_target, csrc/score.hip).
decode_sample(): N i.i.d. draws per source row at a temperature, over the vocabulary or each step's top-k -- decode_beam()'s stages with the
           sampling tail behind the step: generator + Gumbel arg-max on counter-based noise in one kernel (nir_sample_seq2seq_decode,
           csrc/sample.hip).

Kept quirks of the reference:
  * RNNEncoder returns its final state in LENGTH-SORTED order (encoders/rnn_encoder.py:72-74,104-121; only the memory bank is un-sorted), so
    decoder row b starts from the final state of source row order[b], order = torch.sort(lengths, 0, True)[1].  The encoder of this package
    returns original order; the pairing is applied here with the same torch.sort call on the same device tensor.  (Equal lengths: the
    pairing is that call's choice.)
  * there is no input feed: the decoder LSTM reads the previous token's embedding and its own state, attention follows it.
  * tanh follows linear_out for 'general' and 'dot' only; 'mlp' has a bias there and no tanh (modules/global_attention.py:74-75,193-195).
  * nlayers != 1 (hyparam.SEQ2SEQ has 2) constructs, and fails in forward / decode like the reference: the encoder (use_last) hands over one
    layer's state, the decoder LSTM expects nlayers of them.
"""
import torch
import torch.nn as nn

from .. import autograd as A
from .. import lib
from ..constants import BOS, PAD
from ..multitask import suggest
from .layers import ATTN_TYPES, Decoder, Embedder, Encoder, encode_train


def check_supported(args, what, rnn_type="LSTM"):
    """the configurations both attention recommenders refuse (`rnn_type`: the cell the class is built for)"""
    if args.rnn_type != rnn_type:
        raise NotImplementedError("HIP %s implements rnn_type %r (got %r); the GRU decoders are recommender.Seq2seqGRU / recommender.ACGGRU "
                                  "(wrappers.Recommender / CopyRecommender pick them by args.rnn_type)" % (what, rnn_type, args.rnn_type))
    if args.attn_type not in ATTN_TYPES:
        raise NotImplementedError("HIP %s implements attn_type %s (got %r)" % (what, ", ".join(ATTN_TYPES), args.attn_type))


def build_network(net, args, own_copy_attn=False):
    """the modules and attributes Seq2seq and ACG share (seq2seq.py:14-39), in the reference's registration order"""
    net.embedder = Embedder(args.emsize, args.src_vocab_size, args.dropout_emb)
    net.encoder = Encoder(args.rnn_type, args.emsize, args.bidirection, args.nlayers, args.nhid, args.dropout_rnn)
    net.decoder = Decoder(args.emsize, args.nlayers, args.nhid, args.attn_type, args.dropout_rnn, own_copy_attn, args.rnn_type)
    net.dropout = nn.Dropout(args.dropout)
    net.generator = nn.Linear(args.nhid, args.tgt_vocab_size)
    net.attn_type, net.nlayers, net.nhid = args.attn_type, int(args.nlayers), int(args.nhid)
    net.bidirection = bool(args.bidirection)
    net.dec_dropout_p = float(args.dropout_rnn)         # RNNDecoder.dropout (decoders/decoder.py:87)
    net.fold_decoder_step = True             # decode: per-token gate rows folded into a [V, 4H] table + fp16-term recurrent product
    net.fuse_generator_argmax = True         # decode: generator + bias + arg-max in one kernel (no [B, VT] logits)
    net.fuse_generator_topk = True           # decode_beam: generator + bias + (lse, top-W) in one kernel (no [B W, VT] logits)
    net.fold_budget_bytes = 64 << 30
    net._pdec = lib.PackCache(retain=1)


class Seq2seq(nn.Module, lib.IdCheck):
    # ---- the decoder's cell, as data: everything else in this class, and in ACG, is written once over it (the GRU forms: seq2seq_gru.py) ----
    _CELL = "LSTM"                                       # args.rnn_type this class is built for (check_supported)
    _GATES = 4                                           # rows of W_ih / W_hh per hidden unit; the folded gate table is [V, _GATES H]
    _WHH_PACK = "nir_lstm_step"                          # + "_whh_frag_bytes" / "_pack_whh_frag": W_hh as fp16 term fragments
    _LAYER_CHECK = "Expected hidden[0] size (%d, %d, %d), got [1, %d, %d]"        # torch.nn.LSTM's text for a state of the wrong depth
    _ENTRY_CELL = ""                                     # the cell's part of a C entry's name
    _GREEDY_ENTRY = "nir_seq2seq%s_decode"               # + "_greedy" / "_workspace_bytes": nir_seq2seq_decode_greedy, nir_seq2seq_gru_decode_greedy
    _BEAM_ENTRY = "nir_beam_seq2seq%s_decode"            # (+ "_workspace_bytes"): nir_beam_seq2seq_decode, nir_beam_seq2seq_gru_decode
    _SAMPLE_ENTRY = "nir_sample_seq2seq%s_decode"        # (+ "_workspace_bytes"): nir_sample_seq2seq_decode, nir_sample_seq2seq_gru_decode

    @staticmethod
    def _fold_table(table, wih, bih, bhh, H):
        """the per-token gate rows of the folded step, [V, _GATES H]"""
        return lib.fold_lstm_table(table, wih, bih, bhh, H, 1, "f32")

    def _encode_train(self, x, lens):
        """x [B,T,E] -> (memory bank [B,T,nhid], the final state tensors, each [B,nhid]) in ORIGINAL row order, differentiable: the register-resident
        training recurrence up to 128 units per direction (it returns the cell states), one lstm_seq pass per direction beyond."""
        mem, h_n, c_n = encode_train(self.encoder.encoder.rnns[0], x, lens)
        return mem, (h_n, c_n)

    def _cell_train(self, temb, state):
        """the teacher-forced pass of the decoder's cell from `state` (already in the decoder's row order) -> every step's h [B,TL,nhid]"""
        return A.lstm_seq(temb, self.decoder.decoder.rnn, *state)[0]

    def __init__(self, args):
        super().__init__()
        name = type(self).__name__
        if getattr(args, "copy_attn", False):
            raise NotImplementedError("HIP %s has no copy generator (copy_attn=True is ACG: build recommender.%s, or wrappers.CopyRecommender "
                                      "for the reference's batch layout)" % (name, name.replace("Seq2seq", "ACG")))
        check_supported(args, name, self._CELL)
        build_network(self, args)
        self.copy_attn = False

    # ---- shared checks -----------------------------------------------------------------------------------------------------------
    def _check_layers(self, B):
        if self.nlayers != 1:
            raise RuntimeError(self._LAYER_CHECK % (self.nlayers, B, self.nhid, B, self.nhid))

    def _decode_ready(self, what, source_rep, source_len):
        """what every decode checks before any launch (the layer check like the reference's failure) -> (B, QL, the embedding table)"""
        if self.training:
            raise NotImplementedError("HIP %s.%s runs in eval mode" % (type(self).__name__, what))
        B, QL = source_rep.shape
        self._check_layers(B)
        table = self.embedder.word_embeddings.table
        lib.require_device(source_rep, source_len, table)
        return B, QL, table

    def _decoder_weights(self):
        rnn, att = self.decoder.decoder.rnn, self.decoder.decoder.attn
        table = self.embedder.word_embeddings.table

        def build():
            L = lib.load()
            t = dict(rnn_wih=rnn.weight_ih_l0, rnn_whh=rnn.weight_hh_l0, rnn_bih=rnn.bias_ih_l0, rnn_bhh=rnn.bias_hh_l0,
                     attn_out_w=att.linear_out.weight, gen_w=self.generator.weight, gen_b=self.generator.bias)
            if self.attn_type == "general":
                t["attn_in_wt"] = att.linear_in.weight.t()
            elif self.attn_type == "mlp":
                t.update(attn_ctx_w=att.linear_context.weight, attn_query_w=att.linear_query.weight, attn_query_b=att.linear_query.bias,
                         attn_v=att.v.weight, attn_out_b=att.linear_out.bias)
            H, VT = int(rnn.hidden_size), int(self.generator.weight.shape[0])
            pk = lib.Packed(lib.Seq2seqDecoderWeights, t, dict(H=H, attn_type=lib.S2S_ATTN[self.attn_type], VT=VT))
            dev = pk.keep["gen_w"].device
            if dev.type != "cuda":
                return pk
            # both packs behind ONE blocking flag read per weight version; a weight outside the fp16 range of the split leaves its plain form
            flag = torch.zeros(2, dtype=torch.int32, device=dev)
            gfrag = wfrag = None
            nbg, nbw = L.nir_seq2seq_gen_frag_bytes(VT, H), getattr(L, self._WHH_PACK + "_whh_frag_bytes")(H)
            if self.fuse_generator_argmax and nbg:
                gfrag = torch.empty(nbg, dtype=torch.uint8, device=dev)
                lib.check(L.nir_seq2seq_pack_gen_frag(lib.ptr(pk.keep["gen_w"]), VT, H, lib.ptr(gfrag), lib.ptr(flag), lib.stream()),
                          "nir_seq2seq_pack_gen_frag")
            if (self.fold_decoder_step and nbw and table.is_cuda and table.shape[1] == rnn.input_size
                    and table.shape[0] * self._GATES * H * 4 <= self.fold_budget_bytes):
                wfrag = torch.empty(nbw, dtype=torch.uint8, device=dev)
                lib.check(getattr(L, self._WHH_PACK + "_pack_whh_frag")(lib.ptr(pk.keep["rnn_whh"]), H, lib.ptr(wfrag), lib.ptr(flag[1:]), lib.stream()),
                          self._WHH_PACK + "_pack_whh_frag")
            bad = flag.tolist() if (gfrag is not None or wfrag is not None) else [0, 0]
            if gfrag is not None and bad[0] == 0:
                pk.keep["gen_frag"] = gfrag
                pk.struct.gen_frag = gfrag.data_ptr()
            if wfrag is not None and bad[1] == 0:
                pk.keep["rnn_whh_frag"] = wfrag
                pk.keep["rnn_gate_fold"] = self._fold_table(table, pk.keep["rnn_wih"], pk.keep["rnn_bih"], pk.keep["rnn_bhh"], H)
                pk.struct.rnn_whh_frag = wfrag.data_ptr()
                pk.struct.rnn_gate_fold = pk.keep["rnn_gate_fold"].data_ptr()
            return pk
        params = list(self.decoder.parameters()) + list(self.generator.parameters())
        return self._pdec.get(params + [table, self.fold_decoder_step, self.fuse_generator_argmax, self.fold_budget_bytes], build)

    # ---- eval: greedy decode -----------------------------------------------------------------------------------------------------
    def initial_state(self, final, source_len):
        """decoders/decoder.py:160-177 on the encoder's final (h_n, c_n) [ND, B, nhid / ND] (ORIGINAL row order) -> (h, c) [B, nhid]: row b is
        the state of source row order[b] (the reference's length-sorted order), forward and reverse halves along the feature axis."""
        order = torch.sort(source_len, 0, True)[1]
        return tuple(torch.cat([s[d][order] for d in range(s.shape[0])], 1).contiguous() for s in final)

    def _encode_state(self, src, lens):
        """eval: embedding -> encoder -> (the decoder's initial state tensors, each [B, nhid], paired as in initial_state; the bank [B, QL, nhid])"""
        final, bank = self.encoder.encoder(A.embed(src, self.embedder.word_embeddings.table), lens)
        state = self.initial_state(final, lens)
        return (state if isinstance(state, tuple) else (state,)), bank.float().contiguous()

    def _encoded(self, source_rep, source_len, table, repeat=None):
        """the checked source ids through _encode_state -> (lengths as int64, the initial state tensors, the bank); repeat = n: every state tensor
        n times along the rows, row k B + b -- the reference's beam layout (decoders/state.py:65-69), which the sampling entries share"""
        src, _ = self._clean_ids(source_rep, None, table.shape[0])
        lens = lib.ids64(source_len)
        state, bank = self._encode_state(src, lens)
        if repeat is not None:
            state = [s.repeat(repeat, 1).contiguous() for s in state]
        return lens, state, bank

    @staticmethod
    def _generator_form(w, fuse):
        """what an entry takes as the decoder weights: the pack, or -- `fuse` off -- the same pack without the generator fragment, which selects the
        plain generator form (the reference returned keeps the copy alive)"""
        return w.ref() if fuse or not w.struct.gen_frag else lib.C.byref(w.without("gen_frag"))

    def _greedy(self, source_rep, source_len, max_len, src_dict, tgt_dict, tgt2src, extra=None):
        """the greedy decode of Seq2seq and ACG, either cell: encoder, the sorted-order pairing, ONE C call.  extra(B, QL) -> (what the size entry
        takes behind QL, the C arguments the entry takes behind the decoder weights): ACG's copy inputs, checked once the shapes are known."""
        B, QL, table = self._decode_ready("decode", source_rep, source_len)
        ws_extra, tail = ((), ()) if extra is None else extra(B, QL)
        L = lib.load()
        lens, state, bank = self._encoded(source_rep, source_len, table)
        dev = bank.device
        w = self._decoder_weights()
        if tgt2src is None:
            tgt2src = suggest.tgt2src_lut(self, src_dict, tgt_dict, int(w.struct.VT), dev)
        t = table.detach().float().contiguous()
        max_len = int(max_len)
        preds = torch.empty(B, max_len, dtype=torch.int64, device=dev)
        attns = torch.empty(B, max_len, QL, dtype=torch.float32, device=dev)
        if B > 0 and max_len > 0:
            entry = self._GREEDY_ENTRY % self._ENTRY_CELL
            nb = getattr(L, entry + "_workspace_bytes")(B, QL, *ws_extra, w.ref(), *tail[:1])
            if nb == 0 and tail:
                raise ValueError("%s.decode: the shapes are outside the entry's range (%s_greedy)" % (type(self).__name__, entry))
            ws = lib.workspace(nb, dev)
            args = [lib.ptr(s) for s in state] + [lib.ptr(bank), lib.ptr(lens), B, QL, lib.ptr(t), t.shape[0], t.shape[1], lib.ptr(tgt2src), BOS, max_len,
                                                  w.ref(), *tail, lib.ptr(ws), ws.numel(), lib.ptr(preds), lib.ptr(attns), lib.stream()]
            lib.check(getattr(L, entry + "_greedy")(*args), entry + "_greedy")
        return {"predictions": preds, "attentions": attns}

    @torch.no_grad()
    def decode(self, source_rep, source_len, max_len, src_dict, tgt_dict, src_map=None, alignment=None, blank=None, fill=None,
               source_vocabs=None, tgt2src=None):
        """seq2seq.py:118-195 (greedy) -> {'predictions': LongTensor [B, max_len] (target-vocabulary ids), 'attentions': [B, max_len, QL]}.
        The reference maps each predicted token back to a source id on the host (tgt_dict[idx] -> word -> src_dict[word]); here that is one
        device lookup table (identity without dictionaries).  attentions has the padded width QL of `source_rep` (the reference's has
        max(source_len)); masked positions are exactly 0."""
        return self._greedy(source_rep, source_len, max_len, src_dict, tgt_dict, tgt2src)

    # ---- eval: beam search ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode_beam(self, source_rep, source_len, max_len, beam_size, src_dict=None, tgt_dict=None, tgt2src=None, return_backptr=False):
        """Beam search of width `beam_size` (1 .. lib.BEAM_MAX_W) over max_len steps, no early stop (include/neuroir_beam.h)
        -> {'predictions': LongTensor [B, W, max_len] (best beam first, EOS repeated behind the first EOS), 'scores': [B, W] (sum of the
        tokens' log-probabilities, frozen at EOS), 'lengths': LongTensor [B, W], 'attentions': [B, W, max_len, QL]} (+ 'backptr': IntTensor
        [max_len, B, W] on request).  The stages of decode(): encoder, the sorted-order pairing, the state repeated W times in the reference's
        beam layout (row k B + b: decoders/state.py:65-69), ONE C call.  The memory bank is not repeated."""
        if self.training:
            raise NotImplementedError("HIP %s.decode_beam runs in eval mode" % type(self).__name__)
        return self._beam(source_rep, source_len, max_len, beam_size, src_dict, tgt_dict, tgt2src, return_backptr)

    def _beam(self, source_rep, source_len, max_len, beam_size, src_dict, tgt_dict, tgt2src, return_backptr, entry=None, extra=None):
        """the beam search of Seq2seq and ACG, either cell.  entry: the C entry (default: _BEAM_ENTRY, which takes W behind QL); extra(B, QL) ->
        (what the size entry takes between QL and W, the C arguments the entry takes behind the decoder weights, W following them): ACG's copy
        inputs, checked once the shapes are known."""
        W = int(beam_size)
        B, QL, table = self._decode_ready("decode_beam", source_rep, source_len)
        L = lib.load()
        w = self._decoder_weights()
        VT = int(w.struct.VT)
        suggest.check_beam_size(W, VT)
        ws_extra, tail = (None, None) if extra is None else extra(B, QL)
        lens, state, bank = self._encoded(source_rep, source_len, table, repeat=W)
        dev = bank.device
        ws_ref = self._generator_form(w, self.fuse_generator_topk)
        if tgt2src is None:
            tgt2src = suggest.tgt2src_lut(self, src_dict, tgt_dict, VT, dev)
        t = table.detach().float().contiguous()
        max_len = int(max_len)
        out = suggest.beam_outputs(B, W, max_len, dev, return_backptr, QL)
        if B > 0 and max_len > 0:
            entry = (self._BEAM_ENTRY if entry is None else entry) % self._ENTRY_CELL
            outs = [lib.ptr(out["predictions"]), lib.ptr(out["scores"]), lib.ptr(out["lengths"]), lib.ptr(out["attentions"]), lib.ptr(out.get("backptr")),
                    lib.stream()]
            front = [lib.ptr(s) for s in state] + [lib.ptr(bank), lib.ptr(lens), B, QL]
            mid = [lib.ptr(t), t.shape[0], t.shape[1], lib.ptr(tgt2src), BOS, max_len, ws_ref]
            if tail is None:
                ws = lib.workspace(getattr(L, entry + "_workspace_bytes")(B, QL, W, max_len, ws_ref), dev)
                args = front + [W] + mid + [lib.ptr(ws), ws.numel()] + outs
            else:
                nb = getattr(L, entry + "_workspace_bytes")(B, QL, *ws_extra, W, max_len, ws_ref, tail[0])
                if nb == 0:
                    raise ValueError("%s.decode_beam: the shapes are outside the entry's range (%s)" % (type(self).__name__, entry))
                ws = lib.workspace(nb, dev)
                args = front + mid + list(tail) + [W, lib.ptr(ws), ws.numel()] + outs
            lib.check(getattr(L, entry)(*args), entry)
        return out

    # ---- eval: sampling ------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode_sample(self, source_rep, source_len, max_len, num_samples, temperature=1.0, top_k=0, seed=0, src_dict=None, tgt_dict=None,
                      tgt2src=None):
        """`num_samples` i.i.d. draws per source row from the model's next-token distributions at `temperature`, over the whole target
        vocabulary (top_k = 0) or restricted to each step's top_k most likely tokens (1 .. lib.BEAM_MAX_W; top_k = 1 is the greedy decode),
        over max_len steps with no early stop (include/neuroir_sample.h; the reference has no counterpart)
        -> {'predictions': LongTensor [B, N, max_len] (in sample order, EOS repeated behind the first EOS), 'token_logprobs': [B, N, max_len]
        (the model's own log-probability of every token at temperature 1 over the full vocabulary, 0 behind EOS), 'scores': [B, N] (their
        sum: what score_candidates([BOS] + sample) returns for a sample without PAD in front of its first EOS -- a whole-vocabulary draw can
        emit PAD like any id, and score_candidates does not count that position), 'lengths': LongTensor [B, N], 'attentions': [B, N, max_len, QL]}.
        The noise is a counter-based function of (seed, step, source row, sample, token): the same seed gives the same bits, and a source
        row's samples do not depend on the rows decoded next to it.  The stages of decode_beam(): encoder, the sorted-order pairing, the state
        repeated N times (row n B + b), ONE C call; the logits never leave the chip (`fuse_generator_argmax = False`, and for top_k > 0
        `fuse_generator_topk = False`: the plain generator form; over the whole vocabulary it is also the default beyond
        `fuse_sample_max_rows` = suggest.FUSE_SAMPLE_MAX_ROWS decode rows, where it was measured no slower)."""
        return self._sample("decode_sample", source_rep, source_len, max_len, num_samples, temperature, top_k, seed, src_dict, tgt_dict, tgt2src)

    def _sample(self, what, source_rep, source_len, max_len, num_samples, temperature, top_k, seed, src_dict, tgt_dict, tgt2src, entry=None, extra=None):
        """the sampling decode of Seq2seq and ACG, either cell, `what` the method's name in the messages.  entry: the C entry (default:
        _SAMPLE_ENTRY, which takes the draw's arguments behind QL); extra(B, QL) as in _beam, the draw's arguments following the copy inputs."""
        VT = int(self.generator.weight.shape[0])
        N, K, tau, seed = suggest.check_sample_args(self, num_samples, temperature, top_k, seed, VT)      # (its messages say decode_sample: the shared rules)
        B, QL, table = self._decode_ready(what, source_rep, source_len)
        ws_extra, tail = (None, None) if extra is None else extra(B, QL)
        L = lib.load()
        w = self._decoder_weights()
        lens, state, bank = self._encoded(source_rep, source_len, table, repeat=N)
        dev = bank.device
        fuse = self.fuse_generator_topk if K > 0 else (self.fuse_generator_argmax
                                                       and B * N <= getattr(self, "fuse_sample_max_rows", suggest.FUSE_SAMPLE_MAX_ROWS))
        ws_ref = self._generator_form(w, fuse)
        if tgt2src is None:
            tgt2src = suggest.tgt2src_lut(self, src_dict, tgt_dict, VT, dev)
        t = table.detach().float().contiguous()
        max_len = int(max_len)
        out = suggest.sample_outputs(B, N, max_len, dev, QL)
        if B > 0 and max_len > 0:
            entry = (self._SAMPLE_ENTRY if entry is None else entry) % self._ENTRY_CELL
            front = [lib.ptr(s) for s in state] + [lib.ptr(bank), lib.ptr(lens), B, QL]
            mid = [lib.ptr(t), t.shape[0], t.shape[1], lib.ptr(tgt2src), BOS, max_len, ws_ref]
            draw = [N, K, 1.0 / tau, seed]
            if tail is None:
                nb = getattr(L, entry + "_workspace_bytes")(B, QL, N, K, max_len, ws_ref)
                args = front + draw + mid
            else:
                nb = getattr(L, entry + "_workspace_bytes")(B, QL, *ws_extra, N, K, max_len, ws_ref, tail[0])
                args = front + mid + list(tail) + draw
            if nb == 0:
                raise ValueError("%s.%s: the shapes are outside the entry's range (%s)" % (type(self).__name__, what, entry))
            ws = lib.workspace(nb, dev)
            args += [lib.ptr(ws), ws.numel()] + [lib.ptr(out[k]) for k in ("predictions", "token_logprobs", "scores", "lengths", "attentions")]
            lib.check(getattr(L, entry)(*args, lib.stream()), entry)
        return out

    # ---- eval: teacher-forced scoring of given candidates ---------------------------------------------------------------------------------
    @torch.no_grad()
    def score_candidates(self, source_rep, source_len, candidate_seq, candidate_rep=None, src_dict=None, tgt_dict=None, tgt2src=None):
        """log P(candidate | source) for N candidate next queries per source (include/neuroir_score.h; the reference has no
        counterpart beyond its training loss).  candidate_seq [B, N, TL]: target-vocabulary ids, BOS first, PAD behind the end; candidate_rep
        [B, N, TL]: the embedder ids fed to the decoder (default: what decode() and decode_beam() feed -- the first token as it is, tgt2src[token]
        behind it, <unk> outside the source vocabulary) -> {'token_logprobs': [B, N, TL - 1] (step t against token t + 1; 0 at PAD, behind the first EOS and for an
        id outside the vocabulary), 'scores': [B, N] (their sum), 'lengths': LongTensor [B, N] (their number)}.
        The encoder and the initial state are decode()'s; the teacher-forced decoder pass is forward()'s without dropout, the N (TL - 1) rows of
        a source taken as its steps so that the memory bank is not repeated; then ONE generator call over all B N (TL - 1) rows that keeps the
        logits on chip (`fuse_generator_argmax = False`: its plain form) and one pass over the sequences."""
        dec_out, cand, w = self._candidate_rows(source_rep, source_len, candidate_seq, candidate_rep, src_dict, tgt_dict, tgt2src)
        return suggest.score_rows(self, dec_out, cand, w.keep["gen_w"], w.keep["gen_b"], w.keep.get("gen_frag"))

    def _candidate_rows(self, source_rep, source_len, candidate_seq, candidate_rep, src_dict, tgt_dict, tgt2src):
        """score_candidates in front of the generator -> (the decoder outputs of the teacher-forced steps [B, N, TL - 1, nhid], candidate_seq as
        int64, the packed decoder weights)"""
        cand = lib.ids64(candidate_seq)
        if cand.dim() != 3 or cand.shape[0] != source_rep.shape[0] or cand.shape[2] < 2:
            raise ValueError("score_candidates: candidate_seq must be [B, N, TL] with TL >= 2 (got %s)" % (tuple(cand.shape),))
        B, QL, table = self._decode_ready("score_candidates", source_rep, source_len)
        lib.require_device(cand, candidate_rep)
        N, T = int(cand.shape[1]), int(cand.shape[2]) - 1
        lens, state, bank = self._encoded(source_rep, source_len, table)
        w = self._decoder_weights()
        rep = suggest.candidate_inputs(self, cand, candidate_rep, src_dict, tgt_dict, tgt2src, int(w.struct.VT), table.shape[0])
        temb = A.embed(rep[:, :, :-1].reshape(B * N, T), table)
        h_all = self._cell_train(temb, [s.repeat_interleave(N, 0).contiguous() for s in state]).reshape(B, N * T, -1)      # rows (b, n, t)
        att = self.decoder.decoder.attn
        mask = torch.arange(QL, device=bank.device).unsqueeze(0) < lens.unsqueeze(1)
        ctx = A.softmax_pool(self._align(h_all, bank), mask, bank, mask_div=N * T).view(B, N * T, -1)
        mlp = self.attn_type == "mlp"
        dec_out = A.linear(torch.cat((ctx, h_all), 2), att.linear_out.weight, att.linear_out.bias if mlp else None, act=None if mlp else "tanh")
        return dec_out.view(B, N, T, -1), cand, w

    # ---- train: teacher-forced loss ---------------------------------------------------------------------------------------------------
    def _align(self, h_all, mem, att=None):
        """global_attention.py:81-119 -> [B, TL, QL] (tiny: tensor glue around the library's linears, as in multitask/cars.py)"""
        att = self.decoder.decoder.attn if att is None else att
        if self.attn_type == "mlp":
            wq = A.linear(h_all, att.linear_query.weight, att.linear_query.bias)
            uh = A.linear(mem, att.linear_context.weight)
            return A.linear(torch.tanh(wq.unsqueeze(2) + uh.unsqueeze(1)), att.v.weight).squeeze(-1)
        q = A.linear(h_all, att.linear_in.weight) if self.attn_type == "general" else h_all
        return (q.unsqueeze(2) * mem.unsqueeze(1)).sum(3)

    def forward(self, source_rep, source_len, target_rep, target_len, target_seq, source_map=None, alignment=None):
        """seq2seq.py:48-103 -> scalar loss: logits of steps [:-1] against target_seq[:, 1:], NLL masked at PAD, summed over time, averaged
        over rows.  Differentiable through the HIP operators of autograd.py; dropout is active in train mode only."""
        dec_out = self._decoder_outputs(source_rep, source_len, target_rep, target_seq)[0][:, :-1]
        logits = A.linear(dec_out, self.generator.weight, self.generator.bias)
        return A.suggestion_loss(logits, lib.ids64(target_seq)[:, 1:], PAD, 0.0)

    def _decoder_outputs(self, source_rep, source_len, target_rep, target_seq):
        """seq2seq.py:67-81, teacher-forced -> (attentional outputs of every step [B,TL,nhid] behind the decoder's dropout, the attention's
        alignment scores [B,TL,QL], the memory bank [B,QL,nhid], the length mask [B,QL])"""
        B, QL = source_rep.shape
        self._check_layers(B)
        table = self.embedder.word_embeddings.table
        lib.require_device(source_rep, source_len, target_rep, target_seq, table)
        tr = self.training
        src, tgt = self._clean_ids(source_rep, target_rep, table.shape[0])
        lens = lib.ids64(source_len)
        pe = self.embedder.dropout.p
        mem, final = self._encode_train(A.dropout(A.embed(src, table), pe, tr), lens)
        mem = A.dropout(mem, self.dropout.p, tr)
        order = torch.sort(lens, 0, True)[1]                                 # the reference's length-sorted final state (see the module docstring)
        temb = A.dropout(A.embed(tgt, table), pe, tr)
        att = self.decoder.decoder.attn
        h_all = self._cell_train(temb, [s[order].contiguous() for s in final])          # [B,TL,nhid]
        TL = h_all.shape[1]
        align = self._align(h_all, mem)
        mask = torch.arange(QL, device=mem.device).unsqueeze(0) < lens.unsqueeze(1)          # [B,QL]: the TL rows of a source share it
        ctx = A.softmax_pool(align, mask, mem, mask_div=TL).view(B, TL, -1)
        mlp = self.attn_type == "mlp"
        dec_out = A.linear(torch.cat((ctx, h_all), 2), att.linear_out.weight, att.linear_out.bias if mlp else None, act=None if mlp else "tanh")
        return A.dropout(dec_out, self.dec_dropout_p, tr), align, mem, mask
