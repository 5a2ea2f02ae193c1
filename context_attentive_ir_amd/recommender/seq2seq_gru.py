"""Seq2seqGRU / ACGGRU -- the two attention recommenders with rnn_type 'GRU' (the reference's config.py:53; the decoder's GRU branch is
neuroir/decoders/decoder.py:175-177 and decoders/rnn_decoder.py:46-47).

Thin subclasses of Seq2seq / ACG: the attention, linear_out, the generator, the arg-max, the copy generator and both losses are the parents'.
What changes is the cell:

  * the encoder's final state is ONE tensor h_n; the decoder starts from its halves side by side, [B, nhid], in the reference's length-sorted
    row order (seq2seq.py's module docstring), and carries no cell state;
  * decode(): nir_seq2seq_gru_decode_greedy / nir_acg_gru_decode_greedy (csrc/gru_step.hip: torch.nn.GRU's step, b_hn inside the reset
    product).  With `fold_decoder_step` the input side is a per-token table [V, 3H] = table W_ih^T + b_ih + (b_hr, b_hz, 0) and the
    recurrent product runs on fp16 term pairs, one launch per step; otherwise, or when a weight is outside the split's range, the exact fp32
    step;
  * forward(): the GRU encoder through autograd.bigru, its final state read from the memory bank, the decoder through autograd.gru_seq with
    the initial state as a differentiable input.

State-dict keys are the reference's: `decoder.decoder.rnn.*_l0` and `encoder.encoder.rnns.0.*` are [3H, .].
nlayers != 1 constructs and fails in forward / decode with torch.nn.GRU's own text (it says `hidden`, not `hidden[0]`).
"""
import torch
import torch.nn as nn

from .. import autograd as A
from .. import lib
from .acg import ACG
from .layers import CopyGeneratorParams, encode_train_gru
from .seq2seq import Seq2seq, build_network, check_supported


class _GRUDecoderMixin(object):
    """the GRU forms of what Seq2seq keeps in one place each: the layer check, the packed decoder weights, the initial state, the teacher-forced
    decoder pass"""

    def _check_layers(self, B):
        if self.nlayers != 1:
            raise RuntimeError("Expected hidden size (%d, %d, %d), got [1, %d, %d]" % (self.nlayers, B, self.nhid, B, self.nhid))

    def initial_state(self, final, source_len):
        """decoders/decoder.py:160-177 on the GRU encoder's final h_n [ND, B, nhid / ND] (ORIGINAL row order) -> h [B, nhid]: row b is the state
        of source row order[b], forward and reverse halves along the feature axis"""
        order = torch.sort(source_len, 0, True)[1]
        return torch.cat([final[d][order] for d in range(final.shape[0])], 1).contiguous()

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
            # both packs behind ONE blocking flag read per weight version
            flag = torch.zeros(2, dtype=torch.int32, device=dev)
            gfrag = wfrag = None
            nbg, nbw = L.nir_seq2seq_gen_frag_bytes(VT, H), L.nir_gru_step_whh_frag_bytes(H)
            if self.fuse_generator_argmax and nbg:
                gfrag = torch.empty(nbg, dtype=torch.uint8, device=dev)
                lib.check(L.nir_seq2seq_pack_gen_frag(lib.ptr(pk.keep["gen_w"]), VT, H, lib.ptr(gfrag), lib.ptr(flag), lib.stream()),
                          "nir_seq2seq_pack_gen_frag")
            if (self.fold_decoder_step and nbw and table.is_cuda and table.shape[1] == rnn.input_size
                    and table.shape[0] * 3 * H * 4 <= self.fold_budget_bytes):
                wfrag = torch.empty(nbw, dtype=torch.uint8, device=dev)
                lib.check(L.nir_gru_step_pack_whh_frag(lib.ptr(pk.keep["rnn_whh"]), H, lib.ptr(wfrag), lib.ptr(flag[1:]), lib.stream()),
                          "nir_gru_step_pack_whh_frag")
            bad = flag.tolist() if (gfrag is not None or wfrag is not None) else [0, 0]
            if gfrag is not None and bad[0] == 0:
                pk.keep["gen_frag"] = gfrag
                pk.struct.gen_frag = gfrag.data_ptr()
            if wfrag is not None and bad[1] == 0:
                # gate_fold [V, 3H] = table W_ih^T + (b_ih + (b_hr, b_hz, 0)): b_hn stays outside, it belongs inside the reset product
                tb = table.detach().float().contiguous()
                bias = pk.keep["rnn_bih"].clone()
                bias[:2 * H] += pk.keep["rnn_bhh"][:2 * H]
                fold = torch.empty(tb.shape[0], 3 * H, device=dev, dtype=torch.float32)
                lib.check(L.nir_linear_f32(lib.ptr(tb), tb.shape[1], None, None, 0, 0, 0, lib.ptr(pk.keep["rnn_wih"]), tb.shape[1], lib.ptr(bias), None,
                                           lib.ptr(fold), 3 * H, tb.shape[0], 3 * H, tb.shape[1], 0, lib.stream()), "nir_linear_f32")
                pk.keep["rnn_whh_frag"], pk.keep["rnn_gate_fold"], pk.keep["rnn_fold_bias"] = wfrag, fold, bias
                pk.struct.rnn_whh_frag = wfrag.data_ptr()
                pk.struct.rnn_gate_fold = fold.data_ptr()
            return pk
        params = list(self.decoder.parameters()) + list(self.generator.parameters())
        return self._pdec.get(params + [table, self.fold_decoder_step, self.fuse_generator_argmax, self.fold_budget_bytes], build)

    _BEAM_ENTRY = "nir_beam_seq2seq_gru_decode"

    def _beam_state(self, src, lens):
        return self._encode_state(src, lens)

    def _encode_state(self, src, lens):
        """eval: embedding -> GRU encoder -> (initial decoder state [B, nhid], memory bank [B, QL, nhid])"""
        table = self.embedder.word_embeddings.table
        final, bank = self.encoder.encoder(A.embed(src, table), lens)
        return self.initial_state(final, lens), bank.float().contiguous()

    def _decoder_outputs(self, source_rep, source_len, target_rep, target_seq):
        """Seq2seq._decoder_outputs with the GRU cell: (attentional outputs [B,TL,nhid] behind the decoder's dropout, alignment scores
        [B,TL,QL], the memory bank [B,QL,nhid], the length mask [B,QL])"""
        B, QL = source_rep.shape
        self._check_layers(B)
        table = self.embedder.word_embeddings.table
        lib.require_device(source_rep, source_len, target_rep, target_seq, table)
        tr = self.training
        src, tgt = self._clean_ids(source_rep, target_rep, table.shape[0])
        lens = lib.ids64(source_len)
        pe = self.embedder.dropout.p
        mem, h_n = encode_train_gru(self.encoder.encoder.rnns[0], A.dropout(A.embed(src, table), pe, tr), lens)
        mem = A.dropout(mem, self.dropout.p, tr)
        order = torch.sort(lens, 0, True)[1]
        temb = A.dropout(A.embed(tgt, table), pe, tr)
        rnn, att = self.decoder.decoder.rnn, self.decoder.decoder.attn
        h_all = A.gru_seq(temb, rnn, h_n[order].contiguous())              # [B,TL,nhid]
        TL = h_all.shape[1]
        align = self._align(h_all, mem)
        mask = torch.arange(QL, device=mem.device).unsqueeze(0) < lens.unsqueeze(1)
        ctx = A.softmax_pool(align, mask, mem, mask_div=TL).view(B, TL, -1)
        mlp = self.attn_type == "mlp"
        dec_out = A.linear(torch.cat((ctx, h_all), 2), att.linear_out.weight, att.linear_out.bias if mlp else None, act=None if mlp else "tanh")
        return A.dropout(dec_out, self.dec_dropout_p, tr), align, mem, mask


def _gru_defaults(net):
    # the default follows the rule of section 15 (the one-launch step has to beat the plain form at the driver's shape)
    net.fold_decoder_step = True


class Seq2seqGRU(_GRUDecoderMixin, Seq2seq):
    def __init__(self, args):
        nn.Module.__init__(self)
        if getattr(args, "copy_attn", False):
            raise NotImplementedError("HIP Seq2seqGRU has no copy generator (copy_attn=True is ACG: build recommender.ACGGRU, or "
                                      "wrappers.CopyRecommender for the reference's batch layout)")
        check_supported(args, "Seq2seqGRU", "GRU")
        build_network(self, args)
        _gru_defaults(self)
        self.copy_attn = False

    @torch.no_grad()
    def decode(self, source_rep, source_len, max_len, src_dict, tgt_dict, src_map=None, alignment=None, blank=None, fill=None,
               source_vocabs=None, tgt2src=None):
        """Seq2seq.decode with the GRU step: the same three stages (encoder, initial state, ONE C call for the greedy decode)"""
        from ..constants import BOS
        from ..multitask import suggest
        if self.training:
            raise NotImplementedError("HIP Seq2seqGRU.decode runs in eval mode")
        B, QL = source_rep.shape
        self._check_layers(B)                                                # (before any launch, like the reference's failure)
        table = self.embedder.word_embeddings.table
        lib.require_device(source_rep, source_len, table)
        L = lib.load()
        src, _ = self._clean_ids(source_rep, None, table.shape[0])
        lens = lib.ids64(source_len)
        dec_h, bank = self._encode_state(src, lens)
        dev = bank.device
        w = self._decoder_weights()
        if tgt2src is None:
            tgt2src = suggest.tgt2src_lut(self, src_dict, tgt_dict, int(w.struct.VT), dev)
        t = table.detach().float().contiguous()
        max_len = int(max_len)
        preds = torch.empty(B, max_len, dtype=torch.int64, device=dev)
        attns = torch.empty(B, max_len, QL, dtype=torch.float32, device=dev)
        if B > 0 and max_len > 0:
            ws = lib.workspace(L.nir_seq2seq_gru_decode_workspace_bytes(B, QL, w.ref()), dev)
            lib.check(L.nir_seq2seq_gru_decode_greedy(lib.ptr(dec_h), lib.ptr(bank), lib.ptr(lens), B, QL, lib.ptr(t), t.shape[0], t.shape[1],
                                                      lib.ptr(tgt2src), BOS, max_len, w.ref(), lib.ptr(ws), ws.numel(), lib.ptr(preds), lib.ptr(attns),
                                                      lib.stream()), "nir_seq2seq_gru_decode_greedy")
        return {"predictions": preds, "attentions": attns}


class ACGGRU(_GRUDecoderMixin, ACG):
    def __init__(self, args):
        nn.Module.__init__(self)
        if not getattr(args, "copy_attn", False):
            raise ValueError("recommender.ACGGRU is the copy-generator model (copy_attn=True); without it build recommender.Seq2seqGRU")
        self.reuse_copy_attn = bool(getattr(args, "reuse_copy_attn", False))
        if args.attn_type in (None, "none"):                              # the reference's own failures, as in ACG
            if self.reuse_copy_attn:
                raise RuntimeError("Attn is turned off, so reuse_copy_attn flag must be false")
            raise AssertionError("Please select a valid attention type.")
        check_supported(args, "ACGGRU", "GRU")
        build_network(self, args, own_copy_attn=not self.reuse_copy_attn)
        _gru_defaults(self)
        self.copy_attn = True
        self.force_copy = bool(getattr(args, "force_copy", False))
        self.copy_generator = CopyGeneratorParams(args.nhid, self.generator)
        self._pcopy = lib.PackCache(retain=1)

    @torch.no_grad()
    def decode(self, source_rep, source_len, max_len, src_dict, tgt_dict, src_map=None, alignment=None, blank=None, fill=None,
               source_vocabs=None, tgt2src=None, src_map_idx=None, ext2tgt=None, ext2src=None):
        """ACG.decode with the GRU step (the copy inputs and the EXTENDED prediction ids are ACG's)"""
        from ..constants import BOS
        from ..multitask import suggest
        if self.training:
            raise NotImplementedError("HIP ACGGRU.decode runs in eval mode")
        B, QL = source_rep.shape
        self._check_layers(B)
        table = self.embedder.word_embeddings.table
        lib.require_device(source_rep, source_len, table)
        L = lib.load()
        if src_map_idx is None or ext2tgt is None or ext2src is None:
            src_map_idx, ext2tgt, ext2src = self.copy_index(QL, src_map, blank, fill, source_vocabs, src_dict, tgt_dict)
        dev = table.device
        idx, e2t, e2s = (lib.ids64(t).to(dev).contiguous() for t in (src_map_idx, ext2tgt, ext2src))
        CV = int(e2t.shape[1])
        if tuple(idx.shape) != (B, QL) or tuple(e2t.shape) != (B, CV) or tuple(e2s.shape) != (B, CV):
            raise ValueError("ACGGRU.decode: src_map_idx %s, ext2tgt %s, ext2src %s do not fit %d rows of width %d"
                             % (tuple(idx.shape), tuple(e2t.shape), tuple(e2s.shape), B, QL))
        src, _ = self._clean_ids(source_rep, None, table.shape[0])
        lens = lib.ids64(source_len)
        dec_h, bank = self._encode_state(src, lens)
        w, cw = self._decoder_weights(), self._copy_weights()
        if tgt2src is None:
            tgt2src = suggest.tgt2src_lut(self, src_dict, tgt_dict, int(w.struct.VT), dev)
        t = table.detach().float().contiguous()
        max_len = int(max_len)
        preds = torch.empty(B, max_len, dtype=torch.int64, device=dev)
        attns = torch.empty(B, max_len, QL, dtype=torch.float32, device=dev)
        if B > 0 and max_len > 0:
            nb = L.nir_acg_gru_decode_workspace_bytes(B, QL, CV, w.ref(), cw.ref())
            if nb == 0:
                raise ValueError("ACGGRU.decode: QL = %d / CV = %d outside the copy generator's range (QL <= 4096, 2 <= CV <= 1024)" % (QL, CV))
            ws = lib.workspace(nb, dev)
            lib.check(L.nir_acg_gru_decode_greedy(lib.ptr(dec_h), lib.ptr(bank), lib.ptr(lens), B, QL, lib.ptr(t), t.shape[0], t.shape[1],
                                                  lib.ptr(tgt2src), BOS, max_len, w.ref(), cw.ref(), lib.ptr(idx), lib.ptr(e2t), lib.ptr(e2s), CV,
                                                  lib.ptr(ws), ws.numel(), lib.ptr(preds), lib.ptr(attns), lib.stream()), "nir_acg_gru_decode_greedy")
        return {"predictions": preds, "attentions": attns}
