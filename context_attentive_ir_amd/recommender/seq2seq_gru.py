"""Seq2seqGRU / ACGGRU -- the two attention recommenders with rnn_type 'GRU' (the reference's config.py:53; the decoder's GRU branch is
neuroir/decoders/decoder.py:175-177 and decoders/rnn_decoder.py:46-47).

Seq2seq and ACG are written once over a description of their cell (seq2seq.py: class attributes and three hooks); the subclasses here are that
description for the GRU and nothing else -- the constructors, decode(), decode_beam(), the packed decoder weights, the teacher-forced pass and
both losses are the parents'.  What the cell changes:

  * the encoder's final state is ONE tensor h_n; the decoder starts from its halves side by side, [B, nhid], in the reference's length-sorted
    row order (seq2seq.py's module docstring), and carries no cell state;
  * decode() / decode_beam(): nir_seq2seq_gru_decode_greedy / nir_acg_gru_decode_greedy / nir_beam_seq2seq_gru_decode (csrc/gru_step.hip:
    torch.nn.GRU's step, b_hn inside the reset product).  With `fold_decoder_step` the input side is a per-token table [V, 3H] = table
    W_ih^T + b_ih + (b_hr, b_hz, 0) (lib.fold_gru_table) and the recurrent product runs on fp16 term pairs, one launch per step; otherwise,
    or when a weight is outside the split's range, the exact fp32 step;
  * forward(): the GRU encoder through autograd.bigru, its final state read from the memory bank, the decoder through autograd.gru_seq with
    the initial state as a differentiable input.

State-dict keys are the reference's: `decoder.decoder.rnn.*_l0` and `encoder.encoder.rnns.0.*` are [3H, .].
nlayers != 1 constructs and fails in forward / decode with torch.nn.GRU's own text (it says `hidden`, not `hidden[0]`).
"""
import torch

from .. import autograd as A
from .. import lib
from .acg import ACG
from .layers import encode_train_gru
from .seq2seq import Seq2seq


class _GRUDecoderMixin(object):
    """the GRU forms of the cell description Seq2seq carries (seq2seq.py): data, and the three hooks whose body depends on the cell"""
    _CELL = "GRU"
    _GATES = 3
    _WHH_PACK = "nir_gru_step"
    _LAYER_CHECK = "Expected hidden size (%d, %d, %d), got [1, %d, %d]"        # torch.nn.GRU's text: `hidden`, not `hidden[0]`
    _ENTRY_CELL = "_gru"
    _fold_table = staticmethod(lib.fold_gru_table)

    def initial_state(self, final, source_len):
        """decoders/decoder.py:160-177 on the GRU encoder's final h_n [ND, B, nhid / ND] (ORIGINAL row order) -> h [B, nhid]: row b is the state
        of source row order[b], forward and reverse halves along the feature axis"""
        order = torch.sort(source_len, 0, True)[1]
        return torch.cat([final[d][order] for d in range(final.shape[0])], 1).contiguous()

    def _encode_train(self, x, lens):
        """x [B,T,E] -> (memory bank [B,T,nhid], (h_n [B,nhid],)) in ORIGINAL row order, differentiable (autograd.bigru; h_n read from the bank)"""
        mem, h_n = encode_train_gru(self.encoder.encoder.rnns[0], x, lens)
        return mem, (h_n,)

    def _cell_train(self, temb, state):
        return A.gru_seq(temb, self.decoder.decoder.rnn, state[0])


class Seq2seqGRU(_GRUDecoderMixin, Seq2seq):
    pass


class ACGGRU(_GRUDecoderMixin, ACG):
    pass
