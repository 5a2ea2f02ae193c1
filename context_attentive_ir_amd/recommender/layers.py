"""Parameter containers that give Seq2seq and HredQS the reference's attribute / state-dict nesting (mirror of
/root/reference/neuroir/recommender/layers.py:10-93: `embedder.word_embeddings...`, `encoder.encoder.rnns.0...`,
`decoder.decoder.rnn...`, `decoder.decoder.attn...`).  nn.LSTM / nn.Linear hold the parameters only; the forward never calls them.
encode_train is the differentiable encoder both models train through."""
import torch
import torch.nn as nn

from ..multitask.layers import Embedder, Encoder      # noqa: F401  (the same nesting as the session models')

ATTN_TYPES = ("general", "dot", "mlp")


class GlobalAttentionParams(nn.Module):
    """modules/global_attention.py:58-79: `general` has linear_in, `mlp` has linear_context / linear_query (bias) / v and a bias on
    linear_out, `dot` has linear_out alone."""

    def __init__(self, dim, attn_type):
        super().__init__()
        if attn_type not in ATTN_TYPES:
            raise AssertionError("Please select a valid attention type.")
        self.dim, self.attn_type = dim, attn_type
        if attn_type == "general":
            self.linear_in = nn.Linear(dim, dim, bias=False)
        elif attn_type == "mlp":
            self.linear_context = nn.Linear(dim, dim, bias=False)
            self.linear_query = nn.Linear(dim, dim, bias=True)
            self.v = nn.Linear(dim, 1, bias=False)
        self.linear_out = nn.Linear(dim * 2, dim, bias=attn_type == "mlp")


class RNNDecoderParams(nn.Module):
    """decoders/decoder.py:68-118: `rnn` = getattr(nn, rnn_type)(input_size -> hidden_size, num_layers), `attn` = GlobalAttention(hidden_size);
    attn_type 'none' (layers.py:70: HredQS) has no attention module and no attention parameters."""

    def __init__(self, input_size, nlayers, nhid, attn_type, dropout, copy_attn=False, rnn_type="LSTM"):
        super().__init__()
        self.hidden_size = nhid
        self.rnn = (nn.GRU if rnn_type == "GRU" else nn.LSTM)(input_size, nhid, nlayers, batch_first=True)
        if attn_type not in (None, "none"):
            self.attn = GlobalAttentionParams(nhid, attn_type)
        if copy_attn:                                   # decoders/decoder.py:113-116: ACG without reuse_copy_attn, a second attention of the same type
            self.copy_attn = GlobalAttentionParams(nhid, attn_type)
        self.dropout = nn.Dropout(dropout)


class Decoder(nn.Module):
    def __init__(self, input_size, nlayers, nhid, attn_type, dropout_rnn, copy_attn=False, rnn_type="LSTM"):
        super().__init__()
        self.decoder = RNNDecoderParams(input_size, nlayers, nhid, attn_type, dropout_rnn, copy_attn, rnn_type)


class CopyGeneratorParams(nn.Module):
    """modules/copy_generator.py:49-55: `linear` IS the model's generator (one parameter under two state-dict keys), `linear_copy` the switch"""

    def __init__(self, nhid, generator):
        super().__init__()
        self.linear = generator
        self.linear_copy = nn.Linear(nhid, 1)


def encode_train(rnn, x, lens):
    """x [B,T,E] through the single-layer nn.LSTM container `rnn` -> (memory bank [B,T,nhid], zero beyond each length; h_n [B,nhid];
    c_n [B,nhid]) in ORIGINAL row order, differentiable: the register-resident training recurrence up to 128 units per direction (it
    returns the cell states), one lstm_seq pass per direction beyond."""
    from .. import autograd as A
    nd, params = A._lstm_params(rnn)
    H = rnn.hidden_size
    B, T, _ = x.shape
    dev = x.device
    rows = torch.arange(B, device=dev)
    last = (lens - 1).clamp(min=0)
    if H <= 128:
        out, cst = A._BiLSTM.apply(x, lens, nd, None, None, *params)
        hs, cs = [out[rows, last, :H]], [cst[rows, last, 0]]
        if nd == 2:                                                      # the reverse direction ends at position 0
            hs.append(out[:, 0, H:])
            cs.append(cst[:, 0, 1])
        return out, torch.cat(hs, 1), torch.cat(cs, 1)
    pos = torch.arange(T, device=dev).view(1, T)
    valid = (pos < lens.view(B, 1)).unsqueeze(2).float()

    class _Dir(object):                                                  # one direction's parameters under the names lstm_seq reads
        def __init__(self, sfx):
            for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
                setattr(self, n, getattr(rnn, n + sfx))
    hf, cf = A.lstm_seq(x, _Dir(""))
    banks, hs, cs = [hf * valid], [hf[rows, last]], [cf[rows, last]]
    if nd == 2:
        ridx = (lens.view(B, 1) - 1 - pos).clamp(min=0)                  # position read at reverse step t
        xr = torch.gather(x, 1, ridx.unsqueeze(2).expand(B, T, x.shape[2])) * valid
        hr, cr = A.lstm_seq(xr, _Dir("_reverse"))
        banks.append(torch.gather(hr * valid, 1, ridx.unsqueeze(2).expand(B, T, H)) * valid)
        hs.append(hr[rows, last])                                        # after the whole valid part, read backwards
        cs.append(cr[rows, last])
    return torch.cat(banks, 2), torch.cat(hs, 1), torch.cat(cs, 1)


def encode_train_gru(rnn, x, lens):
    """x [B,T,E] through the single-layer nn.GRU container `rnn` -> (memory bank [B,T,nhid], zero beyond each length; h_n [B,nhid]) in ORIGINAL
    row order, differentiable (autograd.bigru).  The final state is read from the bank: the forward half at position len - 1, the reverse
    half at position 0."""
    from .. import autograd as A
    H = rnn.hidden_size
    B = x.shape[0]
    bank = A.bigru(x, lens, rnn)
    last = (lens - 1).clamp(min=0)
    hs = [bank[torch.arange(B, device=x.device), last, :H]]
    if rnn.bidirectional:
        hs.append(bank[:, 0, H:])
    return bank, torch.cat(hs, 1)
