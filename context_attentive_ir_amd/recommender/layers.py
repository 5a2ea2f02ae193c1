"""Parameter containers that give Seq2seq the reference's attribute / state-dict nesting (mirror of
/root/reference/neuroir/recommender/layers.py:10-93: `embedder.word_embeddings...`, `encoder.encoder.rnns.0...`,
`decoder.decoder.rnn...`, `decoder.decoder.attn...`).  nn.LSTM / nn.Linear hold the parameters only; the forward never calls them."""
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
    """decoders/decoder.py:68-118: `rnn` = nn.LSTM(input_size -> hidden_size, num_layers), `attn` = GlobalAttention(hidden_size)."""

    def __init__(self, input_size, nlayers, nhid, attn_type, dropout):
        super().__init__()
        self.hidden_size = nhid
        self.rnn = nn.LSTM(input_size, nhid, nlayers, batch_first=True)
        self.attn = GlobalAttentionParams(nhid, attn_type)
        self.dropout = nn.Dropout(dropout)


class Decoder(nn.Module):
    def __init__(self, input_size, nlayers, nhid, attn_type, dropout_rnn):
        super().__init__()
        self.decoder = RNNDecoderParams(input_size, nlayers, nhid, attn_type, dropout_rnn)
