#!/usr/bin/env python
"""Golden fixtures of the reference's Seq2seq and ACG with rnn_type = 'GRU' (config.py:53; decoders/decoder.py:175-177,
decoders/rnn_decoder.py:46-47) and of Recommender over them, run on CPU.

The data, the acceptance conditions and the recording are those of generate_seq2seq.py and generate_acg.py, whose helpers run here with
rnn_type = 'GRU' passed to the reference's constructor; like there the fixture carries ids, maps and outputs only.

    python tests/golden/generate_seq2seq_gru.py          # rewrites tests/golden/seq2seq_gru.npz

Keys: `s2s_<key of seq2seq.npz>` for the five Seq2seq cases (general / dot / mlp / uni / wide; predictions, attentions, gaps, teacher-forced loss,
three Recommender.update losses with the table fixed and free, the nlayers = 2 error text -- torch.nn.GRU's, which says `hidden`, not
`hidden[0]`), `acg_<key of acg.npz>` for the three ACG cases (general, mlp, own; predictions, attentions, winner classes, copy loss, three
update losses for general).

The seed searches and their asserts are the two generators' own: every gap >= 1e-3, >= 4 distinct tokens (Seq2seq), every winner class
present (ACG).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import generate as G  # noqa: E402  (installs the shims, puts the reference on sys.path)
import generate_acg as GA  # noqa: E402
import generate_seq2seq as GS  # noqa: E402

from neuroir.recommender.seq2seq import Seq2seq  # noqa: E402

ACG_CASES = ("general", "mlp", "own")


def with_gru(args_for):
    def f(cfg, **kw):
        return args_for(cfg, **dict(kw, rnn_type="GRU"))
    return f


def gen_nlayers2(out, data):
    """nlayers = 2 with a GRU decoder: the reference's forward and decode fail with torch.nn.GRU's text"""
    src, lens, tw, ts, tlen = data
    m = GS.load_seed(Seq2seq(G.base_args("SEQ2SEQ", tgt_vocab_size=GS.VT, nhid=64, rnn_type="GRU", copy_attn=False, reuse_copy_attn=False,
                                         force_copy=False)), 1)
    msgs = []
    for call in (lambda: m(source_rep=G.T(src), source_len=G.T(lens), target_rep=G.T(tw), target_len=G.T(tlen), target_seq=G.T(ts), source_map=None,
                           alignment=None),
                 lambda: m.decode(source_rep=G.T(src), source_len=G.T(lens), max_len=GS.MAXLEN, src_dict=list(range(G.V)),
                                  tgt_dict=list(range(GS.VT)), src_map=None, alignment=None, blank=None, fill=None, source_vocabs=None)):
        try:
            with torch.no_grad():
                call()
            msgs.append("")
        except RuntimeError as e:
            msgs.append(str(e))
    assert all(s.startswith("Expected hidden size (2, %d, 64), got [1, %d, 64]" % (GS.B, GS.B)) for s in msgs), msgs
    out.update(nlayers2_error=np.asarray(msgs[0]), nlayers2_error_type=np.asarray("RuntimeError"))


if __name__ == "__main__":
    torch.manual_seed(G.SEED)
    torch.set_num_threads(4)
    GS.args_for = with_gru(GS.args_for)
    GA.args_for = with_gru(GA.args_for)
    GA.CASES = tuple(c for c in GA.CASES if c[0] in ACG_CASES)
    s2s, acg = {}, {}
    seeds, data = GS.gen_decode(s2s)
    gen_nlayers2(s2s, data)
    GS.gen_train(s2s, seeds["general"])
    aseeds = GA.gen_decode(acg)
    GA.gen_train(acg, aseeds["general"])
    out = {"s2s_" + k: v for k, v in s2s.items()}
    out.update({"acg_" + k: v for k, v in acg.items()})
    G.save("seq2seq_gru", **out)
