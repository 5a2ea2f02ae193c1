"""Drop-in check against the reference wrappers' contract, recorded from the REAL reference (tests/golden/reference_dropin.npz, written by
tests/golden/generate.py): the state-dict keys and shapes, parameter counts and vocabularies of the reference's own networks at these
arguments, the arch hyper-parameters of its `hyparam`, the failure of its CARS forward with unequal encoder sizes, and its `tens2sen` output.

Everything the drivers main/ranker.py / main/multitask.py do with a model object is exercised on this package's wrappers, which take the
reference wrappers' place: construction from the arguments `config.get_model_args` builds, state-dict key and
shape identity with the reference's own networks (its `load_state_dict` is strict), count_parameters, load_embeddings, init_optimizer
(fix_embeddings freezes `network.word_embeddings` / `network.embedder.word_embeddings`), save -> load, checkpoint -> load_checkpoint.
predict on CPU tensors must fail loudly (no CPU fallback)."""
import json
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_dropin.npz")


class Vocab(object):
    """The part of the reference's Vocabulary the wrappers use (len, `in`, id <-> token, ind2tok), over a recorded id -> token list."""

    def __init__(self, ind2tok):
        self.ind2tok = dict(enumerate(ind2tok))
        self.tok2ind = {t: i for i, t in enumerate(ind2tok)}

    def __len__(self):
        return len(self.ind2tok)

    def __contains__(self, key):
        return key in (self.ind2tok if isinstance(key, int) else self.tok2ind)

    def __getitem__(self, key):
        return self.ind2tok[key] if isinstance(key, int) else self.tok2ind[key]


@pytest.fixture(scope="module")
def ref():
    z = np.load(GOLDEN)
    g = {k: z[k] for k in z.files}
    return Namespace(g=g, arch=json.loads(str(g["arch_json"])), src=Vocab([str(t) for t in g["src_ind2tok"]]),
                     tgt=Vocab([str(t) for t in g["tgt_ind2tok"]]))


def _args(ref, model, **kw):
    a = dict(emsize=300, dropout_emb=0.2, dropout=0.2, dropout_rnn=0.2, max_doc_len=20, max_query_len=6, num_candidates=4,
             use_word=True, fix_embeddings=True, model_type=model, optimizer="adam", learning_rate=0.001, weight_decay=0,
             momentum=0, grad_clipping=10)
    a.update(ref.arch[model])
    a.update(kw)
    return Namespace(**a)


def _shapes(net):
    return {k: ",".join(str(d) for d in v.shape) for k, v in net.state_dict().items()}


def _ref_shapes(ref, prefix):
    return dict(zip((str(k) for k in ref.g[prefix + "_keys"]), (str(s) for s in ref.g[prefix + "_shapes"])))


def test_arch_hyperparameters_are_the_reference_ones(ref):
    from context_attentive_ir_amd import config
    for model, params in ref.arch.items():
        assert config.get_model_specific_params(model, "arch") == params, model


@pytest.mark.parametrize("model,attr", [("ESM", "ESM"), ("MATCH_TENSOR", "MatchTensor"), ("DRMM", "DRMM"), ("DUET", "DUET")])
def test_reference_ranker_with_swapped_network(ref, model, attr, tmp_path):
    from context_attentive_ir_amd import rankers
    from context_attentive_ir_amd.wrappers import Ranker
    vocab = ref.src
    m = Ranker(_args(ref, model), vocab)
    assert type(m.network) is getattr(rankers, attr)
    assert _shapes(m.network) == _ref_shapes(ref, model)               # the reference's own network: the key set to match
    assert m.count_parameters() == int(ref.g[model + "_count"])
    # load_embeddings -> init_word_vectors on the network's word_embeddings
    emb = tmp_path / "emb.txt"
    emb.write_text("\n".join("tok%d %s" % (i, " ".join(["%.3f" % (0.01 * i)] * 300)) for i in range(5)))
    m.load_embeddings(["tok%d" % i for i in range(5)], str(emb))
    row = m.network.word_embeddings.table[vocab["tok3"]]
    assert torch.allclose(row, torch.full((300,), 0.03), atol=1e-6)
    if model != "ESM":
        m.init_optimizer(use_gpu=False)
        assert all(not p.requires_grad for p in m.network.word_embeddings.parameters())
        m.checkpoint(str(tmp_path / "c.mdl"), 3)
        m2, epoch = Ranker.load_checkpoint(str(tmp_path / "c.mdl"), use_gpu=False)
        assert epoch == 3 and type(m2.network) is type(m.network)
    m.save(str(tmp_path / "m.mdl"))
    m3 = Ranker.load(str(tmp_path / "m.mdl"))
    for k, v in m.network.state_dict().items():
        assert torch.equal(v, m3.network.state_dict()[k])
    ex = dict(que_rep=torch.zeros(2, 6, dtype=torch.long), que_len=torch.full((2,), 6), doc_rep=torch.zeros(2, 4, 20, dtype=torch.long),
              doc_len=torch.full((2, 4), 20), label=torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict(ex)


@pytest.mark.parametrize("kw", [{}, dict(query_session_off=True), dict(doc_session_off=True)])
def test_reference_multitask_with_swapped_cars(ref, kw, tmp_path):
    from context_attentive_ir_amd.multitask import CARS
    from context_attentive_ir_amd.wrappers import Multitask
    m = Multitask(_args(ref, "CARS", **kw), ref.src, ref.tgt)
    assert type(m.network) is CARS
    assert _shapes(m.network) == _ref_shapes(ref, "cars_" + (next(iter(kw)) if kw else "default"))
    m.init_optimizer(use_gpu=False)
    assert all(not p.requires_grad for p in m.network.embedder.word_embeddings.parameters())
    m.save(str(tmp_path / "m.mdl"))
    m2 = Multitask.load(str(tmp_path / "m.mdl"))
    assert type(m2.network) is CARS
    for k, v in m.network.state_dict().items():
        assert torch.equal(v, m2.network.state_dict()[k])
    # every attribute / method Multitask.predict touches on the network exists with the reference's signature
    for name in ("encode", "rank_document", "decode", "forward", "embedder"):
        assert hasattr(m.network, name)
    ex = dict(source_words=torch.zeros(2, 3, 6, dtype=torch.long), source_lens=torch.full((2, 3), 6),
              document_words=torch.zeros(2, 3, 4, 20, dtype=torch.long), document_lens=torch.full((2, 3, 4), 20),
              document_labels=torch.zeros(2, 3, 4), session_len=3, ids=["a", "b"], batch_size=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.predict(ex)


def test_reference_cars_itself_fails_with_unequal_encoder_sizes(ref):
    """`multitask/cars.py` of this package refuses nhid_query != nhid_document.  That mirrors the reference: its session loop multiplies
    session_doc_attn(states) [B, k, nhid_document] with the pooled QUERY [B, nhid_query, 1] (cars.py:357-360), so with the document-session
    encoder and the ranker on (every hyparam configuration) its own forward raises for unequal sizes -- recorded from the real class at these
    sizes, next to the finite ranking loss it gives for the same inputs with equal sizes."""
    from context_attentive_ir_amd.multitask import CARS
    kw = json.loads(str(ref.g["cars_unequal_kw_json"]))
    assert kw["nhid_query"] != kw["nhid_document"]
    assert "batch2" in str(ref.g["cars_unequal_error"])                         # the bmm of cars.py:361 inside the reference's encode_session
    assert np.isfinite(float(ref.g["cars_equal_ranking_loss"]))                 # with equal sizes the reference goes through
    with pytest.raises(NotImplementedError, match="nhid_query == nhid_document"):
        CARS(_args(ref, "CARS", **kw))
    assert type(CARS(_args(ref, "CARS", **dict(kw, nhid_document=kw["nhid_query"])))) is CARS


def test_predict_text_outputs_equal_the_reference_tail(ref):
    """wrappers.Multitask._suggestion_text (the host tail of predict for a batch in the reference's collate layout) against the reference's own
    tail: `tens2sen` over the decoder's ids per step (recorded from the reference for these ids), `ex_ids`, `targets`, `src_sequences` exactly as
    models/multitask.py:294-316 builds them -- what main/multitask.py:validate_official reads from `outputs`."""
    from context_attentive_ir_amd.config import default_args
    from context_attentive_ir_amd.wrappers import Multitask
    tgt = ref.tgt
    w = Multitask(default_args("CARS", src_vocab_size=40, tgt_vocab_size=len(tgt)), tgt_dict=tgt)
    pred = torch.from_numpy(ref.g["tail_pred"].copy())                           # incl. BOS / EOS / PAD and ids past the dictionary
    B, S, ML = pred.shape[0], pred.shape[1] + 1, pred.shape[2]
    assert (pred[0, 0] == 2).all() and pred[1, 1, 2] == 3                        # only BOS: an empty sentence; EOS in the middle
    src_tok = [[["<s>"] + ["q%d_%d_%d" % (b, s, j) for j in range(2 + s)] + ["</s>"] for s in range(S)] for b in range(B)]
    ex = {"ids": ["sess%d_" % b for b in range(B)], "batch_size": B, "session_len": S, "source_tokens": src_tok,
          "target_tokens": [[src_tok[b][s] for s in range(1, S)] for b in range(B)]}
    got = w._suggestion_text(ex, pred)
    # the reference's tail, verbatim semantics
    want_pred, want_tgt, want_src = [str(s) for s in ref.g["tail_predictions"]], [], []
    for sidx in range(S - 1):
        for bidx in range(B):
            tokens = ex["target_tokens"][bidx][sidx]
            want_tgt.append([" ".join(tokens[1:-1])])
            want_src.append(" ".join(" ".join(q[1:-1]) for q in ex["source_tokens"][bidx][0:sidx + 1]))
    assert got["predictions"] == want_pred and got["targets"] == want_tgt and got["src_sequences"] == want_src
    assert got["ex_ids"] == [_id + str(i) for i in range(S) for _id in ex["ids"]]
    assert got["prediction_ids"] is pred and len(got["predictions"]) == B * (S - 1)
