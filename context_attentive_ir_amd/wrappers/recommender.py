"""Recommender -- wrapper with the call shapes of neuroir.models.recommender.Recommender
(/root/reference/neuroir/models/recommender.py:21-420) for Seq2seq: update(ex) is the training step, predict(ex) the greedy decode
(+ the reference's host-side tail for a batch in its collate layout), score(ex, candidates) the log-likelihood of given next queries.  SessionRecommender is the same wrapper for HredQS, whose batches keep
their session axis; CopyRecommender is the same wrapper for ACG, whose batches carry the copy generator's maps."""
import torch

from .. import lib
from ..constants import BOS, EOS, PAD, UNK_WORD
from ..recommender import ACG, ACGGRU, HredQS, Seq2seq, Seq2seqGRU
from .common import WrapperBase

NETWORKS = {"SEQ2SEQ": Seq2seq}
# args.rnn_type 'GRU' (config.py:53) builds the GRU-decoder class of the model; any other value goes to the LSTM class, which refuses what it is not
GRU_NETWORKS = {"SEQ2SEQ": Seq2seqGRU, "ACG": ACGGRU}
FOLLOW_UPS = {"ACG": "ACG's batches carry src_map / alignment / src_vocab: build it with wrappers.CopyRecommender (registering it here is its own "
                     "follow-up)",
              "HREDQS": "HredQS keeps the session axis of its batches: build it with wrappers.SessionRecommender (registering it here is its own "
                        "follow-up)"}


class Recommender(WrapperBase):
    def __init__(self, args, src_dict=None, tgt_dict=None, state_dict=None):
        self.args = args
        self.src_dict, self.tgt_dict = src_dict, tgt_dict
        if src_dict is not None:
            self.args.src_vocab_size = len(src_dict)
        if tgt_dict is not None:
            self.args.tgt_vocab_size = len(tgt_dict)
        self.type = args.model_type.upper()
        self.network = self._network_class()(args)
        if state_dict:
            state_dict = dict(state_dict)
            state_dict.pop("fixed_embedding", None)              # models/recommender.py:50-57: a buffer of the embedding layer, not a parameter
            self.network.load_state_dict(state_dict)
        self.updates, self.use_cuda, self.parallel = 0, False, False
        self.group = None

    def _network_class(self):
        if self.type in FOLLOW_UPS:
            raise NotImplementedError("HIP Recommender: model_type %s is not built yet -- %s" % (self.type, FOLLOW_UPS[self.type]))
        if self.type not in NETWORKS:
            raise RuntimeError("Unsupported model: %s (recommender models on the HIP path: %s)" % (self.args.model_type, sorted(NETWORKS)))
        return GRU_NETWORKS[self.type] if getattr(self.args, "rnn_type", "LSTM") == "GRU" else NETWORKS[self.type]

    def _dev(self, t):
        return t.cuda(non_blocking=True) if self.use_cuda else t

    # ---- training ---------------------------------------------------------------------------------------------------------------------
    def update(self, ex):
        """models/recommender.py:160-227: train-mode forward -> backward -> clip_grad_norm(grad_clipping) -> optimizer step; returns the loss."""
        if self.optimizer is None:
            raise RuntimeError("No optimizer set.")
        self._poll_ids()
        self.optimizer.zero_grad()
        loss = self._update_body(ex)
        self.updates += 1
        self._maybe_check_ids()
        return loss

    def _update_body(self, ex):
        from .. import autograd as A
        self.network.train()
        A.STEP.begin()
        try:
            src, tgt, seq = (self._dev(self._rows3(ex[k])) for k in ("source_words", "target_words", "target_seq"))
            sl, tl = (self._dev(self._rows2(ex[k])) for k in ("source_lens", "target_lens"))
            loss = self.network(source_rep=src, source_len=sl, target_rep=tgt, target_len=tl, target_seq=seq, source_map=None, alignment=None)
            loss.backward()
        except BaseException:
            A.STEP.abort()
            raise
        A.STEP.end()
        self.sync_gradients()
        torch.nn.utils.clip_grad_norm_(self.network.parameters(), self.args.grad_clipping)
        self.optimizer.step()
        # a fused optimizer step (init_optimizer builds Adam that way on a GPU) writes the parameters without bumping their version counters, and
        # every version-keyed cache -- lib.PackCache: the folded gate table, the fragments, the encoders' concatenated weights; the predict graph
        # cache -- would keep serving the weights of before the step to the next decode.  Bump them here, no kernel involved.
        torch.autograd.graph.increment_version([p for g in self.optimizer.param_groups for p in g["params"]])
        return loss

    @staticmethod
    def _rows3(t):
        return t.squeeze(1) if t.dim() == 3 else t

    @staticmethod
    def _rows2(t):
        return t.squeeze(1) if t.dim() == 2 else t

    # ---- prediction -------------------------------------------------------------------------------------------------------------------
    _FIELDS = ("source_words", "source_lens")

    def _predict_body(self, ex):
        self.network.eval()
        dec = self.network.decode(source_rep=self._dev(self._rows3(ex["source_words"])), source_len=self._dev(self._rows2(ex["source_lens"])),
                                  max_len=self.args.max_query_len, src_dict=self.src_dict, tgt_dict=self.tgt_dict, src_map=None, alignment=None,
                                  blank=None, fill=None, source_vocabs=ex.get("src_vocab") if isinstance(ex, dict) else None)
        self._maybe_check_ids()
        return {"prediction_ids": dec["predictions"], "attentions": dec["attentions"]}

    _TEXT_FIELDS = ("ids", "source_tokens", "target_tokens", "src_vocab")      # a batch in the reference's collate layout has all of them
    _NBEST_AXIS = 1                                                            # the beam / sample axis of prediction_ids and attentions

    def _graphed_or_eager(self, ex, flavour, body):
        """body(ex) through the hipGraph cache (WrapperBase._graphed, `flavour` in the key), or eagerly where that declines"""
        out = self._graphed(ex, self._FIELDS, flavour, body)
        if out is None:
            out = body(ex)
        elif self.id_check == "blocking":
            self._maybe_check_ids()
        return out

    def _decode_kw(self, ex):
        """what every decode of the network takes from a batch"""
        return dict(source_rep=self._dev(self._rows3(ex["source_words"])), source_len=self._dev(self._rows2(ex["source_lens"])),
                    max_len=self.args.max_query_len, src_dict=self.src_dict, tgt_dict=self.tgt_dict)

    @staticmethod
    def _ids_first(dec):
        """a decode's dict under the wrappers' key: 'predictions' -> 'prediction_ids' ('predictions' are the strings here)"""
        return {("prediction_ids" if k == "predictions" else k): v for k, v in dec.items()}

    def _nbest_text(self, ex, out):
        """out, for a batch in the reference's collate layout with predict()'s text fields: `predictions` = per row the list of its n strings,
        one _text per beam / sample"""
        if all(k in ex for k in self._TEXT_FIELDS):
            ids, att, ax = out["prediction_ids"], out.get("attentions"), self._NBEST_AXIS
            per = [self._text(ex, ids.select(ax, k), None if att is None else att.select(ax, k)) for k in range(ids.shape[ax])]
            out.update(per[0])
            out["predictions"] = [[p["predictions"][i] for p in per] for i in range(len(per[0]["predictions"]))]
        return out

    @torch.no_grad()
    def predict(self, ex):
        """models/recommender.py:233-329: {'prediction_ids': LongTensor [B, max_query_len] (target-vocabulary ids), 'attentions':
        [B, max_query_len, QL]}; for a batch in the reference's collate layout (`ids`, `source_tokens`, `target_tokens`, `src_vocab`) also the
        reference's `ex_ids`, `predictions` (strings, <unk> replaced by the most attended source token), `targets`, `src_sequences`.
        From the `predict_graph_min_calls`-th call of a batch shape on, the call replays a captured hipGraph (WrapperBase._graphed)."""
        self._poll_ids()
        out = self._graphed_or_eager(ex, "decode", self._predict_body)
        if all(k in ex for k in self._TEXT_FIELDS):
            out.update(self._text(ex, out["prediction_ids"], out.get("attentions")))
        return out

    # ---- beam search ------------------------------------------------------------------------------------------------------------------
    def _predict_beam_body(self, ex, beam_size):
        self.network.eval()
        dec = self.network.decode_beam(beam_size=beam_size, **self._decode_kw(ex))
        self._maybe_check_ids()
        return self._ids_first(dec)

    def _nbest(self, ex, W, flavour):
        """the n-best call of every wrapper here: _predict_beam_body under the graph key flavour % W, then the strings"""
        self._poll_ids()
        return self._nbest_text(ex, self._graphed_or_eager(ex, flavour % W, lambda e: self._predict_beam_body(e, W)))

    @torch.no_grad()
    def predict_beam(self, ex, beam_size):
        """n-best suggestions by beam search (Seq2seq.decode_beam; the reference has no counterpart): {'prediction_ids': LongTensor
        [B, W, max_query_len], 'scores': [B, W], 'lengths': LongTensor [B, W], 'attentions': [B, W, max_query_len, QL]}, best beam first; for
        a batch in the reference's collate layout also `ex_ids`, `targets`, `src_sequences` and `predictions`: per row the list of its W
        strings, each formed like predict()'s.  `beam_size` is an argument of the call, not a field of args.  Graph replay as in predict()."""
        return self._nbest(ex, int(beam_size), "decode_beam%d")

    def predict_nbest(self, ex, beam_size):
        """n-best suggestions, the one name every wrapper has: predict_beam here; CopyRecommender's is ACG's search over the copy generator's
        distribution; SessionRecommender (HredQS) keeps the session axis: predict_session_nbest."""
        return self.predict_beam(ex, beam_size)

    # ---- sampling -------------------------------------------------------------------------------------------------------------------
    def _samples(self, ex, draw, num_samples, temperature, top_k, seed):
        """the sampling call of every wrapper here; draw: the network's sampling method"""
        seed = self._draw_seed(seed)
        self._poll_ids()
        self.network.eval()
        dec = draw(num_samples=int(num_samples), temperature=temperature, top_k=top_k, seed=seed, **self._decode_kw(ex))
        self._maybe_check_ids()
        return self._nbest_text(ex, dict(self._ids_first(dec), seed=int(seed)))

    @torch.no_grad()
    def predict_samples(self, ex, num_samples, temperature=1.0, top_k=0, seed=None):
        """`num_samples` i.i.d. suggestions per row drawn from the model (Seq2seq.decode_sample; the reference has no counterpart):
        {'prediction_ids': LongTensor [B, N, max_query_len], 'token_logprobs': [B, N, max_query_len], 'scores': [B, N], 'lengths': LongTensor
        [B, N], 'attentions': [B, N, max_query_len, QL], 'seed': the seed used}, in sample order (not sorted, duplicates possible); for a batch
        in the reference's collate layout also `ex_ids`, `targets`, `src_sequences` and `predictions`: per row the list of its N strings, each
        formed like predict()'s.  seed=None draws a 63-bit seed from torch's default CPU generator (no device synchronisation); calling again
        with the returned 'seed' replays the draw bit for bit.  Always eager: the seed is a host argument of the C entry, so a captured graph
        would replay one and the same draw."""
        return self._samples(ex, self.network.decode_sample, num_samples, temperature, top_k, seed)

    # ---- scoring --------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def score(self, ex, candidates=None, length_normalize=False):
        """Teacher-forced log-likelihood of given next queries (the network's score_candidates) -> {'token_logprobs',
        'scores', 'lengths'} as it returns them.
        candidates=None: the batch's own `target_seq` is the one candidate of every row (fed `target_words`); additionally 'nll' = -mean over
        rows of `scores`, the reference forward's loss in eval mode, and 'perplexity' = exp(-sum scores / sum lengths).
        With candidates -- a LongTensor [B, N, TL] (HredQS: [B, S, N, TL]) of target-vocabulary ids, BOS first, or ex['candidate_seq'], with
        ex['candidate_rep'] as the ids fed to the decoder where given -- additionally 'ranking' [B, N] (HredQS: [B, S, N]): the candidates
        best first by `scores`, or by scores / lengths with `length_normalize`, ties to the smaller n; usable as it is with eval.MRR /
        eval.MAP.  Eager: candidate shapes vary per call, nothing is captured."""
        self._poll_ids()
        self.network.eval()
        src, sl = self._dev(self._rows3(ex["source_words"])), self._dev(self._rows2(ex["source_lens"]))
        own = candidates is None and "candidate_seq" not in ex
        if own:
            cand = self._rows3(ex["target_seq"]).unsqueeze(-2)
            rep = self._rows3(ex["target_words"]).unsqueeze(-2)
        else:
            cand = ex["candidate_seq"] if candidates is None else candidates
            rep = ex.get("candidate_rep") if isinstance(ex, dict) else None
        out = self.network.score_candidates(source_rep=src, source_len=sl, candidate_seq=self._dev(cand),
                                            candidate_rep=self._dev(rep) if rep is not None else None, src_dict=self.src_dict, tgt_dict=self.tgt_dict)
        self._maybe_check_ids()
        return self._score_summary(out, own, length_normalize)

    def _text(self, ex, pred_ids, attns):
        """the host-side tail of the reference's predict (models/recommender.py:294-309): tens2sen (utils/misc.py:36-62) + replace_unknown
        (utils/copy_utils.py:51-60: token i of the sentence takes the arg-max of attention row i).  The one place predict synchronises."""
        host, att = pred_ids.cpu().tolist(), attns.cpu()
        self._poll_ids()
        words, nw = self.tgt_dict, (len(self.tgt_dict) if self.tgt_dict is not None else 0)
        preds = []
        for b, row in enumerate(host):
            sent = []
            for wd in row:
                if wd == BOS:
                    continue
                if wd == EOS:
                    break
                sent.append(words[wd] if (words is not None and wd < nw) else str(wd))
            if not sent:
                sent = [str(PAD)]
            src_raw = ex["source_tokens"][b][0]
            for i, tok in enumerate(sent):
                if tok == UNK_WORD:
                    sent[i] = src_raw[int(att[b, i].argmax())]
            preds.append(" ".join(sent))
        return {"ex_ids": ex["ids"], "predictions": preds,
                "targets": [[" ".join(q[1:-1]) for q in item] for item in ex["target_tokens"]],
                "src_sequences": [[" ".join(q[1:-1]) for q in session] for session in ex["source_tokens"]]}

    # ---- saving / loading -------------------------------------------------------------------------------------------------------------
    @classmethod
    def load(cls, filename, new_args=None):
        saved = torch.load(filename, map_location="cpu", weights_only=False)
        args = saved["args"]
        if new_args is not None:
            from ..config import override_model_args
            args = override_model_args(args, new_args)
        return cls(args, saved.get("src_dict"), saved.get("tgt_dict"), saved["state_dict"])

    @classmethod
    def load_checkpoint(cls, filename, use_gpu=True):
        saved = torch.load(filename, map_location="cpu", weights_only=False)
        model = cls(saved["args"], saved.get("src_dict"), saved.get("tgt_dict"), saved["state_dict"])
        if use_gpu:
            model.cuda()
        model.init_optimizer(saved["optimizer"], use_gpu)
        return model, saved["epoch"]


class SessionRecommender(Recommender):
    """The same wrapper for HredQS (models/recommender.py:44-45,181-211,260-327): the batch tensors keep their session axis, [B, S, .], and
    predict decodes every prefix of every session -- prediction_ids [B, S, max_query_len]."""

    def _network_class(self):
        if self.type != "HREDQS":
            raise RuntimeError("Unsupported model: %s (SessionRecommender builds HREDQS; Recommender builds %s)" % (self.args.model_type, sorted(NETWORKS)))
        return HredQS

    @staticmethod
    def _rows3(t):
        return t

    @staticmethod
    def _rows2(t):
        return t

    def predict_beam(self, ex, beam_size):
        raise NotImplementedError("SessionRecommender.predict_beam: HredQS's beam search is predict_session_nbest(ex, beam_size) -- its outputs keep "
                                  "the session axis and there are no attentions (DESIGN.md section 25)")

    def predict_nbest(self, ex, beam_size):
        raise NotImplementedError("SessionRecommender.predict_nbest: the n-best suggestions of HredQS are predict_session_nbest(ex, beam_size) -- one "
                                  "list per session prefix, [B, S, W, max_query_len] (DESIGN.md section 25)")

    def predict_samples(self, ex, num_samples, temperature=1.0, top_k=0, seed=None):
        raise NotImplementedError("SessionRecommender.predict_samples: sampling for HredQS is predict_session_samples(ex, num_samples, ...) -- its "
                                  "outputs keep the session axis, [B, S, N, max_query_len], and there are no attentions (the rules of DESIGN.md "
                                  "section 28, built behind the decoder without attention in section 29)")

    _TEXT_FIELDS = ("ids", "source_tokens", "target_tokens")
    _NBEST_AXIS = 2

    @torch.no_grad()
    def predict_session_samples(self, ex, num_samples, temperature=1.0, top_k=0, seed=None):
        """`num_samples` i.i.d. suggestions per session prefix drawn from the model (HredQS.decode_sample; the reference has no counterpart):
        {'prediction_ids': LongTensor [B, S, N, max_query_len], 'token_logprobs': [B, S, N, max_query_len], 'scores': [B, S, N], 'lengths':
        LongTensor [B, S, N], 'seed': the seed used}, in sample order (not sorted, duplicates possible); for a batch in the reference's collate
        layout also predict()'s step-major `ex_ids`, `targets`, `src_sequences` and `predictions`: per prefix the list of its N strings.
        seed=None draws a 63-bit seed from torch's default CPU generator (no device synchronisation); calling again with the returned 'seed'
        replays the draw bit for bit.  Always eager: the seed is a host argument of the C entry, so a captured graph would replay one draw."""
        return self._samples(ex, self.network.decode_sample, num_samples, temperature, top_k, seed)

    @torch.no_grad()
    def predict_session_nbest(self, ex, beam_size):
        """n-best suggestions per session prefix by beam search (HredQS.decode_beam; the reference has no counterpart): {'prediction_ids':
        LongTensor [B, S, W, max_query_len], 'scores': [B, S, W], 'lengths': LongTensor [B, S, W]}, best beam first; for a batch in the
        reference's collate layout also predict()'s step-major `ex_ids`, `targets`, `src_sequences` and `predictions`: per prefix the list of
        its W strings.  There are no attentions, so no <unk> is replaced.  `beam_size` is an argument of the call, not a field of args.  Graph
        replay as in predict(): the width is part of the graph's key."""
        W = int(beam_size)
        if not 1 <= W <= lib.BEAM_MAX_W:
            raise ValueError("predict_session_nbest: beam_size %d outside [1, %d]" % (W, lib.BEAM_MAX_W))
        return self._nbest(ex, W, "decode_session_nbest%d")

    def _predict_body(self, ex):
        self.network.eval()
        dec = self.network.decode(source_rep=self._dev(ex["source_words"]), source_len=self._dev(ex["source_lens"]), max_len=self.args.max_query_len,
                                  src_dict=self.src_dict, tgt_dict=self.tgt_dict, src_map=None, alignment=None, blank=None, fill=None,
                                  source_vocabs=ex.get("src_vocab") if isinstance(ex, dict) else None)
        self._maybe_check_ids()
        return {"prediction_ids": dec["predictions"]}

    @torch.no_grad()
    def predict(self, ex):
        """models/recommender.py:233-329: {'prediction_ids': LongTensor [B, S, max_query_len] (target-vocabulary ids)}; for a batch in the
        reference's collate layout (`ids`, `source_tokens`, `target_tokens`) also the reference's `ex_ids`, `predictions`, `targets` and
        `src_sequences`, step-major (index s B + b).  There are no attentions, so no <unk> is replaced.  From the
        `predict_graph_min_calls`-th call of a batch shape on, the call replays a captured hipGraph (WrapperBase._graphed)."""
        return super().predict(ex)

    def _text(self, ex, pred_ids, attns=None):
        """the host-side tail of the reference's predict for HREDQS (models/recommender.py:310-327; tens2sen: utils/misc.py:36-62).  The one
        place predict synchronises."""
        host = pred_ids.cpu().tolist()                                     # [B][S][max_len]
        self._poll_ids()
        words, nw = self.tgt_dict, (len(self.tgt_dict) if self.tgt_dict is not None else 0)
        B, S = len(host), (len(host[0]) if host else 0)
        out = {"ex_ids": [_id + str(i) for i in range(S) for _id in ex["ids"]], "predictions": [], "targets": [], "src_sequences": []}
        for s in range(S):
            for b in range(B):
                sent = []
                for wd in host[b][s]:
                    if wd == BOS:
                        continue
                    if wd == EOS:
                        break
                    sent.append(words[wd] if (words is not None and wd < nw) else str(wd))
                out["predictions"].append(" ".join(sent) if sent else str(PAD))
                out["targets"].append([" ".join(ex["target_tokens"][b][s][1:-1])])
                out["src_sequences"].append(" ".join(" ".join(q[1:-1]) for q in ex["source_tokens"][b][0:s + 1]))
        return out


class CopyRecommender(Recommender):
    """The same wrapper for ACG (models/recommender.py:168-179,243-258,294-309): update(ex) and predict(ex) take the reference's collate
    layout with `src_map` and `alignment` (lists of per-row index tensors) and `src_vocab` (the rows' dynamic dictionaries).  The dense one-hot
    of make_src_map is never built: the lists become index tensors on the host, once per batch.  prediction_ids are EXTENDED ids."""

    def _network_class(self):
        if self.type != "ACG":
            raise RuntimeError("Unsupported model: %s (CopyRecommender builds ACG; Recommender builds %s)" % (self.args.model_type, sorted(NETWORKS)))
        return GRU_NETWORKS["ACG"] if getattr(self.args, "rnn_type", "LSTM") == "GRU" else ACG

    @staticmethod
    def _rows_of(lists, width):
        out = torch.zeros(len(lists), width, dtype=torch.int64)
        for b, row in enumerate(lists):
            row = torch.as_tensor(row).long().reshape(-1)[:width]
            out[b, :row.numel()] = row
        return out

    def _update_body(self, ex):
        from .. import autograd as A
        if "src_map" not in ex or "alignment" not in ex:
            raise AssertionError("ACG.update needs ex['src_map'] and ex['alignment'] (models/recommender.py:171)")
        self.network.train()
        A.STEP.begin()
        try:
            src, tgt, seq = (self._dev(self._rows3(ex[k])) for k in ("source_words", "target_words", "target_seq"))
            sl, tl = (self._dev(self._rows2(ex[k])) for k in ("source_lens", "target_lens"))
            smap = ex["src_map"] if torch.is_tensor(ex["src_map"]) else self._rows_of(ex["src_map"], src.shape[1])
            al = ex["alignment"] if torch.is_tensor(ex["alignment"]) else self._rows_of(ex["alignment"], seq.shape[1])     # utils/copy_utils.py:42-48
            loss = self.network(source_rep=src, source_len=sl, target_rep=tgt, target_len=tl, target_seq=seq, source_map=self._dev(smap),
                                alignment=self._dev(al))
            loss.backward()
        except BaseException:
            A.STEP.abort()
            raise
        A.STEP.end()
        self.sync_gradients()
        torch.nn.utils.clip_grad_norm_(self.network.parameters(), self.args.grad_clipping)
        self.optimizer.step()
        torch.autograd.graph.increment_version([p for g in self.optimizer.param_groups for p in g["params"]])       # (see Recommender._update_body)
        return loss

    # ---- prediction -------------------------------------------------------------------------------------------------------------------
    _FIELDS = ("source_words", "source_lens", "copy_src_map_idx", "copy_ext2tgt", "copy_ext2src")

    def _copy_fields(self, ex):
        """ex + the three index tensors of ACG.decode (CPU): CV is padded to QL + 2 when every row's dictionary fits -- the reference's loader
        always does: a dictionary holds the four specials and the row's words, <s> and </s> among them -- so that a batch shape has ONE
        graph shape and the tensors are static inputs of the predict graph: every replay gathers THIS batch's maps."""
        if all(k in ex for k in self._FIELDS[2:]):
            return ex
        if "src_map" not in ex or "src_vocab" not in ex:
            raise AssertionError("ACG.predict needs ex['src_map'] and ex['src_vocab'] (models/recommender.py:247-258)")
        QL = self._rows3(ex["source_words"]).shape[1]
        widest = max(len(v) for v in ex["src_vocab"])
        idx, e2t, e2s = self.network.copy_index(QL, ex["src_map"], None, None, ex["src_vocab"], self.src_dict, self.tgt_dict,
                                                CV=max(QL + 2, widest))
        out = dict(ex)
        out.update(copy_src_map_idx=idx, copy_ext2tgt=e2t, copy_ext2src=e2s)
        return out

    def _decode_kw(self, ex):
        """Recommender's + the three copy maps of _copy_fields"""
        return dict(super()._decode_kw(ex), src_map_idx=self._dev(ex["copy_src_map_idx"]), ext2tgt=self._dev(ex["copy_ext2tgt"]),
                    ext2src=self._dev(ex["copy_ext2src"]))

    def _predict_body(self, ex):
        self.network.eval()
        dec = self.network.decode(**self._decode_kw(ex))
        self._maybe_check_ids()
        return {"prediction_ids": dec["predictions"], "attentions": dec["attentions"]}

    _predict_nbest_body = Recommender._predict_beam_body                      # (ACG's n-best body under the name of its call)

    @torch.no_grad()
    def predict(self, ex):
        """models/recommender.py:233-329: {'prediction_ids': LongTensor [B, max_query_len] (EXTENDED ids: from len(tgt_dict) on, slot
        id - len(tgt_dict) of the row's `src_vocab`), 'attentions': [B, max_query_len, QL]}; for a full collate batch also `ex_ids`,
        `predictions` (strings; copied words come from the row's dictionary, a remaining <unk> is replaced by the most attended source token),
        `targets`, `src_sequences`.  Graph replay as in Recommender.predict; the copy maps are inputs of the graph."""
        return super().predict(self._copy_fields(ex))

    def predict_beam(self, ex, beam_size):
        raise NotImplementedError("CopyRecommender.predict_beam: ACG's beam search is predict_nbest(ex, beam_size) -- its ids are EXTENDED ids and its "
                                  "batches carry the copy maps (DESIGN.md section 24)")

    def score(self, ex, candidates=None, length_normalize=False):
        raise NotImplementedError("CopyRecommender.score: the likelihood of a candidate under ACG is a sum over its collapsed extended distribution "
                                  "(generator mass + copy mass per token), not the generator's alone -- scoring it is score_extended(ex, "
                                  "candidates) over EXTENDED ids (DESIGN.md section 31)")

    @torch.no_grad()
    def score_extended(self, ex, candidates=None, length_normalize=False):
        """Teacher-forced log-likelihood under ACG's collapsed extended distribution (ACG.score_extended), by
        Recommender.score's contract -> {'token_logprobs', 'scores', 'lengths'}.
        candidates=None: the batch's own target, as the EXTENDED ids under which the loss finds every gold token (extended_targets of
        `target_seq` and `alignment`), fed `target_words`; additionally 'nll' = -mean over rows of `scores` -- the reference forward's loss in
        eval mode without force_copy, up to the criterion's 1e-20 -- and 'perplexity' = exp(-sum scores / sum lengths).
        With candidates -- a LongTensor [B, N, TL] of EXTENDED ids, BOS first, or ex['candidate_seq'] (then with ex['candidate_rep'] as the ids
        fed to the decoder where given; candidates passed explicitly are fed the default inputs) -- additionally 'ranking' [B, N] as in score().  The copy maps are predict()'s (_copy_fields).  Eager."""
        from ..recommender.acg import extended_targets
        ex = self._copy_fields(ex)
        self._poll_ids()
        self.network.eval()
        src, sl = self._dev(self._rows3(ex["source_words"])), self._dev(self._rows2(ex["source_lens"]))
        own = candidates is None and "candidate_seq" not in ex
        if own:
            if "alignment" not in ex:
                raise AssertionError("CopyRecommender.score_extended needs ex['alignment'] to score the batch's own target")
            seq = self._rows3(ex["target_seq"])
            al = ex["alignment"] if torch.is_tensor(ex["alignment"]) else self._rows_of(ex["alignment"], seq.shape[1])
            cand = extended_targets(seq, al, self.network.generator.weight.shape[0]).unsqueeze(-2)
            rep = self._rows3(ex["target_words"]).unsqueeze(-2)
        else:
            cand = ex["candidate_seq"] if candidates is None else candidates
            rep = ex.get("candidate_rep") if candidates is None else None      # the batch's inputs belong to the batch's candidates only
        out = self.network.score_extended(source_rep=src, source_len=sl, candidate_seq=self._dev(cand),
                                          candidate_rep=self._dev(rep) if rep is not None else None, src_dict=self.src_dict, tgt_dict=self.tgt_dict,
                                          src_map_idx=self._dev(ex["copy_src_map_idx"]), ext2tgt=self._dev(ex["copy_ext2tgt"]),
                                          ext2src=self._dev(ex["copy_ext2src"]))
        self._maybe_check_ids()
        return self._score_summary(out, own, length_normalize)

    def predict_samples(self, ex, num_samples, temperature=1.0, top_k=0, seed=None):
        raise NotImplementedError("CopyRecommender.predict_samples: a draw under ACG comes from its collapsed extended distribution (generator mass "
                                  "+ copy mass per token), not from the generator's softmax alone as in DESIGN.md section 28 -- sampling it is "
                                  "sample_extended(ex, num_samples, ...) over EXTENDED ids (DESIGN.md section 33)")

    @torch.no_grad()
    def sample_extended(self, ex, num_samples, temperature=1.0, top_k=0, seed=None):
        """`num_samples` i.i.d. suggestions per row drawn from ACG's collapsed extended distribution (ACG.sample_extended),
        by Recommender.predict_samples' contract: {'prediction_ids': LongTensor [B, N, max_query_len] (EXTENDED ids), 'token_logprobs',
        'scores', 'lengths', 'attentions', 'seed': the seed used}, in sample order; for a full collate batch also `ex_ids`, `targets`,
        `src_sequences` and `predictions`: per row the list of its N strings, each formed like predict()'s (copied words come from the row's
        dictionary).  seed=None draws 63 bits from torch's default CPU generator; calling again with the returned 'seed' replays the draw bit
        for bit.  The copy maps are predict()'s (_copy_fields).  Always eager: the seed is a host argument of the C entry."""
        return self._samples(self._copy_fields(ex), self.network.sample_extended, num_samples, temperature, top_k, seed)

    @torch.no_grad()
    def predict_nbest(self, ex, beam_size):
        """n-best suggestions by beam search over the collapsed extended distribution (ACG.decode_beam; the reference has no counterpart):
        {'prediction_ids': LongTensor [B, W, max_query_len] (EXTENDED ids), 'scores': [B, W], 'lengths': LongTensor [B, W], 'attentions':
        [B, W, max_query_len, QL]}, best beam first; for a full collate batch also `ex_ids`, `targets`, `src_sequences` and `predictions`: per
        row the list of its W strings, each formed like predict()'s (copied words come from the row's dictionary).  Graph replay as in
        predict(): the width is part of the graph's key, the three copy maps are inputs of the graph."""
        return self._nbest(self._copy_fields(ex), int(beam_size), "decode_nbest%d")

    def _text(self, ex, pred_ids, attns):
        """tens2sen with the rows' dictionaries (utils/misc.py:36-62) + replace_unknown"""
        host, att = pred_ids.cpu().tolist(), attns.cpu()
        self._poll_ids()
        words, nw = self.tgt_dict, len(self.tgt_dict)
        preds = []
        for b, row in enumerate(host):
            sent = []
            for wd in row:
                if wd == BOS:
                    continue
                if wd == EOS:
                    break
                sent.append(words[wd] if wd < nw else ex["src_vocab"][b][wd - nw])
            if not sent:
                sent = [str(PAD)]
            src_raw = ex["source_tokens"][b][0]
            for i, tok in enumerate(sent):
                if tok == UNK_WORD:
                    sent[i] = src_raw[int(att[b, i].argmax())]
            preds.append(" ".join(sent))
        return {"ex_ids": ex["ids"], "predictions": preds,
                "targets": [[" ".join(q[1:-1]) for q in item] for item in ex["target_tokens"]],
                "src_sequences": [[" ".join(q[1:-1]) for q in session] for session in ex["source_tokens"]]}
