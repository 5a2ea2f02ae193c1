"""ACG -- Seq2seq with a copy generator (drop-in for neuroir.recommender.seq2seq.Seq2seq built with copy_attn=True,
/root/reference/neuroir/recommender/seq2seq.py:13-195; modules/copy_generator.py; utils/copy_utils.py).

The network is Seq2seq's; what the copy generator changes is the choice of the next token (decode) and the loss (forward):

decode():  the extended distribution over the VT target words and the CV words of every row's own dynamic dictionary is never written.  ONE
           C-ABI call (nir_acg_decode_greedy, csrc/acg.hip) runs the Seq2seq step and, in two launches more, the copy generator's arg-max.
           The reference's dense one-hot `src_map` [B, QL, CV] and its per-row host loop over `blank` / `fill` become three index tensors:
             src_map_idx [B, QL]   dictionary slot of every source position
             ext2tgt     [B, CV]   target id of a slot's word, -1 where the slot is not collapsed (slots 0 and 1 never are)
             ext2src     [B, CV]   source id of a slot's word (the token fed back when the slot wins)
           decode() takes them directly, or converts the reference's arguments once on the host.  `predictions` are EXTENDED ids in
           [0, VT + CV), as in the reference.
decode_beam(): beam search over the COLLAPSED extended distribution (include/neuroir_acg_beam.h): per beam row the W
           best entries come out of the generator's top-W, its softmax pair and at most CV further candidates (csrc/beam.hip); a slot that
           collapses onto a target word is no candidate of its own.  The same index tensors, not repeated over the beams.
score_extended(): the teacher-forced log-probability of given EXTENDED ids under that same collapsed distribution (include/neuroir_acg_score.h,
           DESIGN.md section 31): ONE grouped attention over all rows, ONE generator call that keeps the logits on chip and gathers each row's
           copy mass; extended_targets() gives the id under which the loss finds a gold token.
forward(): the teacher-forced loss of CopyGeneratorCriterion on the differentiable HIP operators of autograd.py (the [B, TL, QL] gather of
           the copy mass and the [B, TL] switch logit are tensor glue).

State dict: the reference's keys -- `copy_generator.linear.*` is the generator itself under a second name (one parameter, two keys),
`copy_generator.linear_copy.*` the switch, `decoder.decoder.copy_attn.*` a second attention when reuse_copy_attn is off (its linear_out is
loaded and given back but takes no part in any value, as in the reference).

Kept quirks: Seq2seq's (see seq2seq.py), and the PAD logit: the reference overwrites it with -1e-20 behind the generator
(copy_generator.py:79), so PAD takes part in the softmax as a logit of about zero and no gradient reaches the generator through it.
"""
import torch
import torch.nn as nn

from .. import autograd as A
from .. import lib
from ..constants import BOS, EOS, PAD, UNK
from ..multitask import suggest
from .layers import CopyGeneratorParams
from .seq2seq import Seq2seq, build_network, check_supported


def src_map_index(src_map, QL, device=None):
    """the reference's `src_map` -> LongTensor [B, QL]: a list of per-row index tensors (the collate layout, what make_src_map reads), the dense
    one-hot [B, QL', CV] make_src_map builds, or the index tensor itself.  Positions past a row's entries get slot 0 (they lie past its
    length and are never read)."""
    if torch.is_tensor(src_map) and not src_map.is_floating_point() and src_map.dim() == 2:
        idx = src_map.long()
    elif torch.is_tensor(src_map):
        if src_map.dim() != 3:
            raise ValueError("src_map: expected [B, QL, CV] one-hot or [B, QL] indices, got %s" % (tuple(src_map.shape),))
        idx = src_map.argmax(2)
    else:
        idx = torch.zeros(len(src_map), QL, dtype=torch.int64)
        for b, row in enumerate(src_map):
            row = torch.as_tensor(row).long().reshape(-1)[:QL]
            idx[b, :row.numel()] = row
    if idx.shape[1] < QL:
        idx = torch.nn.functional.pad(idx, (0, QL - idx.shape[1]))
    idx = idx[:, :QL].contiguous()
    return idx.to(device) if device is not None else idx


def collapse_index(blank, fill, VT, CV):
    """collapse_copy_scores' (blank, fill) lists -> ext2tgt LongTensor [B, CV] (CPU): ext2tgt[b, blank - VT] = fill, -1 elsewhere"""
    e2t = torch.full((len(blank), CV), -1, dtype=torch.int64)
    for b, (bl, fl) in enumerate(zip(blank, fill)):
        for x, t in zip(bl, fl):
            c = int(x) - VT
            if c < 2 or c >= CV:
                raise ValueError("blank index %d of row %d is outside the row's dictionary [VT + 2, VT + %d)" % (int(x), b, CV))
            e2t[b, c] = int(t)
    return e2t


def vocab_index(source_vocabs, src_dict, tgt_dict, CV=None):
    """the rows' dynamic dictionaries -> (ext2tgt, ext2src) LongTensors [B, CV] (CPU): what collapse_copy_scores (utils/copy_utils.py:5-28) and
    the reference's `src_dict[source_vocabs[b][pred - VT]]` (seq2seq.py:105-116,182-183) look up, for every slot at once.  CV defaults to the
    largest dictionary; shorter rows are padded with slots nothing maps to.  tgt_dict None: nothing is collapsed."""
    n = max(len(v) for v in source_vocabs)
    CV = n if CV is None else int(CV)
    if CV < n:
        raise ValueError("CV = %d is smaller than a row's dictionary (%d)" % (CV, n))
    e2t = torch.full((len(source_vocabs), CV), -1, dtype=torch.int64)
    e2s = torch.full((len(source_vocabs), CV), UNK, dtype=torch.int64)
    for b, vocab in enumerate(source_vocabs):
        for c in range(len(vocab)):
            word = vocab[c]
            e2s[b, c] = int(src_dict[word])
            if c >= 2 and tgt_dict is not None:
                t = int(tgt_dict[word])
                if t != UNK:
                    e2t[b, c] = t
    return e2t, e2s


def extended_targets(target_seq, alignment, VT):
    """the EXTENDED id under which CopyGeneratorCriterion (modules/copy_generator.py:91-135) finds a gold token's probability: VT + alignment
    where the target is <unk> and its alignment is not (a source word outside the target vocabulary: copy mass alone), the target itself
    elsewhere (a target word: generator mass plus the mass of its slot, which collapses onto it).  alignment is padded with 0 to the
    target's width, as forward() pads it."""
    t, al = lib.ids64(target_seq), lib.ids64(alignment).to(target_seq.device)
    if al.shape[-1] < t.shape[-1]:
        al = torch.nn.functional.pad(al, (0, t.shape[-1] - al.shape[-1]))
    al = al[..., :t.shape[-1]]
    return torch.where((t == UNK) & (al != UNK), al + int(VT), t)


class ACG(Seq2seq):
    _GREEDY_ENTRY = "nir_acg%s_decode"                   # + "_greedy" / "_workspace_bytes": nir_acg_decode_greedy, nir_acg_gru_decode_greedy
    _ACG_BEAM_ENTRY = "nir_acg_beam%s_decode"            # (+ "_workspace_bytes"): nir_acg_beam_decode, nir_acg_beam_gru_decode

    def __init__(self, args):
        nn.Module.__init__(self)
        name = type(self).__name__
        if not getattr(args, "copy_attn", False):
            raise ValueError("recommender.%s is the copy-generator model (copy_attn=True); without it build recommender.%s"
                             % (name, name.replace("ACG", "Seq2seq")))
        self.reuse_copy_attn = bool(getattr(args, "reuse_copy_attn", False))
        if args.attn_type in (None, "none"):                              # the reference's own failures (decoders/decoder.py:107-108;
            if self.reuse_copy_attn:                                      # modules/global_attention.py:64-65)
                raise RuntimeError("Attn is turned off, so reuse_copy_attn flag must be false")
            raise AssertionError("Please select a valid attention type.")
        check_supported(args, name, self._CELL)
        build_network(self, args, own_copy_attn=not self.reuse_copy_attn)
        self.copy_attn = True
        self.force_copy = bool(getattr(args, "force_copy", False))
        self.copy_generator = CopyGeneratorParams(args.nhid, self.generator)
        self._pcopy = lib.PackCache(retain=1)

    # ---- eval: greedy decode -----------------------------------------------------------------------------------------------------
    def _copy_weights(self):
        cg = self.copy_generator.linear_copy
        att = None if self.reuse_copy_attn else self.decoder.decoder.copy_attn

        def build():
            t = dict(copy_w=cg.weight.reshape(-1), copy_b=cg.bias)
            if att is not None and self.attn_type == "general":
                t["attn_in_wt"] = att.linear_in.weight.t()
            elif att is not None and self.attn_type == "mlp":
                t.update(attn_ctx_w=att.linear_context.weight, attn_query_w=att.linear_query.weight, attn_query_b=att.linear_query.bias,
                         attn_v=att.v.weight)
            return lib.Packed(lib.AcgCopyWeights, t, dict(reuse_copy_attn=int(self.reuse_copy_attn)))
        return self._pcopy.get(list(cg.parameters()) + (list(att.parameters()) if att is not None else []), build)

    def copy_index(self, QL, src_map=None, blank=None, fill=None, source_vocabs=None, src_dict=None, tgt_dict=None, CV=None):
        """the reference's decode arguments -> (src_map_idx [B,QL], ext2tgt [B,CV], ext2src [B,CV]) on the CPU, once per batch.  CV: given, else
        the width of a dense `src_map`, else the largest dictionary.  `blank` / `fill`, when given, decide what is collapsed (they are what the
        reference's decode reads); otherwise collapse_copy_scores is applied to the dictionaries here."""
        if src_map is None or source_vocabs is None or src_dict is None:
            raise NotImplementedError("ACG.decode needs src_map, source_vocabs and src_dict (seq2seq.py:105-116), or the three index tensors")
        VT = self.generator.weight.shape[0]
        idx = src_map_index(src_map, QL)
        if CV is None and torch.is_tensor(src_map) and src_map.dim() == 3:
            CV = max(int(src_map.shape[2]), max(len(v) for v in source_vocabs))
        e2t, e2s = vocab_index(source_vocabs, src_dict, tgt_dict if blank is None else None, CV)
        if blank is not None:
            e2t = collapse_index(blank, fill, VT, e2t.shape[1])
        return idx, e2t, e2s

    @torch.no_grad()
    def decode(self, source_rep, source_len, max_len, src_dict, tgt_dict, src_map=None, alignment=None, blank=None, fill=None,
               source_vocabs=None, tgt2src=None, src_map_idx=None, ext2tgt=None, ext2src=None):
        """seq2seq.py:118-195 (greedy) -> {'predictions': LongTensor [B, max_len] (EXTENDED ids: below VT a target word, from VT on slot
        pred - VT of the row's dynamic dictionary), 'attentions': [B, max_len, QL] (the decoder's own attention)}.  The copy inputs are the
        reference's (`src_map` as a list of index tensors or the dense one-hot, `blank` / `fill`, `source_vocabs`) or the three index
        tensors (module docstring); `alignment` is unused, as in the reference's decode."""
        return self._greedy(source_rep, source_len, max_len, src_dict, tgt_dict, tgt2src,
                            extra=self._copy_extra("decode", src_dict, tgt_dict, src_map, blank, fill, source_vocabs, src_map_idx, ext2tgt, ext2src))

    def _copy_maps(self, what, B, QL, src_dict, tgt_dict, src_map, blank, fill, source_vocabs, src_map_idx, ext2tgt, ext2src):
        """the copy inputs of `what` (a method's name, for the messages) -> (src_map_idx [B, QL], ext2tgt [B, CV], ext2src [B, CV], CV) as int64 on
        the model's device: the three index tensors where all are given, else copy_index of the reference's arguments; their shapes and the copy
        generator's range are checked here"""
        maps = (src_map_idx, ext2tgt, ext2src)
        if any(t is None for t in maps):
            maps = self.copy_index(QL, src_map, blank, fill, source_vocabs, src_dict, tgt_dict)
        dev = self.embedder.word_embeddings.table.device
        idx, e2t, e2s = (lib.ids64(t).to(dev).contiguous() for t in maps)
        CV = int(e2t.shape[1])
        name = type(self).__name__
        if tuple(idx.shape) != (B, QL) or tuple(e2t.shape) != (B, CV) or tuple(e2s.shape) != (B, CV):
            raise ValueError("%s.%s: src_map_idx %s, ext2tgt %s, ext2src %s do not fit %d rows of width %d"
                             % (name, what, tuple(idx.shape), tuple(e2t.shape), tuple(e2s.shape), B, QL))
        if not (1 <= QL <= 4096 and 2 <= CV <= 1024):
            raise ValueError("%s.%s: QL = %d / CV = %d outside the copy generator's range (QL <= 4096, 2 <= CV <= 1024)" % (name, what, QL, CV))
        return idx, e2t, e2s, CV

    def _copy_extra(self, what, *copy_inputs):
        """_copy_maps' arguments behind B and QL -> the `extra` of Seq2seq._greedy / _beam / _sample: (B, QL) -> ((CV,), the copy arguments of the
        C entries); what the pointers refer to stays alive with the function"""
        keep = []

        def extra(B, QL):
            idx, e2t, e2s, CV = self._copy_maps(what, B, QL, *copy_inputs)
            cw = self._copy_weights()
            keep.extend((idx, e2t, e2s, cw))                               # alive until the call is enqueued
            return (CV,), (cw.ref(), lib.ptr(idx), lib.ptr(e2t), lib.ptr(e2s), CV)
        return extra

    # ---- eval: scoring -------------------------------------------------------------------------------------------------------------
    def score_candidates(self, *args, **kwargs):
        """not Seq2seq's: a token's likelihood under ACG is generator mass plus copy mass of the collapsed extended distribution, not the
        generator's softmax alone; candidates of EXTENDED ids are scored by score_extended"""
        raise NotImplementedError("HIP %s.score_candidates: scoring under the copy generator's collapsed extended distribution is not built yet "
                                  "for target-vocabulary ids (the generator's log-likelihood alone would be another model's); candidates of "
                                  "EXTENDED ids, with the copy maps of decode(), are scored by score_extended" % type(self).__name__)

    # score_extended: ONE nir_tf_attend over all teacher-forced rows for attn_type dot / general.  False: the tensor-glue front forward() composes
    # (what attn_type mlp always takes) -- for tests and tools
    fuse_teacher_front = True

    def _extended_inputs(self, cand, tgt2src, e2s, VT, V):
        """the embedder ids the ACG decodes feed back for candidates of EXTENDED ids [B, N, TL]: the first token as it is, tgt2src[e] below VT (e
        itself without a table), ext2src[b, e - VT] from VT on, <unk> outside [0, V)"""
        B, N, _ = cand.shape
        CV = e2s.shape[1]
        low = cand.clamp(0, VT - 1)
        word_src = low if tgt2src is None else tgt2src[low]
        ext = e2s.unsqueeze(1).expand(B, N, CV).gather(2, (cand - VT).clamp(0, CV - 1))
        rep = torch.cat((cand[..., :1], torch.where(cand < VT, word_src, ext)[..., 1:]), -1)
        return torch.where((rep >= 0) & (rep < V), rep, torch.full_like(rep, UNK))

    def _teacher_front(self, h_all, bank, lens, B, G, w):
        """h_all [B G, H]: the decoder states of the teacher-forced steps, rows (b, n, t), G = N (TL-1) per source row -> (the attentional
        outputs [B G, H], the copy attention [B G, QL], exact 0 past the length).  dot / general: ONE nir_tf_attend with the attention output
        requested -- no [B, G, QL, H] intermediate; mlp, and fuse_teacher_front off: _align and a masked softmax, as forward() composes them.  A
        copy attention of its own: _align with the attentional output as the query."""
        att = self.decoder.decoder.attn
        QL, H = int(bank.shape[1]), int(bank.shape[2])
        R, dev, mlp = B * G, bank.device, self.attn_type == "mlp"
        mask = torch.arange(QL, device=dev).unsqueeze(0) < lens.unsqueeze(1)

        def attention(align):
            return torch.softmax(align.masked_fill(~mask.unsqueeze(1), float("-inf")), -1).reshape(R, QL)
        if mlp or not self.fuse_teacher_front:
            align = self._align(h_all.view(B, G, H), bank)
            ctx = A.softmax_pool(align, mask, bank, mask_div=G).view(B, G, -1)
            cat, a_std = torch.cat((ctx, h_all.view(B, G, H)), 2).reshape(R, 2 * H), attention(align)
        else:
            L = lib.load()
            sbank = bank if self.attn_type == "dot" else A.linear(bank, w.keep["attn_in_wt"]).contiguous()     # score_j = (W_in h) . m_j = h . (W_in^T m_j)
            cat = torch.empty(R, 2 * H, device=dev, dtype=torch.float32)
            a_std = torch.empty(R, QL, device=dev, dtype=torch.float32)
            if R > 0:
                ws = lib.workspace(L.nir_tf_attend_workspace_bytes(B, G, QL, H), dev)
                lib.check(L.nir_tf_attend(lib.ptr(h_all), lib.ptr(bank), lib.ptr(sbank), lib.ptr(lens), None, B, G, B, QL, H, lib.ptr(cat), lib.ptr(a_std),
                                          QL, lib.ptr(ws), ws.numel(), lib.stream()), "nir_tf_attend")
        dec_out = A.linear(cat, att.linear_out.weight, att.linear_out.bias if mlp else None, act=None if mlp else "tanh")
        if self.reuse_copy_attn:
            return dec_out, a_std
        return dec_out, attention(self._align(dec_out.view(B, G, H), bank, self.decoder.decoder.copy_attn))

    @torch.no_grad()
    def score_extended(self, source_rep, source_len, candidate_seq, candidate_rep=None, src_dict=None, tgt_dict=None, tgt2src=None, src_map=None,
                       blank=None, fill=None, source_vocabs=None, src_map_idx=None, ext2tgt=None, ext2src=None):
        """log P(candidate | source) under the COLLAPSED extended distribution decode() and decode_beam() choose from (include/neuroir_acg_score.h,
        DESIGN.md section 31; the reference has no scorer).  candidate_seq [B, N, TL]: EXTENDED ids in [0, VT + CV) -- what the decodes emit --,
        BOS first, PAD behind the end; candidate_rep [B, N, TL]: the embedder ids fed to the decoder (default: what the decodes feed back, so that
        [BOS] + decode_beam(..)['predictions'] reproduces the beam's scores and lengths).  The copy inputs are decode()'s.
        -> {'token_logprobs': [B, N, TL - 1] (step t against token t + 1; 0 at PAD, behind the first EOS and for an id outside [0, VT + CV);
        -inf for an id without mass), 'scores': [B, N], 'lengths': LongTensor [B, N]}.  A slot that collapses onto a target word is scored as
        that word.  `force_copy` is a loss option and takes no part, as in the decodes."""
        return self._score_extended_rows(*self._extended_front(source_rep, source_len, candidate_seq, candidate_rep, src_dict, tgt_dict, tgt2src, src_map,
                                                               blank, fill, source_vocabs, src_map_idx, ext2tgt, ext2src))

    def _extended_front(self, source_rep, source_len, candidate_seq, candidate_rep, src_dict, tgt_dict, tgt2src, src_map, blank, fill, source_vocabs,
                        src_map_idx, ext2tgt, ext2src):
        """score_extended in front of the generator: the checks, the copy maps, the encoder, the default decoder inputs, the decoder's cell over all
        B N sequences and _teacher_front -> the arguments of _score_extended_rows"""
        cand = lib.ids64(candidate_seq)
        if cand.dim() != 3 or cand.shape[0] != source_rep.shape[0] or cand.shape[2] < 2:
            raise ValueError("score_extended: candidate_seq must be [B, N, TL] with TL >= 2 (got %s)" % (tuple(cand.shape),))
        if candidate_rep is not None and candidate_rep.numel() != cand.numel():
            raise ValueError("score_extended: candidate_rep %s does not match candidate_seq %s" % (tuple(candidate_rep.shape), tuple(cand.shape)))
        B, QL, table = self._decode_ready("score_extended", source_rep, source_len)
        lib.require_device(cand, candidate_rep)
        idx, e2t, e2s, _ = self._copy_maps("score_extended", B, QL, src_dict, tgt_dict, src_map, blank, fill, source_vocabs, src_map_idx, ext2tgt, ext2src)
        dev = table.device
        N, T = int(cand.shape[1]), int(cand.shape[2]) - 1
        lens, state, bank = self._encoded(source_rep, source_len, table)
        w = self._decoder_weights()
        VT, H = int(w.struct.VT), int(bank.shape[2])
        if candidate_rep is not None:
            rep = self._clean_ids(candidate_rep.reshape(cand.shape), None, table.shape[0])[0]
        else:
            if tgt2src is None:
                tgt2src = suggest.tgt2src_lut(self, src_dict, tgt_dict, VT, dev)
            rep = self._extended_inputs(cand, tgt2src, e2s, VT, table.shape[0])
        R = B * N * T
        temb = A.embed(rep[:, :, :-1].reshape(B * N, T), table)
        h_all = self._cell_train(temb, [s.repeat_interleave(N, 0).contiguous() for s in state]).reshape(R, H).float().contiguous()   # rows (b, n, t)
        dec_out, a_copy = self._teacher_front(h_all, bank, lens, B, N * T, w)
        return dec_out.reshape(R, H).float().contiguous(), a_copy.float().contiguous(), cand, lens, idx, e2t, w

    def _score_extended_rows(self, dec_out, a_copy, cand, lens, idx, e2t, w):
        """the tail of score_extended: dec_out [B N (TL-1), H] and the copy attention [B N (TL-1), QL] of the teacher-forced rows, rows (b, n, t)
        -> ONE nir_acg_score_gen_target over all rows (the fused form where the packed weights hold the generator fragment) and one
        nir_score_sequences"""
        L = lib.load()
        B, N, T = int(cand.shape[0]), int(cand.shape[1]), int(cand.shape[2]) - 1
        R, H, QL, CV, VT, dev = dec_out.shape[0], dec_out.shape[1], int(idx.shape[1]), int(e2t.shape[1]), int(w.struct.VT), dec_out.device
        target = cand[..., 1:].reshape(-1).contiguous()
        logp = torch.empty(R, dtype=torch.float32, device=dev)
        scores = torch.empty(B * N, dtype=torch.float32, device=dev)
        lengths = torch.empty(B * N, dtype=torch.int64, device=dev)
        if R > 0:
            cw, frag = self._copy_weights(), w.keep.get("gen_frag")
            ws = lib.workspace(L.nir_acg_score_gen_target_workspace_bytes(R, H, VT, 1 if frag is not None else 0), dev)
            lib.check(L.nir_acg_score_gen_target(lib.ptr(dec_out), R, N * T, H, lib.ptr(w.keep["gen_w"]), lib.ptr(w.keep["gen_b"]), lib.ptr(frag), VT,
                                                 lib.ptr(cw.keep["copy_w"]), lib.ptr(cw.keep["copy_b"]), lib.ptr(a_copy), QL, lib.ptr(lens), QL,
                                                 lib.ptr(idx), lib.ptr(e2t), CV, lib.ptr(target), PAD, lib.ptr(ws), ws.numel(), lib.ptr(logp),
                                                 lib.ptr(self._flag_word(dev)), lib.stream()), "nir_acg_score_gen_target")
            lib.check(L.nir_score_sequences(lib.ptr(logp), lib.ptr(target), B * N, T, PAD, EOS, lib.ptr(scores), lib.ptr(lengths), lib.stream()),
                      "nir_score_sequences")
        return {"token_logprobs": logp.view(B, N, T), "scores": scores.view(B, N), "lengths": lengths.view(B, N)}

    # ---- eval: sampling ------------------------------------------------------------------------------------------------------------
    def decode_sample(self, *args, **kwargs):
        """not Seq2seq's: ACG's next-token distribution is the collapsed extended one (generator mass plus copy mass), which the generator's
        Gumbel arg-max does not draw from; the draw over EXTENDED ids, with the copy maps of decode(), is sample_extended"""
        raise NotImplementedError("HIP %s.decode_sample: a draw from the generator's softmax alone would be another model's; sampling from the copy "
                                  "generator's collapsed extended distribution, over EXTENDED ids and with the copy maps of decode(), is "
                                  "sample_extended" % type(self).__name__)

    _ACG_SAMPLE_ENTRY = "nir_acg_sample%s_decode"        # (+ "_workspace_bytes"): nir_acg_sample_decode, nir_acg_sample_gru_decode

    @torch.no_grad()
    def sample_extended(self, source_rep, source_len, max_len, num_samples, temperature=1.0, top_k=0, seed=0, src_dict=None, tgt_dict=None,
                        src_map=None, blank=None, fill=None, source_vocabs=None, tgt2src=None, src_map_idx=None, ext2tgt=None, ext2src=None):
        """`num_samples` i.i.d. draws per source row from the COLLAPSED extended distribution decode() and decode_beam() choose from, at
        `temperature`, over all of it (top_k = 0) or restricted to each step's top_k most probable entries (1 .. lib.BEAM_MAX_W, at most VT;
        top_k = 1 is decode()), over max_len steps with no early stop (include/neuroir_acg_sample.h; the reference has no
        sampler) -> Seq2seq.decode_sample's dict with EXTENDED ids in 'predictions' [B, N, max_len]: below VT a target word, from VT on slot
        id - VT of the row's dynamic dictionary; a slot that collapses onto a target word is never drawn, its mass is part of the word's.
        'token_logprobs' is log P(token) at temperature 1 over the full collapsed distribution whatever temperature and top_k are, so
        score_extended([BOS] + predictions) reproduces 'scores' and 'lengths' (for samples without PAD in front of their first EOS; PAD has
        real mass under ACG).  The noise is Seq2seq.decode_sample's, keyed by the extended id.  The copy inputs are decode()'s; neither they nor
        the memory bank are repeated.  ONE C call; neither logits nor a dense copy distribution is written (`fuse_generator_argmax = False`, and
        for top_k > 0 `fuse_generator_topk = False`: the plain generator forms; over the whole distribution the plain form is also the default
        beyond `fuse_sample_max_rows` decode rows)."""
        return self._sample("sample_extended", source_rep, source_len, max_len, num_samples, temperature, top_k, seed, src_dict, tgt_dict, tgt2src,
                            entry=self._ACG_SAMPLE_ENTRY,
                            extra=self._copy_extra("sample_extended", src_dict, tgt_dict, src_map, blank, fill, source_vocabs, src_map_idx, ext2tgt,
                                                   ext2src))

    # ---- eval: beam search ---------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode_beam(self, source_rep, source_len, max_len, beam_size, src_dict=None, tgt_dict=None, src_map=None, blank=None, fill=None,
                    source_vocabs=None, tgt2src=None, src_map_idx=None, ext2tgt=None, ext2src=None, return_backptr=False):
        """Beam search of width `beam_size` (1 .. lib.BEAM_MAX_W) over the COLLAPSED extended distribution (include/neuroir_acg_beam.h, DESIGN.md
        section 24) -> Seq2seq.decode_beam's dict with EXTENDED ids in 'predictions' [B, W, max_len]: below VT a target word, from VT on slot
        id - VT of the row's dynamic dictionary.  A word is offered once per beam: a slot that collapses onto a target word is no candidate of
        its own, its mass is part of the word's.  The copy inputs are decode()'s; neither they nor the memory bank are repeated."""
        if self.training:
            raise NotImplementedError("HIP %s.decode_beam runs in eval mode" % type(self).__name__)
        lib.require_device(source_rep, source_len, self.embedder.word_embeddings.table)
        return self._beam(source_rep, source_len, max_len, beam_size, src_dict, tgt_dict, tgt2src, return_backptr, entry=self._ACG_BEAM_ENTRY,
                          extra=self._copy_extra("decode_beam", src_dict, tgt_dict, src_map, blank, fill, source_vocabs, src_map_idx, ext2tgt, ext2src))

    # ---- train: teacher-forced loss ---------------------------------------------------------------------------------------------------
    def forward(self, source_rep, source_len, target_rep, target_len, target_seq, source_map=None, alignment=None):
        """seq2seq.py:48-103 with copy_attn -> scalar loss: CopyGeneratorCriterion on steps [:-1] against target_seq[:, 1:] and
        alignment[:, 1:], masked at PAD targets, summed over time, averaged over rows.  source_map: the reference's dense one-hot, a list of
        per-row index tensors, or the index tensor [B, QL]."""
        if source_map is None or alignment is None:
            raise ValueError("ACG.forward needs source_map and alignment (models/recommender.py:170-179)")
        B, QL = source_rep.shape
        dec_all, align, mem, mask = self._decoder_outputs(source_rep, source_len, target_rep, target_seq)
        dev = dec_all.device
        if self.reuse_copy_attn:
            scores = align
        else:                                                             # rnn_decoder.py:82-86: the query is the attentional output behind dropout
            scores = self._align(dec_all, mem, self.decoder.decoder.copy_attn)
        a_copy = torch.softmax(scores.masked_fill(~mask.unsqueeze(1), float("-inf")), -1)[:, :-1]        # [B,TL-1,QL], exact 0 past the length
        dec_out = dec_all[:, :-1]
        TL1 = dec_out.shape[1]
        target = lib.ids64(target_seq)[:, 1:]
        al = lib.ids64(alignment).to(dev)[:, 1:]
        if al.shape[1] < TL1:
            al = torch.nn.functional.pad(al, (0, TL1 - al.shape[1]))
        al = al[:, :TL1]
        idx = src_map_index(source_map, QL, dev)
        hit = (idx.unsqueeze(1) == al.unsqueeze(2)).to(a_copy.dtype)                                        # [B,TL-1,QL]
        mass = (a_copy * hit).sum(2)
        cg = self.copy_generator.linear_copy
        switch = (dec_out * cg.weight.view(1, 1, -1)).sum(2) + cg.bias
        logits = A.linear(dec_out, self.generator.weight, self.generator.bias)
        V = logits.shape[2]
        rows = A.copy_loss(logits.reshape(B * TL1, V), switch.reshape(-1), mass.reshape(-1), target.reshape(-1), al.reshape(-1), self.force_copy)
        return (rows.view(B, TL1) * (target != PAD).to(rows.dtype)).sum(1).mean()
