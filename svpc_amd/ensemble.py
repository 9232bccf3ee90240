"""Ensemble decoding: M checkpoints behind every caption decoder (OpenNMT's ``EnsembleModel`` with ``avg_raw_probs``, fairseq's ensemble
— the decode-strategy lineage the beam search was taken from).

``EnsembleTranslator(opt, checkpoints, models, weights=None, combine="prob", graph=False)`` is a ``Translator`` whose every decode —
greedy, beam with controls and n-best, paragraph scope, diverse, constrained, sampling, stochastic, consensus — and ``score_captions``
see the COMBINED per-step distribution of its M members (1 ≤ M ≤ 8) instead of one model's:

- every member runs its own encoder side once per batch and its own decoder iteration per step, on its own KV caches, all in the
  decode's one stream; the M score matrices of a step (probabilities of the pointer-generator modes, logits in ``video`` mode) go
  through ``ops.ensemble_combine`` and the step kernels take the result as a probability matrix (``logits = False``: the step score of
  a token is the log of its combined probability, UNK never a candidate);
- ``combine="prob"``: out = Σ_m w_m·p_m (``avg_raw_probs=True``); ``"logprob"``: out = exp(Σ_m w_m·log p_m), not renormalised
  (``avg_raw_probs=False``); ``weights``: M numbers ≥ 0, normalised to sum 1 (default uniform); a zero-weight member still runs (the
  graph is the same for any weights) but its scores are never read;
- under ``"prob"`` in the pointer modes M copies of one model — or any members with one weight 1 — decode bit for bit what the single
  ``Translator`` decodes;
- members must agree on ``AGREE`` (the batch structure, the score columns and the decoder's shapes); anything else may differ;
- ``incremental=False`` and ``two_streams`` are not offered; ``self.model`` is member 0, which the plans read their shapes from;
- ``graph=True`` replays the whole M-member decode as one graph; it is re-captured when any member's parameters move;
- the rule itself is one method, ``_combine`` (the decoder side and forced scoring both call it), and the clip features a member's
  encoder side reads another, ``_member_features``: svpc_amd/contrast_decode.py overrides the two for contrastive decoding.

tests/ensemble_reference.py restates the rule and the decodes on the CPU."""
from __future__ import annotations

from . import ops
from .model import _Ctx
from .synthetic import UNK
from .translator import Translator, _DecoderSide

AGREE = ("model_mode", "vocab_size", "max_t_len", "max_v_len", "max_i_len", "video_feature_size", "hidden_size", "num_hidden_layers",
         "num_attention_heads", "word_vec_size")


class _EnsembleSide(object):
    """``_DecoderSide``'s surface over the M members' sides: caches and rows per member, one combined score matrix per iteration"""

    def __init__(self, sides, combine):
        self.sides, self.combine = sides, combine                    # ``combine``: the translator's rule (``EnsembleTranslator._combine``)
        self.model, self.wide = sides[0].model, sides[0].wide        # (the loops read the config and the device from member 0)
        self.member_logits = sides[0].logits
        self.logits = False                                          # ``scores`` returns probabilities in every mode
        self.n_layers = len(sides[0].layers)
        assert all(s.n_mem == sides[0].n_mem and len(s.layers) == self.n_layers for s in sides)

    def caches(self, n_rows):
        """all members' per-layer KV caches as one flat list, member-major (the paragraph loop slices every element)"""
        return [c for s in self.sides for c in s.caches(n_rows)]

    def seq_cross(self, dp):
        return self.sides[0].seq_cross(dp)                           # (the members' memory rows per sentence agree: one segmentation)

    def rows(self, rd=None):
        return [s.rows(rd) for s in self.sides]

    def scores(self, rows, ptr, nxt, i, caches, seq_self, seq_cross, key_rows=None, group=1):
        L = self.n_layers
        mats = [s.scores(rows[m], ptr, nxt, i, caches[m * L:(m + 1) * L], seq_self, seq_cross, key_rows, group)
                for m, s in enumerate(self.sides)]
        return self.combine(mats, ptr["row_c"], self.member_logits, 1, ptr["c_max"])


class EnsembleTranslator(Translator):
    def __init__(self, opt, checkpoints, models, weights=None, combine="prob", graph=False):
        checkpoints, models = list(checkpoints), list(models)
        if not models or len(models) != len(checkpoints):
            raise ValueError("an ensemble needs one checkpoint per model and at least one member, got %d checkpoints for %d models"
                             % (len(checkpoints), len(models)))
        self.weights = ops.ensemble_weights(weights, len(models))
        if combine not in ops.ENSEMBLE_RULES:
            raise ValueError("combine must be one of %s, got %r" % (", ".join(ops.ENSEMBLE_RULES), combine))
        self.combine = combine
        self._adopt(opt, checkpoints, models, graph)

    def _adopt(self, opt, checkpoints, models, graph):
        """the members checked against ``AGREE`` and for one device, member 0 through ``Translator.__init__``, every further member
        loaded and given its weight store"""
        first = checkpoints[0]["model_cfg"]
        for m, (ck, model) in enumerate(zip(checkpoints, models)):
            for cfg in (ck["model_cfg"], model.config):
                for f in AGREE:
                    if getattr(cfg, f) != getattr(first, f):
                        raise ValueError("ensemble member %d differs from member 0 in %s: %r against %r" % (m, f, getattr(cfg, f), getattr(first, f)))
        devs = {next(model.parameters()).device for model in models}
        if len(devs) != 1:
            raise ValueError("the members of an ensemble must be on one device, got %s" % ", ".join(sorted(str(d) for d in devs)))
        Translator.__init__(self, opt, checkpoints[0], model=models[0], incremental=True, graph=graph)
        for ck, model in zip(checkpoints[1:], models[1:]):
            model.load_state_dict(ck["model"])
            model.eval()
            if next(model.parameters()).is_cuda:         # every member its own weight store, as ``Translator.__init__`` gives the one model
                from .optim import WeightStore
                WeightStore.for_model(model)
        self.models = models

    @property
    def two_streams(self):
        return False

    @two_streams.setter
    def two_streams(self, on):
        if on:
            raise ValueError("an ensemble decodes on one stream: two_streams is not offered")

    def translate_batch_contrastive(self, model_inputs, top_k=None, penalty_alpha=None, min_length=None, **unknown):
        raise NotImplementedError("contrastive search is not offered for an ensemble: the degeneration penalty compares hidden states, and "
                                  "M members have M hidden spaces (the combined score rows have none)")

    def _members(self):
        return self.models

    def _combine(self, mats, row_c, logits, rows_per, max_cols):
        """the members' score matrices of one step (or of a forced pass) → the ONE probability matrix the step kernels see: the seam a
        subclass with another rule overrides (svpc_amd/contrast_decode.py)"""
        return ops.ensemble_combine(mats, row_c, weights=self.weights, rule=self.combine, logits=logits, unk=UNK, rows_per=rows_per,
                                    max_cols=max_cols)

    def _member_features(self, k, feats):
        """the clip features member k's encoder side reads: the batch's, for every member of an ensemble"""
        return feats

    def _encode(self, model, dp, feats, ids_all, masks_all, ingr_ids_flat, cx):
        """every member's encoder side → [(model, its context, mem, bank)], member 0 with the decode's own context"""
        out = []
        for k, m in enumerate(self.models):
            cxm = cx if m is model else _Ctx(m.config, False, m.rng(feats.device))
            out.append((m, cxm) + tuple(self._encoder_side(m, dp, self._member_features(k, feats), ids_all, masks_all, ingr_ids_flat, cxm)))
        return out

    def _side(self, model, dp, enc, cx):
        Lt = model.config.max_t_len
        return _EnsembleSide([_DecoderSide(m, cxm, mem, bank, self._text_table(m, Lt, cxm, mem.device), dp.T) for m, cxm, mem, bank in enc],
                             self._combine)

    def _force(self, model, dp, enc, cx):
        """forced scoring: every member's (T·K·Lt, C) score matrix, combined (Lt rows per caption share its column count), scored as
        probabilities"""
        text, tmask, tgt, length, fin = self._force_inputs(model, dp)
        mats = [self._force_scores(m, dp, mem, bank, cxm, text, tmask) for m, cxm, mem, bank in enc]
        scores = self._combine(mats, dp.cap_c, model.config.model_mode == "video", model.config.max_t_len, max(dp.c_list))
        if dp.raw:                                 # ``teacher_scores``: the combined matrix itself, probabilities in every mode
            return self._force_raw(model, dp, scores, False)
        return self._force_finish(model, dp, scores, tgt, length, fin, False)
