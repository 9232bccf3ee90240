"""Contrastive decoding: an expert's scores held against an amateur's (Li et al. 2023; O'Brien & Lewis 2023) — the opposite
combination to ``EnsembleTranslator``'s average.  With the amateur taken as THE SAME MODEL WITHOUT THE VIDEO it is what the vision–language
literature calls visual contrastive decoding (Leng et al. 2024), and algebraically classifier-free guidance: what the language prior and
the ingredient list would have said anyway is taken out of the step score, what the clips add is kept.

``ContrastTranslator(opt, checkpoint, model, amateur_checkpoint=None, amateur_model=None, *, beta=0.5, alpha=0.1, expert_weight=None,
amateur_video="same", amateur_features=None, graph=False)`` is a ``Translator`` with two members on the ensemble's machinery: both run
their encoder side once per batch and their decoder iteration per step, on their own KV caches, in the decode's one stream; the two score
matrices of a step go through ``ops.contrast_combine`` and the step kernels take the result as a probability matrix (``logits=False``):

- the step score of a word is ``expert_weight``·log p_expert − ``beta``·log p_amateur, over the HEAD only — the words the expert itself
  finds plausible, p_expert ≥ ``alpha``·max p_expert —, renormalised over the head (a distribution: the samplers draw from it as it is);
  UNK is never a candidate; the amateur's log-probability is floored at log 1e-30;
- ``expert_weight`` defaults to 1 + ``beta`` (O'Brien & Lewis; classifier-free guidance); ``beta=1, expert_weight=1`` is Li et al.'s
  log p_e − log p_a; ``beta=0`` leaves the expert renormalised over its head (the amateur still runs: a captured graph is the same for
  any coefficients);
- a separate amateur (``amateur_checkpoint`` and ``amateur_model``) must agree with the expert on ``ensemble.AGREE`` and sit on its
  device; it gets its own weight store;
- the expert as its own amateur (both None): the second decoder side runs the same module, with its own encoder side and KV caches, over
  a degraded view of the video — ``amateur_video="zero"``: zero clip features (one cached buffer per shape); ``amateur_features``: any
  callable ``feats -> feats`` over the flat (clips·positions, F) fp32 feature rows ON THE DEVICE (noise, another video's clips …).  It
  runs on every decode, also inside a graph capture: it must not synchronise, must not read host state that changes between calls, and
  must return a tensor of the same shape and dtype.  Both may be combined (the callable sees the zeros) and may be given with a separate
  amateur too.  ``amateur_video="same"`` without a separate amateur and without a callable is refused: the two distributions would be
  identical;
- every decode of the ensemble works unchanged (greedy, beam / n-best with controls, paragraph scope, diverse, constrained, sampling,
  stochastic, consensus), and so do ``score_captions`` and ``teacher_scores`` (hence ``svpc_amd/distill.py``: the 2× decode cost can be
  distilled back into one model); ``translate_batch_contrastive``, ``incremental=False`` and ``two_streams`` are refused as the ensemble
  refuses them;
- ``graph=True`` replays the two-member decode as one graph, re-captured when either member's parameters move.

tests/contrast_decode_reference.py restates the rule and the decodes on the CPU."""
from __future__ import annotations

import torch

from . import ops
from .ensemble import EnsembleTranslator
from .synthetic import UNK

AMATEUR_VIDEO = ("same", "zero")


class ContrastTranslator(EnsembleTranslator):
    def __init__(self, opt, checkpoint, model, amateur_checkpoint=None, amateur_model=None, *, beta=0.5, alpha=0.1, expert_weight=None,
                 amateur_video="same", amateur_features=None, graph=False):
        if (amateur_checkpoint is None) != (amateur_model is None):
            raise ValueError("a separate amateur needs both amateur_checkpoint and amateur_model (give neither for the expert as its own amateur)")
        try:
            b = float(beta)
        except (TypeError, ValueError):
            raise ValueError("beta must be a number, got %r" % (beta,))
        we, wa, al, _ = ops.contrast_coefficients(1.0 + b if expert_weight is None else expert_weight, b, alpha, who="ContrastTranslator")
        if amateur_video not in AMATEUR_VIDEO:
            raise ValueError("amateur_video must be one of %s, got %r" % (", ".join(AMATEUR_VIDEO), amateur_video))
        if amateur_features is not None and not callable(amateur_features):
            raise ValueError("amateur_features must be a callable feats -> feats, got %r" % (amateur_features,))
        separate = amateur_model is not None
        if not separate and amateur_video == "same" and amateur_features is None:
            raise ValueError("the expert as its own amateur needs a degraded view of the video (amateur_video=\"zero\" or amateur_features): "
                             "with the same clips the two distributions are identical")
        self.beta, self.alpha, self.expert_weight, self.amateur_weight = b, al, we, wa
        self.amateur_video, self.amateur_features, self.separate_amateur = amateur_video, amateur_features, separate
        self._zero_feats = {}
        if separate:
            self._adopt(opt, [checkpoint, amateur_checkpoint], [model, amateur_model], graph)
        else:                                  # one module, adopted once, behind two decoder sides
            self._adopt(opt, [checkpoint], [model], graph)
            self.models = [model, model]

    def _combine(self, mats, row_c, logits, rows_per, max_cols):
        return ops.contrast_combine(mats[0], mats[1], row_c, expert_weight=self.expert_weight, amateur_weight=self.amateur_weight,
                                    alpha=self.alpha, logits=logits, unk=UNK, rows_per=rows_per, max_cols=max_cols)

    def _member_features(self, k, feats):
        """member 0, the expert, reads the batch's clip features; member 1, the amateur, its degraded view of them"""
        if k == 0:
            return feats
        if self.amateur_video == "zero":
            key = (tuple(feats.shape), feats.dtype, feats.device)
            z = self._zero_feats.get(key)
            if z is None:                      # (a graphed decode runs eagerly first: the buffer exists before any capture)
                z = self._zero_feats[key] = torch.zeros_like(feats)
            feats = z
        if self.amateur_features is not None:
            feats = self.amateur_features(feats)
        return feats
