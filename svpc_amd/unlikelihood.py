"""Unlikelihood training against repetition (Welleck et al. 2020, "Neural Text Generation with Unlikelihood Training").
Beside raising log p(target) the loss lowers the probability of chosen NEGATIVE words c with −log(1 − p(c)):

- token level (``Unlikelihood.token_step``): on the gold captions, the negatives of a position are the words the caption has already used;
- sequence level (``Unlikelihood.sequence_step``): on the model's own decode, the negatives are the words that sit inside a repeated
  n-gram — with paragraph scope exactly the repeats ``DecodeMetrics``' re-n counts.

Both are one more loss head over ``scst.graded_pass``: the negatives are built on the device (``ops.ul_negatives``) from the tables the pass
already has, and ``ops.seq_ul`` is ``ops.seq_nll`` plus the unlikelihood term.  The caller runs ``graph.backward_all(model, loss)``,
``ops.join_side()`` and the optimizer, as for ``scst.SelfCritical``."""
from types import SimpleNamespace

import torch

from . import ops
from .ops_common import Idx
from .scst import eval_mode, fresh_inputs, graded_pass, loss_result, per_token, row_weights as _fp32_rows
from .synthetic import EOS, UNK

SOURCES = ("greedy", "sample")


def _sent_first(p):
    """the first sentence of every sentence's video (cached on the batch structure's plan: one upload)"""
    sf = p.plan.__dict__.get("_ul_sent_first")
    if sf is None:
        first, o = [], 0
        for s in p.steps:
            first += [o] * s
            o += s
        sf = p.plan.__dict__["_ul_sent_first"] = Idx(first)
    return sf


def _graded(translator, model_inputs, dec_seq_list, row_weights, rule, ngram, scope, who, check=None):
    """``row_weights(p)`` → (w, u) fp32 (R,) on the device, from the pass's tables"""
    def head(p):
        T, K = p.T, p.K
        ops.check_unlikelihood(rule, ngram, scope, lt=p.Lt)
        neg, npen, nrep = ops.ul_negatives(p.tgt, p.length, p.finished, p.cap_c, UNK, EOS, rule, ngram, scope,
                                           sent_first=_sent_first(p) if rule == "ngram" and scope == "paragraph" else None, K=K)
        w, u = row_weights(p)
        loss, cum, step, barred, ul, ulstep = ops.seq_ul(p.scores, p.cap_c, p.tgt, p.length, neg, w, u, p.logits, UNK, max_cols=p.max_cols)
        return loss_result(p, loss, cum, step, barred, ul=ul.view(T, K), ulstep=ulstep.view(T, K, p.Lt - 1), npen=npen.view(T, K),
                           nrep=nrep.view(T, K), weights=w, ul_weights=u)
    return graded_pass(translator, model_inputs, dec_seq_list, check, head, who=who)


def unlikelihood_loss(translator, model_inputs, dec_seq_list, weights, ul_weights, rule="token", ngram=4, scope="caption"):
    """``scst.sequence_loss`` with the unlikelihood term: loss = −Σ w·cum + Σ u·ul over the captions that are not barred, ul[t, k] the sum
    over the caption's scored positions and their negatives c of −log(1 − p(c)) (clamped at 1 − p = 1e-5).  ``weights`` / ``ul_weights``
    (T, K) or (T·K,) floating point on the device; ``rule="token"``: the negatives of a position are the caption's distinct earlier words;
    ``rule="ngram"``: the word of every position inside an ``ngram``-gram that repeats an earlier one of the caption or
    (``scope="paragraph"``) one of the same candidate row of an earlier sentence of the video.  → ``sequence_loss``'s namespace plus ``ul``
    (T, K) fp32, ``ulstep`` (T, K, Lt − 1) fp32, ``npen`` (T, K) int32 the counted negatives and ``nrep`` (T, K) int32 the repeat grams."""
    ops.check_unlikelihood(rule, ngram, scope)
    for t in (weights, ul_weights):
        if not torch.is_tensor(t) or not t.is_floating_point():
            raise ValueError("unlikelihood_loss: weights and ul_weights must be floating point tensors")

    def row_weights(p):
        ops.check_unlikelihood(rule, ngram, scope, weights=weights, ul_weights=ul_weights, shape=(p.T, p.K))
        return tuple(_fp32_rows(t) for t in (weights, ul_weights))
    r = _graded(translator, model_inputs, dec_seq_list, row_weights, rule, ngram, scope, "unlikelihood_loss", check=weights)
    del r.weights, r.ul_weights
    return r


class Unlikelihood(object):
    """The two unlikelihood training steps over a ``Translator``'s model."""

    def __init__(self, translator):
        self.translator = translator

    @staticmethod
    def _per_token(p, alpha, with_nll):
        """w_r = 1 / n (or 0), u_r = α / n (``scst.per_token``)"""
        if with_nll:
            return per_token(p, 1.0, float(alpha))
        return torch.zeros(p.length.shape[0], dtype=torch.float32, device=p.length.device), per_token(p, float(alpha))[0]

    def token_step(self, model_inputs, input_labels_list, alpha=1.0):
        """Token-level unlikelihood on the batch's gold captions (``Translator.gold_captions``): loss = (−Σ cum + α·Σ ul) / n over the
        captions that are not barred, n = max(1, the scored positions of the batch).  → a namespace: ``loss`` () fp32, ``nll`` (T, 1) fp32
        = −cum, ``ul`` (T, 1) fp32, ``npen`` (T, 1) int32, ``barred`` (T, 1) int32.  No host synchronisation."""
        ops.check_unlikelihood("token", alpha=alpha)
        tr = self.translator
        gold = tr.gold_captions(input_labels_list, model_inputs[11])
        r = _graded(tr, model_inputs, gold, lambda p: self._per_token(p, alpha, True), "token", 4, "caption", "token_step")
        return SimpleNamespace(loss=r.loss, nll=-r.cum, ul=r.ul, npen=r.npen, barred=r.barred)

    def sequence_step(self, model_inputs, alpha=1.0, ngram=4, scope="paragraph", source="greedy", seed=None, **sampling_kw):
        """Sequence-level unlikelihood on the model's own decode (``source`` "greedy", or "sample": one random sample per sentence under
        ``seed`` and the sampling keywords of ``translate_batch_sample``): loss = α·Σ ul / n, the negatives the words inside a repeated
        ``ngram``-gram, n = max(1, the decode's scored positions).  The decode runs in eval mode without gradients on copies of the ids
        and masks, as ``SelfCritical.step``'s; the graded pass runs in the model's current mode.  → a namespace: ``loss`` () fp32, ``ul``
        (T, 1) fp32, ``npen`` / ``nrep`` (T, 1) int32, ``dec_seq_list``, ``oov_word_dict``.  No host synchronisation."""
        ops.check_unlikelihood("ngram", ngram, scope, alpha=alpha)
        if source not in SOURCES:
            raise ValueError("source must be one of %s, got %r" % (", ".join(SOURCES), source))
        tr = self.translator
        unknown = set(sampling_kw) - set(tr.SAMPLING) - set(tr.TRUNCATION)
        if unknown:
            raise TypeError("unknown keyword(s): %s" % ", ".join(sorted(unknown)))
        model = tr.model
        inputs = list(model_inputs)
        with eval_mode([model]):
            dec_in = fresh_inputs(model, inputs)
            if source == "sample":
                dec, oov = tr.translate_batch_sample(dec_in, num_samples=1, seed=seed, **sampling_kw)[:2]
            else:
                with torch.no_grad():
                    dec, oov = tr.translate_batch_greedy(*dec_in, model)[:2]
        r = _graded(tr, inputs, dec, lambda p: self._per_token(p, alpha, False), "ngram", ngram, scope, "sequence_step")
        return SimpleNamespace(loss=r.loss, ul=r.ul, npen=r.npen, nrep=r.nrep, dec_seq_list=dec, oov_word_dict=oov)
