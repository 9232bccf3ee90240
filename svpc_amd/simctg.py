"""Contrastive (SimCTG) training: the training counterpart of contrastive search (Su et al. 2022, "A Contrastive Framework for Neural Text
Generation").  A model trained by maximum likelihood alone produces token states whose pairwise cosines sit near 1, and
``Translator.translate_batch_contrastive``'s degeneration penalty then separates almost nothing.  Beside raising log p(target) the loss
pushes the last-layer hidden states of one caption apart with a margin: per caption the mean over its ordered token pairs (i, j), i ≠ j,
of max(0, ρ − 1 + cos(h_i, h_j)) — the token set is the history contrastive search commits for the caption, BOS through EOS.

It is one more loss head over ``scst.graded_pass``, and the first on the decoder's hidden states rather than on its score matrix:
``ops.seq_nll`` on the pass's scores plus ``ops.seq_cl`` on ``ops.to_f32`` of its ``hidden``.  A caption ``seq_nll`` bars still has hidden
states: its contrastive term counts, only its likelihood term drops out.  The caller runs ``graph.backward_all(model, loss)``,
``ops.join_side()`` and the optimizer, as for ``scst.SelfCritical``."""
from types import SimpleNamespace

import torch

from . import ops
from .scst import graded_pass, loss_result, row_weights as _fp32_rows
from .synthetic import UNK


def _graded(translator, model_inputs, dec_seq_list, row_weights, margin, who, check=None):
    """``row_weights(p)`` → (w, v) fp32 (R,) on the device, from the pass's tables"""
    def head(p):
        T, K, Lt = p.T, p.K, p.Lt
        w, v = row_weights(p)
        nll, cum, step, barred = ops.seq_nll(p.scores, p.cap_c, p.tgt, p.length, w, p.logits, UNK, max_cols=p.max_cols)
        con, cl, sim, nact = ops.seq_cl(ops.to_f32(p.hidden), p.length, v, margin, Lt)
        return loss_result(p, nll + con, cum, step, barred, cl=cl.view(T, K), sim=sim.view(T, K), nact=nact.view(T, K))
    return graded_pass(translator, model_inputs, dec_seq_list, check, head, who=who)


def contrastive_loss(translator, model_inputs, dec_seq_list, weights, cl_weights, margin=0.5):
    """``scst.sequence_loss`` with the contrastive term: loss = −Σ w·cum + Σ v·cl, the first sum over the captions that are not barred, the
    second over all of them; cl[t, k] is the mean over the caption's ordered token pairs of max(0, ``margin`` − 1 + cos(h_i, h_j)), h the
    decoder's last-layer output at positions 0 … length (BOS through EOS, or through Lt − 1 without an EOS).  ``weights`` / ``cl_weights``
    (T, K) or (T·K,) floating point on the device; ``margin`` ρ in (0, 2].  → ``sequence_loss``'s namespace plus ``cl`` (T, K) fp32,
    ``sim`` (T, K) fp32 the caption's mean pairwise cosine (its self-similarity) and ``nact`` (T, K) int32 the pairs inside the margin."""
    ops.check_simctg(margin=margin, weights=weights, cl_weights=cl_weights, need_gpu=False)

    def row_weights(p):
        ops.check_simctg(weights=weights, cl_weights=cl_weights, shape=(p.T, p.K))
        return tuple(_fp32_rows(t) for t in (weights, cl_weights))
    return _graded(translator, model_inputs, dec_seq_list, row_weights, margin, "contrastive_loss", check=weights)


class SimCTG(object):
    """The contrastive training step over a ``Translator``'s model."""

    def __init__(self, translator):
        self.translator = translator

    @staticmethod
    def _row_weights(p, cl_weight):
        """w_r = 1 / n_tok, n_tok = max(1, Σ len) (``Unlikelihood._per_token``'s), v_r = cl_weight / max(1, the captions of two tokens or
        more); both formed on the device in fp64 and rounded once; no read-back"""
        R = p.length.shape[0]
        n = p.length.sum(dtype=torch.int64).clamp_(min=1).to(torch.float64)
        m = (p.length >= 1).sum(dtype=torch.int64).clamp_(min=1).to(torch.float64)
        return (1.0 / n).to(torch.float32).expand(R).contiguous(), (float(cl_weight) / m).to(torch.float32).expand(R).contiguous()

    def step(self, model_inputs, input_labels_list, margin=0.5, cl_weight=1.0):
        """SimCTG on the batch's gold captions (``Translator.gold_captions``): loss = −Σ cum / n_tok + cl_weight · Σ cl / n_cap, the first
        sum over the captions that are not barred and n_tok = max(1, the scored positions of the batch), the second over every caption and
        n_cap = max(1, the captions of at least two tokens).  → a namespace: ``loss`` () fp32, ``nll`` (T, 1) fp32 = −cum, ``cl`` / ``sim``
        (T, 1) fp32, ``nact`` (T, 1) int32, ``barred`` (T, 1) int32.  ``cl_weight=0`` is ``Unlikelihood.token_step(alpha=0)``'s loss.  No
        host synchronisation."""
        ops.check_simctg(margin=margin, cl_weight=cl_weight)
        tr = self.translator
        gold = tr.gold_captions(input_labels_list, model_inputs[11])
        r = _graded(tr, model_inputs, gold, lambda p: self._row_weights(p, cl_weight), margin, "SimCTG.step")
        return SimpleNamespace(loss=r.loss, nll=-r.cum, cl=r.cl, sim=r.sim, nact=r.nact, barred=r.barred)
