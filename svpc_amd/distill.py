"""Knowledge distillation: train one model against a teacher — usually an ``EnsembleTranslator`` — so that an ensemble's quality comes back
at a single model's decoding speed (Hinton et al. 2015; Kim & Rush 2016, "Sequence-Level Knowledge Distillation").

- word level (``Distill.word_step``): on the gold captions, beside raising log p(target) the student's whole per-position distribution is
  pulled towards the teacher's: the cross-entropy −Σ_c q_c·log p_c over the candidates of every scored position;
- sequence level (``Distill.sequence_step``): the captions are the teacher's own beam (or greedy) output; α > 0 adds the word-level term
  along it.

Both are one more loss head over ``scst.graded_pass``: the teacher's score matrix over the same T·K·Lt rows comes from
``Translator.teacher_scores`` (no gradient, the teacher in eval mode), and ``ops.seq_kd`` is ``ops.seq_nll`` plus the distillation term.
Student and teacher may differ in width and depth; they must share the mode, the vocabulary and the batch's shapes (``AGREE``).  The
caller runs ``graph.backward_all(model, loss)``, ``ops.join_side()`` and the optimizer, as for ``scst.SelfCritical``."""
from types import SimpleNamespace

import torch

from . import ops
from .scst import eval_mode, fresh_inputs, graded_pass, loss_result, per_token, row_weights as _fp32_rows
from .synthetic import UNK

AGREE = ("model_mode", "vocab_size", "max_t_len", "max_v_len", "max_i_len", "video_feature_size")
SOURCES = ("beam", "greedy")


def _check_pair(translator, teacher):
    """student and teacher agree on what the score rows and the batch mean (ValueError naming the field)"""
    s_cfg, t_cfg = translator.model.config, teacher.model.config
    for f in AGREE:
        if getattr(s_cfg, f) != getattr(t_cfg, f):
            raise ValueError("distillation: student and teacher differ in %s: %r against %r" % (f, getattr(s_cfg, f), getattr(t_cfg, f)))
    devs = [next(m.parameters()).device for m in (translator.model, teacher.model)]
    if devs[0] != devs[1]:
        raise ValueError("distillation: student and teacher differ in device: %s against %s" % (devs[0], devs[1]))


def _graded(translator, teacher, model_inputs, dec_seq_list, row_weights, who, check=None, kd_check=None):
    """``row_weights(p)`` → (w, v) fp32 (R,) on the device, from the pass's tables"""
    _check_pair(translator, teacher)
    inputs = list(model_inputs)
    # the host checks of both passes before either runs: every ValueError comes before any launch
    ids, steps = ops.stack_captions(dec_seq_list)
    if ids.dim() == 2:
        ids = ids.unsqueeze(1)
    if steps != [int(s) for s in inputs[11]]:
        raise ValueError("%s: the captions' rows per video %r are not the batch's step counts %r" % (who, steps, list(inputs[11])))
    if kd_check is not None and ids.dim() == 3:
        ops.check_distill(kd_weights=kd_check, shape=tuple(ids.shape[:2]), need_gpu=False)
    ops.check_scst(ids, baseline="none", lt=translator.max_t_len, steps=steps, weights=check)
    if kd_check is not None:
        ops.check_distill(kd_weights=kd_check, shape=tuple(ids.shape[:2]))
    if inputs[1][0].device.type != "cuda":
        raise ops._lib.SvpcKernelError("%s runs on the GPU only (no CPU fallback exists)" % who)
    with eval_mode(teacher._members()):
        t = teacher.teacher_scores(fresh_inputs(teacher.model, inputs), dec_seq_list)

    def head(p):
        T, K, Lt = p.T, p.K, p.Lt
        if (t.T, t.K, t.Lt) != (T, K, Lt) or list(t.cap_c.host) != list(p.cap_c.host):
            raise ValueError("%s: the teacher's score rows are not the student's" % who)
        w, v = row_weights(p)
        loss, cum, step, barred, kd, kdstep, ent, hstep = ops.seq_kd(p.scores, p.cap_c, p.tgt, p.length, t.scores, w, v, p.logits, t.logits,
                                                                     UNK, max_cols=p.max_cols)
        return loss_result(p, loss, cum, step, barred, kd=kd.view(T, K), ent=ent.view(T, K), kdstep=kdstep.view(T, K, Lt - 1),
                           hstep=hstep.view(T, K, Lt - 1))
    return graded_pass(translator, inputs, dec_seq_list, check, head, who=who)


def distillation_loss(translator, teacher, model_inputs, dec_seq_list, weights, kd_weights):
    """``scst.sequence_loss`` with the distillation term: loss = −Σ w·cum + Σ v·kd over the captions that are not barred, kd[t, k] the sum
    over the caption's scored positions of the cross-entropy −Σ_c q_c·log p_c of the student's distribution against the ``teacher``'s
    (a ``Translator`` or an ``EnsembleTranslator``; ``teacher_scores`` on copies of the ids and masks, its models in eval mode and their
    mode restored).  ``weights`` / ``kd_weights`` (T, K) or (T·K,) floating point on the device.  → ``sequence_loss``'s namespace plus
    ``kd`` / ``ent`` (T, K) fp32 and ``kdstep`` / ``hstep`` (T, K, Lt − 1) fp32 (``ent`` the teacher's entropy: kd − ent is the KL
    divergence of a teacher that sums to 1).  Only the student gets a gradient."""
    for t in (weights, kd_weights):
        if not torch.is_tensor(t) or not t.is_floating_point():
            raise ValueError("distillation_loss: weights and kd_weights must be floating point tensors")

    def row_weights(p):
        return tuple(_fp32_rows(t) for t in (weights, kd_weights))
    return _graded(translator, teacher, model_inputs, dec_seq_list, row_weights, "distillation_loss", check=weights, kd_check=kd_weights)


class Distill(object):
    """The two distillation training steps of a student ``Translator``'s model against a ``teacher`` translator."""

    def __init__(self, translator, teacher):
        _check_pair(translator, teacher)
        self.translator = translator
        self.teacher = teacher

    @staticmethod
    def _per_token(p, alpha):
        """w_r = (1 − α) / n, v_r = α / n (``scst.per_token``)"""
        return per_token(p, 1.0 - float(alpha), float(alpha))

    def word_step(self, model_inputs, input_labels_list, alpha=0.5):
        """Word-level distillation on the batch's gold captions (``Translator.gold_captions``): loss = ((1 − α)·Σ −cum + α·Σ kd) / n over
        the captions that are not barred, n = max(1, the scored positions of the batch).  → a namespace: ``loss`` () fp32, ``nll`` (T, 1)
        fp32 = −cum, ``kd`` / ``ent`` (T, 1) fp32, ``barred`` (T, 1) int32.  No host synchronisation."""
        ops.check_distill(alpha=alpha)
        tr = self.translator
        gold = tr.gold_captions(input_labels_list, model_inputs[11])
        r = _graded(tr, self.teacher, model_inputs, gold, lambda p: self._per_token(p, alpha), "word_step")
        return SimpleNamespace(loss=r.loss, nll=-r.cum, kd=r.kd, ent=r.ent, barred=r.barred)

    def sequence_step(self, model_inputs, alpha=0.0, source="beam", **decode_kw):
        """Sequence-level distillation: the captions are the TEACHER's decode of the batch — ``source="beam"``: the top row of
        ``translate_batch_beam`` under ``beam_size`` (default: the teacher's) and the decoding controls; ``"greedy"`` — and the loss is
        ((1 − α)·Σ −cum + α·Σ kd) / n along them, so α > 0 adds the word-level term on the teacher's own output.  The decode runs in eval
        mode without gradients on copies of the ids and masks; the graded pass runs in the student's current mode.  → a namespace:
        ``loss`` () fp32, ``nll`` / ``kd`` / ``ent`` (T, 1) fp32, ``dec_seq_list``, ``oov_word_dict``.  No host synchronisation."""
        ops.check_distill(alpha=alpha)
        if source not in SOURCES:
            raise ValueError("source must be one of %s, got %r" % (", ".join(SOURCES), source))
        te = self.teacher
        allowed = ({"beam_size"} | set(te.CONTROLS)) if source == "beam" else set()
        unknown = set(decode_kw) - allowed
        if unknown:
            raise TypeError("unknown keyword(s): %s" % ", ".join(sorted(unknown)))
        inputs = list(model_inputs)
        with eval_mode(te._members()):
            dec_in = fresh_inputs(te.model, inputs)
            if source == "beam":
                kw = dict(decode_kw)
                beam = kw.pop("beam_size", None)
                dec, oov = te.translate_batch_beam(dec_in, beam if beam is not None else getattr(te.opt, "beam_size", 2), **kw)[:2]
            else:
                with torch.no_grad():
                    dec, oov = te.translate_batch_greedy(*dec_in, te.model)[:2]
        r = _graded(self.translator, te, inputs, dec, lambda p: self._per_token(p, alpha), "sequence_step")
        return SimpleNamespace(loss=r.loss, nll=-r.cum, kd=r.kd, ent=r.ent, dec_seq_list=dec, oov_word_dict=oov)
