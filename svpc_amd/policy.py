"""Clipped policy-gradient training over decoded candidate sets: PPO's clipped importance-ratio surrogate (Schulman et al.
2017) in its critic-free group form GRPO (Shao et al. 2024), with the per-token "k3" KL estimate against a frozen reference model.

Every scored position i of a candidate caption has its own ratio ρ = exp(step − old_step) against the behaviour policy that decoded the
candidates, and its own term −min(ρ·A, clamp(ρ, 1 − clip_lo, 1 + clip_hi)·A) + kl_beta·(exp(δ) − δ − 1), δ = ref_step − step, with A the
advantage of the position's candidate paragraph.  How the named methods are reached:

- GRPO: ``advantage="grpo"``, ``norm="sequence"``, ``clip_lo = clip_hi = 0.2``, ``kl_beta`` > 0 with a reference;
- PPO-clip without a critic: the same with ``kl_beta=0``; dual clip (Ye et al. 2020): ``dual_clip=3``;
- DAPO (Yu et al. 2025): ``clip_hi=0.28``, ``norm="token"``, ``kl_beta=0``; Dr. GRPO (Liu et al. 2025): ``advantage="center"``, ``norm="none"``;
- RLOO: ``advantage="rloo"``, ``on_policy=True``; with ``weights`` an SFT term is mixed in.

The coefficient of the gradient differs at every position, so ``ops.seq_pg`` forms a weight per position on the device in the forward
(``pos_w``) and its backward is ``seq_nll``'s with that weight read per position.  One decoded candidate set serves several optimiser
steps: ``PolicyOptimization.collect`` decodes, rewards and scores once, ``update`` may then run several times with ``optimizer.step()`` in
between.  The caller runs ``graph.backward_all(model, loss)``, ``ops.join_side()`` and the optimizer, as for ``mrt.MinimumRisk``."""
from types import SimpleNamespace

from . import ops
from .mrt import MinimumRisk, _vid_off
from .scst import frozen_scores, graded_pass, loss_result, row_weights
from .synthetic import UNK

LOSS_KW = ("clip_lo", "clip_hi", "dual_clip", "kl_beta", "norm", "weights")


def position_scores(scorer, model_inputs, dec_seq_list):
    """A frozen policy's log-probability of every position of the given captions: ``scorer.score_captions(model_inputs,
    dec_seq_list).step`` as a (T, K, Lt − 1) fp32 tensor of its own — what a behaviour policy (``old_step``) and a reference model
    (``ref_step``) supply.  ``scorer`` is any ``Translator`` (an ``EnsembleTranslator`` or a ``ContrastTranslator`` too).  The pass runs
    without gradients in eval mode (the previous mode is restored) on copies of the ids and masks (``score_captions`` blanks their text
    half in place), and the result is a clone: with ``graph=True`` the pass's own buffer belongs to a captured graph and the next replay
    overwrites it.  −inf marks a position the scorer bars.  No host synchronisation beyond ``score_captions``'."""
    return frozen_scores(scorer, model_inputs, dec_seq_list, "step")


def policy_loss(translator, model_inputs, dec_seq_list, adv, old_step=None, ref_step=None, clip_lo=0.2, clip_hi=0.2, dual_clip=0.0,
                kl_beta=0.0, norm="sequence", weights=None):
    """``scst.sequence_loss`` with the clipped policy-gradient term: loss = −Σ w·cum + Σ tok / den.  ``dec_seq_list`` per video (S_b, K,
    Lt) ids, candidate paragraph k of a video = row k of each of its sentences; ``adv`` (N, K) float64 on the device, the candidates'
    advantages (``ops.group_advantage`` of their rewards; a non-finite one takes its candidate out, as does a barred sentence or a
    non-finite ``old_step`` / ``ref_step`` entry at a scored position); ``old_step`` / ``ref_step`` (T, K, Lt − 1) fp32 on the device,
    ``position_scores`` of the behaviour policy and of the frozen reference (None: on-policy, ρ = 1 exactly; None: no KL term, and
    ``kl_beta`` must be 0); ``weights`` (T, K) or (T·K,) an optional likelihood weight per caption (None: none).  → ``sequence_loss``'s
    namespace plus ``pos_w`` (T, K, Lt − 1) fp32, the weight per position under which ``sequence_loss``'s gradient is this loss's,
    ``pg`` / ``kl`` (T, K) float64 the captions' sums of −sur and of the KL estimate, ``n_clip`` (T, K, 2) int32 the positions clipped
    from above / from below, ``ratio_max`` (T, K) fp32, ``valid`` (N, K) int32 and ``n_tok`` (1,) int32.  No host synchronisation
    beyond the batch structure's tables."""
    ops.check_pg(adv=adv, old_step=old_step, ref_step=ref_step, clip_lo=clip_lo, clip_hi=clip_hi, dual_clip=dual_clip, kl_beta=kl_beta,
                 norm=norm, has_ref=ref_step is not None)

    def head(p):
        T, K, Lt = p.T, p.K, p.Lt
        ops.check_pg(k=K, adv=adv, vid_off=_vid_off(p), n_sent=T)
        loss, cum, step, barred, pos_w, pg, kl, n_clip, ratio_max, valid, n_tok = ops.seq_pg(
            p.scores, p.cap_c, p.tgt, p.length, adv.detach(), _vid_off(p), None if old_step is None else old_step.detach(),
            None if ref_step is None else ref_step.detach(), row_weights(weights), p.logits, UNK, clip_lo, clip_hi, dual_clip, kl_beta, norm,
            max_cols=p.max_cols)
        return loss_result(p, loss, cum, step, barred, pos_w=pos_w.view(T, K, Lt - 1), pg=pg.view(T, K), kl=kl.view(T, K),
                           n_clip=n_clip.view(T, K, 2), ratio_max=ratio_max.view(T, K), valid=valid, n_tok=n_tok)
    return graded_pass(translator, model_inputs, dec_seq_list, weights, head, who="policy_loss")


class PolicyOptimization(MinimumRisk):
    """Clipped policy-gradient training over a ``Translator``'s model.  ``corpus`` is the ``ReferenceCorpus`` the
    candidates are scored against; ``reference`` the frozen reference model of the KL term, any ``Translator`` (an ``EnsembleTranslator``
    or a ``ContrastTranslator`` too) over the same vocabulary, or None (no KL term).  The candidates and their rewards come exactly as in
    ``MinimumRisk.step`` (its decode is reused)."""

    def __init__(self, translator, corpus, reference=None):
        super(PolicyOptimization, self).__init__(translator, corpus)
        self.reference = reference
        # phase_events (tools/bench_policy.py): a list → ``collect`` appends HIP events: start, decoded, rewards, behaviour scored,
        # reference scored; ``update``: start, graded forward

    def _refuse_self_reference(self):
        if self.reference is self.translator and self.translator.model.training:
            raise ValueError("the reference is the policy's own translator and its model is in training mode: the reference would see dropout")

    def collect(self, model_inputs, videos, num_candidates=4, source="sample", utility="CIDEr", advantage="grpo", on_policy=False, seed=None,
                adv_eps=1e-6, **decode_kw):
        """The rollout: K = ``num_candidates`` candidates per sentence from ``source`` ("sample", "nbest", "diverse", "stochastic"; the
        argument rules of ``MinimumRisk.step``, every further keyword goes to the decoder), their rewards (the ``utility`` column of
        ``caption_scores`` per candidate paragraph), the advantages ``ops.group_advantage(reward, advantage, adv_eps)``, and the step
        scores of the behaviour policy — this translator as it stands — and of the reference.  ``on_policy=True`` skips the behaviour
        pass: ρ is exactly 1, which is right for ONE ``update`` per rollout.  ValueError when the reference is the policy's own translator
        and its model is in training mode.  → a namespace: ``dec_seq_list``, ``oov_word_dict``, ``reward`` / ``adv`` (N, K) float64,
        ``old_step`` / ``ref_step`` (T, K, Lt − 1) fp32 or None.  Decode and both scoring passes run in eval mode without gradients on
        copies of the ids and masks; the model's mode is restored.  No host synchronisation beyond what the decode does."""
        tr = self.translator
        K, _, col, _, _ = ops.check_pg(k=num_candidates, source=source, utility=utility, advantage=advantage, eps=adv_eps)
        self._refuse_self_reference()
        dec, oov, K, reward = self._rollout(model_inputs, videos, K, col, source, seed, decode_kw)
        inputs = list(model_inputs)
        adv = ops.group_advantage(reward, advantage, adv_eps)
        self._stamp()
        old_step = None if on_policy else position_scores(tr, inputs, dec)
        self._stamp()
        ref_step = None if self.reference is None else position_scores(self.reference, inputs, dec)
        self._stamp()
        return SimpleNamespace(dec_seq_list=dec, oov_word_dict=oov, reward=reward, adv=adv, old_step=old_step, ref_step=ref_step)

    def update(self, rollout, model_inputs, **loss_kw):
        """One graded pass over a rollout: ``policy_loss`` with the rollout's candidates, advantages and step scores and the keywords
        ``clip_lo``, ``clip_hi``, ``dual_clip``, ``kl_beta``, ``norm``, ``weights``.  The caller may run it several times per rollout
        with optimiser steps in between: from the second on ρ ≠ 1 and the clip acts.  → ``policy_loss``'s namespace."""
        unknown = [k for k in loss_kw if k not in LOSS_KW]
        if unknown:
            raise TypeError("update() got an unexpected keyword argument %r" % unknown[0])
        ops.check_pg(has_ref=rollout.ref_step is not None, **{k: v for k, v in loss_kw.items() if k != "weights"})
        self._stamp()
        r = policy_loss(self.translator, list(model_inputs), rollout.dec_seq_list, rollout.adv, old_step=rollout.old_step,
                        ref_step=rollout.ref_step, **loss_kw)
        self._stamp()
        return r

    def step(self, model_inputs, videos, num_candidates=4, source="sample", utility="CIDEr", advantage="grpo", on_policy=False, seed=None,
             adv_eps=1e-6, **loss_and_decode_kw):
        """``collect`` and one ``update``: the keywords of ``update`` go to the loss, every other keyword to the decoder.  → ``update``'s
        namespace plus ``reward``, ``adv``, ``old_step``, ``ref_step``, ``dec_seq_list``, ``oov_word_dict`` and ``rollout``."""
        loss_kw = {k: loss_and_decode_kw.pop(k) for k in LOSS_KW if k in loss_and_decode_kw}
        ops.check_pg(k=num_candidates, source=source, utility=utility, advantage=advantage, eps=adv_eps,
                     has_ref=self.reference is not None, **{k: v for k, v in loss_kw.items() if k != "weights"})
        ro = self.collect(model_inputs, videos, num_candidates=num_candidates, source=source, utility=utility, advantage=advantage,
                          on_policy=on_policy, seed=seed, adv_eps=adv_eps, **loss_and_decode_kw)
        r = self.update(ro, model_inputs, **loss_kw)
        r.reward, r.adv, r.old_step, r.ref_step = ro.reward, ro.adv, ro.old_step, ro.ref_step
        r.dec_seq_list, r.oov_word_dict, r.rollout = ro.dec_seq_list, ro.oov_word_dict, ro
        return r
