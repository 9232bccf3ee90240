"""Preference optimisation over decoded candidate sets against a frozen reference model: DPO (Rafailov et al. 2023), its
label-smoothed form cDPO (Mitchell 2023), IPO (Azar et al. 2023), SLiC's hinge (Zhao et al. 2023) and the reference-free, length-normalised
SimPO (Meng et al. 2024).

Of two candidate paragraphs of one video the one of lower cost is preferred.  With u_k = (Σ_t cum[t, k] − Σ_t ref_cum[t, k]) /
(Σ_t len)^length_beta, the policy's log-probability of candidate k held against the reference model's, every pair (i preferred over j) adds a
loss of d = u_i − u_j: −ln σ(β·d − γ) (sigmoid), max(0, 1 − (β·d − γ)) (hinge) or (d − 1 / (2β))² (ipo).  How the named methods are reached:

- DPO: ``loss_type="sigmoid"``, ``gamma=0``, ``length_beta=0``, with a reference; cDPO: DPO with ``label_smoothing`` > 0;
- IPO: ``loss_type="ipo"``; SLiC: ``loss_type="hinge"``;
- SimPO: ``loss_type="sigmoid"``, ``gamma`` > 0, ``length_beta=1``, no reference;
- RPO ("DPO + SFT"): any of them with ``weights`` on the preferred candidate.

The loss is one more head over ``scst.graded_pass``.  Its gradient weights depend on the pass's own ``cum`` and on the reference's scores,
so ``ops.seq_pref`` forms them on the device in the forward (``w_eff``) and its backward is ``seq_nll``'s under those weights.  The caller
runs ``graph.backward_all(model, loss)``, ``ops.join_side()`` and the optimizer, as for ``mrt.MinimumRisk``."""
from types import SimpleNamespace

from . import ops
from .mrt import MinimumRisk, _vid_off
from .scst import frozen_scores, graded_pass, loss_result, row_weights
from .synthetic import UNK

LOSS_KW = ("beta", "gamma", "label_smoothing", "length_beta", "pref_weight", "loss_type", "pairs", "weights")


def reference_scores(reference, model_inputs, dec_seq_list):
    """The frozen reference model's log-probability of the given captions: ``reference.score_captions(model_inputs, dec_seq_list).cum`` as
    a (T, K) fp32 tensor of its own.  ``reference`` is any ``Translator`` (an ``EnsembleTranslator`` or a ``ContrastTranslator`` too).  The
    pass runs without gradients in eval mode (the previous mode is restored) on copies of the ids and masks (``score_captions`` blanks
    their text half in place), and the result is a clone: with ``graph=True`` the pass's own buffer belongs to a captured graph and the
    next replay overwrites it.  −inf marks a caption the reference bars.  No host synchronisation beyond ``score_captions``'."""
    return frozen_scores(reference, model_inputs, dec_seq_list, "cum")


def preference_loss(translator, model_inputs, dec_seq_list, cost, ref_cum=None, beta=0.1, gamma=0.0, label_smoothing=0.0, length_beta=0.0,
                    pref_weight=1.0, loss_type="sigmoid", pairs="all", weights=None):
    """``scst.sequence_loss`` with the preference term: loss = −Σ w·cum + ``pref_weight``·Σ_b pref[b] / N.  ``dec_seq_list`` per video
    (S_b, K, Lt) ids, candidate paragraph k of a video = row k of each of its sentences; ``cost`` (N, K) float64 on the device (lower is
    preferred; a non-finite cost takes its candidate out, as does a barred sentence or a non-finite ``ref_cum``) — costs may come from
    anywhere: a human preference pair is K = 2 with costs (0, 1); ``ref_cum`` (T, K) or (T·K,) fp32 on the device, ``reference_scores`` of
    the frozen reference (None: the reference-free losses); the pairs are all (i, j) with cost_i < cost_j (``pairs="all"``) or the best
    against the worst candidate (``"extremes"``); ``weights`` (T, K) or (T·K,) an optional likelihood weight per caption (None: none).
    Duplicate candidates are allowed and are NOT merged (two copies have equal costs and form no pair with each other).  →
    ``sequence_loss``'s namespace plus ``pref`` (N,) float64 the mean pair loss, ``reward`` (N, K) float64 the implicit reward β·u,
    ``valid`` (N, K) int32, ``n_pairs`` / ``n_correct`` (N,) int32 (the pairs, and those the policy already orders as the costs do),
    ``margin`` (N,) float64 the mean of β·(u_i − u_j), and ``w_eff`` (T, K) fp32, the weights under which ``sequence_loss``'s gradient is
    this loss's.  No host synchronisation beyond the batch structure's tables."""
    ops.check_pref(cost=cost, beta=beta, gamma=gamma, label_smoothing=label_smoothing, length_beta=length_beta, pref_weight=pref_weight,
                   loss_type=loss_type, pairs=pairs)

    def head(p):
        ops.check_pref(k=p.K, cost=cost, vid_off=_vid_off(p), n_sent=p.T)
        rc = None if ref_cum is None else ref_cum.detach().reshape(-1)
        loss, cum, step, barred, pref, reward, valid, n_pairs, n_correct, margin, w_eff = ops.seq_pref(
            p.scores, p.cap_c, p.tgt, p.length, cost.detach(), _vid_off(p), rc, row_weights(weights), p.logits, UNK, beta, gamma,
            label_smoothing, length_beta, pref_weight, loss_type, pairs, max_cols=p.max_cols)
        return loss_result(p, loss, cum, step, barred, pref=pref, reward=reward, valid=valid, n_pairs=n_pairs, n_correct=n_correct,
                           margin=margin, w_eff=w_eff.view(p.T, p.K))
    return graded_pass(translator, model_inputs, dec_seq_list, weights, head, who="preference_loss")


class PreferenceOptimization(MinimumRisk):
    """One preference-optimisation training step over a ``Translator``'s model.  ``corpus`` is the ``ReferenceCorpus`` the
    candidates are scored against; ``reference`` the frozen reference model, any ``Translator`` (an ``EnsembleTranslator`` or a
    ``ContrastTranslator`` too) over the same vocabulary, or None for the reference-free losses (SimPO).  The candidates and their rewards
    come exactly as in ``MinimumRisk.step`` (its decode is reused)."""

    def __init__(self, translator, corpus, reference=None):
        super(PreferenceOptimization, self).__init__(translator, corpus)
        self.reference = reference
        # phase_events (tools/bench_pref.py): a list → ``step`` appends HIP events: start, decoded, rewards, reference scored, graded forward

    def step(self, model_inputs, videos, num_candidates=4, source="stochastic", utility="CIDEr", include_gold=False, input_labels_list=None,
             seed=None, **loss_and_decode_kw):
        """``MinimumRisk.step``'s arguments and candidates: K = ``num_candidates`` rows per sentence from ``source`` ("sample", "nbest",
        "diverse", "stochastic"), optionally the gold captions as one more candidate, cost = −reward with the ``utility`` column of
        ``caption_scores`` per candidate paragraph.  With a reference, ``reference_scores`` then scores the same candidates; the step ends
        in ``preference_loss``.  Its keywords (``beta``, ``gamma``, ``label_smoothing``, ``length_beta``, ``pref_weight``, ``loss_type``,
        ``pairs``, ``weights``) go to the loss, every other keyword to the decoder.  ValueError when the reference is the policy's own
        translator and its model is in training mode at the call: the reference would see dropout.  → a namespace: ``loss`` (),
        ``reward`` (N, K) float64, ``pref`` (N,) float64, ``implicit_reward`` (N, K) float64, ``n_pairs`` / ``n_correct`` (N,) int32,
        ``margin`` (N,) float64, ``ref_cum`` (T, K) fp32 or None, ``w_eff`` / ``cum`` (T, K) fp32, ``barred`` (T, K) int32,
        ``dec_seq_list``, ``oov_word_dict``.  The decode and the reference pass run in eval mode without gradients on copies of the ids
        and masks; the graded pass runs in the model's current mode.  No host synchronisation beyond what the decode does."""
        tr = self.translator
        K, _, col, _, _ = ops.check_pref(k=num_candidates, source=source, utility=utility)
        if include_gold:
            if input_labels_list is None:
                raise ValueError("include_gold needs input_labels_list, the batch's labels")
            ops.check_pref(k=K + 1)
        loss_kw = {k: loss_and_decode_kw.pop(k) for k in LOSS_KW if k in loss_and_decode_kw}
        ops.check_pref(**{k: v for k, v in loss_kw.items() if k != "weights"})
        model = tr.model
        if self.reference is tr and model.training:
            raise ValueError("the reference is the policy's own translator and its model is in training mode: the reference would see dropout")
        dec, oov, K, reward = self._rollout(model_inputs, videos, K, col, source, seed, loss_and_decode_kw, include_gold, input_labels_list)
        self._stamp()
        inputs = list(model_inputs)
        ref_cum = None if self.reference is None else reference_scores(self.reference, inputs, dec)
        self._stamp()
        r = preference_loss(tr, inputs, dec, -reward, ref_cum=ref_cum, **loss_kw)
        self._stamp()
        return SimpleNamespace(loss=r.loss, reward=reward, pref=r.pref, implicit_reward=r.reward, n_pairs=r.n_pairs, n_correct=r.n_correct,
                               margin=r.margin, ref_cum=ref_cum, valid=r.valid, w_eff=r.w_eff, cum=r.cum, barred=r.barred, dec_seq_list=dec,
                               oov_word_dict=oov)
