"""Minimum-risk training (Shen et al. 2016) and the ranking / calibration loss (BRIO, Liu et al. 2022) over decoded candidate sets (DESIGN
§11.18): the sequence-level objectives that compare the K candidate paragraphs of one video WITH EACH OTHER under the model's own scores.

- risk: the candidates' length-normalised scores z are renormalised into a distribution Q over the set and the loss is the expected cost
  Σ_k Q·cost — no baseline is needed, the renormalisation is the baseline;
- rank: a margin loss Σ max(0, z_j − z_i + (pos(j) − pos(i))·λ) over the pairs with cost_i < cost_j makes the model's scores order the
  candidates as the metric does, which is what n-best lists, posterior-weighted consensus and ``score_captions`` rescoring assume.

Both are one more loss head over ``scst.graded_pass``.  Their gradient weights depend on the pass's own ``cum``, so ``ops.seq_risk`` forms
them on the device in the forward (``w_eff``) and its backward is ``seq_nll``'s under those weights.  The caller runs
``graph.backward_all(model, loss)``, ``ops.join_side()`` and the optimizer, as for ``scst.SelfCritical``."""
from types import SimpleNamespace

import torch

from . import ops
from .ops_common import Idx
from .scst import PhaseEvents, eval_mode, fresh_inputs, graded_pass, loss_result, row_weights
from .synthetic import UNK

LOSS_KW = ("alpha", "length_beta", "margin", "risk_weight", "rank_weight", "weights")


def _vid_off(p):
    """the videos' first sentences and the sentence count behind them (cached on the batch structure's plan: one upload)"""
    vo = p.plan.__dict__.get("_risk_vid_off")
    if vo is None:
        off = [0]
        for s in p.steps:
            off.append(off[-1] + s)
        vo = p.plan.__dict__["_risk_vid_off"] = Idx(off)
    return vo


def risk_loss(translator, model_inputs, dec_seq_list, cost, alpha=5e-3, length_beta=0.0, margin=1e-3, risk_weight=1.0, rank_weight=0.0,
              weights=None):
    """``scst.sequence_loss`` with the minimum-risk and ranking terms: loss = −Σ w·cum + (risk_weight·Σ_b risk[b] + rank_weight·Σ_b rank[b])
    / N.  ``dec_seq_list`` per video (S_b, K, Lt) ids, candidate paragraph k of a video = row k of each of its sentences; ``cost`` (N, K)
    float64 on the device (lower is better; a non-finite cost takes its candidate out, as does a barred sentence); z = Σ_t cum /
    (Σ_t len)^``length_beta``; Q = softmax(``alpha``·z) over the valid candidates, risk = Σ Q·cost; rank with the margin λ = ``margin`` per
    position of the cost order; ``weights`` (T, K) or (T·K,) an optional likelihood weight per caption (None: none).  Duplicate candidates
    are allowed and are NOT merged: each copy has its own share of Q and its own pairs (two copies have equal costs and so form no pair
    with each other).  → ``sequence_loss``'s namespace plus ``risk`` / ``rank`` (N,) float64, ``Q`` / ``z`` (N, K) float64, ``valid``
    (N, K) int32 and ``w_eff`` (T, K) fp32, the weights under which ``sequence_loss``'s gradient is this loss's.  No host
    synchronisation beyond the batch structure's tables."""
    ops.check_risk(cost=cost, alpha=alpha, length_beta=length_beta, margin=margin, risk_weight=risk_weight, rank_weight=rank_weight)

    def head(p):
        ops.check_risk(k=p.K, cost=cost, vid_off=_vid_off(p), n_sent=p.T)
        loss, cum, step, barred, risk, rank, Q, z, valid, w_eff = ops.seq_risk(
            p.scores, p.cap_c, p.tgt, p.length, cost.detach(), _vid_off(p), row_weights(weights), p.logits, UNK, alpha, length_beta, margin,
            risk_weight, rank_weight, max_cols=p.max_cols)
        return loss_result(p, loss, cum, step, barred, risk=risk, rank=rank, Q=Q, z=z, valid=valid, w_eff=w_eff.view(p.T, p.K))
    return graded_pass(translator, model_inputs, dec_seq_list, weights, head, who="risk_loss")


class MinimumRisk(PhaseEvents):
    """One minimum-risk / ranking training step over a ``Translator``'s model.  ``corpus`` is the ``ReferenceCorpus`` the
    candidates are scored against (its idf is CIDEr's)."""

    def __init__(self, translator, corpus):
        self.translator = translator
        self.corpus = corpus
        self.phase_events = None    # tools/bench_risk.py: a list → ``step`` appends HIP events: start, decoded, rewards, graded forward

    def _decode(self, inputs, source, K, seed, kw):
        """the K candidates per sentence of the named decoder, with ``translate_batch_consensus``' argument rules → (dec, oov)"""
        tr = self.translator
        kw = dict(kw)
        if source == "sample":
            return tr.translate_batch_sample(inputs, num_samples=K, seed=seed, **kw)[:2]
        if source == "stochastic":
            return tr.translate_batch_stochastic(inputs, K, seed=seed, **kw)[:2]
        if seed is not None:
            raise ValueError("source=%r is deterministic: it takes no seed" % (source,))
        beam = kw.pop("beam_size", K)
        if source == "nbest":
            return tr.translate_batch_nbest(inputs, beam, K, **kw)[:2]
        groups = kw.pop("num_groups", getattr(tr.opt, "num_groups", 1))
        W, G, _, _ = ops.check_diverse(beam, groups, 0.0)
        if K % G or not 1 <= K // G <= W // G:
            raise ValueError("num_candidates must be num_groups times 1..%d rows per group, got %d with %d groups" % (W // G, K, G))
        return tr.translate_batch_diverse(inputs, W, G, kw.pop("diversity_strength", None), K // G, **kw)[:2]

    def _rollout(self, model_inputs, videos, K, col, source, seed, decode_kw, include_gold=False, input_labels_list=None):
        """The rollout the candidate-set steps share, after their argument checks: stamp, the decode of K candidates per sentence in eval
        mode on copies of the ids and masks (the model's mode is restored, also when the decode raises), the gold captions as candidate K
        when asked, stamp, the candidates' rewards (column ``col`` of ``caption_scores``).  → (dec, oov, K, reward (N, K) float64)."""
        tr = self.translator
        model = tr.model
        self._stamp()
        with eval_mode([model]):
            dec, oov = self._decode(fresh_inputs(model, model_inputs), source, K, seed, decode_kw)
        if include_gold:
            gold = tr.gold_captions(input_labels_list, model_inputs[11])
            dec = [torch.cat([d, g.unsqueeze(1).to(d.dtype)], 1) for d, g in zip(dec, gold)]
            K += 1
        self._stamp()
        plan = self.corpus.plan(list(videos))
        reward = torch.stack([tr.caption_scores(dec, plan, row=k)[:, col] for k in range(K)], 1).contiguous()
        return dec, oov, K, reward

    def step(self, model_inputs, videos, num_candidates=4, source="stochastic", utility="CIDEr", include_gold=False, input_labels_list=None,
             seed=None, **loss_and_decode_kw):
        """``model_inputs`` as ``translate_batch`` takes them, ``videos`` the batch's videos as ``corpus.plan`` takes them.  The K =
        ``num_candidates`` candidates per sentence come from ``source``: "sample" (``translate_batch_sample``), "nbest"
        (``translate_batch_nbest``; ``beam_size`` defaults to K), "diverse" (``translate_batch_diverse``; ``beam_size`` defaults to K,
        K rows = ``num_groups`` × rows per group) or "stochastic" (``translate_batch_stochastic``: K DISTINCT samples) — the argument rules
        of ``translate_batch_consensus``; ``seed`` goes to the two random sources.  ``include_gold``: the batch's gold captions
        (``Translator.gold_captions`` of ``input_labels_list``) join as candidate K with their own reward, so K + 1 ≤ 16.  cost = −reward,
        the ``utility`` column of ``caption_scores`` per candidate paragraph.  The keywords of ``risk_loss`` (``alpha``, ``length_beta``,
        ``margin``, ``risk_weight``, ``rank_weight``, ``weights``) go to the loss, every other keyword to the decoder.  Duplicate
        candidates ("sample" draws with replacement) are allowed and not merged; a dead row of stochastic beam search (a sentence with
        fewer than K captions of positive probability) is an empty sentence of its candidate.  → a namespace: ``loss`` (), ``reward``
        (N, K) float64, ``expected_reward`` (N,) float64 = −risk, ``risk`` / ``rank`` (N,) float64, ``Q`` (N, K) float64, ``w_eff`` /
        ``cum`` (T, K) fp32, ``barred`` (T, K) int32, ``dec_seq_list`` (the candidates, per video (S_b, K, Lt) int64), ``oov_word_dict``.
        The decode runs in eval mode without gradients on copies of the ids and masks (it blanks the text half in place); the graded pass
        runs in the model's current mode.  No host synchronisation beyond what the decode does."""
        tr = self.translator
        K, _, col = ops.check_risk(k=num_candidates, source=source, utility=utility)
        if include_gold:
            if input_labels_list is None:
                raise ValueError("include_gold needs input_labels_list, the batch's labels")
            ops.check_risk(k=K + 1)
        loss_kw = {k: loss_and_decode_kw.pop(k) for k in LOSS_KW if k in loss_and_decode_kw}
        ops.check_risk(**{k: v for k, v in loss_kw.items() if k != "weights"})
        dec, oov, K, reward = self._rollout(model_inputs, videos, K, col, source, seed, loss_and_decode_kw, include_gold, input_labels_list)
        self._stamp()
        r = risk_loss(tr, list(model_inputs), dec, -reward, **loss_kw)
        self._stamp()
        return SimpleNamespace(loss=r.loss, reward=reward, expected_reward=-r.risk, risk=r.risk, rank=r.rank, Q=r.Q, w_eff=r.w_eff, cum=r.cum,
                               barred=r.barred, dec_seq_list=dec, oov_word_dict=oov)
