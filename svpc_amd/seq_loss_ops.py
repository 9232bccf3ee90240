"""The sequence losses of the training objectives, bound to their HIP kernels, and their host checks: self-critical weights (DESIGN
§11.10), ``seq_nll`` and the losses that are ``seq_nll`` plus a term of their own — unlikelihood (§11.13), distillation (§11.15), minimum
risk / ranking (§11.18), preference optimisation (§11.21), clipped policy gradient (§11.22) — and the contrastive loss on the decoder's
hidden states (SimCTG, §11.17).  ``ops`` re-exports every public name, and callers say ``ops.<name>``.

What the six score-matrix losses share is stated once: ``_score_head`` and ``_score_tail`` are the argument checks
they open with and what each wrapper checks last (``_candidate_rows``: what the candidate-set objectives check between the two),
``_open`` the forward's allocations and autograd bookkeeping, ``_backward`` the whole backward but the kernel's argument list; the
``check_*`` functions share ``_number``, ``_check_row_vecs``, ``_check_caption_weights`` and ``_check_candidates``.

What this module needs from ``ops`` (``_stream``, ``_need_gpu``, ``CONSENSUS_UTILITIES``) it reads through ``_ops()`` at call time, as
grad_tail.py does: ``ops`` imports this module, not the other way round.
"""
from __future__ import annotations

import math
import numbers

import torch

from . import _lib
from .ops_common import Function, _c, _id_rows, _p, _row_vec, as_idx

__all__ = ["SCST_MAX", "SCST_BASELINES", "check_scst", "scst_weights", "seq_nll",
           "UL_RULES", "UL_SCOPES", "UL_MAX_NEG", "UL_EPS", "check_unlikelihood", "ul_negatives", "seq_ul",
           "KD_LOG_EPS", "check_distill", "seq_kd",
           "CL_MAX_LT", "CL_ROW_BYTES", "check_simctg", "seq_cl",
           "RISK_MAX", "RISK_SOURCES", "check_risk", "seq_risk",
           "PREF_MAX", "PREF_LOSS_TYPES", "PREF_PAIRS", "check_pref", "seq_pref",
           "PG_MAX", "PG_NORMS", "PG_ADVANTAGES", "check_pg", "group_advantage", "seq_pg"]

_OPS = []


def _ops():
    if not _OPS:
        from . import ops
        _OPS.append(ops)
    return _OPS[0]


# ------------------------------------------------------------------------------------------------ what the checks share
def _number(name, v, ok, what, finite=True):
    """``v`` is None or a finite real number (no bool) that ``ok`` accepts; ``what`` says so in the message (``finite`` off: ``ok``
    alone refuses what is not finite)"""
    if v is not None and (isinstance(v, bool) or not isinstance(v, numbers.Real) or (finite and not math.isfinite(v)) or not ok(v)):
        raise ValueError("%s %s, got %r" % (name, what, v))


def _not_negative(name, v):
    _number(name, v, lambda x: x >= 0, "must be a finite number >= 0")


def _check_row_vecs(rows, device, **named):
    for name, t in named.items():
        if t is not None and (not torch.is_tensor(t) or not _row_vec(t, rows, torch.float32, device)):
            raise ValueError("%s must be contiguous fp32 (%s,) on the scores' device" % (name, rows))


def _check_caption_weights(shape, **named):
    for name, t in named.items():
        if t is not None and (not torch.is_tensor(t) or not t.is_floating_point()
                              or tuple(t.shape) not in (tuple(shape), (shape[0] * shape[1],))):
            raise ValueError("%s must be floating point %s or (%d,), got %s"
                             % (name, tuple(shape), shape[0] * shape[1], tuple(t.shape) if torch.is_tensor(t) else type(t).__name__))


def _describe(t):
    return "%s %s" % (tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__


def _check_table(what, t):
    if t is not None and (not torch.is_tensor(t) or t.dim() != 2 or t.dtype != torch.float64):
        raise ValueError("%s must be float64 (N, K), got %s" % (what, _describe(t)))


def _check_candidates(k=None, table=None, vid_off=None, n_sent=None, source=None, utility=None, device=None, what="cost",
                      objective="risk training"):
    """The checks of a candidate-set objective (``check_risk``'s, which ``check_pref`` and ``check_pg`` go through): ``what`` is the name
    of the (N, K) float64 table in the messages, ``objective`` the objective's.  → (K, N, the utility's column or None)."""
    utilities = _ops().CONSENSUS_UTILITIES
    if source is not None and source not in RISK_SOURCES:
        raise ValueError("source must be one of %s, got %r" % (", ".join(RISK_SOURCES), source))
    if utility is not None and utility not in utilities:
        raise ValueError("utility must be one of %s, got %r" % (", ".join(utilities), utility))
    K = N = None
    if k is not None:
        if isinstance(k, bool) or not isinstance(k, numbers.Integral) or not 1 <= int(k) <= RISK_MAX:
            raise ValueError("%s takes 1..%d candidates per sentence, got K = %r" % (objective, RISK_MAX, k))
        K = int(k)
    if table is not None:
        _check_table(what, table)
        N = table.shape[0]
        if not 1 <= table.shape[1] <= RISK_MAX or (K is not None and table.shape[1] != K):
            raise ValueError("%s must have one column per candidate (K = %s in 1..%d), got %d" % (what, K, RISK_MAX, table.shape[1]))
        K = table.shape[1]
        if device is not None and table.device != device:
            raise ValueError("%s must be on the scores' device %s, got %s" % (what, device, table.device))
    if vid_off is not None:
        off = [int(o) for o in as_idx(vid_off).host]
        if (not off or off[0] != 0 or any(b < a for a, b in zip(off, off[1:])) or (n_sent is not None and off[-1] != n_sent)
                or (N is not None and len(off) != N + 1)):
            raise ValueError("vid_off must hold N + 1 = %s offsets that start at 0, never fall and end at the %s sentences, got %r"
                             % (None if N is None else N + 1, n_sent, off if len(off) <= 20 else off[:20] + ["…"]))
        N = len(off) - 1
    if table is not None and not table.is_cuda:
        raise _lib.SvpcKernelError("svpc_amd.ops: %s runs on the GPU only (no CPU fallback exists)" % objective)
    return K, N, None if utility is None else utilities.index(utility)


# ------------------------------------------------------------------------------------------------ what the score-matrix losses share
def _score_head(who, scores, tgt, length):
    """The argument checks every loss over the decoder's score matrix opens with, under the wrapper's name ``who``: ``tgt``, ``scores``,
    ``length``, in this order.  → (R, lt)"""
    if tgt.dim() != 2 or tgt.shape[1] < 2 or not _id_rows(tgt, tgt.shape[0], tgt.shape[1], scores.device):
        raise ValueError("%s: tgt must be a contiguous int32 (R, Lt >= 2) matrix on the scores' device" % who)
    R, lt = tgt.shape
    if scores.dim() != 2 or scores.shape[0] < R * lt or scores.dtype != torch.float32:
        raise ValueError("%s: scores must be fp32 (>= R·Lt, C) rows" % who)
    if not _row_vec(length, R, torch.int32, scores.device):
        raise ValueError("%s: length must be contiguous int32 (R,) on the scores' device" % who)
    return R, lt


def _score_tail(who, scores, row_c, R, max_cols):
    """… and closes with: ``row_c``, ``max_cols``.  → (rc, max_c)"""
    rc = as_idx(row_c)
    if len(rc.host) != R:
        raise ValueError("%s: one column count per caption row (%d), got %d" % (who, R, len(rc.host)))
    max_c = int(max_cols) if max_cols is not None else (max(rc.host) if R else 1)
    if max_c > scores.shape[1] or (R and (min(rc.host) < 1 or max(rc.host) > max_c)):
        raise ValueError("%s: rows of 1..%d columns, inside the score matrix and max_cols" % (who, scores.shape[1]))
    return rc, max_c


def _candidate_rows(who, scores, R, K, table, vid_off, row_w, what="cost", objective="risk training"):
    """What a candidate-set objective checks between the two, after its own ``check_*``: R a multiple of K, ``vid_off`` against the (N, K)
    ``table`` (``_check_candidates``' ``what`` / ``objective``), ``row_w`` (None: zeros).  → (off, row_w)"""
    if R % K:
        raise ValueError("%s: %d caption rows are no multiple of the K = %d candidates per sentence" % (who, R, K))
    off = as_idx(vid_off)
    _check_candidates(table=table, vid_off=off, n_sent=R // K, what=what, objective=objective)
    if row_w is None:
        row_w = torch.zeros(R, dtype=torch.float32, device=scores.device)
    elif not torch.is_tensor(row_w) or not _row_vec(row_w, R, torch.float32, scores.device):
        raise ValueError("%s: row_w must be contiguous fp32 (R,) on the scores' device" % who)
    return off, row_w


def _open(ctx, scores, tgt, cfg, extra=(), bwd="seq_nll_bwd"):
    """The forward's prologue: allocates loss, cum, step, barred and the family's further outputs ``extra`` ((shape, dtype) each), marks
    all but the loss as not differentiable, and leaves on ``ctx`` what ``_backward`` reads — ``cfg`` = (R, lt) + the family's ``cfg`` and
    the name of the backward kernel.  → the outputs in the order the forward returns them."""
    R, lt = tgt.shape
    dev = scores.device
    out = (torch.empty((), dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.float32, device=dev),
           torch.empty(R, lt - 1, dtype=torch.float32, device=dev), torch.empty(R, dtype=torch.int32, device=dev))
    out += tuple(torch.empty(shape, dtype=dtype, device=dev) for shape, dtype in extra)
    ctx.cfg = (R, lt) + tuple(cfg)
    ctx.bwd = bwd
    ctx.mark_non_differentiable(*out[1:])
    ctx.set_materialize_grads(False)
    return out


def _backward(ctx, dl, args):
    """The backward of every score-matrix loss: one launch of ``ctx.bwd`` that writes the whole of dscores but the rows past R·Lt, which
    are zeroed here; ``args(saved tensors, cfg, dl)`` is the kernel's argument list up to dscores.  One gradient per forward input."""
    n = len(ctx.needs_input_grad)
    if dl is None:
        return (None,) * n
    saved = ctx.saved_tensors
    scores = saved[0]
    R, lt = ctx.cfg[:2]
    dl = _c(dl.to(torch.float32))
    dscores = torch.empty(scores.shape, dtype=torch.float32, device=scores.device)     # (every element is written by the kernel)
    if scores.shape[0] > R * lt:
        dscores[R * lt:].zero_()
    _lib.call(ctx.bwd, *args(saved, ctx.cfg, dl), _p(dscores), dscores.shape[1], _ops()._stream())
    return (dscores,) + (None,) * (n - 1)


# ------------------------------------------------------------------------------------------------ self-critical sequence training
SCST_MAX = 16                   # sampled captions per sentence (what ``consensus`` and forced scoring take)
SCST_BASELINES = ("none", "greedy", "mean")


def check_scst(ids=None, num_samples=None, baseline="greedy", utility="CIDEr", lt=None, steps=None, weights=None):
    """Host checks of the self-critical step (ValueError for each): ``num_samples`` K in 1 … 16; ``baseline`` "none",
    "greedy" or "mean" (the leave-one-out mean needs K ≥ 2); ``utility`` one of the six score columns; ``ids`` the stacked captions,
    (T, K, Lt) int32 / int64 with ``lt`` the model's Lt when given; ``steps`` the videos' sentence counts, which must add up to T;
    ``weights`` (T, K) or (T·K,) floating point.  ``SvpcKernelError`` for ids or weights that are not on the GPU (no CPU fallback exists).
    → (baseline rule, utility column, K)."""
    utilities = _ops().CONSENSUS_UTILITIES
    if baseline not in SCST_BASELINES:
        raise ValueError("baseline must be one of %s, got %r" % (", ".join(SCST_BASELINES), baseline))
    if utility not in utilities:
        raise ValueError("utility must be one of %s, got %r" % (", ".join(utilities), utility))
    K = None
    if num_samples is not None:
        if isinstance(num_samples, bool) or not isinstance(num_samples, numbers.Integral) or not 1 <= int(num_samples) <= SCST_MAX:
            raise ValueError("the self-critical step takes 1..%d samples per sentence, got K = %r" % (SCST_MAX, num_samples))
        K = int(num_samples)
    if ids is not None:
        if not torch.is_tensor(ids) or ids.dim() != 3 or ids.dtype not in (torch.int32, torch.int64):
            raise ValueError("the self-critical step takes int32 / int64 ids of shape (T, K, Lt), got %s"
                             % ((tuple(ids.shape), ids.dtype) if torch.is_tensor(ids) else type(ids).__name__,))
        T, k, n = ids.shape
        if not 1 <= k <= SCST_MAX:
            raise ValueError("the self-critical step takes 1..%d captions per sentence, got K = %d" % (SCST_MAX, k))
        if K is not None and k != K:
            raise ValueError("ids of %d captions per sentence, num_samples is %d" % (k, K))
        K = k
        if n < 2:
            raise ValueError("captions need at least two positions (BOS and one word), got Lt = %d" % n)
        if lt is not None and n != int(lt):
            raise ValueError("captions of %d positions, the model's Lt is %d" % (n, lt))
        if steps is not None and (any(int(s) < 0 for s in steps) or sum(int(s) for s in steps) != T):
            raise ValueError("the videos' sentence counts %r do not add up to the %d caption rows given" % (list(steps), T))
        if weights is not None and (not torch.is_tensor(weights) or not weights.is_floating_point()
                                    or tuple(weights.shape) not in ((T, K), (T * K,))):
            raise ValueError("weights must be floating point (%d, %d) or (%d,), got %s"
                             % (T, K, T * K, tuple(weights.shape) if torch.is_tensor(weights) else type(weights).__name__))
    if baseline == "mean" and K is not None and K < 2:
        raise ValueError("baseline=\"mean\" leaves one sample out: it needs K >= 2, got K = %d" % K)
    for t in (ids, weights):
        if t is not None and not t.is_cuda:
            raise _lib.SvpcKernelError("svpc_amd.ops: the self-critical step runs on the GPU only (no CPU fallback exists)")
    return SCST_BASELINES.index(baseline), utilities.index(utility), K


def scst_weights(reward, row_vid, baseline="greedy", greedy=None):
    """Per-caption weights of the self-critical loss from per-video rewards (svpc_scst_weights, one launch, no read-back):
    ``reward`` (N, K) float64, ``greedy`` (N,) float64 (``baseline="greedy"`` only), ``row_vid`` the T sentences' video index (an Idx or
    host ints) → (advantage (N, K) float64 = reward − baseline, w (T·K,) fp32 = fp32(advantage[vid(t), k] / (N·K)) at row t·K + k)."""
    if not torch.is_tensor(reward) or reward.dim() != 2 or reward.dtype != torch.float64:
        raise ValueError("scst_weights: reward must be float64 (N, K)")
    N, K = reward.shape
    rule, _, _ = check_scst(num_samples=K, baseline=baseline)
    if rule == 1:
        if not torch.is_tensor(greedy) or greedy.dtype != torch.float64 or tuple(greedy.shape) != (N,) or greedy.device != reward.device:
            raise ValueError("scst_weights: baseline=\"greedy\" needs the greedy rewards, float64 (%d,) on the rewards' device" % N)
    else:
        greedy = None
    rv = as_idx(row_vid)
    if any(not 0 <= b < N for b in rv.host):
        raise ValueError("scst_weights: a sentence's video index lies outside the %d videos" % N)
    _ops()._need_gpu(reward)
    reward = _c(reward)
    greedy = _c(greedy) if greedy is not None else None
    dev, T = reward.device, len(rv.host)
    adv = torch.empty(N, K, dtype=torch.float64, device=dev)
    w = torch.empty(T * K, dtype=torch.float32, device=dev)
    _lib.call("scst_weights", _p(reward), _p(greedy), _p(rv.dev(dev)) if T else None, N, K, T, rule, _p(adv), _p(w), _ops()._stream())
    return adv, w


class _SeqNll(Function):
    """``seq_nll``, and the base of the losses whose gradient is ``seq_nll``'s under weights of their own: they save those weights where
    ``row_w`` stands here and inherit the backward."""

    @staticmethod
    def forward(ctx, scores, rc, tgt, length, row_w, logits, unk_id, max_c):
        out = loss, cum, step, barred = _open(ctx, scores, tgt, (logits, unk_id, max_c))
        R, lt = tgt.shape
        _lib.call("seq_nll_fwd", _p(scores), scores.stride(0), _p(rc), max_c, _p(tgt), _p(length), _p(row_w), R, lt, logits, unk_id,
                  _p(step), _p(cum), _p(barred), _p(loss), _ops()._stream())
        ctx.save_for_backward(scores, rc, tgt, length, barred, row_w)
        return out

    @staticmethod
    def _bwd_args(saved, cfg, dl):
        scores, rc, tgt, length, barred, w = saved             # (w: a weight per caption, or per position under seq_pos_bwd)
        R, lt, logits, unk_id, max_c = cfg
        return (_p(scores), scores.stride(0), _p(rc), max_c, _p(tgt), _p(length), _p(barred), _p(w), _p(dl), R, lt, logits, unk_id)

    @staticmethod
    def backward(ctx, dl, *_):
        return _backward(ctx, dl, _SeqNll._bwd_args)


def seq_nll(scores, row_c, tgt, length, row_w, logits, unk_id, max_cols=None):
    """The weighted sequence log-likelihood loss of given captions from the decoder's score matrix (svpc_seq_nll_fwd / _bwd; DESIGN
    §11.10), differentiable in ``scores`` only: ``scores`` (≥ R·Lt, ≥ C) fp32 — row r·Lt + i is step i of caption row r; probabilities, or
    logits when ``logits`` —, ``row_c`` the R rows' column counts (an Idx or host ints), ``tgt`` (R, Lt) / ``length`` (R,) int32 as
    ``force_inputs`` returns them, ``row_w`` (R,) fp32 weights → (loss () fp32 = −Σ w_r·cum_r over the captions that are not barred, cum
    (R,) fp32, step (R, Lt − 1) fp32 — ``force_score``'s under ``unk="bar"`` —, barred (R,) int32: a scored position without a finite step
    score; such a caption adds nothing to the loss and gets an exactly zero gradient)."""
    R, lt = _score_head("seq_nll", scores, tgt, length)
    if not _row_vec(row_w, R, torch.float32, scores.device):
        raise ValueError("seq_nll: row_w must be contiguous fp32 (R,) on the scores' device")
    rc, max_c = _score_tail("seq_nll", scores, row_c, R, max_cols)
    _ops()._need_gpu(scores)
    return _SeqNll.apply(_c(scores), rc.dev(scores.device), tgt, length, row_w, 1 if logits else 0, int(unk_id), max_c)


# ------------------------------------------------------------------------------------------------ unlikelihood training
UL_RULES = ("token", "ngram")
UL_SCOPES = ("caption", "paragraph")
UL_MAX_NEG = 64                 # negatives per position: one lane each
UL_EPS = 1e-5                   # the clamp on 1 − p (svpc_seq_ul_fwd): a defined constant


def check_unlikelihood(rule="token", ngram=4, scope="caption", alpha=None, lt=None, m=None, neg=None, rows=None, device=None, row_w=None,
                       row_u=None, weights=None, ul_weights=None, shape=None):
    """Host checks of unlikelihood training (ValueError for each): ``rule`` "token" or "ngram"; ``ngram`` n in 1 … 4;
    ``scope`` "caption" or "paragraph"; ``alpha`` finite and not negative; ``lt`` at most 65 (one lane per scored position); ``m`` in
    1 … 64; ``neg`` a contiguous int32 (``rows``, ``lt`` − 1, M) table on ``device``; ``row_w`` / ``row_u`` contiguous fp32 (``rows``,) on
    ``device``; ``weights`` / ``ul_weights`` floating point of ``shape`` (T, K) or (T·K,).  ``SvpcKernelError`` for a tensor that is not on
    the GPU (no CPU fallback exists).  → (rule index, n, paragraph scope)."""
    if rule not in UL_RULES:
        raise ValueError("rule must be one of %s, got %r" % (", ".join(UL_RULES), rule))
    if isinstance(ngram, bool) or not isinstance(ngram, numbers.Integral) or not 1 <= int(ngram) <= 4:
        raise ValueError("unlikelihood penalises repeated n-grams of 1..4 words, got ngram = %r" % (ngram,))
    if scope not in UL_SCOPES:
        raise ValueError("scope must be one of %s, got %r" % (", ".join(UL_SCOPES), scope))
    _not_negative("alpha", alpha)
    if lt is not None and not 2 <= int(lt) <= UL_MAX_NEG + 1:
        raise ValueError("unlikelihood takes captions of 2..%d positions (one lane per scored position), got Lt = %d" % (UL_MAX_NEG + 1, lt))
    if neg is not None:
        if not torch.is_tensor(neg) or neg.dim() != 3:
            raise ValueError("neg must be an int32 (R, Lt - 1, M) table")
        m = neg.shape[2] if m is None else m
    if m is not None and not 1 <= int(m) <= UL_MAX_NEG:
        raise ValueError("1..%d negatives per position, got M = %d" % (UL_MAX_NEG, m))
    if neg is not None and (neg.dtype != torch.int32 or not neg.is_contiguous() or tuple(neg.shape) != (rows, int(lt) - 1, int(m))
                            or (device is not None and neg.device != device)):
        raise ValueError("neg must be a contiguous int32 (%s, %s, %s) table on the scores' device, got %s %s"
                         % (rows, int(lt) - 1, m, tuple(neg.shape), neg.dtype))
    _check_row_vecs(rows, device, row_w=row_w, row_u=row_u)
    _check_caption_weights(shape, weights=weights, ul_weights=ul_weights)
    for t in (neg, row_w, row_u, weights, ul_weights):
        if t is not None and not t.is_cuda:
            raise _lib.SvpcKernelError("svpc_amd.ops: unlikelihood training runs on the GPU only (no CPU fallback exists)")
    return UL_RULES.index(rule), int(ngram), scope == "paragraph"


def ul_negatives(tgt, length, finished, row_c, unk_id, eos, rule, ngram=4, scope="caption", sent_first=None, K=1):
    """The negatives of unlikelihood training, built on the device (svpc_ul_negatives, one launch, no read-back): ``tgt``
    (R, Lt) / ``length`` / ``finished`` (R,) int32 as ``force_inputs`` returns them under the end-of-caption id ``eos``, ``row_c`` the R
    rows' column counts → (neg (R, Lt − 1, M) int32, npen (R,) int32 the counted negatives, nrep (R,) int32 the repeat grams).
    ``rule="token"``: M = Lt − 1, the distinct earlier words of the caption without the position's target.  ``rule="ngram"``: M = 1, the
    word of every position inside a repeated ``ngram``-gram; ``scope="paragraph"`` also counts a gram of row t′·K + k of an earlier
    sentence t′ of the video — ``sent_first`` (R / K host ints or an Idx) names the first sentence of each sentence's video."""
    if tgt.dim() != 2 or tgt.shape[1] < 2 or not _id_rows(tgt, tgt.shape[0], tgt.shape[1]):
        raise ValueError("ul_negatives: tgt must be a contiguous int32 (R, Lt >= 2) matrix")
    R, lt = tgt.shape
    ri, n, paragraph = check_unlikelihood(rule, ngram, scope, lt=lt)
    if not _row_vec(length, R, torch.int32, tgt.device) or not _row_vec(finished, R, torch.int32, tgt.device):
        raise ValueError("ul_negatives: length and finished must be contiguous int32 (R,) on tgt's device")
    if not 0 <= int(unk_id) or int(eos) < 0:
        raise ValueError("ul_negatives: the UNK and EOS ids are columns")
    rc = as_idx(row_c)
    if len(rc.host) != R:
        raise ValueError("ul_negatives: one column count per caption row (%d), got %d" % (R, len(rc.host)))
    sf = None
    if ri == 1 and paragraph:
        if isinstance(K, bool) or not isinstance(K, numbers.Integral) or K < 1 or R % int(K):
            raise ValueError("ul_negatives: K = %r captions per sentence must divide the %d caption rows" % (K, R))
        if sent_first is None:
            raise ValueError("ul_negatives: scope=\"paragraph\" needs sent_first, the first sentence of every sentence's video")
        sf = as_idx(sent_first)
        if len(sf.host) != R // int(K) or any(not 0 <= int(f) <= t for t, f in enumerate(sf.host)):
            raise ValueError("ul_negatives: sent_first must name, for each of the %d sentences, a sentence at or before it" % (R // int(K)))
    _ops()._need_gpu(tgt)
    dev = tgt.device
    M = lt - 1 if ri == 0 else 1
    neg = torch.empty(R, lt - 1, M, dtype=torch.int32, device=dev)
    npen = torch.empty(R, dtype=torch.int32, device=dev)
    nrep = torch.empty(R, dtype=torch.int32, device=dev)
    _lib.call("ul_negatives", _p(tgt), _p(length), _p(finished), _p(rc.dev(dev)) if R else None, R, lt, int(unk_id), ri, n, 1 if paragraph else 0,
              _p(sf.dev(dev)) if sf is not None and R else None, int(K) if sf is not None else 1, _p(neg), _p(npen), _p(nrep), _ops()._stream())
    return neg, npen, nrep


class _SeqUl(Function):
    @staticmethod
    def forward(ctx, scores, rc, tgt, length, neg, row_w, row_u, logits, unk_id, max_c):
        R, lt = tgt.shape
        out = loss, cum, step, barred, ul, ulstep = _open(ctx, scores, tgt, (logits, unk_id, max_c),
                                                          (((R,), torch.float32), ((R, lt - 1), torch.float32)), bwd="seq_ul_bwd")
        _lib.call("seq_ul_fwd", _p(scores), scores.stride(0), _p(rc), max_c, _p(tgt), _p(length), _p(neg), neg.shape[2], _p(row_w), _p(row_u),
                  R, lt, logits, unk_id, _p(step), _p(ulstep), _p(cum), _p(ul), _p(barred), _p(loss), _ops()._stream())
        ctx.save_for_backward(scores, rc, tgt, length, barred, neg, row_w, row_u)
        return out

    @staticmethod
    def _bwd_args(saved, cfg, dl):
        scores, rc, tgt, length, barred, neg, row_w, row_u = saved
        R, lt, logits, unk_id, max_c = cfg
        return (_p(scores), scores.stride(0), _p(rc), max_c, _p(tgt), _p(length), _p(barred), _p(neg), neg.shape[2], _p(row_w), _p(row_u),
                _p(dl), R, lt, logits, unk_id)

    @staticmethod
    def backward(ctx, dl, *_):
        return _backward(ctx, dl, _SeqUl._bwd_args)


def seq_ul(scores, row_c, tgt, length, neg, row_w, row_u, logits, unk_id, max_cols=None):
    """``seq_nll`` plus the unlikelihood term (svpc_seq_ul_fwd / _bwd), differentiable in ``scores`` only: ``neg``
    (R, Lt − 1, M) int32 lists each position's negative columns (−1: none; ``ul_negatives`` builds the two rules' tables), ``row_u`` (R,)
    fp32 the captions' unlikelihood weights, the rest as ``seq_nll`` takes it → (loss () fp32 = −Σ w_r·cum_r + Σ u_r·ul_r over the captions
    that are not barred, cum, step, barred as ``seq_nll`` returns them — the same bits —, ul (R,) fp32, ulstep (R, Lt − 1) fp32: the sum
    over a position's counted negatives c of −log(1 − p_c), clamped at 1 − p_c = 1e-5).  With ``row_u`` all zero the loss and its gradient
    have ``seq_nll``'s bits."""
    R, lt = _score_head("seq_ul", scores, tgt, length)
    rc, max_c = _score_tail("seq_ul", scores, row_c, R, max_cols)
    check_unlikelihood(lt=lt, neg=neg, rows=R, device=scores.device, row_w=row_w, row_u=row_u)
    _ops()._need_gpu(scores)
    return _SeqUl.apply(_c(scores), rc.dev(scores.device), tgt, length, neg, row_w, row_u, 1 if logits else 0, int(unk_id), max_c)


# ------------------------------------------------------------------------------------------------ knowledge distillation
KD_LOG_EPS = -100.0 * math.log(2.0)     # log ε, ε = 2^-100: the clamp on the student's log-probability (svpc_seq_kd_fwd)


def check_distill(alpha=None, tq=None, tq_rows=None, max_cols=None, device=None, row_w=None, row_v=None, rows=None, weights=None,
                  kd_weights=None, shape=None, need_gpu=True):
    """Host checks of knowledge distillation (ValueError for each): ``alpha`` a finite number in [0, 1]; ``tq`` an fp32
    matrix of ``tq_rows`` rows (the student's row count) and at least ``max_cols`` columns, unit column stride, rows that do not overlap, on
    ``device``; ``row_w`` / ``row_v`` contiguous fp32 (``rows``,) on ``device``; ``weights`` / ``kd_weights`` floating point of ``shape``
    (T, K) or (T·K,).  ``SvpcKernelError`` for a tensor that is not on the GPU (no CPU fallback exists), unless ``need_gpu`` is off (a
    caller whose other checks come first)."""
    _number("alpha", alpha, lambda v: 0.0 <= v <= 1.0, "must be a finite number in [0, 1]")
    if tq is not None:
        if not torch.is_tensor(tq) or tq.dim() != 2 or tq.dtype != torch.float32:
            raise ValueError("tq, the teacher's score matrix, must be an fp32 (rows, columns) tensor, got %s" % _describe(tq))
        if device is not None and tq.device != device:
            raise ValueError("tq must be on the scores' device %s, got %s" % (device, tq.device))
        if tq_rows is not None and tq.shape[0] != tq_rows:
            raise ValueError("tq must have the student's %d score rows, got %d" % (tq_rows, tq.shape[0]))
        if max_cols is not None and tq.shape[1] < max_cols:
            raise ValueError("tq is narrower (%d columns) than max_cols = %d" % (tq.shape[1], max_cols))
        if (tq.shape[1] and tq.stride(1) != 1) or (tq.shape[0] > 1 and tq.stride(0) < (max_cols or tq.shape[1])):
            raise ValueError("tq must have unit column stride and rows that do not overlap, got strides %s" % (tuple(tq.stride()),))
    _check_row_vecs(rows, device, row_w=row_w, row_v=row_v)
    _check_caption_weights(shape, weights=weights, kd_weights=kd_weights)
    for t in (tq, row_w, row_v, weights, kd_weights):
        if need_gpu and t is not None and not t.is_cuda:
            raise _lib.SvpcKernelError("svpc_amd.ops: knowledge distillation runs on the GPU only (no CPU fallback exists)")


class _SeqKd(Function):
    @staticmethod
    def forward(ctx, scores, rc, tgt, length, tq, row_w, row_v, logits, teacher_logits, unk_id, max_c):
        R, lt = tgt.shape
        row, pos = ((R,), torch.float32), ((R, lt - 1), torch.float32)
        out = loss, cum, step, barred, kd, kdstep, ent, hstep = _open(ctx, scores, tgt, (logits, teacher_logits, unk_id, max_c),
                                                                      (row, pos, row, pos), bwd="seq_kd_bwd")
        _lib.call("seq_kd_fwd", _p(scores), scores.stride(0), _p(tq), tq.stride(0), _p(rc), max_c, _p(tgt), _p(length), _p(row_w), _p(row_v),
                  R, lt, logits, teacher_logits, unk_id, _p(step), _p(kdstep), _p(hstep), _p(cum), _p(kd), _p(ent), _p(barred), _p(loss),
                  _ops()._stream())
        ctx.save_for_backward(scores, rc, tgt, length, barred, tq, row_w, row_v)
        return out

    @staticmethod
    def _bwd_args(saved, cfg, dl):
        scores, rc, tgt, length, barred, tq, row_w, row_v = saved
        R, lt, logits, teacher_logits, unk_id, max_c = cfg
        return (_p(scores), scores.stride(0), _p(tq), tq.stride(0), _p(rc), max_c, _p(tgt), _p(length), _p(barred), _p(row_w), _p(row_v),
                _p(dl), R, lt, logits, teacher_logits, unk_id)

    @staticmethod
    def backward(ctx, dl, *_):
        return _backward(ctx, dl, _SeqKd._bwd_args)


def seq_kd(scores, row_c, tgt, length, tq, row_w, row_v, logits, teacher_logits, unk_id, max_cols=None):
    """``seq_nll`` plus the distillation term against a teacher's score matrix (svpc_seq_kd_fwd / _bwd), differentiable in
    ``scores`` only: ``tq`` (R·Lt, ≥ max_cols) fp32 — the teacher's scores of the same rows, any row stride; probabilities, or raw logits when
    ``teacher_logits`` —, ``row_v`` (R,) fp32 the captions' distillation weights, the rest as ``seq_nll`` takes it → (loss () fp32 =
    −Σ w_r·cum_r + Σ v_r·kd_r over the captions that are not barred, cum, step, barred as ``seq_nll`` returns them — the same bits —, kd
    (R,) fp32, kdstep (R, Lt − 1) fp32: the cross-entropy −Σ_c q_c·log p_c of the position's student row against its teacher row over
    the candidates, a log-probability under log 2^-100 clamped there with a zero gradient; ent (R,) / hstep (R, Lt − 1) fp32: the
    teacher's entropy −Σ_c q_c·log q_c, so kd − ent is the KL divergence of a teacher that sums to 1).  The teacher is not renormalised
    and gets no gradient.  With ``row_v`` all zero the loss and its gradient have ``seq_nll``'s bits."""
    R, lt = _score_head("seq_kd", scores, tgt, length)
    rc, max_c = _score_tail("seq_kd", scores, row_c, R, max_cols)
    check_distill(tq=tq, tq_rows=scores.shape[0], max_cols=max_c, device=scores.device, row_w=row_w, row_v=row_v, rows=R)
    _ops()._need_gpu(scores)
    return _SeqKd.apply(_c(scores), rc.dev(scores.device), tgt, length, tq.detach(), row_w, row_v, 1 if logits else 0,
                        1 if teacher_logits else 0, int(unk_id), max_c)


# ------------------------------------------------------------------------------------------------ contrastive (SimCTG) training
CL_MAX_LT = 32                  # a row's active partners are one 32-bit mask (svpc_seq_cl_fwd)
CL_ROW_BYTES = 144 * 1024       # a caption's Lt rows of D floats live in LDS


def check_simctg(margin=None, cl_weight=None, weights=None, cl_weights=None, shape=None, row_v=None, rows=None, device=None, need_gpu=True):
    """Host checks of contrastive (SimCTG) training (ValueError for each): ``margin`` a finite number in (0, 2] → its
    fp32-rounded value (a float); ``cl_weight`` finite and not negative; ``weights`` / ``cl_weights`` floating point of ``shape`` (T, K)
    or (T·K,); ``row_v`` contiguous fp32 (``rows``,) on ``device``.  ``SvpcKernelError`` for a tensor that is not on the GPU (no CPU
    fallback exists), unless ``need_gpu`` is off (a caller whose other checks come first)."""
    rho = None
    if margin is not None:
        _number("margin", margin, lambda v: 0.0 < v <= 2.0, "must be a finite number in (0, 2]")
        rho = float(torch.tensor(float(margin), dtype=torch.float32))
        if not rho > 0.0:
            raise ValueError("margin must be a finite number in (0, 2] after rounding to fp32, got %r" % (margin,))
    _not_negative("cl_weight", cl_weight)
    for name, t in (("weights", weights), ("cl_weights", cl_weights)):
        if t is not None and (not torch.is_tensor(t) or not t.is_floating_point()
                              or (shape is not None and tuple(t.shape) not in (tuple(shape), (shape[0] * shape[1],)))):
            raise ValueError("%s must be a floating point tensor%s, got %s"
                             % (name, " of shape %s or (%d,)" % (tuple(shape), shape[0] * shape[1]) if shape is not None else "",
                                _describe(t)))
    if row_v is not None and (not torch.is_tensor(row_v) or not _row_vec(row_v, rows, torch.float32, device)):
        raise ValueError("row_v must be contiguous fp32 (%s,) on the hidden rows' device" % (rows,))
    for t in (weights, cl_weights, row_v):
        if need_gpu and t is not None and not t.is_cuda:
            raise _lib.SvpcKernelError("svpc_amd.ops: contrastive training runs on the GPU only (no CPU fallback exists)")
    return rho


class _SeqCl(Function):
    @staticmethod
    def forward(ctx, hidden, length, row_v, rho, lt):
        R = length.shape[0]
        dev = hidden.device
        cl = torch.empty(R, dtype=torch.float32, device=dev)
        sim = torch.empty(R, dtype=torch.float32, device=dev)
        nact = torch.empty(R, dtype=torch.int32, device=dev)
        q = torch.empty(R, lt, dtype=torch.float64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        _lib.call("seq_cl_fwd", _p(hidden), hidden.stride(0), hidden.shape[1], _p(length), _p(row_v), R, lt, rho, _p(cl), _p(sim), _p(nact),
                  _p(q), _p(loss), _ops()._stream())
        ctx.save_for_backward(hidden, length, row_v)
        ctx.cfg = (R, lt, rho)
        ctx.mark_non_differentiable(cl, sim, nact, q)
        ctx.set_materialize_grads(False)
        return loss, cl, sim, nact, q

    @staticmethod
    def backward(ctx, dl, *_):
        if dl is None:
            return (None,) * 5
        hidden, length, row_v = ctx.saved_tensors
        R, lt, rho = ctx.cfg
        dl = _c(dl.to(torch.float32))
        dh = torch.empty(hidden.shape, dtype=torch.float32, device=hidden.device)          # (every element is written by the kernel)
        if hidden.shape[0] > R * lt:
            dh[R * lt:].zero_()
        _lib.call("seq_cl_bwd", _p(hidden), hidden.stride(0), hidden.shape[1], _p(length), _p(row_v), _p(dl), R, lt, rho, _p(dh), dh.shape[1],
                  _ops()._stream())
        return dh, None, None, None, None


def seq_cl(hidden, length, row_v, margin, lt, with_norms=False):
    """The contrastive (SimCTG) loss of given captions on the decoder's last-layer hidden states (svpc_seq_cl_fwd / _bwd),
    differentiable in ``hidden`` only: ``hidden`` (≥ R·Lt, D) fp32, unit column stride, any row stride ≥ D — row r·Lt + i is position i of
    caption row r —, ``length`` (R,) int32 as ``force_inputs`` returns it (the caption's token set is positions 0 … length, clamped into
    [0, Lt − 1] on the device), ``row_v`` (R,) fp32 weights, ``margin`` ρ in (0, 2] (rounded to fp32), 2 ≤ ``lt`` ≤ 32 → (loss () fp32 =
    Σ v_r·cl_r, cl (R,) fp32 the mean over the caption's ordered token pairs of max(0, ρ − 1 + cos(h_i, h_j)), sim (R,) fp32 the mean
    cosine of those pairs, nact (R,) int32 the pairs with ρ − 1 + cos > 0; all three 0 for a caption of one token).  ``with_norms``: also
    q (R, Lt) float64, the squared norms |h_i|² in contrastive search's summation order (0 past the end)."""
    rho = check_simctg(margin=margin)
    if rho is None:
        raise ValueError("margin must be a finite number in (0, 2], got None")
    if isinstance(lt, bool) or not isinstance(lt, numbers.Integral) or not 2 <= int(lt) <= CL_MAX_LT:
        raise ValueError("seq_cl takes captions of 2..%d positions, got Lt = %r" % (CL_MAX_LT, lt))
    lt = int(lt)
    if not torch.is_tensor(hidden) or hidden.dim() != 2 or hidden.dtype != torch.float32 or hidden.shape[1] < 1:
        raise ValueError("seq_cl: hidden must be fp32 (>= R·Lt, D >= 1) rows (convert a bf16 / split stream with ops.to_f32)")
    if not torch.is_tensor(length) or length.dim() != 1 or not _row_vec(length, length.shape[0], torch.int32, hidden.device):
        raise ValueError("seq_cl: length must be contiguous int32 (R,) on the hidden rows' device")
    R, D = length.shape[0], hidden.shape[1]
    if hidden.shape[0] < R * lt:
        raise ValueError("seq_cl: %d caption rows of %d positions need %d hidden rows, got %d" % (R, lt, R * lt, hidden.shape[0]))
    if lt * D * 4 > CL_ROW_BYTES:
        raise ValueError("seq_cl: a caption's Lt·D = %d·%d floats do not fit the kernel's %d KB of LDS" % (lt, D, CL_ROW_BYTES // 1024))
    check_simctg(row_v=row_v, rows=R, device=hidden.device)
    _ops()._need_gpu(hidden)
    if hidden.stride(1) != 1 or (hidden.shape[0] > 1 and hidden.stride(0) < D):
        hidden = hidden.contiguous()
    out = _SeqCl.apply(hidden, length, row_v, rho, lt)
    return out if with_norms else out[:4]


# ------------------------------------------------------------------------------------------------ minimum-risk and ranking training
RISK_MAX = SCST_MAX             # candidates per sentence: one lane each (svpc_seq_risk_fwd)
RISK_SOURCES = ("sample", "nbest", "diverse", "stochastic")


def check_risk(k=None, cost=None, vid_off=None, n_sent=None, alpha=None, length_beta=None, margin=None, risk_weight=None, rank_weight=None,
               source=None, utility=None, device=None):
    """Host checks of minimum-risk / ranking training (ValueError for each): ``k`` K in 1 … 16; ``cost`` float64 (N, K)
    (on ``device``, when given); ``vid_off`` N + 1 host ints (or an Idx) that start at 0, never fall and end at ``n_sent``; ``alpha``,
    ``length_beta``, ``margin``, ``risk_weight`` and ``rank_weight`` finite and not negative; ``source`` one of the four candidate-set
    decoders; ``utility`` one of the six score columns.  ``SvpcKernelError`` for a cost that is not on the GPU (no CPU fallback exists).
    → (K, N, the utility's column or None)."""
    for name, v in (("alpha", alpha), ("length_beta", length_beta), ("margin", margin), ("risk_weight", risk_weight),
                    ("rank_weight", rank_weight)):
        _not_negative(name, v)
    return _check_candidates(k, cost, vid_off, n_sent, source, utility, device)


class _SeqRisk(_SeqNll):
    """(the objective's derivative in cum is −w_eff: the gradient is ``seq_nll``'s under the effective weights, bit for bit)"""

    @staticmethod
    def forward(ctx, scores, rc, tgt, length, cost, off, row_w, logits, unk_id, max_c, params):
        R, lt = tgt.shape
        N, K = cost.shape
        vid, table = ((N,), torch.float64), ((N, K), torch.float64)
        out = loss, cum, step, barred, risk, rank, q, z, valid, w_eff = _open(
            ctx, scores, tgt, (logits, unk_id, max_c), (vid, vid, table, table, ((N, K), torch.int32), ((R,), torch.float32)))
        _lib.call("seq_risk_fwd", _p(scores), scores.stride(0), _p(rc), max_c, _p(tgt), _p(length), _p(row_w), _p(cost), _p(off), N, R // K, K,
                  lt, logits, unk_id, *params, _p(step), _p(cum), _p(barred), _p(risk), _p(rank), _p(q), _p(z), _p(valid), _p(w_eff), _p(loss),
                  _ops()._stream())
        ctx.save_for_backward(scores, rc, tgt, length, barred, w_eff)
        return out


def seq_risk(scores, row_c, tgt, length, cost, vid_off, row_w, logits, unk_id, alpha, length_beta, margin, risk_weight, rank_weight,
             max_cols=None):
    """``seq_nll`` plus the minimum-risk and ranking terms over every video's K candidate paragraphs (svpc_seq_risk_fwd, and svpc_seq_nll_bwd
    under the effective weights), differentiable in ``scores`` only: caption row r = t·K + k, ``cost`` (N, K) float64 the
    candidates' costs (a non-finite cost takes its candidate out), ``vid_off`` N + 1 host ints (or an Idx): the sentences of video b are
    t = vid_off[b] … vid_off[b + 1] − 1, ``row_w`` (R,) fp32 the captions' likelihood weights (None: zeros), the rest as ``seq_nll`` takes
    it → (loss () fp32 = −Σ w_r·cum_r + (risk_weight·Σ_b risk + rank_weight·Σ_b rank) / N, cum, step, barred as ``seq_nll`` returns them —
    the same bits —, risk (N,) / rank (N,) / Q (N, K) / z (N, K) float64, valid (N, K) int32, w_eff (R,) fp32: the weights under which
    ``seq_nll``'s gradient is this loss's).  With both weights zero the loss and its gradient have ``seq_nll``'s bits."""
    R, lt = _score_head("seq_risk", scores, tgt, length)
    K, _, _ = check_risk(cost=cost, alpha=alpha, length_beta=length_beta, margin=margin, risk_weight=risk_weight, rank_weight=rank_weight,
                         device=scores.device)
    off, row_w = _candidate_rows("seq_risk", scores, R, K, cost, vid_off, row_w)
    rc, max_c = _score_tail("seq_risk", scores, row_c, R, max_cols)
    _ops()._need_gpu(scores)
    params = tuple(float(v) for v in (alpha, length_beta, margin, risk_weight, rank_weight))
    return _SeqRisk.apply(_c(scores), rc.dev(scores.device) if R else None, tgt, length, _c(cost), off.dev(scores.device), row_w,
                          1 if logits else 0, int(unk_id), max_c, params)


# ------------------------------------------------------------------------------------------------ preference optimisation
PREF_MAX = RISK_MAX             # candidates per sentence: one lane each (svpc_seq_pref_fwd)
PREF_LOSS_TYPES = ("sigmoid", "hinge", "ipo")
PREF_PAIRS = ("all", "extremes")


def check_pref(k=None, cost=None, vid_off=None, n_sent=None, ref_cum=None, rows=None, beta=None, gamma=None, label_smoothing=None,
               length_beta=None, pref_weight=None, loss_type=None, pairs=None, source=None, utility=None, device=None):
    """Host checks of preference optimisation (ValueError for each): ``k`` / ``cost`` / ``vid_off`` / ``n_sent`` /
    ``source`` / ``utility`` as ``check_risk`` takes them; ``beta`` finite and > 0; ``gamma``, ``length_beta`` and ``pref_weight`` finite
    and not negative; ``label_smoothing`` in [0, 0.5) and 0 outside ``loss_type`` "sigmoid"; ``gamma`` 0 under "ipo"; ``loss_type`` one of
    sigmoid / hinge / ipo; ``pairs`` one of all / extremes; ``ref_cum`` a contiguous fp32 tensor of ``rows`` elements (on ``device``, when
    given).  ``SvpcKernelError`` for a cost or a ref_cum that is not on the GPU (no CPU fallback exists).  → (K, N, the utility's column
    or None, the loss type's index or None, the pair mode's index or None)."""
    _number("beta", beta, lambda v: v > 0, "must be a finite number > 0")
    for name, v in (("gamma", gamma), ("length_beta", length_beta), ("pref_weight", pref_weight)):
        _not_negative(name, v)
    _number("label_smoothing", label_smoothing, lambda v: 0 <= v < 0.5, "must lie in [0, 0.5)", finite=False)
    if loss_type is not None and loss_type not in PREF_LOSS_TYPES:
        raise ValueError("loss_type must be one of %s, got %r" % (", ".join(PREF_LOSS_TYPES), loss_type))
    if pairs is not None and pairs not in PREF_PAIRS:
        raise ValueError("pairs must be one of %s, got %r" % (", ".join(PREF_PAIRS), pairs))
    kind = loss_type if loss_type is not None else "sigmoid"
    if label_smoothing and kind != "sigmoid":
        raise ValueError("label_smoothing belongs to the sigmoid loss, got %r with loss_type %r" % (label_smoothing, kind))
    if gamma and kind == "ipo":
        raise ValueError("the ipo loss takes no gamma, got %r" % (gamma,))
    if ref_cum is not None:
        if (not torch.is_tensor(ref_cum) or ref_cum.dtype != torch.float32 or not ref_cum.is_contiguous()
                or (rows is not None and ref_cum.numel() != rows)):
            raise ValueError("ref_cum must be contiguous fp32 of %s elements (one per caption row), got %s" % (rows, _describe(ref_cum)))
        if device is not None and ref_cum.device != device:
            raise ValueError("ref_cum must be on the scores' device %s, got %s" % (device, ref_cum.device))
    K, N, col = _check_candidates(k, cost, vid_off, n_sent, source, utility, device)
    if ref_cum is not None and not ref_cum.is_cuda:
        raise _lib.SvpcKernelError("svpc_amd.ops: preference optimisation runs on the GPU only (no CPU fallback exists)")
    return (K, N, col, None if loss_type is None else PREF_LOSS_TYPES.index(loss_type), None if pairs is None else PREF_PAIRS.index(pairs))


class _SeqPref(_SeqNll):
    """(the objective's derivative in cum is −w_eff: the gradient is ``seq_nll``'s under the effective weights, bit for bit)"""

    @staticmethod
    def forward(ctx, scores, rc, tgt, length, cost, off, ref_cum, row_w, logits, unk_id, max_c, params, kinds):
        R, lt = tgt.shape
        N, K = cost.shape
        out = loss, cum, step, barred, pref, reward, valid, n_pairs, n_correct, margin, w_eff = _open(
            ctx, scores, tgt, (logits, unk_id, max_c),
            (((N,), torch.float64), ((N, K), torch.float64), ((N, K), torch.int32), ((N,), torch.int32), ((N,), torch.int32),
             ((N,), torch.float64), ((R,), torch.float32)))
        _lib.call("seq_pref_fwd", _p(scores), scores.stride(0), _p(rc), max_c, _p(tgt), _p(length), _p(row_w), _p(cost), _p(ref_cum), _p(off),
                  N, R // K, K, lt, logits, unk_id, *params, *kinds, _p(step), _p(cum), _p(barred), _p(pref), _p(reward), _p(valid),
                  _p(n_pairs), _p(n_correct), _p(margin), _p(w_eff), _p(loss), _ops()._stream())
        ctx.save_for_backward(scores, rc, tgt, length, barred, w_eff)
        return out


def seq_pref(scores, row_c, tgt, length, cost, vid_off, ref_cum, row_w, logits, unk_id, beta, gamma, label_smoothing, length_beta,
             pref_weight, loss_type, pairs, max_cols=None):
    """``seq_nll`` plus the preference term over every video's K candidate paragraphs (svpc_seq_pref_fwd, and svpc_seq_nll_bwd under the
    effective weights), differentiable in ``scores`` only: caption row r = t·K + k, ``cost`` (N, K) float64 the candidates'
    costs (lower is preferred; a non-finite cost takes its candidate out), ``vid_off`` as ``seq_risk`` takes it, ``ref_cum`` (R,) fp32 the
    frozen reference model's ``cum`` of the same captions (a non-finite entry takes its candidate out; None: reference-free, the bits of
    an all-zero ``ref_cum``), ``row_w`` (R,) fp32 the captions' likelihood weights (None: zeros), the rest as ``seq_nll`` takes it.  u =
    (Σ_t cum − Σ_t ref_cum) / (Σ_t len)^``length_beta``; over the pairs (i, j) of valid candidates with cost_i < cost_j (``pairs`` "all")
    or the best against the worst (``"extremes"``): d = u_i − u_j, h = ``beta``·d − ``gamma``, ℓ = −(1 − ε)·ln σ(h) − ε·ln σ(−h)
    (``loss_type`` "sigmoid", ε = ``label_smoothing``), max(0, 1 − h) ("hinge") or (d − 1 / (2·beta))² ("ipo"); pref[b] = the mean of ℓ over
    the video's pairs.  → (loss () fp32 = −Σ w_r·cum_r + ``pref_weight``·Σ_b pref / N, cum, step, barred as ``seq_nll`` returns them — the
    same bits —, pref (N,) float64, reward (N, K) float64 = beta·u the implicit reward, valid (N, K) int32, n_pairs / n_correct (N,) int32
    (the pairs, and those with d > 0), margin (N,) float64 = the mean of beta·d over the pairs, w_eff (R,) fp32: the weights under which
    ``seq_nll``'s gradient is this loss's).  With ``pref_weight`` = 0 the loss and its gradient have ``seq_nll``'s bits."""
    R, lt = _score_head("seq_pref", scores, tgt, length)
    K, _, _, kind, mode = check_pref(cost=cost, ref_cum=ref_cum, rows=R, beta=beta, gamma=gamma, label_smoothing=label_smoothing,
                                     length_beta=length_beta, pref_weight=pref_weight, loss_type=loss_type, pairs=pairs, device=scores.device)
    if kind is None or mode is None:
        raise ValueError("seq_pref: loss_type must be one of %s and pairs one of %s" % (", ".join(PREF_LOSS_TYPES), ", ".join(PREF_PAIRS)))
    off, row_w = _candidate_rows("seq_pref", scores, R, K, cost, vid_off, row_w)
    rc, max_c = _score_tail("seq_pref", scores, row_c, R, max_cols)
    _ops()._need_gpu(scores)
    params = tuple(float(v) for v in (beta, gamma, label_smoothing, length_beta, pref_weight))
    return _SeqPref.apply(_c(scores), rc.dev(scores.device) if R else None, tgt, length, _c(cost), off.dev(scores.device), ref_cum, row_w,
                          1 if logits else 0, int(unk_id), max_c, params, (kind, mode))


# ------------------------------------------------------------------------------------------------ clipped policy-gradient training
PG_MAX = RISK_MAX               # candidates per sentence: one lane each (svpc_seq_pg_fwd)
PG_NORMS = ("sequence", "token", "none")
PG_ADVANTAGES = ("grpo", "center", "rloo")
_PG = "policy-gradient training"


def check_pg(k=None, adv=None, vid_off=None, n_sent=None, old_step=None, ref_step=None, rows=None, lt=None, clip_lo=None, clip_hi=None,
             dual_clip=None, kl_beta=None, norm=None, advantage=None, eps=None, has_ref=None, source=None, utility=None, device=None):
    """Host checks of clipped policy-gradient training (ValueError for each): ``k`` / ``vid_off`` / ``n_sent`` / ``source``
    / ``utility`` as ``check_risk`` takes them, ``adv`` as it takes ``cost`` (float64 (N, K)); ``clip_lo`` finite in [0, 1); ``clip_hi``
    and ``kl_beta`` finite and not negative; ``dual_clip`` 0 (off) or finite and > 1; ``norm`` one of sequence / token / none;
    ``advantage`` one of grpo / center / rloo; ``eps`` finite and not negative; ``old_step`` / ``ref_step`` contiguous fp32 tensors of
    ``rows``·(``lt`` − 1) elements (on ``device``, when given); ``kl_beta`` > 0 without a reference (``has_ref`` False, or ``rows`` given
    and no ``ref_step``).  ``SvpcKernelError`` for an adv, old_step or ref_step that is not on the GPU (no CPU fallback exists).  → (K, N,
    the utility's column or None, the norm's index or None, the advantage rule's index or None)."""
    _number("clip_lo", clip_lo, lambda v: 0 <= v < 1, "must be a finite number in [0, 1)")
    _not_negative("clip_hi", clip_hi)
    _number("dual_clip", dual_clip, lambda v: v == 0 or v > 1, "must be 0 (off) or a finite number > 1")
    _not_negative("kl_beta", kl_beta)
    _not_negative("eps", eps)
    if norm is not None and norm not in PG_NORMS:
        raise ValueError("norm must be one of %s, got %r" % (", ".join(PG_NORMS), norm))
    if advantage is not None and advantage not in PG_ADVANTAGES:
        raise ValueError("advantage must be one of %s, got %r" % (", ".join(PG_ADVANTAGES), advantage))
    if has_ref is None and rows is not None:
        has_ref = ref_step is not None
    if kl_beta and has_ref is False:
        raise ValueError("kl_beta = %r needs the reference model's step scores (ref_step)" % (kl_beta,))
    for name, t in (("old_step", old_step), ("ref_step", ref_step)):
        if t is None:
            continue
        want = None if rows is None or lt is None else rows * (lt - 1)
        if not torch.is_tensor(t) or t.dtype != torch.float32 or not t.is_contiguous() or (want is not None and t.numel() != want):
            raise ValueError("%s must be contiguous fp32 of %s elements (one per caption row and scored position), got %s"
                             % (name, want, _describe(t)))
        if device is not None and t.device != device:
            raise ValueError("%s must be on the scores' device %s, got %s" % (name, device, t.device))
    _check_table("adv", adv)                                     # (before the candidate checks, whose first is ``k``)
    K, N, col = _check_candidates(k, adv, vid_off, n_sent, source, utility, device, what="adv", objective=_PG)
    for t in (old_step, ref_step):
        if t is not None and not t.is_cuda:
            raise _lib.SvpcKernelError("svpc_amd.ops: %s runs on the GPU only (no CPU fallback exists)" % _PG)
    return (K, N, col, None if norm is None else PG_NORMS.index(norm), None if advantage is None else PG_ADVANTAGES.index(advantage))


def group_advantage(reward, rule="grpo", eps=1e-6):
    """The candidates' advantages from their rewards (svpc_group_advantage, one launch, no read-back): ``reward`` (N, K)
    float64 → adv (N, K) float64, per video over its candidates with a finite reward in ascending k (the others get 0): ``rule`` "grpo"
    (r − mean) / (std + ``eps``) with the population std, "center" r − mean, "rloo" r − the mean of the other finite rewards
    (``scst_weights``' leave-one-out rule, unscaled).  With fewer than two finite rewards, or the largest equal to the smallest, every
    advantage of the video is exactly 0."""
    if not torch.is_tensor(reward) or reward.dim() != 2 or reward.dtype != torch.float64:
        raise ValueError("group_advantage: reward must be float64 (N, K)")
    N, K = reward.shape
    _, _, _, _, r = check_pg(k=K, advantage=rule, eps=eps)
    _ops()._need_gpu(reward)
    reward = _c(reward)
    adv = torch.empty(N, K, dtype=torch.float64, device=reward.device)
    _lib.call("group_advantage", _p(reward), N, K, r, float(eps), _p(adv), _ops()._stream())
    return adv


class _SeqPg(_SeqNll):
    """(the objective's derivative in step[r, i] is −pos_w[r, i] on every caption that is not barred: ``seq_nll``'s backward with the
    weight read per position, svpc_seq_pos_bwd)"""

    @staticmethod
    def forward(ctx, scores, rc, tgt, length, adv, off, old_step, ref_step, row_w, logits, unk_id, max_c, params, norm):
        R, lt = tgt.shape
        N, K = adv.shape
        dev = scores.device
        out = loss, cum, step, barred, pos_w, pg, kl, n_clip, ratio_max, valid, n_tok = _open(
            ctx, scores, tgt, (logits, unk_id, max_c),
            (((R, lt - 1), torch.float32), ((R,), torch.float64), ((R,), torch.float64), ((R, 2), torch.int32), ((R,), torch.float32),
             ((N, K), torch.int32), ((1,), torch.int32)), bwd="seq_pos_bwd")
        row_f = torch.empty(2, R, dtype=torch.float64, device=dev)           # (the launches' own tables: row_adv, row_tok)
        row_n = torch.empty(R, dtype=torch.int32, device=dev)
        _lib.call("seq_pg_fwd", _p(scores), scores.stride(0), _p(rc), max_c, _p(tgt), _p(length), _p(row_w), _p(adv), _p(old_step),
                  _p(ref_step), _p(off), N, R // K, K, lt, logits, unk_id, *params, norm, _p(step), _p(cum), _p(barred), _p(pos_w), _p(pg),
                  _p(kl), _p(n_clip), _p(ratio_max), _p(valid), _p(n_tok), _p(row_f[0]), _p(row_n), _p(row_f[1]), _p(loss), _ops()._stream())
        ctx.save_for_backward(scores, rc, tgt, length, barred, pos_w)
        return out


def seq_pg(scores, row_c, tgt, length, adv, vid_off, old_step, ref_step, row_w, logits, unk_id, clip_lo=0.2, clip_hi=0.2, dual_clip=0.0,
           kl_beta=0.0, norm="sequence", max_cols=None):
    """``seq_nll`` plus the clipped policy-gradient term over every video's K candidate paragraphs (svpc_seq_pg_fwd / svpc_seq_pos_bwd;
    DESIGN §11.22), differentiable in ``scores`` only: caption row r = t·K + k, ``adv`` (N, K) float64 the candidates' advantages (a
    non-finite one takes its candidate out), ``vid_off`` as ``seq_risk`` takes it, ``old_step`` / ``ref_step`` (R, Lt − 1) fp32 the
    behaviour policy's and the frozen reference model's step scores of the same captions (a non-finite entry at a scored position takes
    its candidate out; no ``old_step``: the ratio is exactly 1; no ``ref_step``: no KL term), ``row_w`` (R,) fp32 the captions'
    likelihood weights (None: zeros), the rest as ``seq_nll`` takes it.  Per scored position of a valid candidate: ρ = exp(step −
    old_step), sur = min(ρ·A, clamp(ρ, 1 − ``clip_lo``, 1 + ``clip_hi``)·A), under ``dual_clip`` = c > 1 and A < 0 max(sur, c·A); kl =
    exp(δ) − δ − 1 with δ = ref_step − step; tok = −sur + ``kl_beta``·kl, divided by N·K·n (``norm`` "sequence", n the candidate's scored
    positions), by the scored positions of all valid candidates ("token") or by N·K ("none").  → (loss () fp32 = −Σ w_r·cum_r + Σ tok /
    den, cum, step, barred as ``seq_nll`` returns them — the same bits —, pos_w (R, Lt − 1) fp32: the weight per position under which
    ``seq_nll``'s gradient is this loss's, pg / kl (R,) float64 the rows' sums of −sur and kl, n_clip (R, 2) int32 the positions clipped
    from above / from below, ratio_max (R,) fp32, valid (N, K) int32, n_tok (1,) int32).  With every advantage 0 and ``kl_beta`` = 0 the
    loss and its gradient have ``seq_nll``'s bits."""
    R, lt = _score_head("seq_pg", scores, tgt, length)
    K, _, _, kind, _ = check_pg(adv=adv, old_step=old_step, ref_step=ref_step, rows=R, lt=lt, clip_lo=clip_lo, clip_hi=clip_hi,
                                dual_clip=dual_clip, kl_beta=kl_beta, norm=norm, device=scores.device)
    if kind is None or K is None:
        raise ValueError("seq_pg: adv must be float64 (N, K) and norm one of %s" % ", ".join(PG_NORMS))
    off, row_w = _candidate_rows("seq_pg", scores, R, K, adv, vid_off, row_w, what="adv", objective=_PG)
    rc, max_c = _score_tail("seq_pg", scores, row_c, R, max_cols)
    _ops()._need_gpu(scores)
    params = tuple(float(v) for v in (clip_lo, clip_hi, dual_clip, kl_beta))
    return _SeqPg.apply(_c(scores), rc.dev(scores.device) if R else None, tgt, length, _c(adv), off.dev(scores.device), old_step, ref_step,
                        row_w, 1 if logits else 0, int(unk_id), max_c, params, kind)
