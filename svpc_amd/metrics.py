"""Training / validation counters kept on the MI355X.

reference: src/train.py:32-38 (cal_performance: correct next-word predictions over labelled positions), :40-49 (calculate_f1:
hits / gold positives / predicted positives of the entity and action probabilities at threshold 0.5), :51-68 (compute_total_f1),
:150-180 (per-step accumulation with ≈10 ``.item()`` host synchronisations).  Here the nine running sums live in one device buffer
updated by two small kernels per video; ``result()`` is the only host read-back.

``DecodeMetrics`` is the evaluation-side counterpart: the captions the reference submits and its repetition / diversity numbers
(src/translate.py:27-42 and :81-83, recursive_caption_dataset.py:472-500, densevid_eval/evaluateRepetition.py,
evaluateCaptionsDiversity.py:219-282, get_caption_stat.py) from the translator's id matrices, three launches per batch and no host
synchronisation until ``result()``.  ``IngredientF1`` adds the ingredient-prediction recall / precision / F1 of
src/calculate_ingredient_f1.py from the same clean captions, ``CaptionScores`` Bleu_1…4, ROUGE_L and CIDEr against
reference paragraphs (densevid_eval/para-evaluate.py without METEOR), ``ForcedScores`` the gold score and perplexity of
given captions under decoding conditions (the GOLD numbers of the reference decoder's OpenNMT lineage).
"""
from __future__ import annotations

import torch

from . import _lib, ops
from .caption_plan import RowTables
from .synthetic import EOS, PAD

IGNORE = -1


def compute_total_f1(n_correct, n_recall, n_precision):
    """src/train.py:51-68."""
    recall = 0 if n_recall == 0 else n_correct / n_recall
    precision = 0 if n_precision == 0 else n_correct / n_precision
    f1 = 0 if (recall == 0 and precision == 0) else 2 * (recall * precision) / (recall + precision)
    return {"recall": recall, "precision": precision, "f1": f1}


class TrainMetrics:
    """counters: [n_word, n_word_correct, ent_correct, ent_recall, ent_precision, ac_correct, ac_recall, ac_precision, loss_sum]"""

    def __init__(self, device="cuda"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SvpcKernelError("svpc_amd.metrics: counters live on the GPU (no CPU fallback)")
        self.c = torch.zeros(9, dtype=torch.float64, device=self.device)

    def reset(self):
        self.c.zero_()

    def _stream(self):
        return torch.cuda.current_stream().cuda_stream

    def add_words(self, pred_scores, labels):
        """pred_scores (S, Lt, C) probabilities / logits of one video, labels (S, Lt) int64 with IGNORE = -1."""
        C = pred_scores.shape[-1]
        p = pred_scores.detach().reshape(-1, C)
        if p.stride(1) != 1:
            p = p.contiguous()
        lab = labels.reshape(-1).to(torch.int64).contiguous()
        _lib.call("metric_argmax", p.data_ptr(), p.stride(0), p.shape[0], C, lab.data_ptr(), IGNORE, self.c.data_ptr(), self._stream())

    def add_f1(self, prob, gold, which):
        """which = "entity" | "action"."""
        off = 2 if which == "entity" else 5
        pr = prob.detach().reshape(-1).float().contiguous()
        gd = gold.reshape(-1).float().contiguous()
        _lib.call("metric_f1", pr.data_ptr(), gd.data_ptr(), pr.numel(), self.c.data_ptr() + 8 * off, self._stream())

    def update(self, loss, pred_scores_list, labels_list, entity_prob_list=(), alignments=(), action_prob_list=(), actions=()):
        """One training / validation step (src/train.py:150-171), no host synchronisation."""
        for p, g in zip(pred_scores_list, labels_list):
            self.add_words(p, g)
        for p, g in zip(entity_prob_list, alignments):
            self.add_f1(p, g, "entity")
        for p, g in zip(action_prob_list, actions):
            self.add_f1(p, g, "action")
        if loss is not None:
            self.c[8] += loss.detach().double()

    def result(self):
        """The single host read-back: totals and the derived numbers the reference logs (src/train.py:178-185)."""
        v = [float(x) for x in self.c.cpu()]
        n_word, n_corr = v[0], v[1]
        return dict(n_word_total=n_word, n_word_correct=n_corr, total_loss=v[8],
                    loss_per_word=(v[8] / n_word) if n_word else 0.0, accuracy=(n_corr / n_word) if n_word else 0.0,
                    entity=compute_total_f1(v[2], v[3], v[4]), action=compute_total_f1(v[5], v[6], v[7]),
                    counts=v[:8])


def _gpu_device(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.SvpcKernelError("svpc_amd.metrics: counters live on the GPU (no CPU fallback)")
    return device


def _clean_rows(dec_seq_list, row, clean=None, video_cap=True, pad=PAD, eos=EOS, remove_dup=True):
    """The opening of every ``update``: a decode's per-video ids as one tensor, checked (``video_cap``: with the 4096 positions a video's
    captions may hold), on the GPU, and cleaned unless ``clean=(words, len)`` brings the clean-up → (words, len, steps, device)."""
    ids, steps = ops.stack_captions(dec_seq_list)
    lt = ids.shape[-1]
    ops.check_caption_metrics(lt, ids.dtype, steps=steps if video_cap else None, k=ids.shape[1] if ids.dim() == 3 else None, row=row)
    if not ids.is_cuda:
        raise _lib.SvpcKernelError("svpc_amd.metrics: captions must be on the GPU (no CPU fallback)")
    if clean is None:
        clean = ops.clean_captions(ids, pad, eos, IGNORE, remove_dup, row=row)
    words, ln = clean
    if tuple(words.shape) != (ids.shape[0], lt):
        raise ValueError("clean=(words, len) must be the clean-up of these %d rows of %d positions" % (ids.shape[0], lt))
    return words, ln, steps, ids.device


class DecodeMetrics:
    """Running repetition / diversity / caption statistics of an evaluation epoch, kept on the device.

    ``update(dec_seq_list, row=0)`` takes what ``Translator.translate_batch`` / ``translate_batch_beam`` (first element) /
    ``translate_batch_nbest`` / ``translate_batch_sample`` return: per video an (S_b, Lt) or (S_b, K, Lt) id tensor (``row`` picks one of
    the K).  Clean caption → per-video n-gram counts → accumulator: three launches for the whole batch, no copy when the list is
    consecutive views of one buffer (one ``torch.cat`` otherwise), nothing uploaded for a recurring (S_b) structure — so ``update`` can be
    captured once its structure has been seen.  ``result()`` is the only read-back.

    accumulator: [Σ re1..4, Σ div1..4, videos, sentences, clean words, empty captions, copied words (id ≥ V)]; ``vocab_bits`` marks the
    ids < V seen among the clean words.  ``last_counts``: the last update's (N, 12) int32 per-video counts (total_1..4, distinct_1..4,
    n_sen, n_words, n_empty, n_copied)."""

    FIELDS = ("re1", "re2", "re3", "re4", "div1", "div2", "div3", "div4")

    def __init__(self, vocab_size, device="cuda", pad=PAD, eos=EOS, period_id=None, comma_id=None, remove_dup=True):
        self.device = _gpu_device(device)
        self.V = int(vocab_size)
        if self.V < 1:
            raise ValueError("vocab_size must be >= 1, got %r" % (vocab_size,))
        ops.check_caption_metrics(1, period_id=period_id, comma_id=comma_id)
        self.pad, self.eos, self.period_id, self.comma_id, self.remove_dup = int(pad), int(eos), period_id, comma_id, bool(remove_dup)
        self.acc = torch.zeros(13, dtype=torch.float64, device=self.device)
        self.vocab_bits = torch.zeros((self.V + 31) // 32, dtype=torch.int32, device=self.device)
        self.last_counts = None
        self.last_clean = None              # the last update's (words, len): IngredientF1.update(..., clean=) reuses it
        self._offs = RowTables()

    def reset(self):
        self.acc.zero_()
        self.vocab_bits.zero_()
        self.last_counts = self.last_clean = None

    def _vid_off(self, steps, dev):
        """the (N + 1,) int32 table of the videos' first rows: uploaded once per (S_b) structure"""
        return self._offs.table(steps, dev)

    def update(self, dec_seq_list, row=0):
        words, ln, steps, dev = _clean_rows(dec_seq_list, row, pad=self.pad, eos=self.eos, remove_dup=self.remove_dup)
        counts = ops.caption_ngram_counts(words, ln, self._vid_off(steps, dev), self.V, self.period_id, self.comma_id,
                                          vocab_bits=self.vocab_bits, steps=steps)
        ops.decode_metric_accum(counts, self.acc)
        self.last_counts, self.last_clean = counts, (words, ln)
        return counts

    def result(self):
        """The single host read-back → re1..re4, div1..div4 (means over the videos seen), num_videos, num_sen, num_words, avg_sen_len,
        num_empty, num_copied, vocab_size."""
        v = [float(x) for x in self.acc.cpu()]
        bits = self.vocab_bits.cpu().numpy().view("uint32")
        nv = int(v[8])
        res = {k: (v[i] / nv if nv else 0.0) for i, k in enumerate(self.FIELDS)}
        num_sen, num_words = int(v[9]), int(v[10])
        res.update(num_videos=nv, num_sen=num_sen, num_words=num_words, avg_sen_len=(num_words / num_sen) if num_sen else 0.0,
                   num_empty=int(v[11]), num_copied=int(v[12]), vocab_size=int(sum(bin(int(x)).count("1") for x in bits[bits != 0])))
        return res


class IngredientF1:
    """Running ingredient-prediction recall / precision / F1 (src/calculate_ingredient_f1.py) of an evaluation epoch, kept on the device.

    ``update(dec_seq_list, plan, row=0, clean=None)`` takes what any ``translate_batch*`` returns and ``lexicon.plan(videos)`` of the same
    videos (with ``gt_sentences``); ``clean=(words, len)`` reuses a clean-up already made with run collapse on (``ops.clean_captions`` of
    the same rows, or ``DecodeMetrics.last_clean`` after its ``update`` of the same result and row), otherwise one ``ops.clean_captions``
    call is made.  Then ``ops.caption_ingredients``:
    two launches, integer atomics into ``acc`` = [correct, precision total, recall total] (int64), so a given sequence of updates always
    gives the same bits; nothing uploaded for a recurring batch, so ``update`` can be captured.  ``result()`` is the only read-back.
    ``last_masks`` / ``last_extra``: the last update's (T,) int64 masks and int32 extra-word counts; ``last_counts``: its (N, 3) int32
    per-video (correct, len(generated lists), len(ground-truth lists))."""

    def __init__(self, lexicon):
        self.lexicon = lexicon
        self.device = _gpu_device(lexicon.device)
        self.acc = torch.zeros(3, dtype=torch.int64, device=self.device)
        self.last_masks = self.last_extra = self.last_counts = None

    def reset(self):
        self.acc.zero_()
        self.last_masks = self.last_extra = self.last_counts = None

    def update(self, dec_seq_list, plan, row=0, clean=None):
        if plan.lexicon is not self.lexicon:
            raise ValueError("the plan was made by another lexicon")
        if not plan.has_gt:
            raise ValueError("IngredientF1 needs the ground-truth sentences of every video (gt_sentences in lexicon.plan)")
        words, ln, steps, _ = _clean_rows(dec_seq_list, row, clean)
        masks, extra, _, counts = ops.caption_ingredients(words, ln, plan, self.acc, steps=steps)
        self.last_masks, self.last_extra, self.last_counts = masks, extra, counts
        return counts

    def result(self):
        """The single host read-back → recall, precision, f1 (``compute_total_f1``: 0 where the reference would divide by zero),
        n_correct, n_recall, n_precision."""
        c, p, r = (int(x) for x in self.acc.cpu())
        res = compute_total_f1(c, r, p)
        res.update(n_correct=c, n_recall=r, n_precision=p)
        return res


class CaptionScores:
    """Running Bleu_1…4, ROUGE_L and CIDEr of an evaluation epoch against a ``caption_scores.ReferenceCorpus``, kept on the device — the
    numbers densevid_eval/para-evaluate.py gives src/train.py:278-331 apart from METEOR (the scores are pinned to the
    published definitions restated there, not to outputs of the third-party scorer).

    ``update(dec_seq_list, plan, row=0, clean=None)`` takes what any ``translate_batch*`` returns and ``corpus.plan(videos)`` of the same
    videos; ``clean=(words, len)`` reuses a clean-up already made with run collapse on (``DecodeMetrics.last_clean`` after its ``update``
    of the same result and row), otherwise one ``ops.clean_captions`` call is made.  Then three launches — token streams, per-video
    counts and scores, accumulation — with nothing uploaded for a recurring batch, so ``update`` can be captured once its structure has
    been seen; integer totals by integer adds and the two fp64 sums in a fixed order, so a given sequence of updates always gives the same
    bits.  ``result()`` is the only read-back.  Updating one video twice in an epoch counts it twice: that is the caller's error.

    ``state`` (int64): [correct_1..4, guess_1..4, testlen, reflen, videos | Σ ROUGE_L, Σ CIDEr (float64 bits) | one flag per video of the
    reference set].  ``last_counts`` (N, 11) int32 and ``last_scores`` (N, 6) float64: the last update's per-video correct_1..4,
    guess_1..4, testlen, reflen, largest LCS and Bleu_1..4, ROUGE_L, CIDEr."""

    KEYS = ("Bleu_1", "Bleu_2", "Bleu_3", "Bleu_4", "ROUGE_L", "CIDEr")

    def __init__(self, corpus):
        self.corpus = corpus
        self.device = _gpu_device(corpus.device)
        self.state = torch.zeros(13 + corpus.n_docs, dtype=torch.int64, device=self.device)
        self.acc_i, self.acc_f, self.seen = self.state[:11], self.state[11:13].view(torch.float64), self.state[13:]
        self.last_counts = self.last_scores = None

    def reset(self):
        self.state.zero_()
        self.last_counts = self.last_scores = None

    def update(self, dec_seq_list, plan, row=0, clean=None):
        if plan.corpus is not self.corpus:
            raise ValueError("the plan was made by another reference corpus")
        words, ln, steps, _ = _clean_rows(dec_seq_list, row, clean, video_cap=False)          # (its cap is plan.check_cap, in caption_tokens)
        tokens, tok_len = ops.caption_tokens(words, ln, plan, steps)
        counts, scores = ops.caption_score_counts(tokens, tok_len, plan, seen=self.seen)
        ops.caption_score_accum(counts, scores, self.acc_i, self.acc_f)
        self.last_counts, self.last_scores = counts, scores
        return scores

    def result(self, missing="skip"):
        """The single host read-back → Bleu_1 … Bleu_4 (from the totals), ROUGE_L and CIDEr (means over the videos), num_videos, testlen,
        reflen, correct, guess.  ``missing="empty"``: every video of the reference set not updated yet counts as an empty hypothesis, as
        ``evaluate_para`` treats a missing prediction (testlen += 0, reflen += its shortest reference, scores 0, means over all videos)."""
        from .caption_scores import bleu_from_totals
        if missing not in ("skip", "empty"):
            raise ValueError("missing must be 'skip' or 'empty', got %r" % (missing,))
        host = self.state.cpu()
        v = [int(x) for x in host[:11]]
        rouge, cider = (float(x) for x in host[11:13].view(torch.float64))
        nv, reflen = v[10], v[9]
        if missing == "empty":
            for i, s in enumerate(host[13:].tolist()):
                if not s:
                    nv += 1
                    reflen += self.corpus.min_ref_len[i]
        bleu = bleu_from_totals(v[0:4], v[4:8], v[8], reflen) if nv else [0.0] * 4
        res = {k: b for k, b in zip(self.KEYS, bleu)}
        res.update(ROUGE_L=rouge / nv if nv else 0.0, CIDEr=cider / nv if nv else 0.0, num_videos=nv, testlen=v[8], reflen=reflen,
                   correct=v[0:4], guess=v[4:8])
        return res


class ForcedScores:
    """Running gold score / perplexity of an evaluation epoch from ``Translator.score_captions`` results, kept on the
    device: ``update(scored)`` takes the namespace it returns (one launch, fixed summation order, nothing uploaded — capturable);
    ``compute()`` is the only read-back.

    accumulator (9,) float64: captions, positions scored (Σ n_scored), Σ cum and Σ n_scored over the captions with a finite cum, captions
    with a non-finite cum, positions of rank 0, Σ rank and the count of the ranked positions, finished captions."""

    def __init__(self, device="cuda"):
        self.device = _gpu_device(device)
        self.acc = torch.zeros(ops.FORCE_ACC_COLS, dtype=torch.float64, device=self.device)

    def reset(self):
        self.acc.zero_()

    def update(self, scored):
        ops.force_accum(scored.cum, scored.n_scored, scored.finished, scored.length, scored.rank, self.acc)
        return self.acc

    def compute(self):
        """→ captions, tokens (positions scored), score_sum (Σ cum over the finite captions), ppl = exp(−score_sum / their positions),
        inf_share (captions with cum = −inf), top1 (share of ranked positions where the target is the decoder's first candidate),
        mean_rank (over the ranked positions), finished_share.  A ratio without a denominator is 0 (ppl: nan)."""
        import math
        v = [float(x) for x in self.acc.cpu()]
        n, ranked = v[0], v[7]
        return dict(captions=int(n), tokens=int(v[1]), score_sum=v[2],
                    ppl=math.exp(-v[2] / v[3]) if v[3] else float("nan"), inf_share=v[4] / n if n else 0.0,
                    top1=v[5] / ranked if ranked else 0.0, mean_rank=v[6] / ranked if ranked else 0.0,
                    finished_share=v[8] / n if n else 0.0)

    result = compute
