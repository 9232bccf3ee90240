"""CPU restatement of contrastive decoding (svpc_amd/contrast_decode.py, svpc_contrast_combine; Li et al. 2023, O'Brien & Lewis 2023):
``combine`` is the rule the HIP kernel must reproduce, and ``contrast_greedy`` / ``contrast_beam_decode`` / ``contrast_sample_decode`` are
per-video oracle decodes over two parameter dicts (expert, amateur), built like their ``ensemble_reference`` counterparts: one encoder
side per member — each over its own view of the clip features, so the zero-video amateur is expressible —, one decoder re-run per member
and step, ``combine``, then the single-model selection rules with ``logits=False``.

The rule, one row at a time.  Two fp32 score matrices with the same rows, expert e and amateur a: probabilities in the pointer-generator
modes, raw logits in ``video`` mode.  Row r has C = row_c[r // rows_per] columns.  Coefficients fp64: we > 0, wa ≥ 0, α in [0, 1].  UNK is
never a candidate: it is left out of every maximum, head and sum in BOTH score modes, and out[UNK] = 0.
  1. Member log-probabilities, fp64, for c < C, c ≠ UNK.  Probability mode: p = raw > 0 ? (double)raw : 0 and l = log p, −inf at 0.
     Logits mode: l = (double)raw − lse, lse = max + log Σ exp(raw − max) over c < C, c ≠ UNK.  A member row without a finite non-UNK
     logit is dead: l = −inf everywhere.
  2. Dead expert row: if the expert has no column with l_e > −inf, the whole output row is 0.
  3. Head H.  Probability mode: p_e,c > 0 and p_e,c ≥ α·p_e,top (one rounded fp64 product).  Logits mode: raw_e,c finite and
     (double)raw_e,c − (double)raw_e,top ≥ log α, log α from ``math.log`` (−inf for α = 0).  No row reduction other than an exact
     maximum: head membership is reproducible bit for bit.
  4. Amateur term: la_c = max(l_a,c, L0), L0 = log(1e-30) (``L0`` below).  It covers a zero amateur probability and a dead amateur row
     without an infinity.  With wa == 0 the amateur matrix is never read.
  5. Score: s_c = we·l_e,c − wa·la_c, the two products and the difference each rounded, never contracted.
  6. Normalise: m = max_H s, Z = Σ_H exp(s_c − m), out_c = fp32(exp((s_c − m) − log Z)) for c in H.  A head of one column gives exactly 1.0.
  7. Everything else — columns outside H, UNK, C ≤ c < ld_out — is 0.
The output is a distribution over the head."""
import math

import numpy as np
import torch

from beam_reference import select
from oracle import svpc_oracle as orc
from sampling_reference import model_ids, sample_select
from svpc_amd.synthetic import BOS, PAD, UNK

L0 = -69.07755278982137          # log(1e-30), the fp64 constant the kernel holds
assert L0 == math.log(1e-30)


def log_alpha(alpha):
    return math.log(alpha) if alpha > 0 else -math.inf


def _member_logp(raw, keep, logits):
    """step 1 for one member row: raw (C,) float64 (exact images of the fp32 entries), keep = c ≠ UNK → l (C,), −inf at UNK"""
    if logits:
        if not (keep & np.isfinite(raw)).any():
            return np.full(raw.shape, -np.inf)
        mx = raw[keep].max()
        lse = mx + np.log(np.exp(raw[keep] - mx).sum())
        return np.where(keep, raw - lse, -np.inf)
    p = np.where(keep & (raw > 0), raw, 0.0)
    return np.where(p > 0, np.log(np.where(p > 0, p, 1.0)), -np.inf)


def head_of(raw_e, keep, alpha, logits):
    """step 3 for one expert row → (head mask (C,) or None for a dead row, the per-column distance |log p_e,c − (log α + log p_e,top)|
    to the head's threshold, inf where the column cannot be a candidate or α = 0)"""
    la = log_alpha(alpha)
    C = raw_e.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        if logits:
            ok = keep & np.isfinite(raw_e)
            if not ok.any():
                return None, np.full(C, np.inf)
            d = np.where(ok, raw_e - raw_e[ok].max(), -np.inf)
            head = ok & (d >= la)
        else:
            p = np.where(keep & (raw_e > 0), raw_e, 0.0)
            top = p.max() if C else 0.0
            if not top > 0:
                return None, np.full(C, np.inf)
            ok = p > 0
            head = ok & (p >= alpha * top)
            d = np.where(ok, np.log(np.where(ok, p, 1.0)) - np.log(top), -np.inf)
        dist = np.where(ok, np.abs(d - la), np.inf) if alpha > 0 else np.full(C, np.inf)
    return head, dist


def combine(expert, amateur, row_c, we, wa, alpha, logits=False, unk=UNK, rows_per=1, ld_out=None, return_margin=False):
    """expert / amateur: float32 (n_rows, ≥ C) arrays → (out (n_rows, ld_out) float32, head_mask (n_rows, ld_out) bool); ld_out defaults
    to max C.  ``return_margin``: also the per-row head margin (n_rows,), the smallest threshold distance of ``head_of`` in the row."""
    we, wa, alpha = float(we), float(wa), float(alpha)
    assert math.isfinite(we) and we > 0 and math.isfinite(wa) and wa >= 0 and 0.0 <= alpha <= 1.0
    expert = np.asarray(expert, dtype=np.float32)
    amateur = None if wa == 0.0 else np.asarray(amateur, dtype=np.float32)          # (wa == 0: never read)
    n_rows = expert.shape[0]
    row_c = [int(c) for c in row_c]
    ld_out = max(row_c) if ld_out is None else ld_out
    out = np.zeros((n_rows, ld_out), np.float32)
    mask = np.zeros((n_rows, ld_out), bool)
    margin = np.full(n_rows, np.inf)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for r in range(n_rows):
            C = row_c[r // rows_per]
            keep = np.ones(C, bool)
            if 0 <= unk < C:
                keep[unk] = False
            raw_e = expert[r, :C].astype(np.float64)
            head, dist = head_of(raw_e, keep, alpha, logits)
            if head is None:                                    # step 2
                continue
            margin[r] = dist.min() if C else np.inf
            le = _member_logp(raw_e, keep, logits)[head]
            s = we * le                                          # (numpy: every product and the difference rounded on its own)
            if wa != 0.0:
                la = np.maximum(_member_logp(amateur[r, :C].astype(np.float64), keep, logits)[head], L0)
                s = s - wa * la
            m = s.max()
            z = np.exp(s - m).sum()
            out[r, :C][head] = np.exp((s - m) - np.log(z)).astype(np.float32)
            mask[r, :C] = head
    return (out, mask, margin) if return_margin else (out, mask)


# ------------------------------------------------------------------------------------------------ the decodes
IDENTITY = (None, None)


def _video_sides(Ps, cfg, b, S_b, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, oov_word_dict,
                 width, transforms):
    """both members' (mem, bank) of video b over its S_b·width hypothesis rows — member k's encoder side over ``transforms[k](feats)``
    (None: the video's own clip features) —, and the video's OOV count; ``ensemble_reference._video_sides`` with a feature view per member"""
    mode, Lv = cfg.model_mode, cfg.max_v_len
    ids = torch.stack([input_ids_list[s][b] for s in range(S_b)]).clone()
    masks = torch.stack([input_masks_list[s][b] for s in range(S_b)]).clone()
    feats = torch.stack([video_features_list[s][b] for s in range(S_b)])
    ids[:, Lv:] = 0; masks[:, Lv:] = 0
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    n_oov = len(oov_word_dict[b]) if mode != "video" else 0
    sides = []
    for P, tf in zip(Ps, transforms):
        ingr = orc.ingredient_embed(P, ingr_input_ids[b:b + 1], ingr_sep_masks[b:b + 1], cfg)[0]
        enc = orc.forward_step(P, ids, feats if tf is None else tf(feats), masks, cfg)
        g = orc.encoder(P, "step_wise_encoder", (enc[:, 0] + pe50[:S_b]).unsqueeze(0), torch.ones(1, S_b), cfg)[0]
        bank = None
        if mode in ("full", "reason_copy"):
            _, _, bar_e, all_e, bar_f = orc.simulator(P, "reasoner", g, ingr)
            mem = torch.stack([g, torch.relu(orc.linear(P, "Went.0", bar_e)), torch.relu(orc.linear(P, "Wac.0", bar_f))], 1)
            bank = all_e
        elif mode == "copy":
            mem = torch.stack([g, ingr.mean(0).unsqueeze(0).expand(S_b, -1)], 1)
            bank = ingr.unsqueeze(0).expand(S_b, -1, -1)
        else:
            mem = g.unsqueeze(1)
        sides.append((mem.repeat_interleave(width, 0), bank.repeat_interleave(width, 0) if bank is not None else None))
    return sides, n_oov


def _step_scores(Ps, cfg, sides, text, i, ingr_dict, n_oov, row_c, coef):
    """the combined (R, C) probability matrix of decoding step i and the rows' head margins"""
    mode = cfg.model_mode
    R = text.shape[0]
    mats = []
    for P, (mem, bank) in zip(Ps, sides):
        dec = orc.decoder(P, orc.text_embed(P, text[:, :i + 1], cfg), torch.ones(R, i + 1), mem, torch.ones(mem.shape[:2]), cfg)
        last = dec[:, i:i + 1]
        sc = orc.lm_head(P, last, cfg)[:, 0] if mode == "video" else orc.pointer_generator(P, last, bank, ingr_dict, n_oov, cfg)[:, 0]
        mats.append(sc.detach().numpy())
    we, wa, alpha = coef
    out, _, hm = combine(mats[0], mats[1], row_c, we, wa, alpha, logits=mode == "video", return_margin=True)
    return out, hm


def _args(ingr_input_ids, ingr_sep_masks):
    return torch.as_tensor(ingr_input_ids), torch.as_tensor(ingr_sep_masks)


def contrast_beam_decode(Ps, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                         ingr_id_dict, oov_word_dict, beam, coef, transforms=IDENTITY):
    """``ensemble_reference.ensemble_beam_decode`` under the contrastive rule, ``coef`` = (we, wa, α) → (ids, scores, margins, head
    margins (S_b,) per video: the smallest over the sentence's beam rows and steps)"""
    ingr_input_ids, ingr_sep_masks = _args(ingr_input_ids, ingr_sep_masks)
    Lt, V, B = cfg.max_t_len, cfg.vocab_size, beam
    out, out_scores, out_margins, out_heads = [], [], [], []
    for b, S_b in enumerate(batch_step_num):
        sides, n_oov = _video_sides(Ps, cfg, b, S_b, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks,
                                    oov_word_dict, B, transforms)
        R, C = S_b * B, V + n_oov
        row_c, row_x = np.full(R, C), np.full(R, n_oov)
        text = torch.full((R, Lt), PAD, dtype=torch.long); text[:, 0] = BOS
        ext = text.clone()
        cum = np.zeros((S_b, B), np.float32); cum[:, 1:] = -np.inf
        cum = cum.reshape(-1)
        fin = np.zeros(R, bool)
        margins = np.zeros((S_b, max(Lt - 1, 0)))
        heads = np.full(S_b, np.inf)
        for i in range(Lt - 1):
            sc, hm = _step_scores(Ps, cfg, sides, text, i, ingr_id_dict[b], n_oov, row_c, coef)
            live = (~fin) & np.isfinite(cum)                    # (a finished or empty beam row's scores are not read)
            heads = np.minimum(heads, np.where(live, hm, np.inf).reshape(S_b, B).min(1))
            parent, nx_ext, nx_mod, cum, fin, margins[:, i] = select(sc, row_c, row_x, B, False, cum, fin, return_margin=True)
            pt = torch.as_tensor(parent)
            text, ext = text[pt].clone(), ext[pt].clone()
            text[:, i + 1] = torch.as_tensor(nx_mod)
            ext[:, i + 1] = torch.as_tensor(nx_ext)
        best = np.array([int(np.argmax(cum[s * B:(s + 1) * B])) for s in range(S_b)], dtype=np.int64)
        rows = np.arange(S_b) * B + best
        out.append(ext[torch.as_tensor(rows)])
        out_scores.append(cum[rows].astype(np.float32))
        out_margins.append(margins)
        out_heads.append(heads)
    return out, out_scores, out_margins, out_heads


def contrast_sample_decode(Ps, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                           ingr_id_dict, oov_word_dict, num_samples, seed, coef, transforms=IDENTITY, temp=1.0, topk=0, topp=0.0,
                           min_length=0):
    """``ensemble_reference.ensemble_sample_decode`` under the contrastive rule → (ids, cums, lens, margins, head margins (S_b, Rs))"""
    ingr_input_ids, ingr_sep_masks = _args(ingr_input_ids, ingr_sep_masks)
    Lt, V, Rs = cfg.max_t_len, cfg.vocab_size, num_samples
    out, out_cum, out_len, out_margins, out_heads = [], [], [], [], []
    t0 = 0
    for b, S_b in enumerate(batch_step_num):
        sides, n_oov = _video_sides(Ps, cfg, b, S_b, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks,
                                    oov_word_dict, Rs, transforms)
        R, C = S_b * Rs, V + n_oov
        row_c, row_x = np.full(R, C), np.full(R, n_oov)
        text = torch.full((R, Lt), PAD, dtype=torch.long); text[:, 0] = BOS
        ext = text.clone()
        cum, fin, ln = np.zeros(R, np.float32), np.zeros(R, bool), np.zeros(R, np.int64)
        margins = np.full(R, np.inf)
        heads = np.full(R, np.inf)
        for i in range(Lt - 1):
            sc, hm = _step_scores(Ps, cfg, sides, text, i, ingr_id_dict[b], n_oov, row_c, coef)
            before = fin.copy()
            heads = np.minimum(heads, np.where(before, np.inf, hm))
            picks, cum, fin, ln, mg = sample_select(sc, row_c, row_x, i, False, cum, fin, ln, seed, temp, topk, topp, min_length,
                                                    row0=t0 * Rs)
            margins = np.minimum(margins, mg.min(1))
            text[:, i + 1] = torch.as_tensor(model_ids(picks, before, row_c, row_x))
            ext[:, i + 1] = torch.as_tensor(picks)
        out.append(ext.view(S_b, Rs, Lt))
        out_cum.append(cum.reshape(S_b, Rs))
        out_len.append(ln.reshape(S_b, Rs))
        out_margins.append(margins.reshape(S_b, Rs))
        out_heads.append(heads.reshape(S_b, Rs))
        t0 += S_b
    return out, out_cum, out_len, out_margins, out_heads


def contrast_greedy(Ps, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                    ingr_id_dict, oov_word_dict, coef, transforms=IDENTITY):
    """``ensemble_reference.ensemble_greedy`` under the contrastive rule → (ids, margins (S_b, Lt − 1), head margins (S_b,))"""
    ingr_input_ids, ingr_sep_masks = _args(ingr_input_ids, ingr_sep_masks)
    Lt, V = cfg.max_t_len, cfg.vocab_size
    out, out_margins, out_heads = [], [], []
    for b, S_b in enumerate(batch_step_num):
        sides, n_oov = _video_sides(Ps, cfg, b, S_b, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks,
                                    oov_word_dict, 1, transforms)
        C = V + n_oov
        row_c = np.full(S_b, C)
        text = torch.full((S_b, Lt), PAD, dtype=torch.long); text[:, 0] = BOS
        ext = text.clone()
        margins = np.full((S_b, max(Lt - 1, 0)), np.inf)
        heads = np.full(S_b, np.inf)
        for i in range(Lt - 1):
            sc, hm = _step_scores(Ps, cfg, sides, text, i, ingr_id_dict[b], n_oov, row_c, coef)
            heads = np.minimum(heads, hm)
            sc = sc.astype(np.float64)
            sc[:, UNK] = -np.inf
            for s in range(S_b):
                order = np.lexsort((np.arange(C), -sc[s, :C]))
                c, c2 = int(order[0]), int(order[1])
                with np.errstate(divide="ignore", invalid="ignore"):
                    margins[s, i] = np.log(sc[s, c]) - np.log(sc[s, c2]) if sc[s, c2] > 0 else np.inf
                ext[s, i + 1] = c
                text[s, i + 1] = UNK if c >= C - n_oov else c
        out.append(text if cfg.model_mode == "video" else ext)
        out_margins.append(margins)
        out_heads.append(heads)
    return out, out_margins, out_heads
