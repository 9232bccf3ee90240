"""Knowledge distillation restated in numpy fp64, sharing no code with svpc_amd: the loss head ``seq_kd`` over a student
and a teacher score matrix — on top of ``scst_reference.seq_nll`` — and the model-level loss under torch autograd over the oracle's forced
rows.

The layout is ``seq_nll``'s: R caption rows of Lt positions, score row r·Lt + i scores position i + 1, scored while i < len[r].  The
candidates of a row are the columns c < C_r, c != UNK.  Per candidate, in fp64:

- teacher probability q_c: ``raw > 0 ? raw : 0`` (probabilities) or exp(raw − lse_q), lse_q the log-sum-exp of the teacher row's
  candidates; a row whose lse_q is not finite (no finite candidate logit) has q = 0 everywhere; never renormalised;
- student log-probability ℓ_c: log(row[c]) (probabilities) or row[c] − lse (logits);
- a column with q_c > 0 is clamped when p_c <= 0 or ℓ_c < LOG_EPS = −100·ln 2: its term is −q_c·LOG_EPS and its gradient zero;
- kdstep = −Σ q_c·ℓ_c, hstep = −Σ q_c·log q_c over the candidates with q_c > 0 (log q_c = raw − lse_q for a logits teacher)."""
import math

import numpy as np
import torch

import forced_score_reference as fr
import scst_reference as sr
from oracle import svpc_oracle as orc
from svpc_amd.synthetic import UNK

LOG_EPS = -100.0 * math.log(2.0)


def _lse(vals):
    """log-sum-exp of fp64 values; −inf for none or all −inf, nan / +inf passed on"""
    if len(vals) == 0:
        return -math.inf
    m = float(np.max(vals))
    if not math.isfinite(m):
        return m if m != m or m > 0 else -math.inf
    return m + math.log(float(np.exp(vals - m).sum()))


def teacher_q(trow, C, teacher_logits, unk=UNK):
    """one teacher row (float32) → (q (C,) fp64 with 0 at UNK, log q (C,) fp64 — only meaningful where q > 0)"""
    raw = np.asarray(trow, np.float32)[:C].astype(np.float64)
    cand = np.arange(C) != unk
    q = np.zeros(C, np.float64)
    logq = np.full(C, -math.inf)
    if teacher_logits:
        lse_q = _lse(raw[cand])
        if math.isfinite(lse_q):
            with np.errstate(over="ignore"):
                q[cand] = np.exp(raw[cand] - lse_q)
            logq[cand] = raw[cand] - lse_q
    else:
        with np.errstate(invalid="ignore"):
            pos = cand & (raw > 0)
        q[pos] = raw[pos]
        logq[pos] = np.log(raw[pos])
    return q, logq


def row_terms(srow, trow, C, logits, teacher_logits, unk=UNK):
    """one student row and one teacher row → a dict over the row's C columns: q, ell (the student's log-probability, nan where it is
    not counted), clamped (bool), p (the student's probability, 0 at UNK in logits mode), kd and h (the two sums before any rounding)"""
    q, logq = teacher_q(trow, C, teacher_logits, unk)
    raw = np.asarray(srow, np.float32)[:C].astype(np.float64)
    cand = np.arange(C) != unk
    if logits:
        lse = _lse(raw[cand])
        ell = raw - lse
        p = np.where(cand, np.exp(ell), 0.0)
        below = ell < LOG_EPS
    else:
        p = raw.copy()
        with np.errstate(divide="ignore", invalid="ignore"):
            ell = np.log(raw)
            below = (raw <= 0) | (ell < LOG_EPS)
    counted = q > 0
    clamped = counted & below
    live = counted & ~clamped
    kd = math.fsum(-q[c] * ell[c] for c in np.flatnonzero(live)) + math.fsum(-q[c] * LOG_EPS for c in np.flatnonzero(clamped))
    h = math.fsum(-q[c] * logq[c] for c in np.flatnonzero(counted))
    return dict(q=q, ell=np.where(counted, ell, np.nan), clamped=clamped, live=live, p=p, kd=kd, h=h)


def seq_kd(scores, tq, ids, row_c, w, v, logits, teacher_logits, dl=1.0):
    """``scores`` / ``tq`` (R·Lt, ≥ C) float32, ``ids`` (R, Lt), ``row_c`` (R,), ``w`` / ``v`` (R,) float32 → a dict: loss (float32), cum /
    step / barred / len (``scst_reference.seq_nll``'s), kd / ent (R,) float32, kdstep / hstep (R, Lt − 1) float32, kdstep64 / hstep64 the
    sums before their rounding, dscores (R·Lt, width) float64 = dl · d loss / d scores, ell: every counted, unclamped ℓ_c."""
    scores = np.asarray(scores, np.float32)
    tq = np.asarray(tq, np.float32)
    ids = np.asarray(ids)
    R, Lt = ids.shape
    base = sr.seq_nll(scores, ids, row_c, w, logits, dl=dl)
    d = base["dscores"]
    kd64 = np.zeros((R, Lt - 1), np.float64)
    h64 = np.zeros((R, Lt - 1), np.float64)
    kd = np.zeros(R, np.float32)
    ent = np.zeros(R, np.float32)
    ells = []
    total = np.float64(0.0)
    for r in range(R):
        n, C = int(base["len"][r]), int(row_c[r])
        ka, ha = np.float32(0.0), np.float32(0.0)
        for i in range(n):
            t = row_terms(scores[r * Lt + i], tq[r * Lt + i], C, logits, teacher_logits)
            ells += [float(x) for x in t["ell"][t["live"]]]
            kd64[r, i], h64[r, i] = t["kd"], t["h"]
            with np.errstate(over="ignore", invalid="ignore"):
                ka = np.float32(ka + np.float32(t["kd"]))
                ha = np.float32(ha + np.float32(t["h"]))
            if base["barred"][r]:
                continue
            sv = np.float64(dl) * np.float64(v[r])
            if sv == 0.0:
                continue
            qp = np.where(t["live"], t["q"], 0.0)
            if logits:
                d[r * Lt + i, :C] += sv * (qp.sum() * t["p"] - qp)
            else:
                live = np.flatnonzero(t["live"])
                d[r * Lt + i, live] -= sv * qp[live] / t["p"][live]
        kd[r], ent[r] = ka, ha
        if not base["barred"][r]:
            total += np.float64(w[r]) * np.float64(base["cum"][r])
            if np.float64(v[r]) != 0.0:
                total -= np.float64(v[r]) * np.float64(ka)
    out = dict(base)
    with np.errstate(over="ignore"):
        out.update(loss=np.float32(-total), kd=kd, ent=ent, kdstep=kd64.astype(np.float32), hstep=h64.astype(np.float32), kdstep64=kd64,
                   hstep64=h64, dscores=d, ell=np.asarray(ells, np.float64))
    return out


def per_token_weights(lengths, alpha):
    """the steps' row weights: w = (1 − α) / n, v = α / n, n = max(1, Σ len), in fp64, rounded once to float32"""
    n = np.float64(max(1, int(np.sum(lengths))))
    R = len(lengths)
    return np.full(R, np.float32((1.0 - np.float64(alpha)) / n), np.float32), np.full(R, np.float32(np.float64(alpha) / n), np.float32)


def forced_rows(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                ingr_id_dict, oov_word_dict, captions):
    """the oracle's forced pass of one model (``scst_reference.sequence_loss``'s construction) → per video the (R, Lt, C) float64 score
    tensor (under autograd when ``P``'s leaves require grad): probabilities, raw logits in ``video`` mode; R = S_b·K rows s·K + k"""
    mode, Lv, Lt, V = cfg.model_mode, cfg.max_v_len, cfg.max_t_len, cfg.vocab_size
    ingr_input_ids = torch.as_tensor(ingr_input_ids)
    ingr_sep_masks = torch.as_tensor(ingr_sep_masks)
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    out = []
    for b, S_b in enumerate(batch_step_num):
        cap = np.asarray(captions[b])
        if cap.ndim == 2:
            cap = cap[:, None]
        K = cap.shape[1]
        ids = torch.stack([input_ids_list[s][b] for s in range(S_b)]).clone()
        masks = torch.stack([input_masks_list[s][b] for s in range(S_b)]).clone()
        feats = torch.stack([video_features_list[s][b] for s in range(S_b)])
        ids[:, Lv:] = 0
        masks[:, Lv:] = 0
        ingr = orc.ingredient_embed(P, ingr_input_ids[b:b + 1], ingr_sep_masks[b:b + 1], cfg)[0]
        enc = orc.forward_step(P, ids, feats, masks, cfg)
        g = orc.encoder(P, "step_wise_encoder", (enc[:, 0] + pe50[:S_b]).unsqueeze(0), torch.ones(1, S_b), cfg)[0]
        n_oov = len(oov_word_dict[b]) if mode != "video" else 0
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
        mem = mem.repeat_interleave(K, 0)
        bank = bank.repeat_interleave(K, 0) if bank is not None else None
        R, C = S_b * K, V + n_oov
        y = cap.reshape(R, Lt)
        dec = orc.decoder(P, orc.text_embed(P, fr.model_side(y, V), cfg), torch.ones(R, Lt), mem, torch.ones(mem.shape[:2]), cfg)
        if mode == "video":
            sc = orc.lm_head(P, dec, cfg)
        else:
            sc = orc.pointer_generator(P, dec, bank, ingr_id_dict[b], n_oov, cfg)
        out.append(sc.reshape(R, Lt, -1)[:, :, :C].double())
    return out


def distillation_loss(student_rows, teacher_mats, teacher_logits, logits, captions, weights, kd_weights):
    """``student_rows``: ``forced_rows`` of the student (under autograd); ``teacher_mats`` per video a float32 (R·Lt, ≥ C) numpy matrix
    (probabilities, or logits when ``teacher_logits``); ``weights`` / ``kd_weights`` per video (S_b, K) → (loss: a float64 torch scalar
    under autograd, cum / kd / ent: per video (S_b, K) float64, barred: per video (S_b, K) bool).  The clamp decisions and the teacher's q
    are taken from the rows rounded to float32, which is what the kernels see."""
    loss = torch.zeros((), dtype=torch.float64)
    cums, kds, ents, bars = [], [], [], []
    for b, sc in enumerate(student_rows):
        cap = np.asarray(captions[b])
        if cap.ndim == 2:
            cap = cap[:, None]
        S_b, K, Lt = cap.shape
        R, C = S_b * K, sc.shape[2]
        y = cap.reshape(R, Lt)
        flat = sc.detach().numpy().astype(np.float32).reshape(R * Lt, -1)
        walk = fr.score_rows(flat, y, np.full(R, C), logits, "bar")
        w = np.asarray(weights[b], np.float64).reshape(R)
        v = np.asarray(kd_weights[b], np.float64).reshape(R)
        tm = np.asarray(teacher_mats[b], np.float32)
        keep = torch.arange(C) != UNK
        cum_b, kd_b, ent_b, bar_b = [], [], [], []
        for c in range(R):
            n = int(walk["len"][c])
            barred = not np.isfinite(walk["step"][c, :n]).all()
            bar_b.append(barred)
            kd_c = torch.zeros((), dtype=torch.float64)
            ent_c = 0.0
            for i in range(n):
                t = row_terms(flat[c * Lt + i], tm[c * Lt + i], C, logits, teacher_logits)
                row = sc[c, i]
                ell = row - torch.logsumexp(row[keep], 0) if logits else torch.log(row)
                live = torch.as_tensor(np.flatnonzero(t["live"]))
                kd_c = kd_c - (torch.as_tensor(t["q"])[live] * ell[live]).sum() - float(t["q"][t["clamped"]].sum()) * LOG_EPS
                ent_c += t["h"]
            kd_b.append(kd_c.detach())
            ent_b.append(torch.tensor(ent_c, dtype=torch.float64))
            if barred or n == 0:
                cum_b.append(torch.zeros((), dtype=torch.float64))
                continue
            rows = sc[c, :n]
            tgt = torch.as_tensor(y[c, 1:n + 1]).long()
            picked = rows.gather(1, tgt.unsqueeze(1)).squeeze(1)
            lp = picked - torch.logsumexp(rows[:, keep], 1) if logits else torch.log(picked)
            cum_b.append(lp.sum().detach())
            loss = loss - w[c] * lp.sum() + v[c] * kd_c
        for lst, src in ((cums, cum_b), (kds, kd_b), (ents, ent_b)):
            lst.append(torch.stack(src).reshape(S_b, K))
        bars.append(np.asarray(bar_b).reshape(S_b, K))
    return loss, cums, kds, ents, bars
