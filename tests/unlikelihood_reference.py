"""CPU restatement of unlikelihood training against repetition (``svpc_amd.unlikelihood``, ``ops.ul_negatives`` / ``ops.seq_ul``; DESIGN
§11.13; Welleck et al. 2020).  Shares no code with the product; the walk over a caption is ``forced_score_reference``'s, the likelihood half
``scst_reference.seq_nll``'s, and ``sequence_loss`` is built on the oracle's blocks the way ``scst_reference.sequence_loss`` is.

The definition.  Layout as seq_nll: R caption rows of Lt ids, score row r·Lt + i scores position p = i + 1 (i = 0 … Lt − 2) while i < len[r];
cum / step / barred are seq_nll's under ``unk="bar"``.

- ``neg`` (R, Lt − 1, M) int32, 1 ≤ M ≤ 64: entry j of position (r, i) is a column or −1.  A listing COUNTS when it is a candidate
  (0 ≤ c < C_r, c ≠ UNK) and i < len[r]; a column listed twice counts twice.  (The "token" rule never lists a position's own target; the
  "ngram" rule lists nothing else: the word that completes a repeat is the word whose probability is lowered.)
- in fp64: p_c = row[c] (probabilities) or exp(row[c] − lse) (logits; lse the log-sum-exp of the row's columns without UNK); q = 1 − p_c;
  term = −log1p(−p_c) when q ≥ EPS, else −log EPS with a zero gradient; EPS = 1e-5, the clamp of the paper's published implementation.
- ulstep[r, i] = fp32(Σ_j term), 0 past the end; ul[r] = the fp32 running sum of ulstep in position order.
- loss = fp32(−Σ_r w_r·cum_r + Σ_r u_r·ul_r) over the captions that are not barred (fp64 products and sums).
- d loss / d scores · dl: seq_nll's zero rows and columns; probabilities — −dl·w / p_y at the target, dl·u / (1 − p_c) added at c per
  counted, unclamped listing; logits — dl·[w·(p_c − [c = y]) + u·(a_c − A·p_c)], a_c = Σ p_c / (1 − p_c) over those listings of c,
  A = Σ_c a_c, 0 at UNK.

Negative rules.  "token" (M = Lt − 1): N(r, i) = the distinct columns among y[1 … i] in order of first occurrence, without y[i + 1] and
non-candidates; −1 after them.  Ids are compared as score columns (``force_inputs``' tgt: an id below −2 or beyond int32 is −2).  "ngram" (M = 1, n in 1 … 4): the words of row r are y[1 … nw], nw = len − [the last scored target is EOS];
gram (r, a) = y[a … a + n − 1], 1 ≤ a ≤ nw − n + 1; it is a REPEAT when an equal gram starts earlier in the same caption or, under paragraph
scope, anywhere in row t′·K + k of an earlier sentence t′ of the same video (r = t·K + k); position p is penalised when a repeat gram
covers it, and then N(r, p − 1) = {y[p]}.  npen[r] = the counted negatives, nrep[r] = the repeat grams (0 under "token")."""
import math

import numpy as np
import torch

import forced_score_reference as fr
import scst_reference as sr
from oracle import svpc_oracle as orc
from svpc_amd.synthetic import EOS, IGNORE, PAD, UNK

EPS = 1e-5
RULES = ("token", "ngram")
SCOPES = ("caption", "paragraph")


def caption_end(y, eos=EOS, pad=PAD, ignore=IGNORE):
    """→ (len, finished) of one id row: finished at its first EOS (len = its position), unfinished before its first PAD / IGNORE"""
    for p in range(1, len(y)):
        if int(y[p]) == eos:
            return p, 1
        if int(y[p]) in (pad, ignore):
            return p - 1, 0
    return len(y) - 1, 0


def _candidate(c, C, unk=UNK):
    return 0 <= c < C and c != unk


def negatives(ids, row_c, rule, ngram=4, scope="caption", sent_first=None, K=1):
    """``ids`` (R, Lt) → (neg (R, Lt − 1, M) int32, npen (R,) int32, nrep (R,) int32)"""
    assert rule in RULES and scope in SCOPES and 1 <= ngram <= 4
    ids = np.asarray(ids).astype(np.int64)
    ids = np.where((ids < -2) | (ids > 2 ** 31 - 1), -2, ids)         # an id as a score column: −2 when it fits none (svpc_force_inputs' tgt)
    R, Lt = ids.shape
    S = Lt - 1
    M = S if rule == "token" else 1
    neg = np.full((R, S, M), -1, np.int32)
    npen, nrep = np.zeros(R, np.int32), np.zeros(R, np.int32)
    ends = [caption_end(ids[r]) for r in range(R)]
    for r in range(R):
        y = [int(v) for v in ids[r]]
        n_r, fin = ends[r]
        C = int(row_c[r])
        if rule == "token":
            for i in range(n_r):
                seen = []
                for j in range(1, i + 1):
                    if y[j] not in seen:
                        seen.append(y[j])
                lst = [c for c in seen if _candidate(c, C) and c != y[i + 1]]
                neg[r, i, :len(lst)] = lst
                npen[r] += len(lst)
            continue
        nw = n_r - fin
        earlier = set()
        if scope == "paragraph":
            t, k = divmod(r, K)
            for s in range(int(sent_first[t]), t):
                q = s * K + k
                z = [int(v) for v in ids[q]]
                nq = ends[q][0] - ends[q][1]
                earlier |= {tuple(z[a:a + ngram]) for a in range(1, nq - ngram + 2)}
        pen = set()
        for a in range(1, nw - ngram + 2):
            gram = tuple(y[a:a + ngram])
            if gram in earlier:
                nrep[r] += 1
                pen |= set(range(a, a + ngram))
            earlier.add(gram)
        for p in sorted(pen):
            neg[r, p - 1, 0] = y[p]
            npen[r] += 1 if _candidate(y[p], C) else 0
    return neg, npen, nrep


def row_terms(row, listing, C, logits, unk=UNK):
    """one score row (float32) and its listed columns → [(column, p, term, clamped)] of the counted listings, in fp64"""
    row = np.asarray(row, np.float32).astype(np.float64)
    lse = 0.0
    if logits:
        keep = np.arange(C) != unk
        m = row[:C][keep].max()
        lse = m + math.log(np.exp(row[:C][keep] - m).sum())
    out = []
    for c in listing:
        c = int(c)
        if not _candidate(c, C, unk):
            continue
        p = math.exp(row[c] - lse) if logits else float(row[c])
        q = 1.0 - p
        if q >= EPS:
            out.append((c, p, -math.log1p(-p), False))
        else:
            out.append((c, p, -math.log(EPS), True))
    return out


def seq_ul(scores, ids, row_c, neg, w, u, logits, dl=1.0):
    """``scores`` (R·Lt, ≥ C) float32, ``ids`` (R, Lt), ``row_c`` (R,), ``neg`` (R, Lt − 1, M), ``w`` / ``u`` (R,) float32 → a dict: loss
    (float32), cum / step / barred / len (``scst_reference.seq_nll``'s), ul (R,) float32, ulstep (R, Lt − 1) float32, ulstep64 the sums
    before their rounding, dscores (R·Lt, width) float64 = dl · d loss / d scores, q: every counted listing's 1 − p."""
    scores = np.asarray(scores, np.float32)
    ids = np.asarray(ids)
    R, Lt = ids.shape
    base = sr.seq_nll(scores, ids, row_c, w, logits, dl=dl)
    d = base["dscores"]
    ulstep64 = np.zeros((R, Lt - 1), np.float64)
    ul = np.zeros(R, np.float32)
    qs = []
    total = np.float64(0.0)
    for r in range(R):
        n, C = int(base["len"][r]), int(row_c[r])
        acc = np.float32(0.0)
        for i in range(n):
            terms = row_terms(scores[r * Lt + i], neg[r, i], C, logits)
            qs += [1.0 - p for _, p, _, _ in terms]
            ulstep64[r, i] = math.fsum(t for _, _, t, _ in terms)
            acc = np.float32(acc + np.float32(ulstep64[r, i]))
            if base["barred"][r]:
                continue
            su = np.float64(dl) * np.float64(u[r])
            if logits:
                row = scores[r * Lt + i, :C].astype(np.float64)
                keep = np.arange(C) != UNK
                m = row[keep].max()
                soft = np.where(keep, np.exp(row - (m + math.log(np.exp(row[keep] - m).sum()))), 0.0)
                a = np.zeros(C, np.float64)
                for c, p, _, clamped in terms:
                    if not clamped:
                        a[c] += p / (1.0 - p)
                d[r * Lt + i, :C] += su * (a - a.sum() * soft)
            else:
                for c, p, _, clamped in terms:
                    if not clamped:
                        d[r * Lt + i, c] += su / (1.0 - p)
        ul[r] = acc
        if not base["barred"][r]:
            total += np.float64(w[r]) * np.float64(base["cum"][r]) - np.float64(u[r]) * np.float64(acc)
    out = dict(base)
    out.update(loss=np.float32(-total), ul=ul, ulstep=ulstep64.astype(np.float32), ulstep64=ulstep64, dscores=d, q=np.asarray(qs, np.float64))
    return out


def per_token_weights(lengths, alpha, with_nll=True):
    """the steps' row weights: w = 1 / n (or 0), u = α / n, n = max(1, Σ len), in fp64, rounded once to float32"""
    n = np.float64(max(1, int(np.sum(lengths))))
    R = len(lengths)
    w = np.full(R, np.float32(1.0 / n if with_nll else 0.0), np.float32)
    return w, np.full(R, np.float32(np.float64(alpha) / n), np.float32)


def sequence_loss(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                  ingr_id_dict, oov_word_dict, captions, weights, ul_weights, rule="token", ngram=4, scope="caption"):
    """``scst_reference.sequence_loss`` with the unlikelihood term: ``captions`` per video (S_b, K, Lt) ids, ``weights`` / ``ul_weights`` per
    video (S_b, K) → (loss: a float64 torch scalar under autograd, ul: per video (S_b, K) float64, barred: per video (S_b, K) bool, npen and
    nrep: per video (S_b, K) int).  Paragraph scope looks at the earlier sentences of the same video, which is this loop's unit."""
    mode, Lv, Lt, V = cfg.model_mode, cfg.max_v_len, cfg.max_t_len, cfg.vocab_size
    ingr_input_ids = torch.as_tensor(ingr_input_ids)
    ingr_sep_masks = torch.as_tensor(ingr_sep_masks)
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    loss = torch.zeros((), dtype=torch.float64)
    uls, bars, npens, nreps = [], [], [], []
    for b, S_b in enumerate(batch_step_num):
        cap = np.asarray(captions[b])
        if cap.ndim == 2:
            cap = cap[:, None]
        K = cap.shape[1]
        ids = torch.stack([input_ids_list[s][b] for s in range(S_b)]).clone()
        masks = torch.stack([input_masks_list[s][b] for s in range(S_b)]).clone()
        feats = torch.stack([video_features_list[s][b] for s in range(S_b)])
        ids[:, Lv:] = 0; masks[:, Lv:] = 0
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
        mem = mem.repeat_interleave(K, 0)                                              # caption rows s·K + k
        bank = bank.repeat_interleave(K, 0) if bank is not None else None
        R, C = S_b * K, V + n_oov
        y = cap.reshape(R, Lt)
        dec = orc.decoder(P, orc.text_embed(P, fr.model_side(y, V), cfg), torch.ones(R, Lt), mem, torch.ones(mem.shape[:2]), cfg)
        if mode == "video":
            sc = orc.lm_head(P, dec, cfg)
        else:
            sc = orc.pointer_generator(P, dec, bank, ingr_id_dict[b], n_oov, cfg)
        sc = sc.reshape(R, Lt, -1)[:, :, :C].double()
        logits = mode == "video"
        flat = sc.detach().numpy().astype(np.float32).reshape(R * Lt, -1)
        walk = fr.score_rows(flat, y, np.full(R, C), logits, "bar")
        neg, npen, nrep = negatives(y, np.full(R, C), rule, ngram, scope, sent_first=[0] * S_b, K=K)
        w = np.asarray(weights[b], np.float64).reshape(R)
        u = np.asarray(ul_weights[b], np.float64).reshape(R)
        ul_b, bar_b = [], []
        keep = torch.arange(C) != UNK
        for c in range(R):
            n = int(walk["len"][c])
            barred = not np.isfinite(walk["step"][c, :n]).all()
            bar_b.append(barred)
            ul_c = torch.zeros((), dtype=torch.float64)
            for i in range(n):
                row = sc[c, i]
                lse = torch.logsumexp(row[keep], 0) if logits else None
                for col, p_np, term, clamped in row_terms(flat[c * Lt + i], neg[c, i], C, logits):
                    if clamped:
                        ul_c = ul_c + term
                    else:
                        p = torch.exp(row[col] - lse) if logits else row[col]
                        ul_c = ul_c - torch.log1p(-p)
            ul_b.append(ul_c.detach())
            if barred or n == 0:
                continue
            rows = sc[c, :n]
            tgt = torch.as_tensor(y[c, 1:n + 1]).long()
            picked = rows.gather(1, tgt.unsqueeze(1)).squeeze(1)
            lp = picked - torch.logsumexp(rows[:, keep], 1) if logits else torch.log(picked)
            loss = loss - w[c] * lp.sum() + u[c] * ul_c
        uls.append(torch.stack(ul_b).reshape(S_b, K))
        bars.append(np.asarray(bar_b).reshape(S_b, K))
        npens.append(npen.reshape(S_b, K))
        nreps.append(nrep.reshape(S_b, K))
    return loss, uls, bars, npens, nreps
