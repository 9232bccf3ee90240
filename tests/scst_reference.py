"""CPU restatement of the self-critical (CIDEr-reward) training step (``svpc_amd.scst``).  Shares no code with the product;
the walk over a caption is ``forced_score_reference``'s, ``sequence_loss`` is built on the oracle's blocks the way
``forced_score_reference.forced_decode`` is, without the ``detach``, under torch autograd.

The definition.  Candidates: per video an (S_b, K, Lt) id tensor, caption row r = t·K + k, candidate paragraph k of a video = row k of each
of its sentences.  cum / step / len of a row are forced decoding's under ``unk="bar"``.  A caption with a scored position whose step score
is not finite (p ≤ 0, a target that is no candidate) is BARRED: it adds 0 to the loss and its gradient is exactly zero.

- reward r[b, k]: a score column of candidate paragraph k of video b (fp64);
- advantage: "greedy" A = r[b, k] − r_g[b]; "mean" A = r[b, k] − Σ_{j≠k} r[b, j] / (K − 1), j ascending (K ≥ 2); "none" A = r;
- row weight w[t, k] = fp32(A[vid(t), k] / (N·K)), computed in fp64 and rounded once;
- loss = fp32(−Σ_{(t,k) not barred} w[t, k]·cum[t, k]) (fp64 products and sums; the kernel adds them in a fixed order);
- d loss / d scores: probabilities — −w / p at the target column of every scored position; logits — w·(softmax without UNK − [c = y]), 0 at
  UNK; 0 at the columns from C_r up, on the never-scored last position row, past the end and on every row of a barred caption."""
import numpy as np
import torch

import forced_score_reference as fr
from oracle import svpc_oracle as orc
from svpc_amd.synthetic import UNK

BASELINES = ("none", "greedy", "mean")


def advantages(reward, baseline, greedy=None):
    """reward (N, K) → advantage (N, K), float64"""
    r = np.asarray(reward, np.float64)
    N, K = r.shape
    if baseline not in BASELINES:
        raise ValueError(baseline)
    if baseline == "none":
        return r.copy()
    if baseline == "greedy":
        return r - np.asarray(greedy, np.float64).reshape(N, 1)
    if K < 2:
        raise ValueError("the leave-one-out mean needs K >= 2")
    A = np.empty_like(r)
    for b in range(N):
        for k in range(K):
            s = np.float64(0.0)
            for j in range(K):
                if j != k:
                    s = s + r[b, j]
            A[b, k] = r[b, k] - s / np.float64(K - 1)
    return A


def row_weights(advantage, steps):
    """advantage (N, K) float64, ``steps`` the videos' sentence counts → w (T·K,) float32 at row t·K + k"""
    A = np.asarray(advantage, np.float64)
    N, K = A.shape
    w = [np.float32(A[b, k] / np.float64(N * K)) for b, s in enumerate(steps) for _ in range(s) for k in range(K)]
    return np.asarray(w, np.float32).reshape(-1)


def seq_nll(scores, ids, row_c, w, logits, dl=1.0):
    """``scores`` (R·Lt, ≥ C) float32 — row r·Lt + i is step i of caption r —, ``ids`` (R, Lt), ``row_c`` (R,), ``w`` (R,) float32 → a dict:
    loss (float32), cum (R,) float32, step (R, Lt − 1) float32, barred (R,) int32, len (R,), dscores (R·Lt, width) float64 = dl · d loss / d scores."""
    scores = np.asarray(scores, np.float32)
    ids = np.asarray(ids)
    R, Lt = ids.shape
    r = fr.score_rows(scores, ids, row_c, logits, "bar")
    step, cum, length = r["step"], r["cum"], r["len"]
    barred = np.zeros(R, np.int32)
    d = np.zeros(scores.shape, np.float64)
    total = np.float64(0.0)
    for c in range(R):
        n, C = int(length[c]), int(row_c[c])
        barred[c] = 0 if np.isfinite(step[c, :n]).all() else 1
        if barred[c]:
            continue
        total += np.float64(w[c]) * np.float64(cum[c])
        s = np.float64(dl) * np.float64(w[c])
        for i in range(n):
            y = int(ids[c, i + 1])
            row = scores[c * Lt + i, :C].astype(np.float64)
            if logits:
                keep = np.arange(C) != UNK
                m = row[keep].max()
                lse = m + np.log(np.exp(row[keep] - m).sum())
                g = np.where(keep, np.exp(row - lse), 0.0)
                g[y] -= 1.0
                d[c * Lt + i, :C] = s * g
            else:
                d[c * Lt + i, y] = -s / row[y]
    return dict(loss=np.float32(-total), cum=cum, step=step, barred=barred, len=length, dscores=d)


def sequence_loss(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                  ingr_id_dict, oov_word_dict, captions, weights):
    """``P`` the oracle's parameter dict (leaves that require grad), ``captions`` per video (S_b, K, Lt) ids, ``weights`` per video
    (S_b, K) → (loss: a float64 torch scalar under autograd, cum: per video (S_b, K) float64, barred: per video (S_b, K) bool).  The
    construction is ``forced_score_reference.forced_decode``'s: text half blanked, the decoder once over all Lt positions of every caption
    under its causal mask."""
    mode, Lv, Lt, V = cfg.model_mode, cfg.max_v_len, cfg.max_t_len, cfg.vocab_size
    ingr_input_ids = torch.as_tensor(ingr_input_ids)
    ingr_sep_masks = torch.as_tensor(ingr_sep_masks)
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    loss = torch.zeros((), dtype=torch.float64)
    cums, bars = [], []
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
        walk = fr.score_rows(sc.detach().numpy().astype(np.float32).reshape(R * Lt, -1), y, np.full(R, C), mode == "video", "bar")
        w = np.asarray(weights[b], np.float64).reshape(R)
        cum_b, bar_b = [], []
        for c in range(R):
            n = int(walk["len"][c])
            barred = not np.isfinite(walk["step"][c, :n]).all()
            bar_b.append(barred)
            if barred or n == 0:
                cum_b.append(torch.zeros((), dtype=torch.float64))
                continue
            rows = sc[c, :n]
            tgt = torch.as_tensor(y[c, 1:n + 1]).long()
            picked = rows.gather(1, tgt.unsqueeze(1)).squeeze(1)
            if mode == "video":
                keep = torch.arange(C) != UNK
                lp = picked - torch.logsumexp(rows[:, keep], 1)
            else:
                lp = torch.log(picked)
            cum = lp.sum()
            cum_b.append(cum)
            loss = loss - w[c] * cum
        cums.append(torch.stack([c_.detach() for c_ in cum_b]).reshape(S_b, K))
        bars.append(np.asarray(bar_b).reshape(S_b, K))
    return loss, cums, bars
