"""CPU restatement of stochastic beam search (Kool, van Hoof and Welling 2019, "Stochastic Beams and Where to Find Them", arXiv
1903.06059; svpc_amd.translator's contract for ``translate_batch_stochastic``), built on the oracle's own functions and shaped like
``beam_reference.beam_decode``.  ``stochastic_beam_select`` is the step the HIP kernel (svpc_beam_step_gumbel) must reproduce: the same
ids, parents, finished flags and lengths, cum bit for bit, phi and G to 1e-9 — wherever the returned margin (the smallest gap that
decides the short lists and the selection) is above the fp64 noise of a log-sum-exp summed in another order.

Rows: sentence t has W rows r = t·W + h carrying cum (float32, the model's summed step score), phi (float64, the log-probability of the
row's sequence under the tempered, renormalised model), G (float64, the perturbed log-probability), finished and len.  A dead row is
finished with G = −inf.  It shares no code with svpc_amd/."""
import numpy as np
import torch

from beam_reference import step_scores
from oracle import svpc_oracle as orc
from sampling_reference import COL_STRIDE, gumbel
from svpc_amd.synthetic import BOS, EOS, PAD, UNK


def initial_state(n_sent, beam):
    """→ (cum float32, phi float64, G float64, finished bool, length int64), all (n_sent·beam,): row 0 of a sentence alive with
    cum = phi = G = 0, rows 1 … beam − 1 dead"""
    cum = np.zeros((n_sent, beam), np.float32)
    cum[:, 1:] = -np.inf
    cum = cum.reshape(-1)
    return cum, cum.astype(np.float64), cum.astype(np.float64), np.isinf(cum), np.zeros(n_sent * beam, np.int64)


def truncated_gumbel(G, g, Z):
    """G̃ = G − max(v, 0) − log1p(exp(−|v|)), v = G − g + log1p(−exp(g − Z)) (appendix B.3, the stable form): the perturbed
    log-probabilities g ≤ Z of a parent's children conditioned on their maximum being the parent's G"""
    with np.errstate(divide="ignore"):
        v = G - g + np.log1p(-np.exp(g - Z))
    return G - np.maximum(v, 0.0) - np.log1p(np.exp(-np.abs(v)))


def row_candidates(scores_row, C, logits, pos, phi_h, seed, r, temp=1.0, min_length=0, unk=UNK, eos=EOS):
    """K0 of one live row r in column order → (columns, step scores float32, φ float64, g float64); empty arrays for an empty K0"""
    raw = np.asarray(scores_row, np.float32)[:C]
    with np.errstate(invalid="ignore", divide="ignore"):
        s = step_scores(raw, logits, unk)
    cols = np.arange(C)
    with np.errstate(invalid="ignore"):
        cand = (cols != unk) & (s > -np.inf)
    if pos + 1 <= min_length and eos < C:
        cand[eos] = False
    k0 = cols[cand]
    if not len(k0):
        return k0, s[k0], np.zeros(0), np.zeros(0)
    z = s[k0].astype(np.float64) / float(temp)
    m = z.max()
    L = m + np.log(np.exp(z - m).sum())
    phi_c = phi_h + (z - L)
    return k0, s[k0], phi_c, phi_c + gumbel(seed, pos, r * COL_STRIDE + k0)


def stochastic_beam_select(scores, row_c, row_x, beam, pos, logits, cum, phi, G, finished, length, seed, temp=1.0, min_length=0, row0=0,
                           unk=UNK, eos=EOS, pad=PAD, detail=None):
    """One selection step over the rows of ``scores`` (T·W, ≥ C) float32; row i is the kernel's row r = row0 + i (its draws are keyed by
    r).  → dict(parent (rows of ``scores``), ext, mod, cum, phi, G, finished, length, margin (T,)): margin is the smallest of the gap
    between the W-th and (W + 1)-th g of a live parent and the gaps between adjacent G̃ through the (W + 1)-th candidate of the
    sentence (+inf where there is none).  ``detail``: a list that receives (row, columns, g, G̃) of every live parent's short list."""
    scores = np.asarray(scores, dtype=np.float32)
    R, W, p = scores.shape[0], beam, pos + 1
    T = R // W
    out = dict(parent=np.zeros(R, np.int64), ext=np.full(R, pad, np.int64), mod=np.full(R, pad, np.int64),
               cum=np.full(R, -np.inf, np.float32), phi=np.full(R, -np.inf), G=np.full(R, -np.inf), finished=np.ones(R, bool),
               length=np.full(R, p, np.int64), margin=np.full(T, np.inf))
    for t in range(T):
        cands = []          # (G̃, g, flat, h, column, cum, phi, finished parent)
        for h in range(W):
            r = t * W + h
            if finished[r]:
                if G[r] > -np.inf:
                    cands.append((float(G[r]), float(G[r]), h * COL_STRIDE + pad, h, pad, np.float32(cum[r]), float(phi[r]), True))
                continue
            k0, s, phi_c, g = row_candidates(scores[r], int(row_c[r]), logits, pos, float(phi[r]), seed, row0 + r, temp, min_length, unk, eos)
            if not len(k0):
                continue
            order = np.lexsort((k0, -g))
            short = order[:W]
            if len(order) > W:
                out["margin"][t] = min(out["margin"][t], float(g[order[W - 1]] - g[order[W]]))
            gt = truncated_gumbel(float(G[r]), g[short], g[short[0]])
            if detail is not None:
                detail.append((r, k0[short], g[short], gt))
            for j, e in enumerate(short):
                cands.append((float(gt[j]), float(g[e]), h * COL_STRIDE + int(k0[e]), h, int(k0[e]),
                              np.float32(np.float32(cum[r]) + s[e]), float(phi_c[e]), False))
        cands.sort(key=lambda c: (-c[0], -c[1], c[2]))
        for a, b in zip(cands[:W], cands[1:W + 1]):
            out["margin"][t] = min(out["margin"][t], a[0] - b[0])
        for k in range(W):
            r = t * W + k
            if k >= len(cands):                  # a leftover slot: a dead row on its own slot's ids
                out["parent"][r] = r
                continue
            gt, _, _, h, col, cu, ph, was_fin = cands[k]
            C, X = int(row_c[t * W + h]), int(row_x[t * W + h])
            out["parent"][r] = t * W + h
            out["ext"][r] = pad if was_fin else col
            out["mod"][r] = pad if was_fin else (unk if col >= C - X else col)
            out["cum"][r], out["phi"][r], out["G"][r] = cu, ph, gt
            out["finished"][r] = was_fin or col == eos
            out["length"][r] = length[t * W + h] if was_fin else p
    return out


def stochastic_beam_decode(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                           ingr_id_dict, oov_word_dict, beam, seed, temp=1.0, min_length=0, bos=BOS, unk=UNK):
    """→ (ids, cums, lens, Gs, phis, margins): per video ids (S_b, W, Lt) int64 (extended ids, PAD after EOS), cum (S_b, W) float32, len
    (S_b, W) int64, G and phi (S_b, W) float64 in the order drawn, and margins (S_b,): the smallest step margin of each sentence.
    Sentence s of video b is the batch's sentence t = Σ_{b' < b} S_b' + s, its rows the kernel rows t·W + h."""
    mode, Lv, Lt = cfg.model_mode, cfg.max_v_len, cfg.max_t_len
    V, W = cfg.vocab_size, beam
    ingr_input_ids = torch.as_tensor(ingr_input_ids)
    ingr_sep_masks = torch.as_tensor(ingr_sep_masks)
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    outs = [[] for _ in range(6)]
    t0 = 0
    for b, S_b in enumerate(batch_step_num):
        ids = torch.stack([input_ids_list[s][b] for s in range(S_b)]).clone()
        masks = torch.stack([input_masks_list[s][b] for s in range(S_b)]).clone()
        feats = torch.stack([video_features_list[s][b] for s in range(S_b)])
        ids[:, Lv:] = 0; masks[:, Lv:] = 0                                             # translator.py:205-228
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
        mem = mem.repeat_interleave(W, 0)                                              # rows s·W + h
        bank = bank.repeat_interleave(W, 0) if bank is not None else None
        R = S_b * W
        C = V + n_oov
        row_c, row_x = np.full(R, C), np.full(R, n_oov)
        text = torch.full((R, Lt), PAD, dtype=torch.long); text[:, 0] = bos
        ext = text.clone()
        cum, phi, G, fin, ln = initial_state(S_b, W)
        margins = np.full(S_b, np.inf)
        for i in range(Lt - 1):
            dec = orc.decoder(P, orc.text_embed(P, text[:, :i + 1], cfg), torch.ones(R, i + 1), mem, torch.ones(mem.shape[:2]), cfg)
            last = dec[:, i:i + 1]
            if mode == "video":
                sc = orc.lm_head(P, last, cfg)[:, 0]
            else:
                sc = orc.pointer_generator(P, last, bank, ingr_id_dict[b], n_oov, cfg)[:, 0]
            o = stochastic_beam_select(sc.detach().numpy(), row_c, row_x, W, i, mode == "video", cum, phi, G, fin, ln, seed, temp,
                                       min_length, row0=t0 * W, unk=unk)
            cum, phi, G, fin, ln = o["cum"], o["phi"], o["G"], o["finished"], o["length"]
            margins = np.minimum(margins, o["margin"])
            pt = torch.as_tensor(o["parent"])
            text, ext = text[pt].clone(), ext[pt].clone()
            text[:, i + 1] = torch.as_tensor(o["mod"])
            ext[:, i + 1] = torch.as_tensor(o["ext"])
        for lst, v in zip(outs, (ext.view(S_b, W, Lt), cum.reshape(S_b, W), ln.reshape(S_b, W), G.reshape(S_b, W), phi.reshape(S_b, W),
                                 margins)):
            lst.append(v)
        t0 += S_b
    return tuple(outs)
