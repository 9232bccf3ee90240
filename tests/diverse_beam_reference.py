"""CPU restatement of diverse (group) beam search (Vijayakumar et al. 2016, arXiv 1610.02424, Hamming diversity; svpc_amd.translator's
``translate_batch_diverse``), in the style of tests/beam_controls_reference.py and built on the same oracle functions.  ``select_groups`` is
the selection rule the HIP kernel (svpc_beam_step_groups) must reproduce bit for bit.  It shares no code with the product: the penalty
table is restated here (``penalty_table``), the candidates of a row are those of ``beam_controls_reference.select_ctl`` and the step
score is ``beam_reference.step_scores``.

Sizes: W rows per sentence in G groups of Bg = W / G; row t·W + g·Bg + j is hypothesis j of group g of sentence t.  State per row:
``cum`` (the model's summed step scores), ``aug`` (the selection score: cum minus every penalty paid), finished, len.  One step, for
g = 0 … G − 1 in order: n(c) = the rows of groups 0 … g − 1 whose pick at this step is a live pick (a word chosen from an unfinished
parent) with extended id c; a child (h, c) of an unfinished parent h of group g has cum' = fp32(cum_h + step), aug' = fp32(fp32(aug_h +
step) − pen[n(c)]), key (double)aug' / lp[p], length p; a finished parent offers itself (PAD, cum / aug / len kept, key (double)aug /
lp[len], raw +inf, no penalty).  Group g's candidates rank by higher key, then higher raw value, then lower flat index h·C + c (h the
row within the sentence); the Bg best become rows g·Bg …; missing ones are fill rows (parent the slot, PAD, −inf, finished, length p).
At the end each group's rows are ordered by (double)cum / lp[len], ties to the lower index."""
import numpy as np
import torch

from beam_controls_reference import _key, banned_words, final_order
from beam_reference import step_scores
from oracle import svpc_oracle as orc
from svpc_amd.synthetic import BOS, EOS, PAD, UNK


def penalty_table(strength, beam):
    """pen[n] = fp32(fp32(λ) · n), n = 0 … beam − 1"""
    lam = np.float32(strength)
    return np.array([np.float32(lam * np.float32(n)) for n in range(beam)], dtype=np.float32)


def length_table(name, alpha, lt):
    """the length-penalty table restated: ``none`` None, ``avg`` len (1 at 0), ``wu`` ((5 + len) / 6) ** alpha — Python floats"""
    if name == "none":
        return None
    if name == "avg":
        return [1.0] + [float(n) for n in range(1, lt)]
    return [((5.0 + n) / 6.0) ** float(alpha) for n in range(lt)]


def start_scores(n_sent, beam, groups):
    """cum = aug = 0 on row 0 of every group, −inf on the others → (n_sent·beam,) float32"""
    c = np.full((n_sent, groups, beam // groups), -np.inf, np.float32)
    c[:, :, 0] = 0.0
    return c.reshape(-1)


def select_groups(scores, row_c, row_x, beam, groups, logits, cum, aug, finished, length, hist, pos, pen, min_length=0,
                  block_ngram_repeat=0, exclusion_tokens=(), lp=None, unk=UNK, eos=EOS, pad=PAD, return_margin=False):
    """One selection step → parent (global rows), next extended ids, next model ids, new cum, new aug, new finished, new length
    [, margin (T,): over the groups, the smallest key of the last kept candidate minus key of the first dropped one; +inf when nothing is
    dropped]."""
    scores = np.asarray(scores, dtype=np.float32)
    cum = np.asarray(cum, dtype=np.float32)
    aug = np.asarray(aug, dtype=np.float32)
    finished = np.asarray(finished).astype(bool)
    length = np.asarray(length).astype(np.int64)
    pen = np.asarray(pen, dtype=np.float32)
    excl = set(int(e) for e in exclusion_tokens)
    R = scores.shape[0]
    W, G = beam, groups
    Bg = W // G
    assert Bg * G == W and R % W == 0
    T = R // W
    p = pos + 1
    parent = np.zeros(R, np.int64)
    ext = np.zeros(R, np.int64)
    mod = np.zeros(R, np.int64)
    cum_new = np.zeros(R, np.float32)
    aug_new = np.zeros(R, np.float32)
    fin_new = np.zeros(R, bool)
    len_new = np.zeros(R, np.int64)
    margin = np.full(T, np.inf)
    for t in range(T):
        picks = []                                  # the live picks of the rows of the groups done so far
        for g in range(G):
            ck, cr, cf, ch, ccol, cfin, cc, ca = [], [], [], [], [], [], [], []
            for j in range(Bg):
                h = g * Bg + j
                r = t * W + h
                C = int(row_c[r])
                if finished[r]:
                    ck.append(np.array([_key(aug[r], length[r], lp)], np.float64)); cr.append(np.array([np.inf], np.float32))
                    cf.append(np.array([h * C + pad], np.int64)); ch.append(np.array([h], np.int64)); ccol.append(np.array([pad], np.int64))
                    cfin.append(np.array([True])); cc.append(np.array([cum[r]], np.float32)); ca.append(np.array([aug[r]], np.float32))
                    continue
                ban = banned_words(hist[r], pos, block_ngram_repeat, excl)
                cols = np.array([c for c in range(C) if c != unk and c not in ban and not (p <= min_length and c == eos)], dtype=np.int64)
                st = step_scores(scores[r, :C], logits, unk)[cols]
                n = np.array([sum(1 for w in picks if w == c) for c in cols], dtype=np.int64) if picks else np.zeros(len(cols), np.int64)
                with np.errstate(invalid="ignore"):
                    cu = (np.float32(cum[r]) + st).astype(np.float32)
                    au = ((np.float32(aug[r]) + st).astype(np.float32) - pen[n]).astype(np.float32)
                ck.append(np.array([_key(v, p, lp) for v in au], np.float64)); cr.append(scores[r, cols])
                cf.append(h * C + cols); ch.append(np.full(len(cols), h, np.int64)); ccol.append(cols)
                cfin.append(np.zeros(len(cols), bool)); cc.append(cu); ca.append(au)
            ck, cr, cf, ch = np.concatenate(ck), np.concatenate(cr), np.concatenate(cf), np.concatenate(ch)
            ccol, cfin, cc, ca = np.concatenate(ccol), np.concatenate(cfin), np.concatenate(cc), np.concatenate(ca)
            order = np.lexsort((cf, -cr.astype(np.float64), -ck))
            if len(order) > Bg:
                with np.errstate(invalid="ignore"):
                    m = ck[order[Bg - 1]] - ck[order[Bg]]
                if not np.isnan(m):
                    margin[t] = min(margin[t], m)
            new_picks = []
            for k in range(Bg):
                slot = g * Bg + k
                r = t * W + slot
                if k < len(order):
                    e = order[k]
                    h, col, was_fin, cu, au = int(ch[e]), int(ccol[e]), bool(cfin[e]), cc[e], ca[e]
                    ln = length[t * W + h] if was_fin else p
                    if not was_fin:
                        new_picks.append(col)
                else:
                    h, col, was_fin, cu, au, ln = slot, pad, True, np.float32(-np.inf), np.float32(-np.inf), p
                C, X = int(row_c[t * W + h]), int(row_x[t * W + h])
                parent[r] = t * W + h
                ext[r] = pad if was_fin else col
                mod[r] = pad if was_fin else (unk if col >= C - X else col)
                cum_new[r], aug_new[r] = cu, au
                fin_new[r] = was_fin or ext[r] == eos
                len_new[r] = ln
            picks += new_picks
    out = (parent, ext, mod, cum_new, aug_new, fin_new, len_new)
    return out + (margin,) if return_margin else out


def diverse_decode(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                   ingr_id_dict, oov_word_dict, beam, groups, strength, min_length=0, block_ngram_repeat=0, exclusion_tokens=(),
                   length_penalty_name="none", length_penalty_alpha=0.0, bos=BOS, unk=UNK):
    """→ (ids, cums, lens, margins): per video all W final hypotheses, group-major, each group's rows in final-key order — ids (S_b, W,
    Lt) int64 (extended ids, PAD after EOS), cum (S_b, W) float32 (the model's score), len (S_b, W) int64 — and margins (S_b, Lt): the
    selection margins of the Lt − 1 steps (``select_groups``) and, last, the smallest finite gap between consecutive final keys of one
    group."""
    mode, Lv, Lt = cfg.model_mode, cfg.max_v_len, cfg.max_t_len
    V = cfg.vocab_size
    W, G = beam, groups
    Bg = W // G
    lp = length_table(length_penalty_name, length_penalty_alpha, Lt)
    pen = penalty_table(strength, W)
    ingr_input_ids = torch.as_tensor(ingr_input_ids)
    ingr_sep_masks = torch.as_tensor(ingr_sep_masks)
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    out, out_cum, out_len, out_margins = [], [], [], []
    for b, S_b in enumerate(batch_step_num):
        ids = torch.stack([input_ids_list[s][b] for s in range(S_b)]).clone()
        masks = torch.stack([input_masks_list[s][b] for s in range(S_b)]).clone()
        feats = torch.stack([video_features_list[s][b] for s in range(S_b)])
        ids[:, Lv:] = 0; masks[:, Lv:] = 0
        ingr = orc.ingredient_embed(P, ingr_input_ids[b:b + 1], ingr_sep_masks[b:b + 1], cfg)[0]
        enc = orc.forward_step(P, ids, feats, masks, cfg)
        g_ = orc.encoder(P, "step_wise_encoder", (enc[:, 0] + pe50[:S_b]).unsqueeze(0), torch.ones(1, S_b), cfg)[0]
        n_oov = len(oov_word_dict[b]) if mode != "video" else 0
        bank = None
        if mode in ("full", "reason_copy"):
            _, _, bar_e, all_e, bar_f = orc.simulator(P, "reasoner", g_, ingr)
            mem = torch.stack([g_, torch.relu(orc.linear(P, "Went.0", bar_e)), torch.relu(orc.linear(P, "Wac.0", bar_f))], 1)
            bank = all_e
        elif mode == "copy":
            mem = torch.stack([g_, ingr.mean(0).unsqueeze(0).expand(S_b, -1)], 1)
            bank = ingr.unsqueeze(0).expand(S_b, -1, -1)
        else:
            mem = g_.unsqueeze(1)
        mem = mem.repeat_interleave(W, 0)
        bank = bank.repeat_interleave(W, 0) if bank is not None else None
        R = S_b * W
        C = V + n_oov
        row_c, row_x = np.full(R, C), np.full(R, n_oov)
        text = torch.full((R, Lt), PAD, dtype=torch.long); text[:, 0] = bos
        ext = text.clone()
        cum = start_scores(S_b, W, G)
        aug = cum.copy()
        fin = np.zeros(R, bool)
        ln = np.zeros(R, np.int64)
        margins = np.full((S_b, Lt), np.inf)
        for i in range(Lt - 1):
            dec = orc.decoder(P, orc.text_embed(P, text[:, :i + 1], cfg), torch.ones(R, i + 1), mem, torch.ones(mem.shape[:2]), cfg)
            last = dec[:, i:i + 1]
            if mode == "video":
                sc = orc.lm_head(P, last, cfg)[:, 0]
            else:
                sc = orc.pointer_generator(P, last, bank, ingr_id_dict[b], n_oov, cfg)[:, 0]
            parent, nx_ext, nx_mod, cum, aug, fin, ln, margins[:, i] = select_groups(
                sc.detach().numpy(), row_c, row_x, W, G, mode == "video", cum, aug, fin, ln, ext.numpy(), i, pen, min_length=min_length,
                block_ngram_repeat=block_ngram_repeat, exclusion_tokens=exclusion_tokens, lp=lp, unk=unk, return_margin=True)
            pt = torch.as_tensor(parent)
            text, ext = text[pt].clone(), ext[pt].clone()
            text[:, i + 1] = torch.as_tensor(nx_mod)
            ext[:, i + 1] = torch.as_tensor(nx_ext)
        rows = []
        for s in range(S_b):
            row, gaps = [], []
            for g in range(G):
                lo = s * W + g * Bg
                order, keys = final_order(cum[lo:lo + Bg], ln[lo:lo + Bg], lp)
                row += [lo + h for h in order]
                gaps += [keys[order[k]] - keys[order[k + 1]] for k in range(Bg - 1)]
            rows.append(row)
            gaps = [v for v in gaps if np.isfinite(v)]
            margins[s, Lt - 1] = min(gaps) if gaps else np.inf
        rows = np.array(rows, dtype=np.int64).reshape(S_b, W)
        out.append(ext[torch.as_tensor(rows)])
        out_cum.append(cum[rows].astype(np.float32))
        out_len.append(ln[rows])
        out_margins.append(margins)
    return out, out_cum, out_len, out_margins
