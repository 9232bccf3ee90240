"""CPU restatement of paragraph-scope n-gram blocking (svpc_amd.translator's ``block_ngram_scope="paragraph"``), built on the oracle
functions like tests/beam_controls_reference.py.  ``select_para`` is the selection rule the HIP kernel (svpc_beam_step_para) must reproduce
exactly: ``select_ctl`` plus the bans of the earlier captions of the sentence's video, with the same margins.  ``beam_decode_para`` decodes
each video sentence by sentence; its ``history=`` override decodes sentence s under given captions of sentences 0 … s − 1 (a GPU result
can then be checked one sentence at a time under its own earlier captions, so an early near-tie does not cascade)."""
import numpy as np
import torch

from beam_controls_reference import _key, banned_words, final_order
from beam_reference import step_scores
from oracle import svpc_oracle as orc
from svpc_amd.ops import length_penalty_table
from svpc_amd.synthetic import BOS, EOS, PAD, UNK


def caption_grams(z, n, bos=BOS, eos=EOS, pad=PAD):
    """the n-grams of one chosen caption z (extended ids, position 0 BOS): its words are the ids at positions 1 … L, L + 1 its first EOS
    or PAD (L = len(z) − 1 without one), BOS excepted; a gram is n consecutive positions that are all words (none spans two captions)"""
    z = [int(v) for v in z]
    last = len(z) - 1
    for j in range(1, len(z)):
        if z[j] in (eos, pad):
            last = j - 1
            break
    return [tuple(z[j:j + n]) for j in range(1, last - n + 2) if bos not in z[j:j + n]]


def caption_words(z, bos=BOS, eos=EOS, pad=PAD):
    """the words of one caption, in order (its 1-grams)"""
    return [g[0] for g in caption_grams(z, 1, bos, eos, pad)]


def paragraph_banned_words(y, pos, n, exclusion, history):
    """The words w that candidate (h, w) may not pick at p = pos + 1 because the gram (y_{p−n+1} … y_pos, w) is a gram of one of the
    captions ``history`` (the chosen captions of the video's earlier sentences) and none of its tokens is excluded.  (The hypothesis's own
    repeats are ``banned_words``.)"""
    p = pos + 1
    if n <= 0 or p < n:
        return set()
    y = [int(v) for v in y[:pos + 1]]
    suffix = tuple(y[p - n + 1:p])
    if any(t in exclusion for t in suffix):
        return set()
    out = set()
    for z in history:
        for g in caption_grams(z, n):
            if g[:-1] == suffix and g[-1] not in exclusion:
                out.add(g[-1])
    return out


def select_para(scores, row_c, row_x, beam, logits, cum, finished, length, hist, pos, history, min_length=0, block_ngram_repeat=0,
                exclusion_tokens=(), lp=None, unk=UNK, eos=EOS, pad=PAD, return_margin=False):
    """``select_ctl`` with paragraph scope: ``history[t]`` is the list of earlier captions of sentence t's video (each an id sequence with
    BOS at position 0); a candidate is banned by its own hypothesis (``banned_words``) or by them (``paragraph_banned_words``).
    → as ``select_ctl``."""
    scores = np.asarray(scores, dtype=np.float32)
    cum = np.asarray(cum, dtype=np.float32)
    finished = np.asarray(finished).astype(bool)
    length = np.asarray(length).astype(np.int64)
    excl = set(int(e) for e in exclusion_tokens)
    R = scores.shape[0]
    B = beam
    T = R // B
    p = pos + 1
    parent = np.zeros(R, np.int64)
    ext = np.zeros(R, np.int64)
    mod = np.zeros(R, np.int64)
    cum_new = np.zeros(R, np.float32)
    fin_new = np.zeros(R, bool)
    len_new = np.zeros(R, np.int64)
    margin = np.full(T, np.inf)
    for t in range(T):
        ck, cc, cr, cf, ch, ccol, cfin = [], [], [], [], [], [], []
        for h in range(B):
            r = t * B + h
            C = int(row_c[r])
            if finished[r]:
                ck.append([_key(cum[r], length[r], lp)]); cc.append(np.array([cum[r]], np.float32)); cr.append(np.array([np.inf], np.float32))
                cf.append([h * C + pad]); ch.append([h]); ccol.append([pad]); cfin.append([True])
                continue
            ban = banned_words(hist[r], pos, block_ngram_repeat, excl) | paragraph_banned_words(hist[r], pos, block_ngram_repeat, excl,
                                                                                                   history[t])
            cols = np.array([c for c in range(C) if c != unk and c not in ban and not (p <= min_length and c == eos)], dtype=np.int64)
            st = step_scores(scores[r, :C], logits, unk)[cols]        # (banned columns stay in the log-sum-exp)
            cu = (np.float32(cum[r]) + st).astype(np.float32)
            ck.append([_key(v, p, lp) for v in cu]); cc.append(cu); cr.append(scores[r, cols])
            cf.append(h * C + cols); ch.append(np.full(len(cols), h)); ccol.append(cols); cfin.append(np.zeros(len(cols), bool))
        ck = np.concatenate([np.asarray(k, np.float64) for k in ck])
        cc, cr = np.concatenate(cc), np.concatenate(cr)
        cf, ch = np.concatenate([np.asarray(v, np.int64) for v in cf]), np.concatenate([np.asarray(v, np.int64) for v in ch])
        ccol, cfin = np.concatenate([np.asarray(v, np.int64) for v in ccol]), np.concatenate([np.asarray(v, bool) for v in cfin])
        order = np.lexsort((cf, -cr.astype(np.float64), -ck))
        if len(order) > B:
            with np.errstate(invalid="ignore"):
                margin[t] = ck[order[B - 1]] - ck[order[B]]
        for k in range(B):
            r = t * B + k
            if k < len(order):
                e = order[k]
                h, col, was_fin, cu = int(ch[e]), int(ccol[e]), bool(cfin[e]), cc[e]
                ln = length[t * B + h] if was_fin else p
            else:
                h, col, was_fin, cu, ln = k, pad, True, np.float32(-np.inf), p
            C, X = int(row_c[t * B + h]), int(row_x[t * B + h])
            parent[r] = t * B + h
            ext[r] = pad if was_fin else col
            mod[r] = pad if was_fin else (unk if col >= C - X else col)
            cum_new[r] = cu
            fin_new[r] = was_fin or ext[r] == eos
            len_new[r] = ln
    out = (parent, ext, mod, cum_new, fin_new, len_new)
    return out + (margin,) if return_margin else out


def beam_decode_para(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                     ingr_id_dict, oov_word_dict, beam, min_length=0, block_ngram_repeat=0, exclusion_tokens=(), length_penalty_name="none",
                     length_penalty_alpha=0.0, history=None, bos=BOS, unk=UNK):
    """Paragraph-scope beam decode → (ids, cums, lens, margins) shaped as ``beam_decode_ctl``'s.  Sentence s of video b is decoded over B
    hypothesis rows after sentences 0 … s − 1, under the captions ``history[b][0 … s − 1]`` when given (each an id sequence with BOS at
    position 0), else under its own chosen captions (row 0 in final-key order)."""
    mode, Lv, Lt = cfg.model_mode, cfg.max_v_len, cfg.max_t_len
    V = cfg.vocab_size
    B = beam
    lp = None if length_penalty_name == "none" else length_penalty_table(length_penalty_name, length_penalty_alpha, Lt)
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
        g = orc.encoder(P, "step_wise_encoder", (enc[:, 0] + pe50[:S_b]).unsqueeze(0), torch.ones(1, S_b), cfg)[0]
        n_oov = len(oov_word_dict[b]) if mode != "video" else 0
        bank_all = None
        if mode in ("full", "reason_copy"):
            _, _, bar_e, all_e, bar_f = orc.simulator(P, "reasoner", g, ingr)
            mem_all = torch.stack([g, torch.relu(orc.linear(P, "Went.0", bar_e)), torch.relu(orc.linear(P, "Wac.0", bar_f))], 1)
            bank_all = all_e
        elif mode == "copy":
            mem_all = torch.stack([g, ingr.mean(0).unsqueeze(0).expand(S_b, -1)], 1)
            bank_all = ingr.unsqueeze(0).expand(S_b, -1, -1)
        else:
            mem_all = g.unsqueeze(1)
        C = V + n_oov
        row_c, row_x = np.full(B, C), np.full(B, n_oov)
        v_ids = torch.full((S_b, B, Lt), PAD, dtype=torch.long)
        v_cum = np.zeros((S_b, B), np.float32)
        v_len = np.zeros((S_b, B), np.int64)
        margins = np.full((S_b, Lt), np.inf)
        chosen = []
        for s in range(S_b):
            hist_s = [list(map(int, z)) for z in (history[b][:s] if history is not None else chosen)]
            mem = mem_all[s:s + 1].repeat_interleave(B, 0)
            bank = bank_all[s:s + 1].repeat_interleave(B, 0) if bank_all is not None else None
            text = torch.full((B, Lt), PAD, dtype=torch.long); text[:, 0] = bos
            ext = text.clone()
            cum = np.zeros(B, np.float32); cum[1:] = -np.inf
            fin = np.zeros(B, bool)
            ln = np.zeros(B, np.int64)
            for i in range(Lt - 1):
                dec = orc.decoder(P, orc.text_embed(P, text[:, :i + 1], cfg), torch.ones(B, i + 1), mem, torch.ones(mem.shape[:2]), cfg)
                last = dec[:, i:i + 1]
                if mode == "video":
                    sc = orc.lm_head(P, last, cfg)[:, 0]
                else:
                    sc = orc.pointer_generator(P, last, bank, ingr_id_dict[b], n_oov, cfg)[:, 0]
                parent, nx_ext, nx_mod, cum, fin, ln, mg = select_para(
                    sc.detach().numpy(), row_c, row_x, B, mode == "video", cum, fin, ln, ext.numpy(), i, [hist_s], min_length=min_length,
                    block_ngram_repeat=block_ngram_repeat, exclusion_tokens=exclusion_tokens, lp=lp, unk=unk, return_margin=True)
                margins[s, i] = mg[0]
                pt = torch.as_tensor(parent)
                text, ext = text[pt].clone(), ext[pt].clone()
                text[:, i + 1] = torch.as_tensor(nx_mod)
                ext[:, i + 1] = torch.as_tensor(nx_ext)
            order, keys = final_order(cum, ln, lp)
            d = [keys[order[k]] - keys[order[k + 1]] for k in range(B - 1)]
            d = [v for v in d if np.isfinite(v)]
            margins[s, Lt - 1] = min(d) if d else np.inf
            v_ids[s] = ext[torch.as_tensor(order)]
            v_cum[s] = cum[order]
            v_len[s] = ln[order]
            chosen.append(v_ids[s, 0].tolist())
        out.append(v_ids)
        out_cum.append(v_cum)
        out_len.append(v_len)
        out_margins.append(margins)
    return out, out_cum, out_len, out_margins

