"""CPU restatement of beam search with decoding controls (svpc_amd.translator's contract: ``block_ngram_repeat``, ``exclusion_tokens``,
``min_length``, ``length_penalty_name`` / ``length_penalty_alpha``, ``n_best``), in the style of tests/beam_reference.py and built on the
same oracle functions.  ``select_ctl`` is the selection rule the HIP kernel (svpc_beam_step_ctl) must reproduce exactly; with every
control off it is ``beam_reference.select``.

The length-penalty table is ``svpc_amd.ops.length_penalty_table``: computed once on the host, the kernel divides by the same float64
numbers, so the ranking key (double)cum / lp[len] is reproduced bit for bit."""
import numpy as np
import torch

from beam_reference import step_scores
from oracle import svpc_oracle as orc
from svpc_amd.ops import length_penalty_table
from svpc_amd.synthetic import BOS, EOS, PAD, UNK


def banned_words(y, pos, n, exclusion):
    """The words w that candidate (h, w) may not pick at position p = pos + 1: h's extended ids y (positions 0 … pos, y[0] = BOS not a
    word) already hold the gram (y_{p−n+1} … y_pos, w) at some start j = 1 … p − n, and no token of that gram is excluded."""
    p = pos + 1
    if n <= 0 or p < n:
        return set()
    y = [int(v) for v in y[:pos + 1]]
    suffix = tuple(y[p - n + 1:p])
    out = set()
    for j in range(1, p - n + 1):
        gram = tuple(y[j:j + n])
        if gram[:-1] == suffix and not any(t in exclusion for t in gram):
            out.add(gram[-1])
    return out


def _key(cum, ln, lp):
    return float(np.float32(cum)) if lp is None else float(np.float64(np.float32(cum)) / np.float64(lp[int(ln)]))


def select_ctl(scores, row_c, row_x, beam, logits, cum, finished, length, hist, pos, min_length=0, block_ngram_repeat=0,
               exclusion_tokens=(), lp=None, unk=UNK, eos=EOS, pad=PAD, return_margin=False):
    """One selection step with controls.  ``hist`` (T·B, ≥ pos + 1): every hypothesis's extended ids at positions 0 … pos; ``length``
    (T·B,) its length; ``lp`` a length-penalty table (None: none).  Candidates of a sentence: (h, c) for c ≠ UNK, c < C, not banned, not
    EOS while pos + 1 ≤ min_length, of an unfinished h (key (double)cum / lp[pos + 1]), and (h, PAD) of a finished one (its own cum and
    length, raw +inf); ranked by higher key, then higher raw value, then lower flat index h·C + c.
    → parent, next extended ids, next model ids, new cum, new finished, new length [, margin (T,): key of the last kept candidate minus
    key of the first dropped one, +inf when nothing is dropped]."""
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
            ban = banned_words(hist[r], pos, block_ngram_repeat, excl)
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
            with np.errstate(invalid="ignore"):            # (−inf − −inf: no margin to speak of)
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


def final_order(cum, length, lp):
    """indices of one sentence's B final hypotheses by higher final key, ties to the lower index"""
    keys = [_key(c, ln, lp) for c, ln in zip(cum, length)]
    return sorted(range(len(keys)), key=lambda h: (-keys[h], h)), keys


def beam_decode_ctl(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                    ingr_id_dict, oov_word_dict, beam, min_length=0, block_ngram_repeat=0, exclusion_tokens=(), length_penalty_name="none",
                    length_penalty_alpha=0.0, bos=BOS, unk=UNK):
    """→ (ids, cums, lens, margins): per video all B final hypotheses in final-key order — ids (S_b, B, Lt) int64 (extended ids, PAD after
    EOS), cum (S_b, B) float32, len (S_b, B) int64 — and margins (S_b, Lt): the selection margins of the Lt − 1 steps (``select_ctl``) and,
    last, the smallest finite gap between consecutive final keys."""
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
        mem = mem.repeat_interleave(B, 0)
        bank = bank.repeat_interleave(B, 0) if bank is not None else None
        R = S_b * B
        C = V + n_oov
        row_c, row_x = np.full(R, C), np.full(R, n_oov)
        text = torch.full((R, Lt), PAD, dtype=torch.long); text[:, 0] = bos
        ext = text.clone()
        cum = np.zeros((S_b, B), np.float32); cum[:, 1:] = -np.inf
        cum = cum.reshape(-1)
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
            parent, nx_ext, nx_mod, cum, fin, ln, margins[:, i] = select_ctl(
                sc.detach().numpy(), row_c, row_x, B, mode == "video", cum, fin, ln, ext.numpy(), i, min_length=min_length,
                block_ngram_repeat=block_ngram_repeat, exclusion_tokens=exclusion_tokens, lp=lp, unk=unk, return_margin=True)
            pt = torch.as_tensor(parent)
            text, ext = text[pt].clone(), ext[pt].clone()
            text[:, i + 1] = torch.as_tensor(nx_mod)
            ext[:, i + 1] = torch.as_tensor(nx_ext)
        rows, gaps = [], []
        for s in range(S_b):
            order, keys = final_order(cum[s * B:(s + 1) * B], ln[s * B:(s + 1) * B], lp)
            rows.append([s * B + h for h in order])
            d = [keys[order[k]] - keys[order[k + 1]] for k in range(B - 1)]
            d = [v for v in d if np.isfinite(v)]
            margins[s, Lt - 1] = min(d) if d else np.inf
        rows = torch.as_tensor(np.array(rows, dtype=np.int64).reshape(S_b, B))
        out.append(ext[rows])
        out_cum.append(cum[rows.numpy()].astype(np.float32))
        out_len.append(ln[rows.numpy()])
        out_margins.append(margins)
    return out, out_cum, out_len, out_margins
