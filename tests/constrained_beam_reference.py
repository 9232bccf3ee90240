"""CPU restatement of lexically constrained beam search (Post & Vilar 2018, dynamic beam allocation; fairseq's unordered ``--constraints``;
svpc_amd.translator's ``translate_batch_constrained``), in the style of tests/diverse_beam_reference.py and built on the same oracle
functions.  ``select_cons`` is the selection rule the HIP kernel (svpc_beam_step_cons) must reproduce bit for bit, ``final_order_cons``
the order of svpc_beam_finalize_cons.  It shares no code with the product: the tracker, the banks and the allocation are restated here;
the allowed columns are those of ``beam_controls_reference.select_ctl`` and the step score is ``beam_reference.step_scores``.

A sentence has M ≤ 4 constraints, each a phrase (a tuple of 1 … 4 extended ids), unordered, duplicates met one after the other.  State
per row: met (one bit per constraint), cur (the phrase in progress, −1: none), off (its ids matched so far), packed as
met | (cur + 1) << 4 | off << 8; the start state is 0.  The tracker is not a string matcher: with phrase ``a a b`` the text ``a a a b``
does not complete it."""
import numpy as np
import torch

from beam_controls_reference import _key, banned_words
from beam_reference import step_scores
from diverse_beam_reference import length_table
from oracle import svpc_oracle as orc
from svpc_amd.synthetic import BOS, EOS, PAD, UNK

CONS_MAX, CONS_LEN = 4, 4


def pack(met, cur, off):
    return met | ((cur + 1) << 4) | (off << 8)


def unpack(state):
    state = int(state)
    return state & 15, ((state >> 4) & 7) - 1, (state >> 8) & 7


def track(state, c, phrases):
    """the state of the child that picks word ``c`` (a live pick from an unfinished parent)"""
    met, cur, off = unpack(state)
    if cur >= 0 and c == phrases[cur][off]:
        off += 1
        if off == len(phrases[cur]):
            met, cur, off = met | (1 << cur), -1, 0
    else:
        cur, off = -1, 0
        for j, ph in enumerate(phrases):
            if not (met >> j) & 1 and ph[0] == c:
                if len(ph) == 1:
                    met |= 1 << j
                else:
                    cur, off = j, 1
                break
    return pack(met, cur, off)


def bank(state, phrases):
    """n(state): the constraint tokens a hypothesis has banked"""
    met, _, off = unpack(state)
    return sum(len(ph) for j, ph in enumerate(phrases) if (met >> j) & 1) + off


def forced_columns(state, phrases):
    met, cur, off = unpack(state)
    if cur >= 0:
        return [phrases[cur][off]]
    return [ph[0] for j, ph in enumerate(phrases) if not (met >> j) & 1]


def table(cons):
    """the device form: (n_sent, 4, 4) int32, a phrase the leading ids of its row, the rest −1"""
    out = np.full((len(cons), CONS_MAX, CONS_LEN), -1, np.int32)
    for t, phrases in enumerate(cons):
        for j, ph in enumerate(phrases or ()):
            out[t, j, :len(ph)] = ph
    return out


def select_cons(scores, row_c, row_x, beam, logits, cum, cstate, finished, length, hist, pos, cons, min_length=0, block_ngram_repeat=0,
                exclusion_tokens=(), lp=None, unk=UNK, eos=EOS, pad=PAD, return_margin=False):
    """One selection step.  ``cons``: per sentence its list of phrases (None / empty: none).
    → parent (global rows), next extended ids, next model ids, new cum, new cstate, new finished, new length [, margin (T,): over the
    banks, the smallest key of a bank's last kept candidate minus the key of its first dropped one; +inf when no bank drops one]."""
    scores = np.asarray(scores, dtype=np.float32)
    cum = np.asarray(cum, dtype=np.float32)
    cstate = np.asarray(cstate).astype(np.int64)
    finished = np.asarray(finished).astype(bool)
    length = np.asarray(length).astype(np.int64)
    excl = set(int(e) for e in exclusion_tokens)
    R = scores.shape[0]
    W = beam
    T = R // W
    p = pos + 1
    parent = np.zeros(R, np.int64)
    ext = np.zeros(R, np.int64)
    mod = np.zeros(R, np.int64)
    cum_new = np.zeros(R, np.float32)
    st_new = np.zeros(R, np.int64)
    fin_new = np.zeros(R, bool)
    len_new = np.zeros(R, np.int64)
    margin = np.full(T, np.inf)
    for t in range(T):
        phrases = [tuple(int(w) for w in ph) for ph in (cons[t] or ())]
        full = (1 << len(phrases)) - 1
        cands = []                                  # (key, raw, flat, h, col, was_fin, cum', state')
        for h in range(W):
            r = t * W + h
            C = int(row_c[r])
            if finished[r]:
                cands.append((_key(cum[r], length[r], lp), np.float32(np.inf), h * C + pad, h, pad, True, np.float32(cum[r]), int(cstate[r])))
                continue
            met = unpack(cstate[r])[0]
            ban = banned_words(hist[r], pos, block_ngram_repeat, excl)
            allowed = [c for c in range(C) if c != unk and c not in ban and not (c == eos and (p <= min_length or met != full))]
            st = step_scores(scores[r, :C], logits, unk)
            with np.errstate(invalid="ignore"):
                cu = (np.float32(cum[r]) + st).astype(np.float32)
            top = sorted(allowed, key=lambda c: (-float(scores[r, c]), c))[:W]
            aset = set(allowed)
            forced = [c for c in forced_columns(cstate[r], phrases) if c in aset and cu[c] > -np.inf]
            for c in sorted(set(top) | set(forced)):
                cands.append((_key(cu[c], p, lp), scores[r, c], h * C + c, h, c, False, cu[c], track(cstate[r], c, phrases)))
        today = lambda e: (-e[0], -float(e[1]), e[2])
        live = [e for e in cands if np.isfinite(e[6])]
        dead = sorted((e for e in cands if not np.isfinite(e[6])), key=today)
        banks = {}
        for e in live:
            banks.setdefault(bank(e[7], phrases), []).append(e)
        order = []
        for n, lst in banks.items():
            lst.sort(key=today)
            order += [(k, -n, e) for k, e in enumerate(lst)]
        order.sort(key=lambda v: v[:2])
        kept = {}
        for k, n, e in order[:W]:
            kept[-n] = k + 1
        for n, lst in banks.items():                # every bank's kept / dropped boundary
            k = kept.get(n, 0)
            if 0 < k < len(lst):
                margin[t] = min(margin[t], lst[k - 1][0] - lst[k][0])
        order = [e for _, _, e in order] + dead
        for k in range(W):
            r = t * W + k
            if k < len(order):
                _, _, _, h, col, was_fin, cu, state = order[k]
                ln = length[t * W + h] if was_fin else p
            else:
                h, col, was_fin, cu, state, ln = k, pad, True, np.float32(-np.inf), 0, p
            C, X = int(row_c[t * W + h]), int(row_x[t * W + h])
            parent[r] = t * W + h
            ext[r] = pad if was_fin else col
            mod[r] = pad if was_fin else (unk if col >= C - X else col)
            cum_new[r], st_new[r] = cu, state
            fin_new[r] = was_fin or ext[r] == eos
            len_new[r] = ln
    out = (parent, ext, mod, cum_new, st_new, fin_new, len_new)
    return out + (margin,) if return_margin else out


def popcount(state):
    return bin(int(state) & 15).count("1")


def final_order_cons(cum, length, cstate, lp):
    """indices of one sentence's W final hypotheses: rows with cum = −inf last (by index); above them more constraints met first, then
    the higher final key, then the lower index → (order, keys)"""
    keys = [_key(c, ln, lp) for c, ln in zip(cum, length)]
    dead = [bool(np.isneginf(np.float32(c))) for c in cum]
    return sorted(range(len(keys)), key=lambda h: (1, 0, 0.0, h) if dead[h] else (0, -popcount(cstate[h]), -keys[h], h)), keys


def contains(ids, phrase):
    """a plain search: ``phrase`` as a contiguous run of ``ids``"""
    ids, phrase = [int(v) for v in ids], [int(v) for v in phrase]
    return any(ids[i:i + len(phrase)] == phrase for i in range(len(ids) - len(phrase) + 1))


def constrained_decode(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                       ingr_id_dict, oov_word_dict, beam, constraints, min_length=0, block_ngram_repeat=0, exclusion_tokens=(),
                       length_penalty_name="none", length_penalty_alpha=0.0, bos=BOS, unk=UNK):
    """``constraints``: per video a list of S_b lists of phrases.  → (ids, cums, lens, mets, margins): per video all W final hypotheses in
    the final order — ids (S_b, W, Lt) int64, cum (S_b, W) float32, len (S_b, W) int64, met (S_b, W) int64 — and margins (S_b, Lt): the
    selection margins of the Lt − 1 steps (``select_cons``) and, last, the smallest finite gap between the final keys of consecutive rows
    of equal popcount."""
    mode, Lv, Lt = cfg.model_mode, cfg.max_v_len, cfg.max_t_len
    V = cfg.vocab_size
    W = beam
    lp = length_table(length_penalty_name, length_penalty_alpha, Lt)
    ingr_input_ids = torch.as_tensor(ingr_input_ids)
    ingr_sep_masks = torch.as_tensor(ingr_sep_masks)
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    out, out_cum, out_len, out_met, out_margins = [], [], [], [], []
    for b, S_b in enumerate(batch_step_num):
        ids = torch.stack([input_ids_list[s][b] for s in range(S_b)]).clone()
        masks = torch.stack([input_masks_list[s][b] for s in range(S_b)]).clone()
        feats = torch.stack([video_features_list[s][b] for s in range(S_b)])
        ids[:, Lv:] = 0; masks[:, Lv:] = 0
        ingr = orc.ingredient_embed(P, ingr_input_ids[b:b + 1], ingr_sep_masks[b:b + 1], cfg)[0]
        enc = orc.forward_step(P, ids, feats, masks, cfg)
        g_ = orc.encoder(P, "step_wise_encoder", (enc[:, 0] + pe50[:S_b]).unsqueeze(0), torch.ones(1, S_b), cfg)[0]
        n_oov = len(oov_word_dict[b]) if mode != "video" else 0
        bank_ = None
        if mode in ("full", "reason_copy"):
            _, _, bar_e, all_e, bar_f = orc.simulator(P, "reasoner", g_, ingr)
            mem = torch.stack([g_, torch.relu(orc.linear(P, "Went.0", bar_e)), torch.relu(orc.linear(P, "Wac.0", bar_f))], 1)
            bank_ = all_e
        elif mode == "copy":
            mem = torch.stack([g_, ingr.mean(0).unsqueeze(0).expand(S_b, -1)], 1)
            bank_ = ingr.unsqueeze(0).expand(S_b, -1, -1)
        else:
            mem = g_.unsqueeze(1)
        mem = mem.repeat_interleave(W, 0)
        bank_ = bank_.repeat_interleave(W, 0) if bank_ is not None else None
        R = S_b * W
        C = V + n_oov
        row_c, row_x = np.full(R, C), np.full(R, n_oov)
        text = torch.full((R, Lt), PAD, dtype=torch.long); text[:, 0] = bos
        ext = text.clone()
        cum = np.zeros((S_b, W), np.float32); cum[:, 1:] = -np.inf
        cum = cum.reshape(-1)
        state = np.zeros(R, np.int64)
        fin = np.zeros(R, bool)
        ln = np.zeros(R, np.int64)
        margins = np.full((S_b, Lt), np.inf)
        cons = [list(c or ()) for c in constraints[b]]
        for i in range(Lt - 1):
            dec = orc.decoder(P, orc.text_embed(P, text[:, :i + 1], cfg), torch.ones(R, i + 1), mem, torch.ones(mem.shape[:2]), cfg)
            last = dec[:, i:i + 1]
            if mode == "video":
                sc = orc.lm_head(P, last, cfg)[:, 0]
            else:
                sc = orc.pointer_generator(P, last, bank_, ingr_id_dict[b], n_oov, cfg)[:, 0]
            parent, nx_ext, nx_mod, cum, state, fin, ln, margins[:, i] = select_cons(
                sc.detach().numpy(), row_c, row_x, W, mode == "video", cum, state, fin, ln, ext.numpy(), i, cons, min_length=min_length,
                block_ngram_repeat=block_ngram_repeat, exclusion_tokens=exclusion_tokens, lp=lp, unk=unk, return_margin=True)
            pt = torch.as_tensor(parent)
            text, ext = text[pt].clone(), ext[pt].clone()
            text[:, i + 1] = torch.as_tensor(nx_mod)
            ext[:, i + 1] = torch.as_tensor(nx_ext)
        rows = []
        for s in range(S_b):
            lo = s * W
            order, keys = final_order_cons(cum[lo:lo + W], ln[lo:lo + W], state[lo:lo + W], lp)
            rows.append([lo + h for h in order])
            gaps = [keys[order[k]] - keys[order[k + 1]] for k in range(W - 1)
                    if popcount(state[lo + order[k]]) == popcount(state[lo + order[k + 1]])]
            gaps = [v for v in gaps if np.isfinite(v)]
            margins[s, Lt - 1] = min(gaps) if gaps else np.inf
        rows = np.array(rows, dtype=np.int64).reshape(S_b, W)
        out.append(ext[torch.as_tensor(rows)])
        out_cum.append(cum[rows].astype(np.float32))
        out_len.append(ln[rows])
        out_met.append(state[rows] & 15)
        out_margins.append(margins)
    return out, out_cum, out_len, out_met, out_margins
