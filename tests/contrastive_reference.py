"""CPU restatement of contrastive search (Su et al. 2022; svpc_amd.translator's ``translate_batch_contrastive``), built on the oracle's
own functions and shaped like ``beam_reference.beam_decode``.  ``select`` is the rule the HIP kernel (svpc_contrastive_step) must
reproduce; ``contrastive_decode`` re-runs the oracle's decoder over k candidate rows per sentence for Lt iterations.

Per sentence: k candidate rows, each carrying one word for position i with p (the model's probability of it) and s (its step score,
``beam_reference.step_scores``).  After the decoder pass, h_r is row r's last-layer output:
  penalty_r = max_{j < i} cos(h_r, H[j]) (0 at i = 0; cos = dot / (sqrt(|a|²)·sqrt(|b|²)), 0 when a norm is 0; fp64);
  score_r   = (1 − α)·p_r − α·penalty_r;  the winner is the live (p > 0) row with the highest score, ties to the lowest row;
  commit ids[i], cum += s (fp32), len = i, pen[i], H[i] = h_winner (and its squared norm); EOS finishes;
  expansion (i + 1 < Lt, not finished): the top k columns of the winner's score row by (higher raw value, lower column), UNK excluded, EOS
  excluded while i + 1 ≤ min_length, nothing renormalised; p = raw (≤ 0: 0) or, in logits mode, fp32(exp(raw − lse)); p = 0: dead (PAD).
A finished sentence writes PAD children; a sentence without a live row finishes with PAD and cum = −inf.

Dot products and squared norms are summed in the kernel's order (``wave_dot``: 64 partial sums over the elements lane, lane + 64, …, then
a butterfly over lane distances 32 … 1), so a stored squared norm is the kernel's bit for bit; the product of two fp32 is exact in fp64."""
import functools

import numpy as np
import torch

import beam_reference as br
from oracle import svpc_oracle as orc
from svpc_amd.synthetic import BOS, EOS, PAD, UNK

_LANES = np.arange(64)


def wave_dot(x, y):
    """Σ x·y in float64 in the kernel's fixed order"""
    p = np.asarray(x, np.float32).astype(np.float64) * np.asarray(y, np.float32).astype(np.float64)
    n = p.shape[0]
    if n % 64:
        p = np.concatenate([p, np.zeros(64 - n % 64)])
    s = np.zeros(64)
    for row in p.reshape(-1, 64):
        s = s + row
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[_LANES ^ o]
    return float(s[0])


def cosine(dot, n2a, n2b):
    return dot / (np.sqrt(n2a) * np.sqrt(n2b)) if n2a > 0.0 and n2b > 0.0 else 0.0


def new_state(T, k, lt, D, pad=PAD):
    """the state before iteration 0: row 0 of every sentence alone live (p 1, step score 0)"""
    cand_p = np.zeros((T, k), np.float32); cand_p[:, 0] = 1.0
    cand_s = np.full((T, k), -np.inf, np.float32); cand_s[:, 0] = 0.0
    return dict(cand_p=cand_p.reshape(-1), cand_s=cand_s.reshape(-1), ids=np.full((T, lt), pad, np.int64), cum=np.zeros(T, np.float32),
                len=np.zeros(T, np.int64), pen=np.zeros((T, lt), np.float32), fin=np.zeros(T, bool), H=np.zeros((T, lt, D), np.float32),
                Hn=np.zeros((T, lt), np.float64))


def select(scores, row_c, row_x, k, logits, pos, hidden, cand_ext, st, alpha, min_length=0, unk=UNK, eos=EOS, pad=PAD):
    """One step at position ``pos`` for all T sentences.  ``scores`` (T·k, ≥ C) float32 (None at the last position), ``hidden`` (T·k, D)
    float32, ``cand_ext`` (T·k,) the extended id every row carries at ``pos``, ``st`` the state (``new_state``; not modified), ``alpha``
    a float.  → (the new state, dict(winner (T,) — −1: none —, pen_all (T·k,) float64 every row's penalty, score_all (T·k,) float64 (nan: a
    dead row), parent / ext / mod (T·k,) the children (None without expansion), margin_sel (T,): best minus second-best score, +inf with
    fewer than two live rows, margin_top (T,): log p of the k-th minus the (k + 1)-th column of the winner's row, +inf when there is no
    (k + 1)-th candidate of positive probability or no expansion))."""
    hidden = np.asarray(hidden, np.float32)
    R, D = hidden.shape
    T = R // k
    lt = st["ids"].shape[1]
    st = {n: v.copy() for n, v in st.items()}
    old_p, old_s = st["cand_p"].copy(), st["cand_s"].copy()
    expand = pos + 1 < lt
    alpha = float(alpha)
    winner = np.full(T, -1, np.int64)
    pen_all, score_all = np.zeros(R), np.full(R, np.nan)
    parent = np.zeros(R, np.int64); ext = np.full(R, pad, np.int64); mod = np.full(R, pad, np.int64)
    m_sel, m_top = np.full(T, np.inf), np.full(T, np.inf)
    for t in range(T):
        r0 = t * k
        parent[r0:r0 + k] = r0
        if expand:
            st["cand_p"][r0:r0 + k] = 0.0
            st["cand_s"][r0:r0 + k] = -np.inf
        if st["fin"][t]:
            continue
        live = [h for h in range(k) if old_p[r0 + h] > 0]
        if not live:
            st["ids"][t, pos] = pad; st["cum"][t] = -np.inf; st["fin"][t] = True
            continue
        n2 = {}
        for h in live:
            n2[h] = wave_dot(hidden[r0 + h], hidden[r0 + h])
            pn = 0.0
            if pos > 0:
                pn = max(cosine(wave_dot(hidden[r0 + h], st["H"][t, j]), n2[h], st["Hn"][t, j]) for j in range(pos))
            pen_all[r0 + h] = pn
            score_all[r0 + h] = (1.0 - alpha) * float(old_p[r0 + h]) - alpha * pn
        order = sorted(live, key=lambda h: (-score_all[r0 + h], h))
        w = order[0]
        if len(order) > 1:
            m_sel[t] = score_all[r0 + w] - score_all[r0 + order[1]]
        winner[t] = w
        wid = int(cand_ext[r0 + w])
        st["ids"][t, pos] = wid
        st["cum"][t] = np.float32(st["cum"][t]) + np.float32(old_s[r0 + w])
        st["len"][t] = pos
        st["pen"][t, pos] = np.float32(pen_all[r0 + w])
        st["H"][t, pos] = hidden[r0 + w]
        st["Hn"][t, pos] = n2[w]
        st["fin"][t] = wid == eos
        r = r0 + w
        parent[r0:r0 + k] = r                          # (the PAD children of a sentence that finishes now descend from the winner too)
        if not expand or st["fin"][t]:
            continue
        C, X = int(row_c[r]), int(row_x[r])
        row = np.asarray(scores[r, :C], np.float32)
        cols = np.array([c for c in range(C) if c != unk and not (c == eos and pos + 1 <= min_length)], dtype=np.int64)
        cols = cols[np.lexsort((cols, -row[cols].astype(np.float64)))]
        step = br.step_scores(row, logits, unk)
        r64 = row.astype(np.float64)
        if logits:
            keep = np.arange(C) != unk
            mx = r64[keep].max()
            lse = mx + np.log(np.exp(r64[keep] - mx).sum())
            with np.errstate(under="ignore"):
                p = np.exp(r64 - lse).astype(np.float32)
            logp = r64 - lse
        else:
            p = np.where(row > 0, row, np.float32(0.0)).astype(np.float32)
            with np.errstate(divide="ignore"):
                logp = np.where(r64 > 0, np.log(np.where(r64 > 0, r64, 1.0)), -np.inf)
        for h, c in enumerate(cols[:k]):
            if not p[c] > 0:
                continue
            ext[r0 + h] = c
            mod[r0 + h] = unk if c >= C - X else c
            st["cand_p"][r0 + h] = p[c]
            st["cand_s"][r0 + h] = step[c]
        if len(cols) > k and p[cols[k]] > 0:
            m_top[t] = logp[cols[k - 1]] - logp[cols[k]]
    out = dict(winner=winner, pen_all=pen_all, score_all=score_all, parent=parent if expand else None, ext=ext if expand else None,
               mod=mod if expand else None, margin_sel=m_sel, margin_top=m_top)
    return st, out


def contrastive_decode(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                       ingr_id_dict, oov_word_dict, top_k, alpha, min_length=0, bos=BOS, unk=UNK):
    """→ (ids, cum, len, pen, margin_sel, margin_top): per video (S_b, Lt) int64 ids (BOS first, PAD after EOS), (S_b,) float32 cum, (S_b,)
    int64 len, (S_b, Lt) float32 pen, and the (S_b, Lt) margin tables of every step (see ``select``).  ``alpha`` is used as given: pass
    the fp32-rounded value the product holds."""
    mode, Lv, Lt = cfg.model_mode, cfg.max_v_len, cfg.max_t_len
    V, D = cfg.vocab_size, cfg.hidden_size
    k = top_k
    ingr_input_ids = torch.as_tensor(ingr_input_ids)
    ingr_sep_masks = torch.as_tensor(ingr_sep_masks)
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    outs = [[] for _ in range(6)]
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
        mem = mem.repeat_interleave(k, 0)                                              # candidate rows s·k + h
        bank = bank.repeat_interleave(k, 0) if bank is not None else None
        R = S_b * k
        C = V + n_oov
        row_c, row_x = np.full(R, C), np.full(R, n_oov)
        text = torch.full((R, Lt), PAD, dtype=torch.long); text[:, 0] = bos
        ext = text.clone()
        st = new_state(S_b, k, Lt, D)
        m_sel, m_top = np.full((S_b, Lt), np.inf), np.full((S_b, Lt), np.inf)
        for i in range(Lt):
            # causal decoder: position i depends on positions 0 … i only
            dec = orc.decoder(P, orc.text_embed(P, text[:, :i + 1], cfg), torch.ones(R, i + 1), mem, torch.ones(mem.shape[:2]), cfg)
            last = dec[:, i:i + 1]
            sc = None
            if i + 1 < Lt:
                sc = (orc.lm_head(P, last, cfg) if mode == "video" else
                      orc.pointer_generator(P, last, bank, ingr_id_dict[b], n_oov, cfg))[:, 0].detach().numpy()
            st, o = select(sc, row_c, row_x, k, mode == "video", i, dec[:, i].detach().numpy(), ext[:, i].numpy(), st, alpha, min_length,
                           unk=unk)
            m_sel[:, i], m_top[:, i] = o["margin_sel"], o["margin_top"]
            if o["parent"] is not None:
                pt = torch.as_tensor(o["parent"])
                text, ext = text[pt].clone(), ext[pt].clone()
                text[:, i + 1] = torch.as_tensor(o["mod"])
                ext[:, i + 1] = torch.as_tensor(o["ext"])
        for lst, v in zip(outs, (torch.from_numpy(st["ids"]), st["cum"], st["len"], st["pen"], m_sel, m_top)):
            lst.append(v)
    return tuple(outs)


@functools.lru_cache(maxsize=None)
def decode_case(golden_dir, case, mt, top_k, alpha, min_length=0):
    """``contrastive_decode`` of a golden fixture, computed once per process and shared by the tests that need it (treat as read-only)"""
    from test_oracle_golden import load_case
    _, cfg, batch, P = load_case(golden_dir, case, mt)
    P = {n: v.detach() for n, v in P.items()}
    return contrastive_decode(P, cfg, batch["input_ids_list"], batch["video_features_list"], batch["input_masks_list"], batch["ingr_input_ids"],
                              batch["ingr_sep_masks"], batch["batch_step_num"], batch["ingr_id_dict"], batch["oov_word_dict"], top_k,
                              float(np.float32(alpha)), min_length)
