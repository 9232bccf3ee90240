"""CPU restatement of forced decoding (``Translator.score_captions``): the decoder's scores of captions it is handed.
Shares no code with the product; ``forced_decode`` is built on the oracle's decoder blocks the way ``beam_reference.beam_decode`` is.

The definition.  A caption row is Lt extended ids y_0 … y_{Lt−1}, y_0 = BOS; its score row i (i = 0 … Lt − 2) scores position p = i + 1
with target w = y_p while the row is live; C columns (V + X of its video, X = 0 in ``video`` mode):

- w == EOS: its step score is added, the row is finished, len = p;
- w == PAD or w == IGNORE: the row ends unfinished, len = p − 1, nothing is added and nothing after it is looked at;
- otherwise the step score of column w is added; a row that never ends has len = Lt − 1.

The step score is the decoder's (``beam_reference.step_scores``: fp64, rounded once to fp32; log p, −inf for p ≤ 0; or logit − the
log-sum-exp of the row's columns without UNK).  A target that is no candidate (w == UNK, w < 0, w ≥ C) scores −inf (``unk="bar"``) or
contributes 0 and is not counted in n_scored (``"skip"``).  cum = fp32(cum + s) in position order.  rank: the candidate columns (c < C,
c ≠ UNK) that precede w in the decoder's order (higher raw value, then lower column), −1 for a non-candidate and past the end; top /
top_step: the first candidate and its step score; past the end step 0, rank −1, top −1, top_step 0."""
import numpy as np
import torch

from oracle import svpc_oracle as orc
from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD, UNK


def step_scores(row, logits, unk=UNK):
    """float32 step scores of every column of one score row (restated from the definition: fp64, one rounding)"""
    r = np.asarray(row, np.float32).astype(np.float64)
    if logits:
        keep = np.arange(r.shape[0]) != unk
        m = r[keep].max()
        return (r - (m + np.log(np.exp(r[keep] - m).sum()))).astype(np.float32)
    out = np.full(r.shape[0], -np.inf)
    pos = r > 0
    out[pos] = np.log(r[pos])
    return out.astype(np.float32)


def score_caption(rows, y, C, logits, unk_rule="bar", unk=UNK, eos=EOS, pad=PAD, ignore=IGNORE, with_gap=False):
    """One caption: ``rows`` (≥ Lt − 1, ≥ C) float32 score rows (row i scores position i + 1), ``y`` its Lt ids → a dict: cum (float32), len,
    n_scored, finished, and (Lt − 1,) step, rank, top, top_step [, gap: the distance in step score from the target to its nearer
    neighbour in the decoder's order, +inf where there is none or the position is not ranked]."""
    assert unk_rule in ("bar", "skip")
    y = [int(v) for v in y]
    Lt = len(y)
    step = np.zeros(Lt - 1, np.float32)
    top_step = np.zeros(Lt - 1, np.float32)
    rank = np.full(Lt - 1, -1, np.int32)
    top = np.full(Lt - 1, -1, np.int32)
    gap = np.full(Lt - 1, np.inf)
    cum = np.float32(0.0)
    length, n_scored, finished = Lt - 1, 0, 0
    for i in range(Lt - 1):
        p, w = i + 1, y[i + 1]
        if w == pad or w == ignore:
            length = p - 1
            break
        raw = np.asarray(rows[i][:C], np.float32)
        st = step_scores(raw, logits, unk)
        cols = np.array([c for c in range(C) if c != unk], np.int64)
        order = cols[np.lexsort((cols, -raw[cols].astype(np.float64)))] if len(cols) else cols     # higher raw value, then lower column
        if len(order):
            top[i], top_step[i] = order[0], st[order[0]]
        else:
            top_step[i] = -np.inf
        if 0 <= w < C and w != unk:
            k = int(np.nonzero(order == w)[0][0])
            rank[i] = k
            step[i] = st[w]
            n_scored += 1
            if with_gap:
                with np.errstate(invalid="ignore"):
                    near = [abs(float(st[order[j]]) - float(st[w])) for j in (k - 1, k + 1) if 0 <= j < len(order)]
                gap[i] = min([g for g in near if not np.isnan(g)] + [np.inf])
        elif unk_rule == "bar":
            step[i] = -np.inf
            n_scored += 1
        cum = np.float32(cum + step[i])
        if w == eos:
            length, finished = p, 1
            break
    out = dict(cum=cum, len=length, n_scored=n_scored, finished=finished, step=step, rank=rank, top=top, top_step=top_step)
    if with_gap:
        out["gap"] = gap
    return out


def score_rows(scores, ids, row_c, logits, unk_rule="bar", with_gap=False):
    """``scores`` (R·Lt, ≥ C) float32 — row r·Lt + i is step i of caption r —, ``ids`` (R, Lt), ``row_c`` (R,) → stacked results: cum (R,)
    float32, len / n_scored / finished (R,) int32, step / rank / top / top_step (R, Lt − 1) [, gap]."""
    ids = np.asarray(ids)
    R, Lt = ids.shape
    res = [score_caption(scores[r * Lt:(r + 1) * Lt], ids[r], int(row_c[r]), logits, unk_rule, with_gap=with_gap) for r in range(R)]
    out = {k: np.stack([np.asarray(x[k]) for x in res]) for k in res[0]}
    for k in ("len", "n_scored", "finished"):
        out[k] = out[k].astype(np.int32)
    return out


def model_side(y, V, unk=UNK, pad=PAD):
    """the ids the decoder is fed: a copied word (or anything outside the text vocabulary) is UNK"""
    y = torch.as_tensor(np.asarray(y)).long()
    return torch.where((y >= 0) & (y < V), y, torch.full_like(y, unk))


def forced_decode(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                  ingr_id_dict, oov_word_dict, captions, unk_rule="bar", with_gap=True):
    """``captions``: per video (S_b, K, Lt) or (S_b, Lt) ids → per video a dict of (S_b, K, …) arrays (``score_rows``'s fields).  The
    encoder side is ``beam_reference.beam_decode``'s (text half blanked); the decoder runs once over the Lt positions of every caption
    under its causal mask, so position i sees positions 0 … i of the caption."""
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
        dec = orc.decoder(P, orc.text_embed(P, model_side(y, V), cfg), torch.ones(R, Lt), mem, torch.ones(mem.shape[:2]), cfg)
        if mode == "video":
            sc = orc.lm_head(P, dec, cfg)
        else:
            sc = orc.pointer_generator(P, dec, bank, ingr_id_dict[b], n_oov, cfg)
        sc = sc.detach().numpy().astype(np.float32).reshape(R * Lt, -1)
        r = score_rows(sc, y, np.full(R, C), mode == "video", unk_rule, with_gap=with_gap)
        out.append({k: v.reshape((S_b, K) + v.shape[1:]) for k, v in r.items()})
    return out


def gold_rows(labels_list, batch_step_num, Lv, Lt):
    """the fixture's reference captions per video (S_b, Lt): BOS, then the labels of text positions 0 … Lt − 2, IGNORE → PAD"""
    out = []
    for b, S_b in enumerate(batch_step_num):
        rows = np.full((S_b, Lt), PAD, np.int64)
        rows[:, 0] = BOS
        for s in range(S_b):
            lab = np.asarray(labels_list[s][b])[Lv:Lv + Lt - 1]
            rows[s, 1:] = np.where(lab == IGNORE, PAD, lab)
        out.append(rows)
    return out
