"""CPU restatement of ensemble decoding (svpc_amd/ensemble.py, svpc_ensemble_combine; OpenNMT's ``EnsembleModel`` / ``avg_raw_probs``):
``combine`` is the rule the HIP kernel must reproduce, and ``ensemble_greedy`` / ``ensemble_beam_decode`` / ``ensemble_sample_decode`` are
per-video oracle decodes over a list of parameter dicts, built like ``beam_reference.beam_decode``: one encoder side per member, one
decoder re-run per member and step, ``combine``, then the single-model selection rules with ``logits=False``.

The rule.  M members (1 … 8), fp64 weights w_m ≥ 0 normalised to sum 1 (default uniform; a member with w_m = 0 is skipped entirely), one
fp32 score matrix per member with the same rows; row r has C = row_c[r // rows_per] columns.  Member probability, fp64, c < C:
probability mode ``raw > 0 ? raw : 0``; logits mode ``exp(raw − lse_m)``, lse_m = max + log Σ exp(raw − max) over c < C, c ≠ UNK,
p_{m,UNK} = 0, and a member row without a finite non-UNK logit contributes 0 everywhere.  ``"prob"``: out_c = fp32(Σ_m w_m·p_{m,c}), terms
in ascending m, every product and every sum rounded (no FMA).  ``"logprob"``: out_c = fp32(exp(Σ_m w_m·log p_{m,c})), 0 as soon as a counted
member has p = 0, not renormalised; in logits mode log p is taken as raw − lse_m itself (the same quantity without the exp / log round
trip).  Columns ≥ C are 0.  The output is a probability matrix in both modes."""
import numpy as np
import torch

from beam_reference import select
from oracle import svpc_oracle as orc
from sampling_reference import model_ids, sample_select
from svpc_amd.synthetic import BOS, PAD, UNK

RULES = ("prob", "logprob")


def normalise(weights, n):
    w = np.ones(n, np.float64) if weights is None else np.asarray(weights, dtype=np.float64)
    assert w.shape == (n,) and np.all(np.isfinite(w)) and np.all(w >= 0)
    total = 0.0
    for v in w:
        total += float(v)
    assert total > 0
    return np.array([float(v) / total for v in w], np.float64)


def combine(mats, row_c, weights=None, rule="prob", logits=False, unk=UNK, rows_per=1, ld_out=None):
    """mats: M float32 (n_rows, ≥ C) arrays → out (n_rows, ld_out) float32 (ld_out defaults to max C)"""
    assert rule in RULES and 1 <= len(mats) <= 8
    mats = [np.asarray(m, dtype=np.float32) for m in mats]
    n_rows = mats[0].shape[0]
    w = normalise(weights, len(mats))
    row_c = [int(c) for c in row_c]
    ld_out = max(row_c) if ld_out is None else ld_out
    out = np.zeros((n_rows, ld_out), np.float32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        for r in range(n_rows):
            C = row_c[r // rows_per]
            acc = np.zeros(C, np.float64)
            for m, mat in enumerate(mats):
                if w[m] == 0.0:
                    continue
                raw = mat[r, :C].astype(np.float64)
                if logits:
                    keep = np.ones(C, bool)
                    if 0 <= unk < C:
                        keep[unk] = False
                    finite = keep & np.isfinite(raw)
                    if finite.any():
                        mx = raw[keep].max()
                        lse = mx + np.log(np.exp(raw[keep] - mx).sum())
                        logp = np.where(keep, raw - lse, -np.inf)
                    else:
                        logp = np.full(C, -np.inf)
                    term = np.exp(logp) if rule == "prob" else logp
                else:
                    p = np.where(raw > 0, raw, 0.0)
                    term = p if rule == "prob" else np.where(p > 0, np.log(np.where(p > 0, p, 1.0)), -np.inf)
                acc = acc + w[m] * term                      # (numpy: one rounded product, one rounded sum)
            out[r, :C] = (acc if rule == "prob" else np.exp(acc)).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ the decodes
def _video_sides(Ps, cfg, b, S_b, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, oov_word_dict,
                 width):
    """every member's (mem, bank) of video b over its S_b·width hypothesis rows, and the video's OOV count"""
    mode, Lv = cfg.model_mode, cfg.max_v_len
    ids = torch.stack([input_ids_list[s][b] for s in range(S_b)]).clone()
    masks = torch.stack([input_masks_list[s][b] for s in range(S_b)]).clone()
    feats = torch.stack([video_features_list[s][b] for s in range(S_b)])
    ids[:, Lv:] = 0; masks[:, Lv:] = 0
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    n_oov = len(oov_word_dict[b]) if mode != "video" else 0
    sides = []
    for P in Ps:
        ingr = orc.ingredient_embed(P, ingr_input_ids[b:b + 1], ingr_sep_masks[b:b + 1], cfg)[0]
        enc = orc.forward_step(P, ids, feats, masks, cfg)
        g = orc.encoder(P, "step_wise_encoder", (enc[:, 0] + pe50[:S_b]).unsqueeze(0), torch.ones(1, S_b), cfg)[0]
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
        sides.append((mem.repeat_interleave(width, 0), bank.repeat_interleave(width, 0) if bank is not None else None))
    return sides, n_oov


def _step_scores(Ps, cfg, sides, text, i, ingr_dict, n_oov, row_c, weights, rule):
    """the combined (R, C) probability matrix of decoding step i: every member's decoder over positions 0 … i, its head, ``combine``"""
    mode = cfg.model_mode
    R = text.shape[0]
    mats = []
    for P, (mem, bank) in zip(Ps, sides):
        dec = orc.decoder(P, orc.text_embed(P, text[:, :i + 1], cfg), torch.ones(R, i + 1), mem, torch.ones(mem.shape[:2]), cfg)
        last = dec[:, i:i + 1]
        sc = orc.lm_head(P, last, cfg)[:, 0] if mode == "video" else orc.pointer_generator(P, last, bank, ingr_dict, n_oov, cfg)[:, 0]
        mats.append(sc.detach().numpy())
    return combine(mats, row_c, weights, rule, logits=mode == "video")


def _args(ingr_input_ids, ingr_sep_masks):
    return torch.as_tensor(ingr_input_ids), torch.as_tensor(ingr_sep_masks)


def ensemble_beam_decode(Ps, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                         ingr_id_dict, oov_word_dict, beam, weights=None, rule="prob"):
    """``beam_reference.beam_decode`` over the members ``Ps`` → (ids, scores, margins), as it returns them"""
    ingr_input_ids, ingr_sep_masks = _args(ingr_input_ids, ingr_sep_masks)
    Lt, V, B = cfg.max_t_len, cfg.vocab_size, beam
    out, out_scores, out_margins = [], [], []
    for b, S_b in enumerate(batch_step_num):
        sides, n_oov = _video_sides(Ps, cfg, b, S_b, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks,
                                    oov_word_dict, B)
        R, C = S_b * B, V + n_oov
        row_c, row_x = np.full(R, C), np.full(R, n_oov)
        text = torch.full((R, Lt), PAD, dtype=torch.long); text[:, 0] = BOS
        ext = text.clone()
        cum = np.zeros((S_b, B), np.float32); cum[:, 1:] = -np.inf
        cum = cum.reshape(-1)
        fin = np.zeros(R, bool)
        margins = np.zeros((S_b, max(Lt - 1, 0)))
        for i in range(Lt - 1):
            sc = _step_scores(Ps, cfg, sides, text, i, ingr_id_dict[b], n_oov, row_c, weights, rule)
            parent, nx_ext, nx_mod, cum, fin, margins[:, i] = select(sc, row_c, row_x, B, False, cum, fin, return_margin=True)
            pt = torch.as_tensor(parent)
            text, ext = text[pt].clone(), ext[pt].clone()
            text[:, i + 1] = torch.as_tensor(nx_mod)
            ext[:, i + 1] = torch.as_tensor(nx_ext)
        best = np.array([int(np.argmax(cum[s * B:(s + 1) * B])) for s in range(S_b)], dtype=np.int64)
        rows = np.arange(S_b) * B + best
        out.append(ext[torch.as_tensor(rows)])
        out_scores.append(cum[rows].astype(np.float32))
        out_margins.append(margins)
    return out, out_scores, out_margins


def ensemble_sample_decode(Ps, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                           ingr_id_dict, oov_word_dict, num_samples, seed, weights=None, rule="prob", temp=1.0, topk=0, topp=0.0,
                           min_length=0):
    """``sampling_reference.sample_decode`` over the members ``Ps`` → (ids, cums, lens, margins), as it returns them"""
    ingr_input_ids, ingr_sep_masks = _args(ingr_input_ids, ingr_sep_masks)
    Lt, V, Rs = cfg.max_t_len, cfg.vocab_size, num_samples
    out, out_cum, out_len, out_margins = [], [], [], []
    t0 = 0
    for b, S_b in enumerate(batch_step_num):
        sides, n_oov = _video_sides(Ps, cfg, b, S_b, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks,
                                    oov_word_dict, Rs)
        R, C = S_b * Rs, V + n_oov
        row_c, row_x = np.full(R, C), np.full(R, n_oov)
        text = torch.full((R, Lt), PAD, dtype=torch.long); text[:, 0] = BOS
        ext = text.clone()
        cum, fin, ln = np.zeros(R, np.float32), np.zeros(R, bool), np.zeros(R, np.int64)
        margins = np.full(R, np.inf)
        for i in range(Lt - 1):
            sc = _step_scores(Ps, cfg, sides, text, i, ingr_id_dict[b], n_oov, row_c, weights, rule)
            before = fin.copy()
            picks, cum, fin, ln, mg = sample_select(sc, row_c, row_x, i, False, cum, fin, ln, seed, temp, topk, topp, min_length,
                                                    row0=t0 * Rs)
            margins = np.minimum(margins, mg.min(1))
            text[:, i + 1] = torch.as_tensor(model_ids(picks, before, row_c, row_x))
            ext[:, i + 1] = torch.as_tensor(picks)
        out.append(ext.view(S_b, Rs, Lt))
        out_cum.append(cum.reshape(S_b, Rs))
        out_len.append(ln.reshape(S_b, Rs))
        out_margins.append(margins.reshape(S_b, Rs))
        t0 += S_b
    return out, out_cum, out_len, out_margins


def ensemble_greedy(Ps, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                    ingr_id_dict, oov_word_dict, weights=None, rule="prob"):
    """Greedy over the members ``Ps``, as ``Translator.translate_batch`` decodes: Lt iterations, iteration i picks position i + 1 (the
    last pick is discarded) — the column of the highest combined probability, UNK excepted, ties to the lower column; nothing stops at
    EOS → (ids per video (S_b, Lt) int64: extended ids, the text ids in ``video`` mode; margins (S_b, Lt − 1): the step-score gap
    log best − log second of every pick that is kept)."""
    ingr_input_ids, ingr_sep_masks = _args(ingr_input_ids, ingr_sep_masks)
    Lt, V = cfg.max_t_len, cfg.vocab_size
    out, out_margins = [], []
    for b, S_b in enumerate(batch_step_num):
        sides, n_oov = _video_sides(Ps, cfg, b, S_b, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks,
                                    oov_word_dict, 1)
        C = V + n_oov
        row_c = np.full(S_b, C)
        text = torch.full((S_b, Lt), PAD, dtype=torch.long); text[:, 0] = BOS
        ext = text.clone()
        margins = np.full((S_b, max(Lt - 1, 0)), np.inf)
        for i in range(Lt - 1):
            sc = _step_scores(Ps, cfg, sides, text, i, ingr_id_dict[b], n_oov, row_c, weights, rule).astype(np.float64)
            sc[:, UNK] = -np.inf
            for s in range(S_b):
                order = np.lexsort((np.arange(C), -sc[s, :C]))
                c, c2 = int(order[0]), int(order[1])
                with np.errstate(divide="ignore", invalid="ignore"):
                    margins[s, i] = np.log(sc[s, c]) - np.log(sc[s, c2]) if sc[s, c2] > 0 else np.inf
                ext[s, i + 1] = c
                text[s, i + 1] = UNK if c >= C - n_oov else c
        out.append(text if cfg.model_mode == "video" else ext)
        out_margins.append(margins)
    return out, out_margins
