"""CPU restatement of beam-search caption decoding (svpc_amd.translator's contract, the reference CLI's ``--use_beam --beam_size``,
test.py:207-209), built on the oracle's own functions and shaped like ``oracle.greedy_decode``: per video, the decoder re-run over every
hypothesis's tokens each step.  ``select`` is the selection rule the HIP kernel (svpc_beam_step) must reproduce exactly.

Step scores are computed in float64 and rounded once to float32 (as the kernel does), and summed in float32:
pointer modes log p (p <= 0: -inf); ``video`` mode logit - log-sum-exp over the row's columns without UNK."""
import numpy as np
import torch

from oracle import svpc_oracle as orc
from svpc_amd.synthetic import BOS, EOS, PAD, UNK


def step_scores(row, logits, unk=UNK):
    """float32 step scores of the columns of one score row (the UNK column's value is meaningless: it is never a candidate)."""
    r64 = np.asarray(row, dtype=np.float32).astype(np.float64)
    if logits:
        keep = np.ones(r64.shape[0], bool)
        if unk < r64.shape[0]:
            keep[unk] = False
        m = r64[keep].max()
        lse = m + np.log(np.exp(r64[keep] - m).sum())
        return (r64 - lse).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(r64 > 0, np.log(np.where(r64 > 0, r64, 1.0)), -np.inf).astype(np.float32)


def select(scores, row_c, row_x, beam, logits, cum, finished, unk=UNK, eos=EOS, pad=PAD, return_margin=False):
    """One selection step.  scores (T·B, ≥ C) float32, row_c / row_x per row, cum (T·B,) float32, finished (T·B,) bool.
    Candidates of a sentence: every (hypothesis h, column c ≠ UNK, c < C) of an unfinished h, and (h, PAD) of a finished one, ranked by
    higher cum (float32 cum_h + step), then higher raw value (+inf for a finished one), then lower flat index h·C + c.
    → parent (global rows), next extended ids, next model ids (OOV → UNK), new cum, new finished [, margin (T,): cum of the last kept
    candidate minus cum of the first dropped one, +inf when nothing is dropped]."""
    scores = np.asarray(scores, dtype=np.float32)
    cum = np.asarray(cum, dtype=np.float32)
    finished = np.asarray(finished).astype(bool)
    R = scores.shape[0]
    B = beam
    T = R // B
    parent = np.zeros(R, np.int64)
    ext = np.zeros(R, np.int64)
    mod = np.zeros(R, np.int64)
    cum_new = np.zeros(R, np.float32)
    fin_new = np.zeros(R, bool)
    margin = np.full(T, np.inf)
    for t in range(T):
        cc, cr, cf, ch, ccol, cfin = [], [], [], [], [], []
        for h in range(B):
            r = t * B + h
            C = int(row_c[r])
            if finished[r]:
                cc.append(np.array([cum[r]], np.float32)); cr.append(np.array([np.inf], np.float32))
                cf.append(np.array([h * C + pad])); ch.append(np.array([h])); ccol.append(np.array([pad])); cfin.append(np.array([True]))
                continue
            cols = np.array([c for c in range(C) if c != unk], dtype=np.int64)
            st = step_scores(scores[r, :C], logits, unk)[cols]
            cc.append((np.float32(cum[r]) + st).astype(np.float32)); cr.append(scores[r, cols])
            cf.append(h * C + cols); ch.append(np.full(len(cols), h)); ccol.append(cols); cfin.append(np.zeros(len(cols), bool))
        cc, cr, cf = np.concatenate(cc), np.concatenate(cr), np.concatenate(cf)
        ch, ccol, cfin = np.concatenate(ch), np.concatenate(ccol), np.concatenate(cfin)
        order = np.lexsort((cf, -cr.astype(np.float64), -cc.astype(np.float64)))
        if len(order) > B:
            margin[t] = float(cc[order[B - 1]]) - float(cc[order[B]])
        for k in range(B):
            r = t * B + k
            if k < len(order):
                e = order[k]
                h, col, was_fin, cu = int(ch[e]), int(ccol[e]), bool(cfin[e]), cc[e]
            else:
                h, col, was_fin, cu = k, pad, True, np.float32(-np.inf)
            C, X = int(row_c[t * B + h]), int(row_x[t * B + h])
            parent[r] = t * B + h
            ext[r] = pad if was_fin else col
            mod[r] = pad if was_fin else (unk if col >= C - X else col)
            cum_new[r] = cu
            fin_new[r] = was_fin or ext[r] == eos
    out = (parent, ext, mod, cum_new, fin_new)
    return out + (margin,) if return_margin else out


def beam_decode(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                ingr_id_dict, oov_word_dict, beam, bos=BOS, unk=UNK):
    """→ (ids, scores, margins): per video an (S_b, Lt) int64 matrix of the best hypotheses (extended ids, PAD after EOS), their
    float32 scores (S_b,), and the selection margins (S_b, Lt − 1) of every step (see ``select``)."""
    mode, Lv, Lt = cfg.model_mode, cfg.max_v_len, cfg.max_t_len
    V = cfg.vocab_size
    B = beam
    ingr_input_ids = torch.as_tensor(ingr_input_ids)
    ingr_sep_masks = torch.as_tensor(ingr_sep_masks)
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    out, out_scores, out_margins = [], [], []
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
        mem = mem.repeat_interleave(B, 0)                                              # hypothesis rows s·B + h
        bank = bank.repeat_interleave(B, 0) if bank is not None else None
        R = S_b * B
        C = V + n_oov
        row_c, row_x = np.full(R, C), np.full(R, n_oov)
        text = torch.full((R, Lt), PAD, dtype=torch.long); text[:, 0] = bos
        ext = text.clone()
        cum = np.zeros((S_b, B), np.float32); cum[:, 1:] = -np.inf
        cum = cum.reshape(-1)
        fin = np.zeros(R, bool)
        margins = np.zeros((S_b, max(Lt - 1, 0)))
        for i in range(Lt - 1):
            # causal decoder: position i depends on positions 0 … i only
            dec = orc.decoder(P, orc.text_embed(P, text[:, :i + 1], cfg), torch.ones(R, i + 1), mem, torch.ones(mem.shape[:2]), cfg)
            last = dec[:, i:i + 1]
            if mode == "video":
                sc = orc.lm_head(P, last, cfg)[:, 0]
            else:
                sc = orc.pointer_generator(P, last, bank, ingr_id_dict[b], n_oov, cfg)[:, 0]
            parent, nx_ext, nx_mod, cum, fin, margins[:, i] = select(sc.detach().numpy(), row_c, row_x, B, mode == "video", cum, fin, unk=unk,
                                                                     return_margin=True)
            pt = torch.as_tensor(parent)
            text, ext = text[pt].clone(), ext[pt].clone()
            text[:, i + 1] = torch.as_tensor(nx_mod)
            ext[:, i + 1] = torch.as_tensor(nx_ext)
        best = np.array([int(np.argmax(cum[s * B:(s + 1) * B])) for s in range(S_b)], dtype=np.int64)   # (first maximum: lowest index)
        rows = np.arange(S_b) * B + best
        out.append(ext[torch.as_tensor(rows)])
        out_scores.append(cum[rows].astype(np.float32))
        out_margins.append(margins)
    return out, out_scores, out_margins


def greedy_equivalent(greedy_ids):
    """greedy's id matrix as a B = 1 beam returns it: identical up to and including the first EOS (position ≥ 1), PAD after."""
    g = greedy_ids.clone()
    for s in range(g.shape[0]):
        hit = (g[s, 1:] == EOS).nonzero()
        if len(hit):
            g[s, int(hit[0]) + 2:] = PAD
    return g
