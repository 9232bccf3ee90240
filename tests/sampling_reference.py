"""CPU restatement of random-sampling caption decoding (svpc_amd.translator's contract for ``translate_batch_sample``: temperature, top-k,
top-p, min length, a counter-based Gumbel-max draw), built on the oracle's own functions and shaped like ``beam_reference.beam_decode``.
``sample_select`` is the step the HIP kernel (svpc_sample_step) must reproduce: the same picks, cum bit for bit, the same finished flags
and lengths — except where a draw is decided by less than the fp64 summation-order noise, which the returned margins expose.

The counter-based hash is ``svpc_mix32`` / ``svpc_hash32`` of svpc_amd/csrc/common.h, ported to Python integers (and to numpy uint64
arrays for whole rows); tests/test_sampling_host.py pins both against known answers of the C++ function."""
import numpy as np
import torch

from beam_reference import step_scores
from oracle import svpc_oracle as orc
from svpc_amd.synthetic import BOS, EOS, PAD, UNK

M32 = 0xFFFFFFFF
COL_STRIDE = 4096          # the draw of row r, column c is keyed by r·4096 + c


def mix32(x):
    x &= M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    x = (x * 0x846CA68B) & M32
    x ^= x >> 16
    return x


def hash32(seed, site, idx):
    """svpc_hash32(seed, site, idx) for Python ints (seed, idx 64-bit, site 32-bit)"""
    key = (((seed ^ (seed >> 32)) & M32) + ((site + 1) & M32) * 0x9E3779B9) & M32
    hi = (idx >> 32) & M32
    return mix32((((idx & M32) ^ key) + hi * 0x85EBCA6B) & M32)


def hash32_np(seed, site, idx):
    """svpc_hash32 over an array of indices (uint64 arithmetic, 32-bit wrap by masking)"""
    seed, idx = int(seed), np.asarray(idx, dtype=np.uint64)
    m = np.uint64(M32)
    key = np.uint64((((seed ^ (seed >> 32)) & M32) + ((int(site) + 1) & M32) * 0x9E3779B9) & M32)
    x = (((idx & m) ^ key) + (idx >> np.uint64(32)) * np.uint64(0x85EBCA6B)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & m
    x ^= x >> np.uint64(16)
    return x


def gumbel(seed, step, idx):
    """g = −log(−log u), u = (h + 0.5)·2⁻³² in float64, h = svpc_hash32(seed, step, idx)"""
    u = (hash32_np(seed, step, idx).astype(np.float64) + 0.5) * (1.0 / 4294967296.0)
    return -np.log(-np.log(u))


def order_desc(raw, cols):
    """the columns ``cols`` in ≻ order: higher raw value, then lower column"""
    cols = np.asarray(cols, dtype=np.int64)
    return cols[np.lexsort((cols, -np.asarray(raw, np.float32)[cols].astype(np.float64)))]


def filtered(scores_row, C, logits, pos, temp=1.0, topk=0, topp=0.0, min_length=0, unk=UNK, eos=EOS):
    """The kept set of one live row: → (K2 columns in ≻ order, their z (float64), step scores (float32, all C columns), margins
    (top-p cut: |prefix mass − q·W| / W at the two prefixes around the cut; top-k: relative raw gap between the k-th and the next
    column)), or None for an empty K0."""
    raw = np.asarray(scores_row, np.float32)[:C]
    s = step_scores(raw, logits, unk)
    cols = np.arange(C)
    cand = (cols != unk) & (s > -np.inf)
    if pos + 1 <= min_length and eos < C:
        cand[eos] = False
    k0 = order_desc(raw, cols[cand])
    if not len(k0):
        return None
    mk = np.inf
    k1 = k0
    if 0 < topk < len(k0):
        k1 = k0[:topk]
        a, b = float(raw[k0[topk - 1]]), float(raw[k0[topk]])
        mk = abs(a - b) / max(abs(a), 1e-30)
    z = s[k1].astype(np.float64) / float(temp)
    mp = np.inf
    if 0.0 < topp < 1.0:
        w = np.exp(z - z[0])
        W = float(w.sum())
        target = topp * W
        cs = np.cumsum(w)
        hit = np.nonzero(cs >= target)[0]
        n2 = int(hit[0]) + 1 if len(hit) else len(k1)
        mp = abs(cs[n2 - 1] - target)
        if n2 >= 2:
            mp = min(mp, abs(cs[n2 - 2] - target))
        mp /= W
        k1, z = k1[:n2], z[:n2]
    return k1, z, s, (mp, mk)


def sample_select(scores, row_c, row_x, pos, logits, cum, finished, length, seed, temp=1.0, topk=0, topp=0.0, min_length=0, row0=0,
                  unk=UNK, eos=EOS, pad=PAD):
    """One sampling step over the rows of ``scores`` (R, ≥ C) float32; row i is the kernel's row r = row0 + i (its draws are keyed by
    r).  cum (R,) float32, finished (R,) bool, length (R,) int.
    → picks (extended ids, PAD for finished / empty rows), new cum, new finished, new length, margins (R, 3) float64: the gap between
    the best and second-best Gumbel key, the relative top-p cut gap, the relative top-k raw gap (+inf where there is none)."""
    scores = np.asarray(scores, dtype=np.float32)
    R = scores.shape[0]
    p = pos + 1
    picks = np.full(R, pad, np.int64)
    cum_new = np.array(cum, dtype=np.float32, copy=True)
    fin_new = np.array(finished, dtype=bool, copy=True)
    len_new = np.array(length, dtype=np.int64, copy=True)
    margins = np.full((R, 3), np.inf)
    topk = max(int(topk), 0)
    for i in range(R):
        if fin_new[i]:
            continue
        f = filtered(scores[i], int(row_c[i]), logits, pos, temp, topk, topp, min_length, unk, eos)
        len_new[i] = p
        fin_new[i] = True
        if f is None:
            cum_new[i] = -np.inf
            continue
        k2, z, s, (mp, mk) = f
        key = z + gumbel(seed, pos, (row0 + i) * COL_STRIDE + k2)
        best = key.max()
        j = int(np.nonzero(key == best)[0][np.argmin(k2[key == best])])      # ties: the lower column
        if len(key) > 1:
            margins[i, 0] = float(best - np.partition(key, -2)[-2]) if np.sum(key == best) == 1 else 0.0
        margins[i, 1:] = (mp, mk)
        c = int(k2[j])
        picks[i] = c
        cum_new[i] = np.float32(np.float32(cum[i]) + s[c])
        fin_new[i] = c == eos
    return picks, cum_new, fin_new, len_new, margins


def model_ids(picks, finished_before, row_c, row_x, unk=UNK, pad=PAD):
    """the model-side ids of a step's picks: UNK for a copied word (c ≥ C − X), PAD for a row that was already finished"""
    out = np.array(picks, dtype=np.int64, copy=True)
    for i, c in enumerate(out):
        if not finished_before[i] and c != pad and c >= int(row_c[i]) - int(row_x[i]):
            out[i] = unk
    return out


def sample_decode(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                  ingr_id_dict, oov_word_dict, num_samples, seed, temp=1.0, topk=0, topp=0.0, min_length=0, bos=BOS, unk=UNK):
    """→ (ids, cums, lens, margins): per video ids (S_b, R, Lt) int64 (extended ids, PAD after EOS), cum (S_b, R) float32, len (S_b, R)
    int64, and margins (S_b, R): the smallest of each sample's step margins (``sample_select``).  Sentence s of video b is the batch's
    sentence t = Σ_{b' < b} S_b' + s, its samples the kernel rows t·R + j."""
    mode, Lv, Lt = cfg.model_mode, cfg.max_v_len, cfg.max_t_len
    V = cfg.vocab_size
    Rs = num_samples
    ingr_input_ids = torch.as_tensor(ingr_input_ids)
    ingr_sep_masks = torch.as_tensor(ingr_sep_masks)
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    out, out_cum, out_len, out_margins = [], [], [], []
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
        mem = mem.repeat_interleave(Rs, 0)                                             # sample rows s·R + j
        bank = bank.repeat_interleave(Rs, 0) if bank is not None else None
        R = S_b * Rs
        C = V + n_oov
        row_c, row_x = np.full(R, C), np.full(R, n_oov)
        text = torch.full((R, Lt), PAD, dtype=torch.long); text[:, 0] = bos
        ext = text.clone()
        cum = np.zeros(R, np.float32)
        fin = np.zeros(R, bool)
        ln = np.zeros(R, np.int64)
        margins = np.full(R, np.inf)
        for i in range(Lt - 1):
            dec = orc.decoder(P, orc.text_embed(P, text[:, :i + 1], cfg), torch.ones(R, i + 1), mem, torch.ones(mem.shape[:2]), cfg)
            last = dec[:, i:i + 1]
            if mode == "video":
                sc = orc.lm_head(P, last, cfg)[:, 0]
            else:
                sc = orc.pointer_generator(P, last, bank, ingr_id_dict[b], n_oov, cfg)[:, 0]
            before = fin.copy()
            picks, cum, fin, ln, mg = sample_select(sc.detach().numpy(), row_c, row_x, i, mode == "video", cum, fin, ln, seed, temp, topk,
                                                    topp, min_length, row0=t0 * Rs, unk=unk)
            margins = np.minimum(margins, mg.min(1))
            text[:, i + 1] = torch.as_tensor(model_ids(picks, before, row_c, row_x, unk=unk))
            ext[:, i + 1] = torch.as_tensor(picks)
        out.append(ext.view(S_b, Rs, Lt))
        out_cum.append(cum.reshape(S_b, Rs))
        out_len.append(ln.reshape(S_b, Rs))
        out_margins.append(margins.reshape(S_b, Rs))
        t0 += S_b
    return out, out_cum, out_len, out_margins


def chi_square(counts, probs):
    """Pearson's statistic of observed ``counts`` against ``probs`` (cells with probability 0 must hold no counts) → (statistic, dof)"""
    counts = np.asarray(counts, np.float64)
    probs = np.asarray(probs, np.float64)
    n = counts.sum()
    on = probs > 0
    e = n * probs[on]
    return float(((counts[on] - e) ** 2 / e).sum()), int(on.sum()) - 1


def chi_square_bound(dof, z=4.265):
    """the upper quantile of the chi-square distribution with ``dof`` degrees of freedom at the normal deviate ``z`` (Wilson–Hilferty;
    4.265 ≈ the 1e-5 tail)"""
    a = 2.0 / (9.0 * dof)
    return dof * (1.0 - a + z * np.sqrt(a)) ** 3


def target_distribution(scores_row, C, logits, pos, temp=1.0, topk=0, topp=0.0, min_length=0):
    """the distribution a draw follows: softmax(z) over K2, as a (C,) float64 vector"""
    f = filtered(scores_row, C, logits, pos, temp, topk, topp, min_length)
    out = np.zeros(C)
    if f is None:
        return out
    k2, z = f[0], f[1]
    e = np.exp(z - z.max())
    out[k2] = e / e.sum()
    return out
