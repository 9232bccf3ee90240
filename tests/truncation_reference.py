"""CPU restatement of the truncation stages of sampling decoding (svpc_sample_step_trunc; svpc_amd.translator's contract for the
``min_p`` / ``typical_p`` / ``epsilon_cutoff`` / ``eta_cutoff`` keywords of ``translate_batch_sample``), built on
``sampling_reference.filtered``: ``truncate`` takes today's kept set K2 to the final set, ``trunc_select`` is the step the HIP kernel must
reproduce, ``trunc_decode`` the whole decode.  Everything in float64.

Two kinds of margin tell a real difference from rounding:

- the SET margin of ``truncate`` (kernel against reference on identical fp32 scores, where only the fp64 summation order and libm's last
  bits differ): the relative distance of any w or q to its threshold, the mass gap at the typical cut and at the cut before it, and the
  gap between d* and its neighbouring distinct d.  The last one is taken relative to max(d*, H, 1), not to d* alone: d is a difference
  of −ln q and H, so its absolute error is an ulp of those operands however small d itself is.
- the PICK margin of ``decided`` (GPU decode against CPU oracle, whose fp32 scores differ in their last bits): with ~950 columns some
  column always sits within 1e-4 of a cut, so the set margin would flag nearly every sample; but a borderline column changes the pick
  only if it also wins the Gumbel race.  A step is decided when the Gumbel winner over a LOOSENED chain (every threshold ×(1 − δ), the
  typical mass target + δ, the d cut widened by δ(1 + d*)) lies inside a TIGHTENED chain (the opposite changes; the typical crossing
  column stays unless another distinct d lies within the band)."""
import functools

import numpy as np
import torch

import sampling_reference as sr
from oracle import svpc_oracle as orc
from svpc_amd.synthetic import BOS, EOS, PAD, UNK

OFF = dict(min_p=0.0, typical_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0)


def renorm(z):
    """the distribution over a set whose ≻-first column is z[0] → (w, W, q, ln q); ln q = −inf where w = 0"""
    w = np.exp(z - z[0])
    W = float(w.sum())
    with np.errstate(divide="ignore"):
        lq = np.where(w > 0, (z - z[0]) - np.log(W), -np.inf)
    return w, W, w / W, lq


def entropy(w, q, lq):
    on = w > 0
    return float(-(q[on] * lq[on]).sum())


def typical_cut(q, d, m):
    """→ (index i into u = the ascending distinct d, u, mass of {d ≤ u[j]} for every j): u[i] = d*"""
    order = np.argsort(d, kind="stable")
    ds = d[order]
    cs = np.cumsum(q[order])
    last = np.nonzero(np.append(ds[1:] != ds[:-1], True))[0]          # the last position of every distinct d
    u, mass = ds[last], cs[last]
    hit = np.nonzero(mass >= m)[0]
    return (int(hit[0]) if len(hit) else len(u) - 1), u, mass


def truncate(k2, z, min_p=0.0, typical_p=0.0, epsilon_cutoff=0.0, eta_cutoff=0.0, sign=0, delta=0.0):
    """K2 (columns in ≻ order, their z) → (the final set in ≻ order, its z, the set margin).  ``sign`` = +1 / −1 with ``delta`` > 0: the
    loosened / tightened chain of the pick margin (module docstring); 0: the exact chain."""
    k, z = np.asarray(k2), np.asarray(z, np.float64)
    mg = np.inf
    if 0.0 < min_p < 1.0:
        w = np.exp(z - z[0])
        keep = w >= min_p * (1 - sign * delta)
        keep[0] = True
        mg = min(mg, float(np.min(np.abs(w - min_p))) / min_p)
        k, z = k[keep], z[keep]
    if 0.0 < typical_p < 1.0:
        w, W, q, lq = renorm(z)
        H = entropy(w, q, lq)
        d = np.abs(-lq - H)
        i, u, mass = typical_cut(q, d, min(max(typical_p + sign * delta, 0.0), 1.0))
        mg = min(mg, abs(float(mass[i]) - typical_p))
        if i > 0:
            mg = min(mg, abs(float(mass[i - 1]) - typical_p))
        if np.isfinite(u[i]):
            gap = min(u[i + 1] - u[i] if i + 1 < len(u) else np.inf, u[i] - u[i - 1] if i > 0 else np.inf)
            mg = min(mg, float(gap) / max(float(u[i]), H, 1.0))
        if sign >= 0:
            keep = d <= (u[i] + sign * delta * (1 + u[i]) if np.isfinite(u[i]) else u[i])
        else:
            band = delta * (1 + u[i]) if np.isfinite(u[i]) else 0.0
            keep = d <= u[i]
            if np.sum(np.abs(u - u[i]) <= band) > 1:
                keep &= ~(np.abs(d - u[i]) <= band)
            if not keep.any():
                keep[np.argmin(d)] = True
        k, z = k[keep], z[keep]
    for par, eta in ((epsilon_cutoff, False), (eta_cutoff, True)):
        if par > 0.0:
            w, W, q, lq = renorm(z)
            thr = min(par, np.sqrt(par) * np.exp(-entropy(w, q, lq))) if eta else par
            keep = q >= thr * (1 - sign * delta)
            keep[0] = True
            mg = min(mg, float(np.min(np.abs(q - thr))) / thr)
            k, z = k[keep], z[keep]
    return k, z, mg


def decided(k2, z, seed, pos, row, trunc, delta):
    """the pick margin of one step (module docstring): the Gumbel winner over the loosened chain lies inside the tightened one"""
    kl, zl, _ = truncate(k2, z, sign=1, delta=delta, **trunc)
    kt = truncate(k2, z, sign=-1, delta=delta, **trunc)[0]
    key = zl + sr.gumbel(seed, pos, row * sr.COL_STRIDE + kl)
    return int(kl[int(np.argmax(key))]) in set(kt.tolist())


def loosened_set(k2, z, trunc, delta):
    return set(truncate(k2, z, sign=1, delta=delta, **trunc)[0].tolist())


def trunc_select(scores, row_c, row_x, pos, logits, cum, finished, length, seed, temp=1.0, topk=0, topp=0.0, min_length=0, row0=0,
                 unk=UNK, eos=EOS, pad=PAD, delta=None, forced=None, **trunc):
    """``sampling_reference.sample_select`` with the truncation stages ``trunc`` between top-p and the draw.
    → picks, new cum, new finished, new length, margins (R, 4) float64 (the Gumbel gap, the top-p cut gap, the top-k raw gap, the set
    margin of ``truncate``; +inf where there is none), kept (R,) int64 (the size of the final set; 0 for finished / empty rows), and
    undecided (R,) bool: with ``delta`` the rows whose pick margin fails (``decided``).  ``forced`` (R,) ids: the rows take these picks
    instead of their own (a replay along another decode's prefix); undecided then marks the rows whose forced pick lies OUTSIDE the
    loosened set."""
    scores = np.asarray(scores, dtype=np.float32)
    R = scores.shape[0]
    p = pos + 1
    picks = np.full(R, pad, np.int64)
    cum_new = np.array(cum, dtype=np.float32, copy=True)
    fin_new = np.array(finished, dtype=bool, copy=True)
    len_new = np.array(length, dtype=np.int64, copy=True)
    margins = np.full((R, 4), np.inf)
    kept = np.zeros(R, np.int64)
    undecided = np.zeros(R, bool)
    for i in range(R):
        if fin_new[i]:
            continue
        f = sr.filtered(scores[i], int(row_c[i]), logits, pos, temp, max(int(topk), 0), topp, min_length, unk, eos)
        len_new[i] = p
        fin_new[i] = True
        if f is None:
            cum_new[i] = -np.inf
            continue
        k2, z2, s, (mp, mk) = f
        k3, z3, ms = truncate(k2, z2, **trunc)
        kept[i] = len(k3)
        key = z3 + sr.gumbel(seed, pos, (row0 + i) * sr.COL_STRIDE + k3)
        best = key.max()
        c = int(k3[key == best].min())                                       # ties: the lower column
        if len(key) > 1:
            margins[i, 0] = float(best - np.partition(key, -2)[-2]) if np.sum(key == best) == 1 else 0.0
        margins[i, 1:] = (mp, mk, ms)
        if forced is not None:
            c = int(forced[i])
            undecided[i] = c not in loosened_set(k2, z2, trunc, delta)
            if not 0 <= c < len(s) or not np.isfinite(s[c]):                 # (not a candidate at all: nothing to follow)
                cum_new[i] = -np.inf
                continue
        elif delta is not None:
            undecided[i] = not decided(k2, z2, seed, pos, row0 + i, trunc, delta)
        picks[i] = c
        cum_new[i] = np.float32(np.float32(cum[i]) + s[c])
        fin_new[i] = c == eos
    return picks, cum_new, fin_new, len_new, margins, kept, undecided


def trunc_decode(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                 ingr_id_dict, oov_word_dict, num_samples, seed, temp=1.0, topk=0, topp=0.0, min_length=0, bos=BOS, unk=UNK, delta=1e-4,
                 forced=None, **trunc):
    """``sampling_reference.sample_decode`` (its loop, restated) with ``trunc_select`` as the step → (ids, cums, lens, margins, undecided,
    kept): per video ids (S_b, R, Lt) int64, cum (S_b, R) float32, len (S_b, R) int64, margins (S_b, R) — the smallest Gumbel / top-p /
    top-k margin of each sample's steps, as ``sample_decode``'s — undecided (S_b, R) int64 — the number of the sample's steps whose pick
    margin at ``delta`` fails — and kept (S_b, R, Lt − 1) int64.  ``forced``: per video (S_b, R, Lt) ids of another decode; every step
    is then replayed along ITS prefix, and undecided counts the steps whose forced word lies outside the loosened set."""
    mode, Lv, Lt = cfg.model_mode, cfg.max_v_len, cfg.max_t_len
    V = cfg.vocab_size
    Rs = num_samples
    ingr_input_ids = torch.as_tensor(ingr_input_ids)
    ingr_sep_masks = torch.as_tensor(ingr_sep_masks)
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    out, out_cum, out_len, out_margins, out_und, out_kept = [], [], [], [], [], []
    t0 = 0
    with torch.no_grad():
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
            mem = mem.repeat_interleave(Rs, 0)
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
            und = np.zeros(R, np.int64)
            kept = np.zeros((R, Lt - 1), np.int64)
            given = None if forced is None else np.asarray(forced[b].cpu() if torch.is_tensor(forced[b]) else forced[b]).reshape(R, Lt)
            for i in range(Lt - 1):
                dec = orc.decoder(P, orc.text_embed(P, text[:, :i + 1], cfg), torch.ones(R, i + 1), mem, torch.ones(mem.shape[:2]), cfg)
                last = dec[:, i:i + 1]
                if mode == "video":
                    sc = orc.lm_head(P, last, cfg)[:, 0]
                else:
                    sc = orc.pointer_generator(P, last, bank, ingr_id_dict[b], n_oov, cfg)[:, 0]
                before = fin.copy()
                picks, cum, fin, ln, mg, kp, ud = trunc_select(sc.detach().numpy(), row_c, row_x, i, mode == "video", cum, fin, ln, seed, temp,
                                                               topk, topp, min_length, row0=t0 * Rs, unk=unk, delta=delta,
                                                               forced=None if given is None else given[:, i + 1], **trunc)
                margins = np.minimum(margins, mg[:, :3].min(1))
                und += ud
                kept[:, i] = kp
                text[:, i + 1] = torch.as_tensor(sr.model_ids(picks, before, row_c, row_x, unk=unk))
                ext[:, i + 1] = torch.as_tensor(picks)
            out.append(ext.view(S_b, Rs, Lt))
            out_cum.append(cum.reshape(S_b, Rs))
            out_len.append(ln.reshape(S_b, Rs))
            out_margins.append(margins.reshape(S_b, Rs))
            out_und.append(und.reshape(S_b, Rs))
            out_kept.append(kept.reshape(S_b, Rs, Lt - 1))
            t0 += S_b
    return out, out_cum, out_len, out_margins, out_und, out_kept


def target_distribution(scores_row, C, logits, pos, temp=1.0, topk=0, topp=0.0, min_length=0, **trunc):
    """the distribution a truncated draw follows: softmax(z) over the final set, as a (C,) float64 vector"""
    f = sr.filtered(scores_row, C, logits, pos, temp, topk, topp, min_length)
    out = np.zeros(C)
    if f is None:
        return out
    k, z, _ = truncate(f[0], f[1], **trunc)
    e = np.exp(z - z.max())
    out[k] = e / e.sum()
    return out


# ------------------------------------------------------------------------------------------------ the tables of the kernel tests
KERNEL_TIE = 1e-9
BASE = [(0, 0.0, 1.0), (5, 0.0, 0.5), (0, 0.9, 2.0), (40, 0.0, 1.0)]          # (k, q, τ) every truncation setting is crossed with
TRUNC = [dict(min_p=0.07), dict(min_p=0.3), dict(typical_p=0.37), dict(typical_p=0.9), dict(epsilon_cutoff=3e-3), dict(epsilon_cutoff=0.04),
         dict(eta_cutoff=3e-3), dict(eta_cutoff=0.04), dict(min_p=0.07, typical_p=0.9, epsilon_cutoff=3e-3, eta_cutoff=3e-3)]
KERNEL_POS, KERNEL_LT = 4, 9


def tables(rng, T, R, logits, adversarial, cmax_hi=700):
    """scores / row_c / row_x / cum / finished / length for T sentences × R samples, drawn as tests/test_sampling_gpu.py draws them: ragged
    C per sentence, OOV columns, finished rows, rows without candidates, and (adversarial) few distinct values: exact ties everywhere"""
    Cs = rng.integers(16, cmax_hi, size=T)
    Xs = np.array([rng.integers(0, min(4, c - UNK - 1)) for c in Cs])
    cmax = int(Cs.max())
    n = T * R
    if adversarial:
        vals = np.array([0.0, 0.125, 0.25, 0.5] if not logits else [-np.inf, -1.0, 0.0, 2.0], np.float32)
        s = vals[rng.integers(0, len(vals), size=(n, cmax))]
    else:
        s = (rng.random((n, cmax)) ** 4).astype(np.float32) if not logits else rng.standard_normal((n, cmax)).astype(np.float32) * 3
    s[:, UNK] = 1.0 if not logits else 50.0
    empty = rng.random(n) < 0.05
    s[empty] = 0.0 if not logits else -np.inf
    s[empty, UNK] = 1.0 if not logits else 50.0
    cum = (-rng.random(n) * 5).astype(np.float32)
    fin = (rng.random(n) < 0.3).astype(np.int32)
    length = rng.integers(1, 6, size=n).astype(np.int32)
    return s, np.repeat(Cs, R), np.repeat(Xs, R), cum, fin, length


@functools.lru_cache(maxsize=None)
def kernel_cases(R, logits):
    """the launches of the kernel test for (R, score mode) with their reference results, computed once: a list of (tables, dict(k, q, t,
    m, seed), truncation setting, ``trunc_select``'s result) over 29 sentences × R samples, plain then adversarial tables, every
    truncation setting × BASE, EOS barred (m = 6 ≥ p = 5) in every fourth launch"""
    rng = np.random.default_rng(1000 + 10 * R + logits)
    out = []
    for adversarial in (False, True):
        tb = tables(rng, 29, R, logits, adversarial)
        s, row_c, row_x, cum, fin, length = tb
        n = 0
        for trunc in TRUNC:
            for k, q, t in BASE:
                m = 6 if n % 4 == 3 else 0
                n += 1
                seed = int(rng.integers(0, 1 << 63))
                ref = trunc_select(s, row_c, row_x, KERNEL_POS, logits, cum, fin.astype(bool), length, seed, temp=t, topk=k, topp=q,
                                   min_length=m, **trunc)
                out.append((tb, dict(k=k, q=q, t=t, m=m, seed=seed), trunc, ref))
    return out


def flagged_rows(ref, fin):
    """the live rows of one launch whose set or Gumbel margin (or top-p cut) is within KERNEL_TIE: counted, not compared"""
    mg = ref[4]
    return (np.minimum(np.minimum(mg[:, 0], mg[:, 1]), mg[:, 3]) < KERNEL_TIE) & ~np.asarray(fin, bool)


@functools.lru_cache(maxsize=None)
def wide_cases():
    """rows of 1,025 … 4,096 columns (the wide kernel variant): 12 sentences × 2 samples, both score modes, four settings each"""
    rng = np.random.default_rng(5)
    out = []
    for logits in (False, True):
        s, row_c, row_x, cum, fin, length = tables(rng, 12, 2, logits, False, cmax_hi=4097)
        row_c = np.maximum(row_c, 1025)
        row_c[0] = 4096
        s = np.pad(s, ((0, 0), (0, 4096 - s.shape[1])), constant_values=0.01 if not logits else -1.0)
        tb = (s, row_c, row_x, cum, fin, length)
        for (k, q, t), trunc in zip(BASE, (dict(min_p=0.07, eta_cutoff=3e-3), dict(typical_p=0.37), dict(typical_p=0.9, epsilon_cutoff=3e-3),
                                           TRUNC[-1])):
            seed = int(rng.integers(0, 1 << 63))
            ref = trunc_select(s, row_c, row_x, 3, logits, cum, fin.astype(bool), length, seed, temp=t, topk=k, topp=q, **trunc)
            out.append((logits, tb, dict(k=k, q=q, t=t, m=0, seed=seed), trunc, ref))
    return out


# ------------------------------------------------------------------------------------------------ the pairs of the translator tests
# (case, model type, truncation setting): the pairs whose ids are compared with ``trunc_decode``'s; tests/test_truncation_host.py asserts
# that the reference alone counts no undecided step on any of them (R = 3, seed 1234, τ = 1, δ = 1e-4)
DECODE_DELTA = 1e-4
DECODE_R, DECODE_SEED = 3, 1234
DECODE_PAIRS = ([(c, mt, kw) for c, mt in (("tiny", "v"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt"))
                 for kw in (dict(min_p=0.3), dict(epsilon_cutoff=0.04), dict(eta_cutoff=0.04))] +
                [(c, mt, dict(typical_p=m)) for c, mt in (("tiny", "v"), ("tiny", "vivt"), ("c1", "v")) for m in (0.2, 0.9)] +
                [("tiny", "v", dict(typical_p=0.37)), ("c1", "v", dict(typical_p=0.37))])
# checked by membership instead (typical on c1 vivt leaves 1 … 15 undecided steps of 441): δ = 1e-3, a hard assertion
MEMBER_PAIRS = [("c1", "vivt", dict(typical_p=0.9)), ("c1", "vivt", dict(min_p=0.07, typical_p=0.9, epsilon_cutoff=3e-3, eta_cutoff=3e-3))]
MEMBER_DELTA = 1e-3
