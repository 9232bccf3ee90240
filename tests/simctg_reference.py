"""CPU restatement of contrastive (SimCTG) training (``svpc_amd.simctg``; Su et al. 2022).  Shares no code with the product;
the summation order of the dot products is ``contrastive_reference.wave_dot``'s, ``contrastive_loss`` is ``scst_reference.sequence_loss``'s
construction with the decoder's output exposed, under torch autograd.

The definition.  One caption row r of the graded pass (R = T·K rows, ``force_inputs``' ``length``, Lt positions): its token set is
positions 0 … len_r, n = len_r + 1 — the history entries contrastive search commits for that caption, BOS through EOS (through Lt − 1 without
an EOS); len_r is clamped into [0, Lt − 1].  h_i is row r·Lt + i of the decoder's last-layer output as fp32, ρ the margin rounded to fp32.

- q_i = Σ_d h_i[d]² and every h_i·h_j are summed in fp64 in the kernel's order (``wave_dot``): a q_i has ``hist_n2``'s bits;
- c_ij = (h_i·h_j) / (sqrt(q_i)·sqrt(q_j)) in fp64, 0 when either norm is 0;  m_ij = (ρ − 1) + c_ij for i ≠ j;  the ordered pair (i, j) is
  ACTIVE iff m_ij > 0, strictly (at the kink the pair is inactive and its gradient 0);
- cl_r = Σ_{i≠j} max(0, m_ij) / (n(n − 1)),  sim_r = Σ_{i≠j} c_ij / (n(n − 1)) — fp64, each rounded once to fp32 —, nact_r = the active ordered
  pairs (int32); all three 0 when n < 2;
- loss = fp32(Σ_r v_r·cl_r), v (R,) fp32 and cl_r the fp32 value, products and sums in fp64 (the kernel adds them in a fixed order);
- with u_i = h_i / sqrt(q_i) (0 for a zero row) and g_i = Σ_{j : (i, j) active} u_j:
  ∂loss/∂h_i = dl·v_r·(2 / (n(n − 1)))·(g_i − (g_i·u_i)·u_i) / sqrt(q_i) in fp64 (the 2: (i, j) and (j, i) both hold c_ij); exactly 0 for a
  zero row, for positions > len_r and for n < 2.
A caption ``seq_nll`` bars still has hidden states: its term counts."""
import numpy as np
import torch

import forced_score_reference as fr
from oracle import svpc_oracle as orc
from svpc_amd.synthetic import UNK

_LANES = np.arange(64)


def gram(H):
    """H (n, D) float32 → (n, n) float64, every entry ``contrastive_reference.wave_dot``'s sum (the same operations in the same order,
    all pairs at once; tests/test_simctg_host.py holds the two against each other)"""
    H = np.asarray(H, np.float32).astype(np.float64)
    n, D = H.shape
    if D % 64:
        H = np.concatenate([H, np.zeros((n, 64 - D % 64))], 1)
    H = H.reshape(n, -1, 64)
    s = np.zeros((n, n, 64))
    for k in range(H.shape[1]):
        s = s + H[:, None, k, :] * H[None, :, k, :]
    for o in (32, 16, 8, 4, 2, 1):
        s = s + s[:, :, _LANES ^ o]
    return s[:, :, 0].copy()


def tokens(length, lt):
    return min(max(int(length), 0), lt - 1) + 1


def caption(G, rho):
    """the Gram matrix of a caption's n token states → (c, m, active): (n, n) float64 cosines (0 on the diagonal), margins ρ − 1 + c
    (−inf on the diagonal) and the active pairs"""
    n = G.shape[0]
    q = np.diag(G).copy()
    c = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            if i != j and q[i] > 0.0 and q[j] > 0.0:
                c[i, j] = G[i, j] / (np.sqrt(q[i]) * np.sqrt(q[j]))
    m = (np.float64(rho) - 1.0) + c
    m[np.arange(n), np.arange(n)] = -np.inf
    return c, m, m > 0.0


def grams(hidden, length, lt):
    """hidden (≥ R·Lt, D) float32, length (R,) → per caption the Gram matrix of its token states (shared by the margins of one case)"""
    hidden = np.asarray(hidden, np.float32)
    return [gram(hidden[r * lt:r * lt + tokens(length[r], lt)]) for r in range(len(length))]


def seq_cl(hidden, length, v, margin, lt, dl=1.0, G=None):
    """``hidden`` (≥ R·Lt, D) float32 — row r·Lt + i is position i of caption r —, ``length`` (R,), ``v`` (R,) float32, ``margin`` a
    number (rounded to fp32 here) → a dict: loss (float32), cl / sim (R,) float32, cl64 / sim64 (R,) float64, nact (R,) int32, q (R, Lt)
    float64, dh (rows, D) float64 = dl · d loss / d hidden, zero_rows (rows,) bool: the rows whose gradient is 0 by definition (a zero row, a
    position past the end, a caption of one token), min_abs_m: per caption the smallest |m_ij| over its pairs (inf: none) — how far
    the caption is from a kink of the hinge."""
    hidden = np.asarray(hidden, np.float32)
    rho = float(np.float32(margin))
    R, D = len(length), hidden.shape[1]
    G = grams(hidden, length, lt) if G is None else G
    cl64, sim64 = np.zeros(R), np.zeros(R)
    nact = np.zeros(R, np.int32)
    q = np.zeros((R, lt))
    dh = np.zeros(hidden.shape, np.float64)
    near = np.full(R, np.inf)
    zero = np.zeros(hidden.shape[0], bool)
    mats = []
    for r in range(R):
        n = tokens(length[r], lt)
        qr = np.diag(G[r]).copy()
        q[r, :n] = qr
        zero[r * lt:(r + 1) * lt] = True
        if n >= 2:
            zero[r * lt:r * lt + n] = ~(qr > 0.0)
        c, m, act = caption(G[r], rho)
        mats.append(m)
        if n < 2:
            continue
        off = ~np.eye(n, dtype=bool)
        pairs = np.float64(n) * np.float64(n - 1)
        cl64[r] = np.where(act, m, 0.0).sum() / pairs
        sim64[r] = c[off].sum() / pairs
        nact[r] = int(act.sum())
        near[r] = np.abs(m[off]).min()
        H = hidden[r * lt:r * lt + n].astype(np.float64)
        u = np.zeros_like(H)
        for i in range(n):
            if qr[i] > 0.0:
                u[i] = H[i] / np.sqrt(qr[i])
        s = np.float64(dl) * np.float64(v[r]) * (2.0 / pairs)
        for i in range(n):
            if not qr[i] > 0.0:
                continue
            g = np.zeros(D)
            for j in range(n):
                if act[i, j]:
                    g = g + u[j]
            dh[r * lt + i] = s * (g - np.dot(g, u[i]) * u[i]) / np.sqrt(qr[i])
    cl, sim = cl64.astype(np.float32), sim64.astype(np.float32)
    total = np.float64(0.0)
    for r in range(R):
        total += np.float64(v[r]) * np.float64(cl[r])
    return dict(loss=np.float32(total), cl=cl, sim=sim, cl64=cl64, sim64=sim64, nact=nact, q=q, dh=dh, min_abs_m=near, m=mats, zero_rows=zero)


def cl_autograd(h, rho):
    """the caption's term written as the textbook formula under torch autograd: h (n, D) float64 → (cl, sim) float64 scalars, the mean
    over i ≠ j of max(0, ρ − 1 + cos(h_i, h_j)) and of the cosine; a zero row has cosine 0 with everything; n < 2: zeros"""
    n = h.shape[0]
    if n < 2:
        z = h.sum() * 0.0
        return z, z.detach()
    q = h.pow(2).sum(1)
    ok = q > 0
    norm = torch.where(ok, q, torch.ones_like(q)).sqrt()                       # (sqrt has no derivative at 0)
    u = torch.where(ok.unsqueeze(1), h / norm.unsqueeze(1), torch.zeros_like(h))
    c = u @ u.t()
    off = ~torch.eye(n, dtype=torch.bool)
    m = (float(rho) - 1.0) + c
    return torch.where(m > 0, m, torch.zeros_like(m))[off].mean(), c[off].mean().detach()


def per_caption_weights(lens, cl_weight):
    """``SimCTG.step``'s row weights from the captions' lengths: w = fp32(1 / max(1, Σ len)), v = fp32(cl_weight / max(1, the captions of
    at least two tokens)), formed in fp64 and rounded once"""
    lens = np.asarray(lens).reshape(-1)
    n = np.float64(max(1, int(lens.sum())))
    m = np.float64(max(1, int((lens >= 1).sum())))
    R = lens.shape[0]
    return np.full(R, np.float32(1.0 / n), np.float32), np.full(R, np.float32(np.float64(cl_weight) / m), np.float32)


def contrastive_loss(P, cfg, input_ids_list, video_features_list, input_masks_list, ingr_input_ids, ingr_sep_masks, batch_step_num,
                     ingr_id_dict, oov_word_dict, captions, weights, cl_weights, margin):
    """``scst_reference.sequence_loss``'s construction with ``dec`` exposed: ``P`` the oracle's parameter dict (leaves that require grad),
    ``captions`` per video (S_b, K, Lt) ids, ``weights`` / ``cl_weights`` per video (S_b, K) → (loss: a float64 torch scalar under
    autograd = −Σ w·cum over the captions not barred + Σ v·cl over all, cum / bars / cl / sim per video (S_b, K), min_abs_m: the smallest
    |m_ij| of the batch, and hidden: per video the (S_b·K, Lt, D) float32 decoder output)."""
    mode, Lv, Lt, V = cfg.model_mode, cfg.max_v_len, cfg.max_t_len, cfg.vocab_size
    rho = float(np.float32(margin))
    ingr_input_ids = torch.as_tensor(ingr_input_ids)
    ingr_sep_masks = torch.as_tensor(ingr_sep_masks)
    pe50 = orc.sinusoid_table(50, cfg.hidden_size)
    loss = torch.zeros((), dtype=torch.float64)
    cums, bars, cls, sims, hid = [], [], [], [], []
    near = np.inf
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
        dec = orc.decoder(P, orc.text_embed(P, fr.model_side(y, V), cfg), torch.ones(R, Lt), mem, torch.ones(mem.shape[:2]), cfg)
        hid.append(dec.detach().reshape(R, Lt, -1).numpy().astype(np.float32))
        if mode == "video":
            sc = orc.lm_head(P, dec, cfg)
        else:
            sc = orc.pointer_generator(P, dec, bank, ingr_id_dict[b], n_oov, cfg)
        sc = sc.reshape(R, Lt, -1)[:, :, :C].double()
        walk = fr.score_rows(sc.detach().numpy().astype(np.float32).reshape(R * Lt, -1), y, np.full(R, C), mode == "video", "bar")
        w = np.asarray(weights[b], np.float64).reshape(R)
        v = np.asarray(cl_weights[b], np.float64).reshape(R)
        h64 = dec.reshape(R, Lt, -1).double()
        cum_b, bar_b, cl_b, sim_b = [], [], [], []
        for c in range(R):
            n = int(walk["len"][c])
            cl, sim = cl_autograd(h64[c, :tokens(n, Lt)], rho)
            loss = loss + v[c] * cl
            cl_b.append(cl.detach()); sim_b.append(sim)
            near = min(near, float(seq_cl(hid[-1][c], [n], [0.0], rho, Lt)["min_abs_m"][0]))
            barred = not np.isfinite(walk["step"][c, :n]).all()
            bar_b.append(barred)
            if barred or n == 0:
                cum_b.append(torch.zeros((), dtype=torch.float64))
                continue
            rows = sc[c, :n]
            tgt = torch.as_tensor(y[c, 1:n + 1]).long()
            picked = rows.gather(1, tgt.unsqueeze(1)).squeeze(1)
            if mode == "video":
                keep = torch.arange(C) != UNK
                lp = picked - torch.logsumexp(rows[:, keep], 1)
            else:
                lp = torch.log(picked)
            cum = lp.sum()
            cum_b.append(cum)
            loss = loss - w[c] * cum
        cums.append(torch.stack([c_.detach() for c_ in cum_b]).reshape(S_b, K))
        bars.append(np.asarray(bar_b).reshape(S_b, K))
        cls.append(torch.stack(cl_b).reshape(S_b, K))
        sims.append(torch.stack(sim_b).reshape(S_b, K))
    return loss, cums, bars, cls, sims, near, hid
