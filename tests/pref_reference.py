"""CPU restatement of preference optimisation over decoded candidate sets (``svpc_amd.prefopt``, ``ops.seq_pref``): DPO
(Rafailov et al. 2023), cDPO (Mitchell 2023), IPO (Azar et al. 2023), SLiC's hinge (Zhao et al. 2023) and SimPO (Meng et al. 2024).
float64 numpy, plain loops; shares no code with the product.

The definition.  T sentences, 1 ≤ K ≤ 16 candidates per sentence, caption row r = t·K + k; the sentences of video b are t = vid_off[b] …
vid_off[b + 1] − 1; candidate paragraph k of a video is row k of each of its sentences.  cum / len / barred of a row are ``seq_nll``'s;
ref_cum is the reference model's cum of the same captions, or absent (reference-free: all zero).  Per video b, in float64:

- s[b, k] = Σ_t cum[t, k] and s_ref[b, k] = Σ_t ref_cum[t, k] in sentence order, n[b, k] = max(1, Σ_t len[t, k]);
- valid: no sentence barred, every ref_cum of the candidate's sentences finite, cost[b, k] finite; an invalid candidate stands in no pair
  and has G = 0;
- u[b, k] = (s − s_ref) / n^length_beta — reported as 0 for an invalid candidate;
- pos(k): the number of valid candidates before k in the order (cost ascending, k ascending);
- pairs "all": every (i, j) of valid candidates with cost_i < cost_j (strict: equal costs form no pair); "extremes": the first and the
  last valid candidate of the order, if their costs differ; P_b the number of pairs;
- d = u_i − u_j, h = β·d − γ; ℓ = −(1 − ε)·ln σ(h) − ε·ln σ(−h) with ln σ(x) = min(x, 0) − log1p(exp(−|x|)) (sigmoid), max(0, 1 − h)
  (hinge) or (d − 1 / (2β))² (ipo); D = ∂ℓ / ∂d = β·(−(1 − ε)·σ(−h) + ε·σ(h)), −β or 0, 2·(d − 1 / (2β));
- pref[b] = (1 / P_b)·Σ_i Σ_j ℓ — per i the sum over j ascending, then the sums over i ascending —, 0 when P_b = 0;
- G[b, k] = (ρ / P_b)·(Σ_{pairs with k as i} D − Σ_{pairs with k as j} D);
- loss = fp32(−Σ_{r not barred} w_r·cum_r + ρ·Σ_b pref[b] / N); with ρ = 0 the group term is not added at all;
- ∂loss / ∂cum[t, k] = −w[t, k] + G[vid(t), k] / (N·n^length_beta), so w_eff[t, k] = fp32(w[t, k] − G / (N·n^length_beta)) and the gradient
  in the scores is ``seq_nll``'s under w_eff;
- reward = β·u, n_correct = the pairs with d > 0, margin = the mean of β·d over the pairs (0 with none)."""
import numpy as np

LOSS_TYPES = ("sigmoid", "hinge", "ipo")
PAIRS = ("all", "extremes")


def _lnsig(x):
    return min(x, 0.0) - np.log1p(np.exp(-abs(x)))


def _sig(x):
    e = np.exp(-abs(x))
    return 1.0 / (1.0 + e) if x >= 0 else e / (1.0 + e)


def pair_loss(d, beta, gamma, eps, loss_type):
    """→ (ℓ, D = ∂ℓ / ∂d, h) of one pair"""
    d, beta = np.float64(d), np.float64(beta)
    h = beta * d - np.float64(gamma)
    if loss_type == "sigmoid":
        return -(1.0 - eps) * _lnsig(h) - eps * _lnsig(-h), beta * (-(1.0 - eps) * _sig(-h) + eps * _sig(h)), h
    if loss_type == "hinge":
        a = 1.0 - h
        return (a, -beta, h) if a > 0 else (np.float64(0.0), np.float64(0.0), h)
    a = d - 1.0 / (2.0 * beta)
    return a * a, 2.0 * a, h


def groups(cum, length, barred, cost, vid_off, w, ref_cum, beta, gamma, eps, length_beta, rho, loss_type, pairs):
    """``cum`` / ``length`` / ``barred`` / ``w`` / ``ref_cum`` (T·K,) or (T, K) (w None: zeros; ref_cum None: no reference), ``cost``
    (N, K) float64, ``vid_off`` (N + 1,) → a dict: pref / margin (N,), u / reward / G / n (N, K) float64, valid (N, K) int32, n_pairs /
    n_correct (N,) int32, pos (N, K) (−1: invalid), pair (N, K, K) bool (i, j): the pair exists, d / h (N, K, K) float64 (nan where there
    is no pair), w_eff64 (T, K) float64, w_eff (T, K) float32, nll / total float64, loss float32."""
    assert loss_type in LOSS_TYPES and pairs in PAIRS and beta > 0 and gamma >= 0 and 0 <= eps < 0.5 and length_beta >= 0 and rho >= 0
    assert (eps == 0 or loss_type == "sigmoid") and (gamma == 0 or loss_type != "ipo")
    cost = np.asarray(cost, np.float64)
    N, K = cost.shape
    cum = np.asarray(cum, np.float32).reshape(-1, K)
    T = cum.shape[0]
    length = np.asarray(length).reshape(T, K)
    barred = np.asarray(barred).reshape(T, K)
    w = np.zeros((T, K), np.float32) if w is None else np.asarray(w, np.float32).reshape(T, K)
    ref = None if ref_cum is None else np.asarray(ref_cum, np.float32).reshape(T, K)
    off = [int(o) for o in vid_off]
    assert len(off) == N + 1 and off[0] == 0 and off[-1] == T and all(a <= b for a, b in zip(off, off[1:]))
    pref, margin = np.zeros(N), np.zeros(N)
    u, G, n = np.zeros((N, K)), np.zeros((N, K)), np.ones((N, K))
    valid = np.zeros((N, K), np.int32)
    n_pairs, n_correct = np.zeros(N, np.int32), np.zeros(N, np.int32)
    pos = np.full((N, K), -1)
    pair = np.zeros((N, K, K), bool)
    dd = np.full((N, K, K), np.nan)
    hh = np.full((N, K, K), np.nan)
    w_eff64 = w.astype(np.float64)
    with np.errstate(all="ignore"):
        for b in range(N):
            for k in range(K):
                s, sr, words, bad = np.float64(0.0), np.float64(0.0), 0, False
                for t in range(off[b], off[b + 1]):
                    s = s + np.float64(cum[t, k])
                    words += int(length[t, k])
                    bad |= bool(barred[t, k])
                    if ref is not None:
                        sr = sr + np.float64(ref[t, k])
                        bad |= not np.isfinite(ref[t, k])
                n[b, k] = np.float64(max(1, words)) ** np.float64(length_beta)
                valid[b, k] = int(not bad and np.isfinite(cost[b, k]))
                u[b, k] = (s - sr) / n[b, k] if valid[b, k] else 0.0
            ks = [k for k in range(K) if valid[b, k]]
            for k in ks:
                pos[b, k] = sum(1 for j in ks if cost[b, j] < cost[b, k] or (cost[b, j] == cost[b, k] and j < k))
            for i in ks:
                for j in ks:
                    if cost[b, i] < cost[b, j] and (pairs == "all" or (pos[b, i] == 0 and pos[b, j] == len(ks) - 1)):
                        pair[b, i, j] = True
            P = int(pair[b].sum())
            n_pairs[b] = P
            if not P:
                continue
            total, msum = np.float64(0.0), np.float64(0.0)
            Dsum = np.zeros(K)
            for i in ks:
                li, mi = np.float64(0.0), np.float64(0.0)
                for j in ks:
                    if pair[b, i, j]:
                        d = u[b, i] - u[b, j]
                        l, D, h = pair_loss(d, beta, gamma, eps, loss_type)
                        dd[b, i, j], hh[b, i, j] = d, h
                        li = li + l
                        mi = mi + np.float64(beta) * d
                        n_correct[b] += int(d > 0)
                        Dsum[i] += D
                        Dsum[j] -= D
                total = total + li
                msum = msum + mi
            pref[b] = total / P
            margin[b] = msum / P
            for k in ks:
                G[b, k] = (np.float64(rho) / P) * Dsum[k]
            for t in range(off[b], off[b + 1]):
                for k in range(K):
                    w_eff64[t, k] = np.float64(w[t, k]) - G[b, k] / (np.float64(N) * n[b, k])
    nll = np.float64(0.0)
    for t in range(T):
        for k in range(K):
            if not barred[t, k]:
                nll += np.float64(w[t, k]) * np.float64(cum[t, k])
    total = -nll
    if N and rho != 0:
        total = total + np.float64(rho) * pref.sum() / np.float64(N)
    return dict(pref=pref, margin=margin, u=u, reward=np.float64(beta) * u, G=G, n=n, valid=valid, n_pairs=n_pairs, n_correct=n_correct, pos=pos,
                pair=pair, d=dd, h=hh, w_eff64=w_eff64, w_eff=w_eff64.astype(np.float32), nll=nll, total=total, loss=np.float32(total))


# ------------------------------------------------------------------------------------------------ conditions on test inputs
def min_hinge_distance(r):
    """the smallest |1 − h| over the pairs of a ``groups`` result (inf: no pair): a hinge argument this close to 0 could flip the active
    set between two correct fp64 evaluations"""
    h = r["h"][r["pair"]]
    return float(np.abs(1.0 - h).min()) if h.size else float("inf")


def min_d_distance(r):
    """the smallest |d| over the pairs (inf: no pair): a d this close to 0 could flip ``n_correct``"""
    d = r["d"][r["pair"]]
    return float(np.abs(d).min()) if d.size else float("inf")


def pref_conditioning(r, beta):
    """the smallest pref[b] / (β·max_k |u[b, k]| + 1) over the videos with a pair (inf: none).  A hinge or ipo pair loss is a DIFFERENCE of
    two u (against 1 + γ, or 1 / (2β)): two correct float64 evaluations of u differ by about an ulp, 2⁻⁵²·|u|, so pref[b] carries an absolute
    error of about 4·2⁻⁵²·(β·max|u| + 1), whatever its own size.  A relative bound of 1e-12 on pref[b] is therefore meaningful only for inputs
    with pref[b] ≥ 1e-3·(β·max|u| + 1): the tests assert that of their hinge and ipo inputs (§11.18's ``rank_conditioning`` argument)."""
    worst = float("inf")
    for b in range(r["pref"].shape[0]):
        if r["n_pairs"][b]:
            us = np.abs(r["u"][b][r["valid"][b] == 1]).max()
            worst = min(worst, float(r["pref"][b] / (beta * us + 1.0)))
    return worst


# ------------------------------------------------------------------------------------------------ the written objective, for autograd
def objective_torch(cum, length, barred, cost, vid_off, w, ref_cum, beta, gamma, eps, length_beta, rho, loss_type, pairs):
    """the written objective as a float64 torch expression of ``cum`` (T, K), a leaf that requires grad → the loss before rounding; the
    validity, the order and the pair set are data (no gradient flows through them), everything else is differentiated by autograd"""
    import torch
    import torch.nn.functional as F
    cost = np.asarray(cost, np.float64)
    N, K = cost.shape
    T = cum.shape[0]
    length = np.asarray(length).reshape(T, K)
    barred = np.asarray(barred).reshape(T, K)
    w = np.zeros((T, K)) if w is None else np.asarray(w, np.float64).reshape(T, K)
    ref = np.zeros((T, K)) if ref_cum is None else np.asarray(ref_cum, np.float64).reshape(T, K)
    off = [int(o) for o in vid_off]
    total = torch.zeros((), dtype=torch.float64)
    for t in range(T):
        for k in range(K):
            if not barred[t, k]:
                total = total - float(w[t, k]) * cum[t, k]
    for b in range(N):
        rows = range(off[b], off[b + 1])
        ks = [k for k in range(K) if np.isfinite(cost[b, k]) and not any(barred[t, k] or not np.isfinite(ref[t, k]) for t in rows)]
        if not ks:
            continue
        us = {}
        for k in ks:
            s = torch.zeros((), dtype=torch.float64)
            for t in rows:
                s = s + cum[t, k] - float(ref[t, k])
            us[k] = s / float(max(1, sum(int(length[t, k]) for t in rows))) ** float(length_beta)
        order = sorted(ks, key=lambda k: (cost[b, k], k))
        if pairs == "all":
            ps = [(i, j) for i in ks for j in ks if cost[b, i] < cost[b, j]]
        else:
            ps = [(order[0], order[-1])] if cost[b, order[0]] < cost[b, order[-1]] else []
        if not ps:
            continue
        acc = torch.zeros((), dtype=torch.float64)
        for i, j in ps:
            d = us[i] - us[j]
            h = float(beta) * d - float(gamma)
            if loss_type == "sigmoid":
                acc = acc - (1.0 - float(eps)) * F.logsigmoid(h) - float(eps) * F.logsigmoid(-h)
            elif loss_type == "hinge":
                acc = acc + torch.clamp(1.0 - h, min=0.0)
            else:
                acc = acc + (d - 1.0 / (2.0 * float(beta))) ** 2
        total = total + float(rho) * acc / len(ps) / N
    return total
