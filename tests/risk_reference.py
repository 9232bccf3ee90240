"""CPU restatement of minimum-risk (Shen et al. 2016) and ranking (BRIO, Liu et al. 2022) training over decoded candidate sets
(``svpc_amd.mrt``, ``ops.seq_risk``).  float64 numpy, plain loops; shares no code with the product.

The definition.  T sentences, K candidates per sentence, caption row r = t·K + k; the sentences of video b are t = vid_off[b] …
vid_off[b + 1] − 1; candidate paragraph k of a video is row k of each of its sentences.  cum / len / barred of a row are ``seq_nll``'s.
Per video b and candidate k, in float64:

- s = Σ_t cum[t, k] in sentence order, n = max(1, Σ_t len[t, k]), z = s / n^β — reported as 0 when a sentence of the candidate is barred;
- valid: no sentence barred and cost[b, k] finite; an invalid candidate has Q = 0, stands in no pair and has G = 0;
- Q = exp(α(z − max z)) / Σ_{valid k'} exp(α(z' − max z)), k' ascending; risk[b] = Σ_k Q·cost (0 when no candidate is valid);
- pos(k): the number of valid candidates before k in the order (cost ascending, k ascending);
- the pair (i, j) exists when cost_i < cost_j (strict: equal costs form no pair), its hinge argument is h = z_j − z_i + (pos(j) − pos(i))·λ,
  it is ACTIVE iff h > 0, and rank[b] = Σ_pairs max(0, h), j ascending inside i ascending;
- G[b, k] = ρ_risk·α·Q_k·(cost_k − risk[b]) + ρ_rank·(#active pairs with k as j − #active pairs with k as i), the difference cost_k − risk[b]
  formed as Σ_{valid k'} Q_k'·(cost_k − cost_k') (the same number since Σ Q = 1, and exactly 0 when the costs are equal);
- loss = fp32(−Σ_{r not barred} w_r·cum_r + (ρ_risk·Σ_b risk[b] + ρ_rank·Σ_b rank[b]) / N);
- ∂loss / ∂cum[t, k] = −w[t, k] + G[vid(t), k] / (N·n^β), so w_eff[t, k] = fp32(w[t, k] − G / (N·n^β)) and the gradient in the scores is
  ``seq_nll``'s under w_eff."""
import numpy as np


def groups(cum, length, barred, cost, vid_off, w, alpha, beta, margin, rho_risk, rho_rank):
    """``cum`` / ``length`` / ``barred`` / ``w`` (T·K,) or (T, K) (w None: zeros), ``cost`` (N, K) float64, ``vid_off`` (N + 1,) → a dict:
    risk / rank (N,), Q / z / G / n (N, K) float64, valid (N, K) int32, pos (N, K) (−1: invalid), pair (N, K, K) bool (i, j): the pair
    exists, hinge (N, K, K) float64 its argument (nan where there is no pair), active (N, K, K) bool, w_eff64 (T, K) float64, w_eff (T, K)
    float32, nll / total float64, loss float32."""
    cost = np.asarray(cost, np.float64)
    N, K = cost.shape
    cum = np.asarray(cum, np.float32).reshape(-1, K)
    T = cum.shape[0]
    length = np.asarray(length).reshape(T, K)
    barred = np.asarray(barred).reshape(T, K)
    w = np.zeros((T, K), np.float32) if w is None else np.asarray(w, np.float32).reshape(T, K)
    off = [int(o) for o in vid_off]
    assert len(off) == N + 1 and off[0] == 0 and off[-1] == T and all(a <= b for a, b in zip(off, off[1:]))
    risk, rank = np.zeros(N), np.zeros(N)
    Q, z, G, n = np.zeros((N, K)), np.zeros((N, K)), np.zeros((N, K)), np.ones((N, K))
    valid = np.zeros((N, K), np.int32)
    pos = np.full((N, K), -1)
    pair = np.zeros((N, K, K), bool)
    active = np.zeros((N, K, K), bool)
    hinge = np.full((N, K, K), np.nan)
    w_eff64 = w.astype(np.float64)
    with np.errstate(all="ignore"):
        for b in range(N):
            bar = np.zeros(K, bool)
            for k in range(K):
                s, words = np.float64(0.0), 0
                for t in range(off[b], off[b + 1]):
                    s = s + np.float64(cum[t, k])
                    words += int(length[t, k])
                    bar[k] |= bool(barred[t, k])
                n[b, k] = np.float64(max(1, words)) ** np.float64(beta)
                z[b, k] = 0.0 if bar[k] else s / n[b, k]
                valid[b, k] = int(not bar[k] and np.isfinite(cost[b, k]))
            ks = [k for k in range(K) if valid[b, k]]
            if ks:
                zmax = max(z[b, k] for k in ks)
                den = np.float64(0.0)
                for k in ks:
                    den = den + np.exp(np.float64(alpha) * (z[b, k] - zmax))
                for k in ks:
                    Q[b, k] = np.exp(np.float64(alpha) * (z[b, k] - zmax)) / den
                    risk[b] = risk[b] + Q[b, k] * cost[b, k]
            for k in ks:
                pos[b, k] = sum(1 for j in ks if cost[b, j] < cost[b, k] or (cost[b, j] == cost[b, k] and j < k))
            as_i, as_j = np.zeros(K), np.zeros(K)
            for i in ks:
                for j in ks:
                    if cost[b, i] < cost[b, j]:
                        pair[b, i, j] = True
                        h = z[b, j] - z[b, i] + np.float64(pos[b, j] - pos[b, i]) * np.float64(margin)
                        hinge[b, i, j] = h
                        if h > 0:
                            active[b, i, j] = True
                            rank[b] = rank[b] + h
                            as_i[i] += 1
                            as_j[j] += 1
            for k in ks:
                dev = np.float64(0.0)
                for j in ks:
                    dev = dev + Q[b, j] * (cost[b, k] - cost[b, j])
                G[b, k] = np.float64(rho_risk) * np.float64(alpha) * Q[b, k] * dev + np.float64(rho_rank) * (as_j[k] - as_i[k])
            for t in range(off[b], off[b + 1]):
                for k in range(K):
                    w_eff64[t, k] = np.float64(w[t, k]) - G[b, k] / (np.float64(N) * n[b, k])
    nll = np.float64(0.0)
    for t in range(T):
        for k in range(K):
            if not barred[t, k]:
                nll += np.float64(w[t, k]) * np.float64(cum[t, k])
    total = -nll
    if N and (rho_risk != 0 or rho_rank != 0):
        total = total + (np.float64(rho_risk) * risk.sum() + np.float64(rho_rank) * rank.sum()) / np.float64(N)
    return dict(risk=risk, rank=rank, Q=Q, z=z, G=G, n=n, valid=valid, pos=pos, pair=pair, hinge=hinge, active=active, w_eff64=w_eff64,
                w_eff=w_eff64.astype(np.float32), nll=nll, total=total, loss=np.float32(total))


def min_hinge_distance(r):
    """the smallest |hinge argument| over the pairs of a ``groups`` result (inf: no pair): a pair this close to 0 could flip between two
    correct fp64 evaluations"""
    h = r["hinge"][r["pair"]]
    return float(np.abs(h).min()) if h.size else float("inf")


def rank_conditioning(r):
    """the smallest rank[b] / (A_b·max_k |z[b, k]|) over the videos with A_b > 0 active pairs (inf: none).  A hinge argument is a
    DIFFERENCE of two z: two correct float64 evaluations of z (the power n^β is not correctly rounded everywhere) differ by about an ulp,
    2⁻⁵²·|z|, so rank[b] carries an absolute error of about 4·2⁻⁵²·A_b·max|z| ≈ 1e-15·A_b·max|z|, whatever its own size.  A relative bound of
    1e-12 on rank[b] is therefore meaningful only for inputs with rank[b] ≥ 1e-3·A_b·max|z|: the tests assert that of their inputs."""
    worst = float("inf")
    for b in range(r["rank"].shape[0]):
        A = int(r["active"][b].sum())
        if A:
            zs = np.abs(r["z"][b][r["valid"][b] == 1]).max()
            if zs > 0:
                worst = min(worst, float(r["rank"][b] / (A * zs)))
    return worst


def objective_torch(cum, length, barred, cost, vid_off, w, alpha, beta, margin, rho_risk, rho_rank):
    """the written objective as a float64 torch expression of ``cum`` (T, K), a leaf that requires grad → the loss before rounding; the
    validity, the order and the pair set are data (no gradient flows through them), everything else is differentiated by autograd"""
    import torch
    cost = np.asarray(cost, np.float64)
    N, K = cost.shape
    T = cum.shape[0]
    length = np.asarray(length).reshape(T, K)
    barred = np.asarray(barred).reshape(T, K)
    w = np.zeros((T, K)) if w is None else np.asarray(w, np.float64).reshape(T, K)
    off = [int(o) for o in vid_off]
    total = torch.zeros((), dtype=torch.float64)
    for t in range(T):
        for k in range(K):
            if not barred[t, k]:
                total = total - float(w[t, k]) * cum[t, k]
    for b in range(N):
        rows = range(off[b], off[b + 1])
        ks = [k for k in range(K) if np.isfinite(cost[b, k]) and not any(barred[t, k] for t in rows)]
        if not ks:
            continue
        zs = []
        for k in ks:
            s = torch.zeros((), dtype=torch.float64)
            for t in rows:
                s = s + cum[t, k]
            zs.append(s / float(max(1, sum(int(length[t, k]) for t in rows))) ** float(beta))
        zv = torch.stack(zs)
        c = torch.tensor([cost[b, k] for k in ks], dtype=torch.float64)
        q = torch.softmax(float(alpha) * zv, 0)
        total = total + float(rho_risk) * (q * c).sum() / N
        order = sorted(range(len(ks)), key=lambda a: (cost[b, ks[a]], ks[a]))
        p = {a: i for i, a in enumerate(order)}
        for i in range(len(ks)):
            for j in range(len(ks)):
                if c[i] < c[j]:
                    total = total + float(rho_rank) * torch.clamp(zv[j] - zv[i] + (p[j] - p[i]) * float(margin), min=0.0) / N
    return total
