"""The fixed inputs of the minimum-risk / ranking tests, shared by tests/test_risk_host.py (which checks their margins on
the CPU) and tests/test_risk_gpu.py (which runs the kernels on them)."""
import numpy as np

from svpc_amd.synthetic import BOS, EOS, PAD, UNK

HINGE_MARGIN = 1e-9             # no hinge argument of a seeded input may lie this close to 0: the active set could flip
RANK_CONDITION = 1e-3           # rank[b] >= this times (active pairs · max |z|) in every video (risk_reference.rank_conditioning)

#          C,  Lt, K,  sentence counts,   logits, wide stride, beta, alpha, margin
KERNEL_CASES = [
    (7, 2, 1, [1], False, False, 0.0, 5e-3, 1e-3),
    (7, 2, 1, [1], True, False, 0.6, 2.0, 1e-3),
    (65, 6, 2, [3, 1, 2], False, True, 0.6, 5e-3, 1e-3),
    (65, 6, 3, [3, 1, 2], True, False, 0.0, 2.0, 0.5),
    (65, 22, 16, [3, 1, 2], False, False, 0.6, 2.0, 0.25),
    (1025, 6, 3, [3, 1, 2], True, True, 0.6, 0.0, 1e-3),
    (1025, 22, 2, [20], False, False, 0.0, 2.0, 1e-3),
    (65, 6, 16, [20], True, False, 0.6, 5e-3, 0.5),
    (7, 6, 3, [2] * 70, False, False, 0.6, 2.0, 0.25),
    (65, 2, 3, [2] * 70, True, True, 0.0, 5e-3, 1e-3),
    (1025, 22, 1, [3, 0, 2], True, False, 0.6, 2.0, 1e-3),
    (65, 22, 3, [3, 1, 2], False, False, 0.0, 40.0, 1e-3),       # α·z spreads over more than 700: the max-subtraction must hold
]


def costs(rng, N, K):
    """(N, K) float64 costs in [−3, 0) (the negative of a reward); K ≥ 2: candidates 0 and 1 of every odd video tie; K ≥ 3: the last
    candidate of video 1 costs +inf and candidate 0 of video 2 nan"""
    c = -3.0 * rng.random((N, K))
    if K >= 2:
        for b in range(1, N, 2):
            c[b, 1] = c[b, 0]
    if K >= 3 and N >= 2:
        c[1, K - 1] = np.inf
    if K >= 3 and N >= 3:
        c[2, 0] = np.nan
    return c


def vid_off(steps):
    off = [0]
    for s in steps:
        off.append(off[-1] + int(s))
    return off


def group_case(seed, steps, K):
    """cum-level inputs: cum (T, K) float32 < 0, len (T, K), barred (T, K) — K ≥ 3: candidate 1 of video 0 barred in one sentence; from
    two videos up: every candidate of the last video barred —, cost (N, K), w (T, K) float32 with negative and zero entries"""
    rng = np.random.default_rng(seed)
    N, T = len(steps), sum(steps)
    length = rng.integers(1, 9, size=(T, K))
    cum = (-rng.random((T, K)) * length * 2.0).astype(np.float32)
    barred = np.zeros((T, K), np.int32)
    off = vid_off(steps)
    if K >= 3 and steps[0] >= 1:
        barred[off[0] + steps[0] - 1, 1] = 1
    if N >= 2 and steps[-1] >= 1:
        barred[off[-2], :] = 1
    cum[barred == 1] = -np.inf
    w = rng.standard_normal((T, K)).astype(np.float32) * 0.1
    w[rng.integers(0, T), rng.integers(0, K)] = 0.0
    return dict(cum=cum, length=length, barred=barred, cost=costs(rng, N, K), w=w, vid_off=off)


def score_case(seed, C, Lt, K, steps, logits, wide):
    """kernel-level inputs: score rows (R·Lt, ld) float32 (ld = C + 5 under ``wide``), captions (R, Lt) int64, mixed column counts, weights
    with negative and zero entries, costs.  Row kinds by caption row: most end with EOS after 0 … Lt − 2 words, some never end; K ≥ 3: candidate 1
    of video 0 has a UNK target (barred: the candidate is invalid); from two videos up: every candidate of the last video has one (a
    video with no valid candidate)."""
    rng = np.random.default_rng(seed)
    N, T = len(steps), sum(steps)
    R = T * K
    ld = C + 5 if wide else C
    row_c = np.array([C if r % 3 == 0 else int(rng.integers(max(UNK + 1, C // 2), C + 1)) for r in range(R)])
    if logits:
        s = (rng.standard_normal((R * Lt, ld)) * 3).astype(np.float32)
        s[:, UNK] = 50.0
    else:
        s = (rng.random((R * Lt, ld)) ** 4 + 1e-3).astype(np.float32)
        s[:, UNK] = 1.0
    ids = np.zeros((R, Lt), np.int64)
    ids[:, 0] = BOS
    off = vid_off(steps)
    for r in range(R):
        c = int(row_c[r])
        words = rng.integers(0, c, size=Lt - 1)
        words[(words == EOS) | (words == PAD) | (words == UNK)] = 1
        n = int(rng.integers(0, Lt - 1))
        if r % 5 == 0:
            row = list(words)                                              # never ends
        else:
            row = list(words[:n]) + [EOS] + [PAD] * (Lt - 2 - n)
        ids[r, 1:] = row[:Lt - 1]
    bar_rows = []
    if K >= 3 and steps[0] >= 1:
        bar_rows.append((off[0] + steps[0] - 1) * K + 1)
    if N >= 2 and steps[-1] >= 1:
        bar_rows += [off[-2] * K + k for k in range(K)]
    for r in bar_rows:
        ids[r, 1] = UNK
    w = (rng.standard_normal(R) * 0.1).astype(np.float32)
    w[rng.integers(0, R)] = 0.0
    return dict(scores=s, ids=ids, row_c=row_c, w=w, cost=costs(rng, N, K), vid_off=off, bar_rows=bar_rows, ld=ld)
