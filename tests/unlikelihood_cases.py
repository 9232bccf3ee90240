"""The fixed inputs of the unlikelihood tests, shared by tests/test_unlikelihood_gpu.py (which runs the kernels on them) and
tests/test_unlikelihood_host.py (which checks their margins without a GPU: no counted 1 − p lies in [ε/2, 2ε], and every entry built to
be clamped, or to sit just outside the clamp, is so in fp64).  Seeded numpy only."""
import numpy as np

from svpc_amd.synthetic import BOS, EOS, IGNORE, PAD, UNK

EPS = 1e-5
#        C,  Lt,  T,  K      (R = T·K caption rows, no multiple of the 4 per workgroup but for the one-row case; M = Lt − 1, 64 at Lt = 65)
KERNEL_SHAPES = [(7, 2, 1, 1), (64, 22, 3, 3), (65, 6, 7, 1), (951, 22, 3, 2), (1025, 6, 3, 3), (4097, 6, 5, 1), (65, 65, 3, 1)]
P_CLAMPED = (1.0, 1.0 - 2.0 ** -20)            # probabilities whose 1 − p is 0 and 9.5e-7: clamped
P_NEAR = 1.0 - 2.0 ** -10                      # 1 − p = 9.8e-4: not clamped, a gradient of 1024·u
Z_CLAMPED = 40.0                               # a logit that leaves the rest of an N(0, 3) row less than e^-25 of the softmax


def captions(rng, C, Lt, R, row_c):
    """caption rows as tests/test_scst_gpu.py builds them: rows that never end, end at position 1, are all PAD, stop at IGNORE, end at EOS,
    and rows with a non-candidate target (UNK, C_r, below 0, above C_r) before the end; words drawn from few columns so that they repeat"""
    ids = np.zeros((R, Lt), np.int64)
    ids[:, 0] = BOS
    for r in range(R):
        c = int(row_c[r])
        pool = [int(v) for v in rng.integers(0, c, size=4) if v not in (EOS, PAD, UNK)] + [1, c - 1 if c - 1 != UNK else 2]
        words = np.array([pool[int(j)] for j in rng.integers(0, len(pool), size=Lt - 1)])
        kind = r % 6
        n = int(rng.integers(0, Lt - 1))                                   # words before the end
        if kind == 0:
            row = list(words)                                              # never ends
        elif kind == 1:
            row = [EOS] + [PAD] * (Lt - 2)                                 # ends at position 1
        elif kind == 2:
            row = [PAD] * (Lt - 1)                                         # all PAD
        elif kind == 3:
            row = list(words[:n]) + [IGNORE] * (Lt - 1 - n)
        else:
            row = list(words[:n]) + [EOS] + [PAD] * (Lt - 2 - n)
            if n and kind == 5:                                            # a non-candidate target somewhere before the end: barred
                row[int(rng.integers(0, n))] = [UNK, c, -7, c + 3][int(rng.integers(0, 4))]
        ids[r, 1:] = row[:Lt - 1]
    return ids


def kernel_case(C, Lt, R, logits, seed=0):
    """→ a dict: scores (R·Lt, C) float32, ids (R, Lt) int64, row_c (R,), neg (R, Lt − 1, M) int32, w / u (R,) float32, and the listings
    built to be clamped (``clamped``) or to sit just outside the clamp (``near``; probabilities only) as (r, i, column)"""
    rng = np.random.default_rng(7919 * C + 31 * Lt + 2 * R + int(logits) + 100003 * seed)
    M = min(Lt - 1, 64)
    row_c = np.array([C if r % 3 == 0 else int(rng.integers(max(UNK + 1, C // 2), C + 1)) for r in range(R)])
    if logits:
        s = (rng.standard_normal((R * Lt, C)) * 3).astype(np.float32)
        s[:, UNK] = 50.0                                                   # UNK would dominate the softmax were it a candidate
    else:
        s = (rng.random((R * Lt, C)) ** 4 * 0.9 + 1e-3).astype(np.float32)
        s[:, UNK] = 1.0
    ids = captions(rng, C, Lt, R, row_c)
    neg = np.full((R, Lt - 1, M), -1, np.int32)
    clamped, near = [], []
    for r in range(R):
        c = int(row_c[r])
        for i in range(Lt - 1):
            y = int(ids[r, i + 1])
            lst = [int(v) for v in rng.integers(0, c, size=M)]
            special = [-1, UNK, c, c + 2, y, -3]                           # none, UNK, from C_r up, the target itself, below 0
            for j in range(M):
                roll = int(rng.integers(0, 8))
                if roll < len(special) and (r + i + j) % 2:
                    lst[j] = special[roll]
            if M >= 3:
                lst[2] = lst[0]                                            # a column listed twice
            if M == 1:
                lst[0] = [1, y, UNK, -1, c][(r + i) % 5]
            neg[r, i] = lst
            live = [v for v in lst if 0 <= v < c and v != UNK and v != y]
            if live and (r + i) % 4 == 1:                                  # a clamped listing
                col = live[0]
                s[r * Lt + i, col] = Z_CLAMPED if logits else P_CLAMPED[(r + i) % 8 // 4]
                clamped.append((r, i, col))
            elif live and (r + i) % 4 == 3 and not logits:
                col = live[-1]
                s[r * Lt + i, col] = P_NEAR
                near.append((r, i, col))
    w = rng.standard_normal(R).astype(np.float32)
    u = rng.standard_normal(R).astype(np.float32)
    if R > 2:
        w[int(rng.integers(0, R))] = 0.0
        u[int(rng.integers(0, R))] = 0.0
    return dict(scores=s, ids=ids, row_c=row_c, neg=neg, w=w, u=u, clamped=clamped, near=near, C=C, Lt=Lt, R=R, M=M, logits=logits)


#          Lt, K, the videos' sentence counts
NEGATIVE_SHAPES = [(2, 1, [1]), (6, 1, [2, 1]), (6, 3, [1, 2, 12]), (22, 1, [12, 2]), (22, 3, [2, 12, 1]), (65, 1, [2, 1]), (65, 3, [12])]


def negatives_case(Lt, K, steps, seed=0):
    """→ ids (T·K, Lt) int64, row_c (T·K,), sent_first (T,): few distinct words, so that they repeat inside and across the captions of a
    video; the same candidate row of two sentences sometimes shares a whole caption"""
    rng = np.random.default_rng(1009 * Lt + 17 * K + len(steps) + 100003 * seed)
    T = sum(steps)
    R = T * K
    C = 12
    row_c = np.array([C - (r % 3) for r in range(R)])                      # 12, 11, 10: column 10 / 11 is from C_r up on some rows
    ids = captions(rng, 9, Lt, R, np.full(R, 9))
    for r in range(R):
        if r % 5 == 0 and Lt > 4 and not {int(ids[r, 1]), int(ids[r, 2])} & {PAD, IGNORE, EOS}:
            ids[r, 2] = [UNK, 11, 10][r % 3]                               # a word that is UNK or from C_r up, inside grams
        if r >= 2 * K and r % 4 == 1:
            ids[r] = ids[r - 2 * K]                                        # the caption of the same candidate row two sentences earlier
    sent_first, o = [], 0
    for s in steps:
        sent_first += [o] * s
        o += s
    return ids, row_c, sent_first
