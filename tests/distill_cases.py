"""The fixed inputs of the distillation tests, shared by tests/test_distill_gpu.py (which runs the kernels on them) and
tests/test_distill_host.py (which checks their margins without a GPU: no counted ℓ_c lies within ln 2 of log ε, and every entry built to
be clamped or unclamped is so in fp64).  Seeded numpy only."""
import numpy as np

from svpc_amd.synthetic import EOS, PAD, UNK
from unlikelihood_cases import captions

#        C,  Lt,  R      (R caption rows, no multiple of the 4 per workgroup)
KERNEL_SHAPES = [(7, 2, 1), (64, 22, 9), (65, 6, 7), (951, 22, 6), (1025, 6, 9), (4097, 6, 5)]
FLAGS = [(False, False), (False, True), (True, False), (True, True)]            # (student logits, teacher logits)
P_CLAMPED = (0.0, 2.0 ** -110, -0.5)           # student probabilities under ε = 2^-100 (or not positive): clamped
P_UNCLAMPED = 2.0 ** -90                       # log p = −62.4: 6.9 above log ε
Z_CLAMPED = -100.0                             # a student logit whose ℓ lies under −100 + (−lse) < log ε − ln 2 on an N(0, 3) row
Z_UNCLAMPED = -35.0                            # ℓ in (−35 − lse): above log ε + ln 2 while lse < 33
PAD_S, PAD_T = 3, 8                            # columns behind C in the student's and the teacher's matrix (ld_student != ld_teacher)


def kernel_case(C, Lt, R, logits, teacher_logits, seed=0):
    """→ a dict: scores (R·Lt, C + PAD_S) float32, tq (R·Lt, C + PAD_T) float32 — NaN behind C —, ids (R, Lt) int64, row_c (R,) mixed,
    w / v (R,) float32 of mixed signs with zeros, and the entries built to be clamped / unclamped as (r, i, column)"""
    rng = np.random.default_rng(104729 * C + 31 * Lt + 2 * R + int(logits) + 2 * int(teacher_logits) + 100003 * seed)
    n = R * Lt
    row_c = np.array([C if r % 3 == 0 else int(rng.integers(max(UNK + 1, C // 2), C + 1)) for r in range(R)])
    s = np.full((n, C + PAD_S), np.nan, np.float32)
    t = np.full((n, C + PAD_T), np.nan, np.float32)
    if logits:
        s[:, :C] = (rng.standard_normal((n, C)) * 3).astype(np.float32)
        s[:, UNK] = 50.0                                                   # UNK would dominate the softmax were it a candidate
    else:
        s[:, :C] = (rng.random((n, C)) ** 4 * 0.9 + 1e-3).astype(np.float32)
        s[:, UNK] = 1.0
    if teacher_logits:
        tl = (rng.standard_normal((n, C)) * 2).astype(np.float32)
        tl[rng.random((n, C)) < 0.1] = -np.inf                             # columns the teacher rules out
        tl[:, UNK] = 80.0                                                  # a huge value at UNK: ignored
        t[:, :C] = tl
    else:
        tp = rng.random((n, C)) ** 3
        tp = tp / tp.sum(1, keepdims=True) * rng.uniform(0.6, 1.1, size=(n, 1))   # not normalised: Q in 0.6 … 1.1
        tp[rng.random((n, C)) < 0.2] = 0.0                                 # exact zeros
        tp[rng.random((n, C)) < 0.05] = -0.25                              # negatives: q = 0
        tp[rng.random((n, C)) < 0.02] = 1e-42                              # fp32 denormals: counted
        tp[:, UNK] = 1e30                                                  # a huge value at UNK: ignored
        t[:, :C] = tp.astype(np.float32)
    ids = captions(rng, C, Lt, R, row_c)
    if R >= 5 and Lt >= 4:                                                 # one caption that is barred for certain: a non-candidate target
        ids[4, 1:] = PAD
        ids[4, 1:4] = [1, [UNK, int(row_c[4]), -7][(C + Lt) % 3], EOS]
    clamped, unclamped, dead = [], [], []
    for r in range(R):
        c = int(row_c[r])
        for i in range(Lt - 1):
            g = r * Lt + i
            y = int(ids[r, i + 1])
            if (r + i) % 5 == 2:                                           # a teacher row with no mass at all
                t[g, :C] = -np.inf if teacher_logits else 0.0
                dead.append((r, i))
                continue
            cols = [int(x) for x in rng.permutation(c) if int(x) not in (UNK, y)][:2]
            if len(cols) < 2:
                continue
            a, b = cols
            t[g, a] = 1.0 if teacher_logits else 0.05                      # both carry teacher mass
            t[g, b] = 0.5 if teacher_logits else 0.03
            if (r + i) % 2:
                s[g, a] = Z_CLAMPED if logits else P_CLAMPED[(r + i) // 2 % 3]
                clamped.append((r, i, a))
            s[g, b] = Z_UNCLAMPED if logits else P_UNCLAMPED
            unclamped.append((r, i, b))
    w = rng.standard_normal(R).astype(np.float32)
    v = rng.standard_normal(R).astype(np.float32)
    if R > 2:
        w[int(rng.integers(0, R))] = 0.0
        v[int(rng.integers(0, R))] = 0.0
    return dict(scores=s, tq=t, ids=ids, row_c=row_c, w=w, v=v, clamped=clamped, unclamped=unclamped, dead=dead, C=C, Lt=Lt, R=R,
                logits=logits, teacher_logits=teacher_logits)
