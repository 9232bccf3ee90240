"""The fixed inputs of the policy-gradient tests, shared by tests/test_pg_host.py (which checks their conditions on the CPU)
and tests/test_pg_gpu.py (which runs the kernels on them).  The score rows, captions and weights are built as tests/risk_cases.py builds
them (the same special rows: a barred candidate, a video with no valid candidate); this file adds the advantages (with nan, ±inf and exact
zeros), the behaviour policy's and the reference model's step scores — the case's own float64 step rounded to float32 plus seeded offsets —
and the settings."""
import numpy as np

import scst_reference as sr
from risk_cases import score_case as _risk_score_case, vid_off  # noqa: F401

BOUND_MARGIN = 1e-5             # no ρ of a seeded input may lie this close (relative) to a bound that can switch it, but the ρ set ON one

#   seed,  C,  Lt, K, sentence counts, logits, wide stride, old_step, ref_step, norm, clip_lo, clip_hi, dual_clip, kl_beta
KERNEL_CASES = [
    (300, 7, 2, 1, [1], False, False, True, True, "sequence", 0.2, 0.2, 0.0, 0.04),
    (301, 7, 2, 1, [1], True, False, False, False, "none", 0.2, 0.28, 0.0, 0.0),
    (302, 65, 6, 2, [3, 1, 2], False, True, True, True, "token", 0.2, 0.28, 0.0, 0.04),              # DAPO's clip and norm, with a KL
    (303, 65, 6, 3, [3, 1, 2], True, False, True, False, "sequence", 0.0, 0.0, 3.0, 0.0),            # a ρ exactly on both bounds
    (304, 65, 22, 16, [3, 1, 2], False, False, True, True, "sequence", 0.2, 0.2, 3.0, 0.04),         # GRPO with dual clip
    (305, 1025, 6, 3, [3, 1, 2], True, True, False, True, "none", 0.2, 0.2, 0.0, 0.04),              # on-policy with a KL
    (306, 1025, 22, 2, [20], False, False, True, True, "token", 0.2, 0.2, 3.0, 0.0),
    (307, 65, 6, 16, [20], True, False, True, False, "token", 0.2, 0.28, 0.0, 0.0),                  # DAPO
    (308, 7, 6, 3, [2] * 70, False, False, True, True, "sequence", 0.2, 0.2, 3.0, 0.04),
    (309, 65, 2, 3, [2] * 70, True, True, True, False, "none", 0.0, 0.0, 0.0, 0.0),                  # Dr. GRPO's norm, clip 0 / 0
    (310, 1025, 22, 1, [3, 0, 2], True, False, True, True, "sequence", 0.2, 0.28, 3.0, 0.04),
    (311, 65, 22, 3, [3, 0, 2], False, False, False, False, "sequence", 0.2, 0.2, 0.0, 0.0),         # neither: REINFORCE per position
]

# every case also runs under these (norm, clip_lo, clip_hi, dual_clip, kl_beta — 0 where the case has no ref_step)
ALT_SETTINGS = [("sequence", 0.2, 0.2, 0.0, 0.0), ("token", 0.2, 0.28, 3.0, 0.04), ("none", 0.0, 0.0, 3.0, 0.04)]


def advantages(rng, N, K):
    """(N, K) float64 advantages of both signs; K ≥ 2: candidate K − 1 of every third video is exactly 0; K ≥ 3: the last candidate of
    video 1 is −inf and candidate 0 of video 2 nan; K = 1: the only candidate of video 1 (if any) is exactly 0"""
    a = rng.standard_normal((N, K))
    for b in range(0, N, 3):
        if K >= 2:
            a[b, K - 1] = 0.0
    if K == 1 and N >= 2:
        a[1, 0] = 0.0
    if K >= 3 and N >= 2:
        a[1, K - 1] = -np.inf
    if K >= 3 and N >= 3:
        a[2, 0] = np.nan
    return a


def _offsets(rng, shape):
    """what is added to the own step: mostly a normal draw of 0.25 (ρ = exp(−offset) between about 0.5 and 2), one in eight between −1.6
    and −1.2 (ρ between 3.3 and 5: beyond a dual clip of 3)"""
    off = rng.standard_normal(shape) * 0.25
    far = rng.random(shape) < 0.125
    return np.where(far, -1.2 - 0.4 * rng.random(shape), off)


def own_step(c, C, logits):
    """the case's own step / len / barred: ``scst_reference.seq_nll`` (float64 arithmetic, step rounded to float32)"""
    return sr.seq_nll(c["scores"][:, :C], c["ids"], c["row_c"], c["w"], logits)


def score_case(seed, C, Lt, K, steps, logits, wide, clip_zero=False):
    """kernel-level inputs: ``risk_cases.score_case`` plus adv (N, K) float64, old_step / ref_step (R, Lt − 1) float32, and
    - ``inf_inside``: (name, row, i) — that tensor is −inf at a scored position of a live candidate (the candidate is invalid for it);
    - ``inf_past``: (name, row, i) — −inf past the caption's end (no effect);
    - ``exact``: under ``clip_zero`` the (row, i) whose old_step IS the own step (ρ = 1 sits on both bounds 1 − 0 and 1 + 0)."""
    c = _risk_score_case(seed, C, Lt, K, steps, logits, wide)
    rng = np.random.default_rng(seed + 7000)
    N, T = len(steps), sum(steps)
    R, S = T * K, Lt - 1
    nl = own_step(c, C, logits)
    own, length = nl["step"].astype(np.float32), nl["len"]
    c["adv"] = advantages(rng, N, K)
    old = (own.astype(np.float64) + _offsets(rng, (R, S))).astype(np.float32)
    ref = (own.astype(np.float64) + rng.standard_normal((R, S)) * 0.3).astype(np.float32)
    off = c["vid_off"]
    live = [r for r in range(R) if not nl["barred"][r] and length[r] >= 1]
    c["inf_inside"], c["inf_past"], c["exact"] = [], [], []
    # from four videos up (the long cases): −inf inside a caption of video 3 in old_step (candidate 0) and in ref_step (candidate K − 1)
    if N >= 5:
        for name, arr, k in (("old_step", old, 0), ("ref_step", ref, K - 1)):
            r = off[3] * K + k
            if r in live:
                arr[r, int(length[r]) - 1] = -np.inf
                c["inf_inside"].append((name, r, int(length[r]) - 1))
    elif K >= 2 and live:
        r = [x for x in live if x % K == K - 1][0]          # a candidate K − 1 of the first video that has one alive
        old[r, 0] = -np.inf
        c["inf_inside"].append(("old_step", r, 0))
    short = [r for r in live if length[r] < S and all(r != x[1] for x in c["inf_inside"])]
    if short:
        r = short[len(short) // 2]
        old[r, S - 1] = -np.inf
        ref[r, int(length[r])] = -np.inf
        c["inf_past"] += [("old_step", r, S - 1), ("ref_step", r, int(length[r]))]
    if clip_zero:
        for r in live[::4]:
            if all(r != x[1] for x in c["inf_inside"]):
                i = int(length[r]) // 2
                old[r, i] = own[r, i]
                c["exact"].append((r, i))
    c["old_step"], c["ref_step"], c["own_step"], c["len"], c["own_barred"] = old, ref, own, length, nl["barred"]
    return c
