"""The fixed inputs of the preference-optimisation tests, shared by tests/test_pref_host.py (which checks their margins on
the CPU) and tests/test_pref_gpu.py (which runs the kernels on them).  The score rows, captions, weights and costs are built as
tests/risk_cases.py builds them (the same special rows: a barred candidate, a video with no valid candidate, cost ties, +inf / nan costs);
this file adds the reference model's scores and the settings."""
import numpy as np

from risk_cases import costs, group_case as _risk_group_case, score_case as _risk_score_case, vid_off  # noqa: F401

HINGE_MARGIN = 1e-9             # no hinge argument 1 − h of a seeded input may lie this close to 0: the active set could flip
D_MARGIN = 1e-9                 # no d of a seeded input may lie this close to 0: n_correct could flip
PREF_CONDITION = 1e-3           # hinge / ipo: pref[b] >= this times (β·max |u| + 1) in every video with a pair (pref_reference.pref_conditioning)

#   seed,  C,  Lt, K, sentence counts, logits, wide stride, reference, length_beta, beta, gamma, eps, loss_type, pairs
KERNEL_CASES = [
    (200, 7, 2, 1, [1], False, False, True, 0.0, 0.1, 0.0, 0.0, "sigmoid", "all"),
    (201, 7, 2, 1, [1], True, False, False, 1.0, 2.0, 0.5, 0.0, "sigmoid", "extremes"),
    (202, 65, 6, 2, [3, 1, 2], False, True, True, 0.0, 0.1, 0.0, 0.1, "sigmoid", "all"),              # cDPO
    (203, 65, 6, 3, [3, 1, 2], True, False, False, 1.0, 2.0, 0.5, 0.0, "sigmoid", "all"),             # SimPO
    (204, 65, 22, 16, [3, 1, 2], False, False, True, 0.0, 50.0, 0.0, 0.0, "sigmoid", "all"),          # DPO; β·d reaches several hundred
    (205, 1025, 6, 3, [3, 1, 2], True, True, True, 1.0, 0.1, 0.5, 0.0, "hinge", "all"),               # SLiC
    (206, 1025, 22, 2, [20], False, False, True, 0.0, 2.0, 0.0, 0.0, "ipo", "all"),                   # IPO
    (207, 65, 6, 16, [20], True, False, True, 1.0, 2.0, 0.0, 0.0, "hinge", "all"),                   # active and idle pairs
    (208, 7, 6, 3, [2] * 70, False, False, True, 0.0, 0.1, 0.0, 0.1, "sigmoid", "extremes"),
    (209, 65, 2, 3, [2] * 70, True, True, False, 1.0, 0.1, 0.5, 0.0, "hinge", "extremes"),
    (210, 1025, 22, 1, [3, 0, 2], True, False, True, 1.0, 50.0, 0.0, 0.0, "ipo", "all"),
    (211, 65, 22, 3, [3, 0, 2], False, False, True, 0.0, 50.0, 0.5, 0.1, "sigmoid", "all"),
    (212, 65, 6, 16, [3, 1, 2], False, False, False, 1.0, 50.0, 0.0, 0.0, "ipo", "extremes"),
    (213, 7, 6, 2, [2] * 70, True, False, True, 1.0, 2.0, 0.5, 0.0, "sigmoid", "all"),
]


def ref_bar_rows(steps, K):
    """the caption rows whose reference score is −inf (the reference bars the caption: its candidate is invalid): K ≥ 4: candidate K − 2 of
    video 0 in its first sentence; from five videos up and K ≥ 2: candidate 0 of video 3 in its first sentence"""
    off = vid_off(steps)
    rows = []
    if K >= 4 and steps[0] >= 1:
        rows.append(off[0] * K + K - 2)
    if len(steps) >= 5 and K >= 2 and steps[3] >= 1:
        rows.append(off[3] * K)
    return rows


def _reference(rng, T, K, Lt, steps, centre=None):
    """(T, K) float32 reference scores < 0: a draw of the policy's range, or (``centre``) the policy's cum moved by a draw; −inf at
    ``ref_bar_rows``"""
    if centre is None:
        ref = (-rng.random((T, K)) * (Lt - 1) * 2.0).astype(np.float32)
    else:
        ref = (np.where(np.isfinite(centre), centre, -1.0) + rng.standard_normal((T, K))).astype(np.float32)
    flat = ref.reshape(-1)
    for r in ref_bar_rows(steps, K):
        flat[r] = -np.inf
    return ref


def group_case(seed, steps, K):
    """cum-level inputs: ``risk_cases.group_case`` plus ref_cum (T, K) float32, the policy's cum moved by a unit normal draw"""
    c = _risk_group_case(seed, steps, K)
    rng = np.random.default_rng(seed + 5000)
    T = sum(steps)
    c["ref_cum"] = _reference(rng, T, K, 9, steps, centre=c["cum"])
    c["ref_bar_rows"] = ref_bar_rows(steps, K)
    return c


def score_case(seed, C, Lt, K, steps, logits, wide):
    """kernel-level inputs: ``risk_cases.score_case`` plus ref_cum (T·K,) float32"""
    c = _risk_score_case(seed, C, Lt, K, steps, logits, wide)
    rng = np.random.default_rng(seed + 5000)
    T = sum(steps)
    c["ref_cum"] = _reference(rng, T, K, Lt, steps).reshape(-1)
    c["ref_bar_rows"] = ref_bar_rows(steps, K)
    return c
