"""The fixed inputs of the contrastive (SimCTG) kernel tests, shared by tests/test_simctg_host.py — which checks on the
restatement alone that no pair outside the constructed exact cases sits within 1e-9 of the hinge's kink — and tests/test_simctg_gpu.py.

The shapes are the smallest at which the kernels can go wrong: D = 32 (half a wave's lanes idle), 96 and 100 (a ragged last round of 64),
768 (the headline width, the rows past 64 KB of LDS at Lt ≥ 22); Lt = 2 (the smallest caption), 5, 22 (the headline) and 32 (the active
mask's last bit); R = 1 and 21 (more workgroups than one, an odd count).  Captions of R = 21, in order: 0 one token (len 0); 1 two tokens;
2 all Lt; 3 two IDENTICAL rows (cos = 1: active under every margin); 4 rows 0 and 1 of DISJOINT support (cos = 0 exactly: m = 0 at ρ = 1,
inactive); 5 a ZERO row at position 1 (cos = 0 with everything, gradient 0); 6 a length below 0 and 7 a length past Lt − 1 (clamped on the
device); the rest random lengths.  R = 1: one caption of all Lt positions."""
import functools

import numpy as np
import torch

import simctg_reference as sr

DS = (32, 96, 100, 768)
LTS = (2, 5, 22, 32)
RS = (1, 21)
MARGINS = (0.5, 1.0, 2.0)
EXTRA_STRIDE = 5                 # the strided variant: rows of D + 5 floats, the padding NaN (never read)


@functools.lru_cache(maxsize=None)
def kernel_case(D, Lt, R):
    """→ dict(hidden (R·Lt, D) float32, length (R,) int32 — 6 and 7 out of range on purpose —, v (R,) float32 of mixed signs, exact: the
    {(caption, i, j)} whose margin is an exact 0 at ρ = 1 by construction, G: the captions' Gram matrices).  Treat as read-only."""
    rng = np.random.default_rng(1000 * D + 10 * Lt + R)
    hidden = rng.standard_normal((R * Lt, D)).astype(np.float32)
    # a shared direction, so that cosines spread over (−0.3, 0.9) and every margin has active and inactive pairs
    hidden += (rng.random((R * Lt, 1)) * 1.5).astype(np.float32) * rng.standard_normal((1, D)).astype(np.float32)
    length = rng.integers(1, Lt, size=R).astype(np.int32)
    exact = set()
    if R == 1:
        length[0] = Lt - 1
    else:
        length[0], length[1], length[2] = 0, 1, Lt - 1
        length[3] = max(length[3], 1)
        hidden[3 * Lt + 1] = hidden[3 * Lt]
        length[4] = min(2, Lt - 1)
        hidden[4 * Lt, D // 2:] = 0.0
        hidden[4 * Lt + 1, :D // 2] = 0.0
        exact |= {(4, 0, 1), (4, 1, 0)}
        length[5] = min(3, Lt - 1)
        hidden[5 * Lt + 1] = 0.0
        exact |= {(5, 1, j) for j in range(length[5] + 1) if j != 1} | {(5, j, 1) for j in range(length[5] + 1) if j != 1}
        length[6], length[7] = -3, Lt + 5
    v = ((-1.0) ** np.arange(R) * (0.05 + 0.01 * (np.arange(R) % 7))).astype(np.float32)
    return dict(hidden=hidden, length=length, v=v, exact=exact, G=sr.grams(hidden, length, Lt), D=D, Lt=Lt, R=R)


def reference(D, Lt, R, margin, dl=1.0):
    case = kernel_case(D, Lt, R)
    return sr.seq_cl(case["hidden"], case["length"], case["v"], margin, Lt, dl=dl, G=case["G"])


def kink_distance(D, Lt, R, margin):
    """the smallest |m_ij| over the pairs that are not constructed exact cases (at ρ = 1 those have m = 0 exactly; at other margins they
    are ordinary pairs)"""
    case, ref = kernel_case(D, Lt, R), reference(D, Lt, R, margin)
    worst = np.inf
    for r, m in enumerate(ref["m"]):
        n = m.shape[0]
        for i in range(n):
            for j in range(n):
                if i != j and not (float(np.float32(margin)) == 1.0 and (r, i, j) in case["exact"]):
                    worst = min(worst, abs(m[i, j]))
    return worst


# model level: the margin of each fixture, chosen so that the restatement alone shows no pair with |m_ij| <= 1e-4 (the hinge has kinks;
# tests/test_simctg_host.py asserts it on the recorded distances, tests/test_simctg_gpu.py on the restatement's own run)
MODEL_CASES = [("tiny", "v"), ("tiny", "vivt"), ("c1", "v"), ("c1", "vivt")]
MODEL_KS = (1, 2)
KINK = 1e-4
# (distances of the K = 2 captions on the restatement: 5.5e-3, 7.2e-3, 3.0e-3, 7.8e-3; at ρ = 0.5 c1 vivt sits 1.3e-4 from a kink)
MODEL_MARGIN = {("tiny", "v"): 0.25, ("tiny", "vivt"): 0.45, ("c1", "v"): 0.3, ("c1", "vivt"): 0.7}


def captions(batch, cfg, K):
    """the fixture's gold rows (``Translator.gold_captions``) and, for K = 2, beside each the gold row of the video's NEXT sentence (the
    last one wraps round): a second caption under the same memory rows that needs no decode, so the host tests see the same captions"""
    from svpc_amd.translator import Translator
    tr = object.__new__(Translator)
    tr.max_v_len, tr.max_t_len = cfg.max_v_len, cfg.max_t_len
    gold = tr.gold_captions(batch["input_labels_list"], batch["batch_step_num"])
    if K == 1:
        return [g.unsqueeze(1).contiguous() for g in gold]
    assert K == 2
    return [torch.cat([g.unsqueeze(1), g.roll(-1, 0).unsqueeze(1)], 1).contiguous() for g in gold]


def weights(steps, K, flip=0):
    """hand-set, mixed signs, different on every row (tests/test_unlikelihood_gpu.py's)"""
    T = sum(steps)
    w = [[(-1.0) ** (t + k + flip) * (0.05 + 0.01 * ((3 * t + k + 2 * flip) % 7)) for k in range(K)] for t in range(T)]
    return torch.tensor(w, dtype=torch.float32)


def per_video(t, steps):
    out, o = [], 0
    for s in steps:
        out.append(t[o:o + s])
        o += s
    return out


_MODEL_REF = {}


def model_reference(golden_dir, case, mt, K, with_grads):
    """The CPU restatement of ``contrastive_loss`` on a golden fixture at MODEL_MARGIN, computed once per process and left unchanged →
    dict(loss, grads {name: tensor or None} (``with_grads``), cum, barred, cl, sim (T, K), min_abs_m, hidden, caps, w, v, margin)."""
    from helpers import build_model
    key = (case, mt, K)
    got = _MODEL_REF.get(key)
    if got is not None and (got["grads"] is not None or not with_grads):
        return got
    _, cfg, batch, model = build_model(case, mt, golden_dir, "cpu")
    names = {n for n, _ in model.named_parameters()}
    P = {k: v.detach().clone().requires_grad_(with_grads and k in names and v.is_floating_point()) for k, v in model.state_dict().items()}
    steps = [int(s) for s in batch["batch_step_num"]]
    caps = captions(batch, cfg, K)
    w, v = weights(steps, K), weights(steps, K, flip=1)
    margin = MODEL_MARGIN[(case, mt)]
    with torch.set_grad_enabled(with_grads):
        loss, cums, bars, cls, sims, near, hid = sr.contrastive_loss(
            P, cfg, batch["input_ids_list"], batch["video_features_list"], batch["input_masks_list"], batch["ingr_input_ids"],
            batch["ingr_sep_masks"], steps, batch["ingr_id_dict"], batch["oov_word_dict"], [x.numpy() for x in caps],
            [x.numpy() for x in per_video(w, steps)], [x.numpy() for x in per_video(v, steps)], margin)
        if with_grads:
            loss.backward()
    got = _MODEL_REF[key] = dict(loss=float(loss.detach()), grads={n: (P[n].grad.clone() if P[n].grad is not None else None) for n in names}
                                 if with_grads else None, cum=torch.cat(cums).numpy(), barred=np.concatenate(bars),
                                 cl=torch.cat(cls).numpy(), sim=torch.cat(sims).numpy(), min_abs_m=near, hidden=hid, caps=caps, w=w, v=v,
                                 margin=margin)
    return got
