"""Wrong calls of the sequence-loss bindings and of their host checks: what tools/make_golden_seq_loss_errors.py records (exception type
and full message, tests/golden/seq_loss_errors.json) and tests/test_seq_loss_shared_host.py replays.  Everything runs on CPU tensors.  A
tensor from ``gpu()`` answers ``is_cuda`` with True, so that the checks behind a "runs on the GPU only" refusal are reached too; no case
passes all of its checks, and both users put a refusing stub in place of the kernel library's ``call`` all the same.  Several cases are
wrong in two ways: they pin the order in which the checks fire."""
import torch

from svpc_amd import ops
from svpc_amd.synthetic import UNK

R, LT, C, K = 4, 3, 9, 2          # four caption rows = two sentences of two candidates, one video
CUDA = torch.device("cuda:0")


class _OnGpu(torch.Tensor):
    is_cuda = property(lambda self: True)


def gpu(t):
    return t.as_subclass(_OnGpu)


def f32(*shape):
    return torch.zeros(*shape, dtype=torch.float32)


def i32(*shape):
    return torch.zeros(*shape, dtype=torch.int32)


def f64(*shape):
    return torch.zeros(*shape, dtype=torch.float64)


def _defaults():
    return dict(scores=f32(R * LT, C), row_c=[C] * R, tgt=i32(R, LT), length=i32(R) + 1, row_w=f32(R), logits=False, unk_id=UNK,
                max_cols=None, neg=i32(R, LT - 1, 1) - 1, row_u=f32(R), tq=f32(R * LT, C), row_v=f32(R), teacher_logits=False,
                cost=gpu(f64(1, K)), vid_off=[0, 2], alpha=5e-3, length_beta=0.0, margin=1e-3, risk_weight=1.0, rank_weight=0.0,
                ref_cum=None, beta=0.1, gamma=0.0, label_smoothing=0.0, pref_weight=1.0, loss_type="sigmoid", pairs="all",
                old_step=None, ref_step=None, clip_lo=0.2, clip_hi=0.2, dual_clip=0.0, kl_beta=0.0, norm="sequence")


def wrapper(fam, **over):
    """a call of ``ops.seq_<fam>`` on the small right arguments with ``over`` laid over them"""
    d = _defaults()
    d.update(over)
    head = (d["scores"], d["row_c"], d["tgt"], d["length"])
    if fam == "nll":
        return lambda: ops.seq_nll(*head, d["row_w"], d["logits"], d["unk_id"], max_cols=d["max_cols"])
    if fam == "ul":
        return lambda: ops.seq_ul(*head, d["neg"], d["row_w"], d["row_u"], d["logits"], d["unk_id"], max_cols=d["max_cols"])
    if fam == "kd":
        return lambda: ops.seq_kd(*head, d["tq"], d["row_w"], d["row_v"], d["logits"], d["teacher_logits"], d["unk_id"], max_cols=d["max_cols"])
    if fam == "risk":
        return lambda: ops.seq_risk(*head, d["cost"], d["vid_off"], d["row_w"], d["logits"], d["unk_id"], d["alpha"], d["length_beta"],
                                    d["margin"], d["risk_weight"], d["rank_weight"], max_cols=d["max_cols"])
    if fam == "pref":
        return lambda: ops.seq_pref(*head, d["cost"], d["vid_off"], d["ref_cum"], d["row_w"], d["logits"], d["unk_id"], d["beta"], d["gamma"],
                                    d["label_smoothing"], d["length_beta"], d["pref_weight"], d["loss_type"], d["pairs"], max_cols=d["max_cols"])
    assert fam == "pg"
    return lambda: ops.seq_pg(*head, d["cost"], d["vid_off"], d["old_step"], d["ref_step"], d["row_w"], d["logits"], d["unk_id"], d["clip_lo"],
                              d["clip_hi"], d["dual_clip"], d["kl_beta"], d["norm"], max_cols=d["max_cols"])


FAMILIES = ("nll", "ul", "kd", "risk", "pref", "pg")
CANDIDATE_FAMILIES = ("risk", "pref", "pg")


def _wrapper_cases():
    out = []
    for fam in FAMILIES:
        bad = dict(tgt=i32(R, LT).long(), scores=f32(R * LT, C).double(), length=(i32(R) + 1).long(), row_w=f32(R + 1), row_c=[C] * (R + 1),
                   max_cols=C + 1)
        names = list(bad)
        for n in names:                                   # wrong in one way
            out.append(("seq_%s/%s" % (fam, n), wrapper(fam, **{n: bad[n]})))
        for i, a in enumerate(names):                     # wrong in two ways: which of the two is reported
            for b in names[i + 1:]:
                out.append(("seq_%s/%s+%s" % (fam, a, b), wrapper(fam, **{a: bad[a], b: bad[b]})))
        out += [("seq_%s/tgt_1d" % fam, wrapper(fam, tgt=i32(R))),
                ("seq_%s/tgt_one_position" % fam, wrapper(fam, tgt=i32(R, 1))),
                ("seq_%s/tgt_other_device" % fam, wrapper(fam, tgt=torch.zeros(R, LT, dtype=torch.int32, device="meta"))),
                ("seq_%s/tgt_strided" % fam, wrapper(fam, tgt=i32(R, 2 * LT)[:, ::2])),
                ("seq_%s/scores_short" % fam, wrapper(fam, scores=f32(R * LT - 1, C))),
                ("seq_%s/scores_3d" % fam, wrapper(fam, scores=f32(R * LT, C, 1))),
                ("seq_%s/length_strided" % fam, wrapper(fam, length=i32(2 * R)[::2])),
                ("seq_%s/row_w_f64" % fam, wrapper(fam, row_w=f32(R).double())),
                ("seq_%s/row_c_zero" % fam, wrapper(fam, row_c=[C, 0, C, C])),
                ("seq_%s/row_c_over_max_cols" % fam, wrapper(fam, row_c=[C] * R, max_cols=C - 1)),
                ("seq_%s/row_c_wider_than_scores" % fam, wrapper(fam, row_c=[C + 1] * R)),
                ("seq_%s/cpu" % fam, wrapper(fam))]
        if fam == "nll":                                  # (the one wrapper that takes its row_w for a tensor unasked: AttributeError)
            out += [("seq_nll/row_w_none", wrapper(fam, row_w=None)), ("seq_nll/row_w_list", wrapper(fam, row_w=[0.0] * R)),
                    ("seq_nll/row_w_none+row_c", wrapper(fam, row_w=None, row_c=[C] * (R + 1)))]
        if fam in CANDIDATE_FAMILIES:
            out += [("seq_%s/row_w_none_then_row_c" % fam, wrapper(fam, row_w=None, row_c=[C] * (R + 1))),
                    ("seq_%s/row_w_list" % fam, wrapper(fam, row_w=[0.0] * R)),
                    ("seq_%s/cost_f32" % fam, wrapper(fam, cost=gpu(f32(1, K)))),
                    ("seq_%s/cost_f32+row_w" % fam, wrapper(fam, cost=gpu(f32(1, K)), row_w=f32(R + 1))),
                    ("seq_%s/length+cost_f32" % fam, wrapper(fam, length=(i32(R) + 1).long(), cost=gpu(f32(1, K)))),
                    ("seq_%s/cost_cpu" % fam, wrapper(fam, cost=f64(1, K))),
                    ("seq_%s/cost_other_device" % fam, wrapper(fam, cost=torch.zeros(1, K, dtype=torch.float64, device="meta"))),
                    ("seq_%s/rows_no_multiple_of_k" % fam, wrapper(fam, cost=gpu(f64(1, 3)))),
                    ("seq_%s/rows_no_multiple_of_k+vid_off" % fam, wrapper(fam, cost=gpu(f64(1, 3)), vid_off=[1, 2])),
                    ("seq_%s/vid_off_start" % fam, wrapper(fam, vid_off=[1, 2])),
                    ("seq_%s/vid_off_end" % fam, wrapper(fam, vid_off=[0, 3])),
                    ("seq_%s/vid_off_count" % fam, wrapper(fam, vid_off=[0, 1, 2])),
                    ("seq_%s/vid_off+row_w" % fam, wrapper(fam, vid_off=[0, 3], row_w=f32(R + 1))),
                    ("seq_%s/cost_17_columns" % fam, wrapper(fam, cost=gpu(f64(1, 17))))]
    out += [("seq_ul/neg_list", wrapper("ul", neg=[[-1]])),
            ("seq_ul/neg_2d", wrapper("ul", neg=i32(R, LT - 1))),
            ("seq_ul/neg_65_columns", wrapper("ul", neg=i32(R, LT - 1, 65))),
            ("seq_ul/neg_int64", wrapper("ul", neg=i32(R, LT - 1, 1).long())),
            ("seq_ul/neg_rows", wrapper("ul", neg=i32(R + 1, LT - 1, 1))),
            ("seq_ul/row_u", wrapper("ul", row_u=f32(R + 1))),
            ("seq_ul/row_w+row_u", wrapper("ul", row_w=f32(R + 1), row_u=f32(R + 1))),
            ("seq_ul/neg+row_w", wrapper("ul", neg=i32(R, LT - 1), row_w=f32(R + 1))),
            ("seq_ul/lt_66", wrapper("ul", tgt=i32(1, 67), scores=f32(67, C), length=i32(1) + 1, row_c=[C], row_w=f32(1), row_u=f32(1),
                                     neg=i32(1, 66, 1))),
            ("seq_kd/tq_list", wrapper("kd", tq=[[0.0]])),
            ("seq_kd/tq_f64", wrapper("kd", tq=f32(R * LT, C).double())),
            ("seq_kd/tq_other_device", wrapper("kd", tq=torch.zeros(R * LT, C, device="meta"))),
            ("seq_kd/tq_rows", wrapper("kd", tq=f32(R * LT + 1, C))),
            ("seq_kd/tq_narrow", wrapper("kd", tq=f32(R * LT, C - 1))),
            ("seq_kd/tq_column_stride", wrapper("kd", tq=f32(R * LT, 2 * C)[:, ::2])),
            ("seq_kd/tq_overlapping_rows", wrapper("kd", tq=f32(1, C).expand(R * LT, C))),
            ("seq_kd/row_v", wrapper("kd", row_v=f32(R + 1))),
            ("seq_kd/tq+row_w", wrapper("kd", tq=f32(R * LT + 1, C), row_w=f32(R + 1))),
            ("seq_kd/row_w+row_v", wrapper("kd", row_w=f32(R + 1), row_v=f32(R + 1)))]
    for name in ("alpha", "length_beta", "margin", "risk_weight", "rank_weight"):
        out.append(("seq_risk/%s" % name, wrapper("risk", **{name: -1.0})))
    out += [("seq_risk/alpha+cost_f32", wrapper("risk", alpha=float("nan"), cost=gpu(f32(1, K)))),
            ("seq_risk/length+alpha", wrapper("risk", length=(i32(R) + 1).long(), alpha=True)),
            ("seq_pref/beta", wrapper("pref", beta=0.0)),
            ("seq_pref/beta+gamma", wrapper("pref", beta=0.0, gamma=-1.0)),
            ("seq_pref/gamma+label_smoothing", wrapper("pref", gamma=-1.0, label_smoothing=0.5)),
            ("seq_pref/label_smoothing+loss_type", wrapper("pref", label_smoothing=0.5, loss_type="dpo")),
            ("seq_pref/loss_type+pairs", wrapper("pref", loss_type="dpo", pairs="some")),
            ("seq_pref/pairs", wrapper("pref", pairs="some")),
            ("seq_pref/loss_type_none", wrapper("pref", loss_type=None)),
            ("seq_pref/pairs_none", wrapper("pref", pairs=None)),
            ("seq_pref/label_smoothing_hinge", wrapper("pref", label_smoothing=0.1, loss_type="hinge")),
            ("seq_pref/gamma_ipo", wrapper("pref", gamma=0.5, loss_type="ipo")),
            ("seq_pref/ref_cum_f64", wrapper("pref", ref_cum=gpu(f64(R)))),
            ("seq_pref/ref_cum_rows", wrapper("pref", ref_cum=gpu(f32(R + 1)))),
            ("seq_pref/ref_cum_other_device", wrapper("pref", ref_cum=torch.zeros(R, device="meta"))),
            ("seq_pref/ref_cum_cpu", wrapper("pref", ref_cum=f32(R))),
            ("seq_pref/ref_cum+cost_f32", wrapper("pref", ref_cum=gpu(f32(R + 1)), cost=gpu(f32(1, K)))),
            ("seq_pref/ref_cum_cpu+cost_cpu", wrapper("pref", ref_cum=f32(R), cost=f64(1, K))),
            ("seq_pg/adv_none", wrapper("pg", cost=None)),
            ("seq_pg/norm_none", wrapper("pg", norm=None)),
            ("seq_pg/norm", wrapper("pg", norm="mean")),
            ("seq_pg/clip_lo+clip_hi", wrapper("pg", clip_lo=1.0, clip_hi=-1.0)),
            ("seq_pg/dual_clip+kl_beta", wrapper("pg", dual_clip=1.0, kl_beta=-1.0)),
            ("seq_pg/kl_beta_without_ref", wrapper("pg", kl_beta=0.04)),
            ("seq_pg/kl_beta+norm", wrapper("pg", kl_beta=0.04, norm="mean")),
            ("seq_pg/old_step_f64", wrapper("pg", old_step=gpu(f64(R, LT - 1)))),
            ("seq_pg/old_step_size", wrapper("pg", old_step=gpu(f32(R, LT)))),
            ("seq_pg/ref_step_size+adv_f32", wrapper("pg", ref_step=gpu(f32(R, LT)), cost=gpu(f32(1, K)))),
            ("seq_pg/old_step_other_device", wrapper("pg", old_step=torch.zeros(R, LT - 1, device="meta"))),
            ("seq_pg/old_step_cpu", wrapper("pg", old_step=f32(R, LT - 1))),
            ("seq_pg/ref_step_cpu+adv_cpu", wrapper("pg", ref_step=f32(R, LT - 1), cost=f64(1, K)))]
    return out


def _check_cases():
    ids = torch.zeros(2, 2, LT, dtype=torch.int64)
    adv = f64(3, 4)
    st = f32(6, 2)
    o = ops
    out = [
        # ---- check_scst / scst_weights
        ("check_scst/baseline", lambda: o.check_scst(baseline="best")),
        ("check_scst/baseline+utility", lambda: o.check_scst(baseline="best", utility="METEOR")),
        ("check_scst/utility+num_samples", lambda: o.check_scst(utility="METEOR", num_samples=0)),
        ("check_scst/num_samples_0", lambda: o.check_scst(num_samples=0)),
        ("check_scst/num_samples_17", lambda: o.check_scst(num_samples=17)),
        ("check_scst/num_samples_bool", lambda: o.check_scst(num_samples=True)),
        ("check_scst/num_samples_float", lambda: o.check_scst(num_samples=2.0)),
        ("check_scst/ids_list", lambda: o.check_scst(ids=[[1, 2]])),
        ("check_scst/ids_2d", lambda: o.check_scst(ids=ids[0])),
        ("check_scst/ids_float", lambda: o.check_scst(ids=ids.float())),
        ("check_scst/ids_17", lambda: o.check_scst(ids=torch.zeros(2, 17, LT, dtype=torch.int64))),
        ("check_scst/ids_against_num_samples", lambda: o.check_scst(ids=ids, num_samples=3)),
        ("check_scst/one_position", lambda: o.check_scst(ids=ids[:, :, :1])),
        ("check_scst/lt", lambda: o.check_scst(ids=ids, lt=LT + 1)),
        ("check_scst/lt+steps", lambda: o.check_scst(ids=ids, lt=LT + 1, steps=[3])),
        ("check_scst/steps", lambda: o.check_scst(ids=ids, steps=[3])),
        ("check_scst/steps_negative", lambda: o.check_scst(ids=ids, steps=[3, -1])),
        ("check_scst/steps+weights", lambda: o.check_scst(ids=ids, steps=[3], weights=f32(5))),
        ("check_scst/weights_shape", lambda: o.check_scst(ids=ids, weights=f32(5))),
        ("check_scst/weights_int", lambda: o.check_scst(ids=ids, weights=i32(2, 2))),
        ("check_scst/weights_list", lambda: o.check_scst(ids=ids, weights=[0.0] * 4)),
        ("check_scst/mean_of_one", lambda: o.check_scst(num_samples=1, baseline="mean")),
        ("check_scst/weights+mean_of_one", lambda: o.check_scst(ids=ids[:, :1], weights=f32(5), baseline="mean")),
        ("check_scst/ids_cpu", lambda: o.check_scst(ids=ids)),
        ("check_scst/weights_cpu", lambda: o.check_scst(ids=gpu(ids), weights=f32(2, 2))),
        ("scst_weights/reward_f32", lambda: o.scst_weights(f32(2, 2), [0, 1])),
        ("scst_weights/reward_1d", lambda: o.scst_weights(f64(2), [0, 1])),
        ("scst_weights/reward_17", lambda: o.scst_weights(f64(2, 17), [0, 1])),
        ("scst_weights/baseline", lambda: o.scst_weights(f64(2, 2), [0, 1], baseline="best")),
        ("scst_weights/mean_of_one", lambda: o.scst_weights(f64(2, 1), [0, 1], baseline="mean")),
        ("scst_weights/greedy_missing", lambda: o.scst_weights(f64(2, 2), [0, 1])),
        ("scst_weights/greedy_shape", lambda: o.scst_weights(f64(2, 2), [0, 1], greedy=f64(3))),
        ("scst_weights/greedy+row_vid", lambda: o.scst_weights(f64(2, 2), [0, 2], greedy=f64(3))),
        ("scst_weights/row_vid", lambda: o.scst_weights(f64(2, 2), [0, 2], baseline="none")),
        ("scst_weights/cpu", lambda: o.scst_weights(f64(2, 2), [0, 1], baseline="none")),
        # ---- check_unlikelihood / ul_negatives
        ("check_unlikelihood/rule", lambda: o.check_unlikelihood(rule="word")),
        ("check_unlikelihood/rule+ngram", lambda: o.check_unlikelihood(rule="word", ngram=5)),
        ("check_unlikelihood/ngram_5", lambda: o.check_unlikelihood(ngram=5)),
        ("check_unlikelihood/ngram_bool", lambda: o.check_unlikelihood(ngram=True)),
        ("check_unlikelihood/ngram+scope", lambda: o.check_unlikelihood(ngram=0, scope="video")),
        ("check_unlikelihood/scope", lambda: o.check_unlikelihood(scope="video")),
        ("check_unlikelihood/scope+alpha", lambda: o.check_unlikelihood(scope="video", alpha=-1.0)),
        ("check_unlikelihood/alpha_negative", lambda: o.check_unlikelihood(alpha=-1.0)),
        ("check_unlikelihood/alpha_nan", lambda: o.check_unlikelihood(alpha=float("nan"))),
        ("check_unlikelihood/alpha_str", lambda: o.check_unlikelihood(alpha="1")),
        ("check_unlikelihood/alpha+lt", lambda: o.check_unlikelihood(alpha=True, lt=1)),
        ("check_unlikelihood/lt_1", lambda: o.check_unlikelihood(lt=1)),
        ("check_unlikelihood/lt_66", lambda: o.check_unlikelihood(lt=66)),
        ("check_unlikelihood/neg_list", lambda: o.check_unlikelihood(lt=LT, neg=[[-1]], rows=R)),
        ("check_unlikelihood/m_0", lambda: o.check_unlikelihood(m=0)),
        ("check_unlikelihood/m_65", lambda: o.check_unlikelihood(m=65)),
        ("check_unlikelihood/neg_against_m", lambda: o.check_unlikelihood(lt=LT, m=2, neg=i32(R, LT - 1, 1), rows=R)),
        ("check_unlikelihood/neg_other_device", lambda: o.check_unlikelihood(lt=LT, neg=i32(R, LT - 1, 1), rows=R, device=CUDA)),
        ("check_unlikelihood/row_w", lambda: o.check_unlikelihood(row_w=f32(R + 1), rows=R)),
        ("check_unlikelihood/row_u_list", lambda: o.check_unlikelihood(row_u=[0.0] * R, rows=R)),
        ("check_unlikelihood/row_w_other_device", lambda: o.check_unlikelihood(row_w=f32(R), rows=R, device=CUDA)),
        ("check_unlikelihood/weights", lambda: o.check_unlikelihood(weights=f32(5), shape=(2, 2))),
        ("check_unlikelihood/ul_weights_int", lambda: o.check_unlikelihood(ul_weights=i32(2, 2), shape=(2, 2))),
        ("check_unlikelihood/weights+ul_weights", lambda: o.check_unlikelihood(weights=[0.0], ul_weights=f32(5), shape=(2, 2))),
        ("check_unlikelihood/row_u+weights", lambda: o.check_unlikelihood(row_u=f32(R + 1), rows=R, weights=f32(5), shape=(2, 2))),
        ("check_unlikelihood/weights_cpu", lambda: o.check_unlikelihood(weights=f32(2, 2), shape=(2, 2))),
        ("check_unlikelihood/row_u_cpu", lambda: o.check_unlikelihood(row_u=f32(R), rows=R)),
        ("ul_negatives/tgt", lambda: o.ul_negatives(i32(R, LT).long(), i32(R), i32(R), [C] * R, UNK, 5, "token")),
        ("ul_negatives/tgt_one_position", lambda: o.ul_negatives(i32(R, 1), i32(R), i32(R), [C] * R, UNK, 5, "token")),
        ("ul_negatives/tgt+rule", lambda: o.ul_negatives(i32(R), i32(R), i32(R), [C] * R, UNK, 5, "word")),
        ("ul_negatives/rule+length", lambda: o.ul_negatives(i32(R, LT), i32(R).long(), i32(R), [C] * R, UNK, 5, "word")),
        ("ul_negatives/lt_66", lambda: o.ul_negatives(i32(R, 67), i32(R), i32(R), [C] * R, UNK, 5, "token")),
        ("ul_negatives/length", lambda: o.ul_negatives(i32(R, LT), i32(R).long(), i32(R), [C] * R, UNK, 5, "token")),
        ("ul_negatives/finished", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R + 1), [C] * R, UNK, 5, "token")),
        ("ul_negatives/length+ids", lambda: o.ul_negatives(i32(R, LT), i32(R + 1), i32(R), [C] * R, -1, 5, "token")),
        ("ul_negatives/unk", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R), [C] * R, -1, 5, "token")),
        ("ul_negatives/eos", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R), [C] * R, UNK, -1, "token")),
        ("ul_negatives/eos+row_c", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R), [C] * 3, UNK, -1, "token")),
        ("ul_negatives/row_c", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R), [C] * 3, UNK, 5, "token")),
        ("ul_negatives/row_c+k", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R), [C] * 3, UNK, 5, "ngram", scope="paragraph", K=3)),
        ("ul_negatives/k", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R), [C] * R, UNK, 5, "ngram", scope="paragraph", K=3)),
        ("ul_negatives/k_bool", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R), [C] * R, UNK, 5, "ngram", scope="paragraph", K=True)),
        ("ul_negatives/sent_first_missing", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R), [C] * R, UNK, 5, "ngram", scope="paragraph", K=2)),
        ("ul_negatives/sent_first_count", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R), [C] * R, UNK, 5, "ngram", scope="paragraph", K=2,
                                                                 sent_first=[0])),
        ("ul_negatives/sent_first_later", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R), [C] * R, UNK, 5, "ngram", scope="paragraph", K=2,
                                                                 sent_first=[1, 1])),
        ("ul_negatives/cpu", lambda: o.ul_negatives(i32(R, LT), i32(R), i32(R), [C] * R, UNK, 5, "token")),
        # ---- check_distill
        ("check_distill/alpha_above_1", lambda: o.check_distill(alpha=1.5)),
        ("check_distill/alpha_bool", lambda: o.check_distill(alpha=True)),
        ("check_distill/alpha_inf", lambda: o.check_distill(alpha=float("inf"))),
        ("check_distill/alpha+tq", lambda: o.check_distill(alpha=-0.5, tq=[[0.0]])),
        ("check_distill/tq_list", lambda: o.check_distill(tq=[[0.0]])),
        ("check_distill/tq_1d", lambda: o.check_distill(tq=f32(4))),
        ("check_distill/tq_other_device", lambda: o.check_distill(tq=f32(4, C), device=CUDA)),
        ("check_distill/tq_rows", lambda: o.check_distill(tq=f32(4, C), tq_rows=5)),
        ("check_distill/tq_rows+narrow", lambda: o.check_distill(tq=f32(4, C), tq_rows=5, max_cols=C + 1)),
        ("check_distill/tq_narrow", lambda: o.check_distill(tq=f32(4, C), max_cols=C + 1)),
        ("check_distill/tq_column_stride", lambda: o.check_distill(tq=f32(4, 2 * C)[:, ::2])),
        ("check_distill/tq_strides+row_w", lambda: o.check_distill(tq=f32(1, C).expand(4, C), row_w=f32(R + 1), rows=R)),
        ("check_distill/row_w", lambda: o.check_distill(row_w=f32(R + 1), rows=R)),
        ("check_distill/row_v_list", lambda: o.check_distill(row_v=[0.0] * R, rows=R)),
        ("check_distill/row_v+kd_weights", lambda: o.check_distill(row_v=f32(R + 1), rows=R, kd_weights=f32(5), shape=(2, 2))),
        ("check_distill/weights", lambda: o.check_distill(weights=f32(5), shape=(2, 2))),
        ("check_distill/kd_weights_list", lambda: o.check_distill(kd_weights=[0.0], shape=(2, 2))),
        ("check_distill/kd_weights_no_gpu_needed", lambda: o.check_distill(kd_weights=i32(4), shape=(2, 2), need_gpu=False)),
        ("check_distill/tq_cpu", lambda: o.check_distill(tq=f32(4, C))),
        ("check_distill/weights_cpu", lambda: o.check_distill(weights=f32(2, 2), shape=(2, 2))),
        # ---- check_simctg / seq_cl
        ("check_simctg/margin_0", lambda: o.check_simctg(margin=0.0)),
        ("check_simctg/margin_above_2", lambda: o.check_simctg(margin=2.5)),
        ("check_simctg/margin_bool", lambda: o.check_simctg(margin=True)),
        ("check_simctg/margin_rounds_to_0", lambda: o.check_simctg(margin=1e-50)),
        ("check_simctg/margin+cl_weight", lambda: o.check_simctg(margin=float("nan"), cl_weight=-1.0)),
        ("check_simctg/cl_weight", lambda: o.check_simctg(cl_weight=-1.0)),
        ("check_simctg/cl_weight+weights", lambda: o.check_simctg(cl_weight="1", weights=[0.0])),
        ("check_simctg/weights_list", lambda: o.check_simctg(weights=[0.0])),
        ("check_simctg/weights_shape", lambda: o.check_simctg(weights=f32(5), shape=(2, 2))),
        ("check_simctg/cl_weights_int", lambda: o.check_simctg(cl_weights=i32(2, 2))),
        ("check_simctg/cl_weights+row_v", lambda: o.check_simctg(cl_weights=i32(2, 2), row_v=f32(R + 1), rows=R)),
        ("check_simctg/row_v", lambda: o.check_simctg(row_v=f32(R + 1), rows=R)),
        ("check_simctg/row_v_list", lambda: o.check_simctg(row_v=[0.0], rows=R)),
        ("check_simctg/row_v_other_device", lambda: o.check_simctg(row_v=f32(R), rows=R, device=CUDA)),
        ("check_simctg/weights_cpu", lambda: o.check_simctg(weights=f32(2, 2), shape=(2, 2))),
        ("check_simctg/row_v_cpu", lambda: o.check_simctg(row_v=f32(R), rows=R)),
        ("seq_cl/margin_none", lambda: o.seq_cl(f32(R * LT, 8), i32(R), f32(R), None, LT)),
        ("seq_cl/margin", lambda: o.seq_cl(f32(R * LT, 8), i32(R), f32(R), 3.0, LT)),
        ("seq_cl/margin+lt", lambda: o.seq_cl(f32(R * LT, 8), i32(R), f32(R), 3.0, 1)),
        ("seq_cl/lt_1", lambda: o.seq_cl(f32(R * LT, 8), i32(R), f32(R), 0.5, 1)),
        ("seq_cl/lt_33", lambda: o.seq_cl(f32(R * 33, 8), i32(R), f32(R), 0.5, 33)),
        ("seq_cl/lt_float", lambda: o.seq_cl(f32(R * LT, 8), i32(R), f32(R), 0.5, 3.0)),
        ("seq_cl/lt+hidden", lambda: o.seq_cl(f32(R * LT, 8).double(), i32(R), f32(R), 0.5, True)),
        ("seq_cl/hidden_f64", lambda: o.seq_cl(f32(R * LT, 8).double(), i32(R), f32(R), 0.5, LT)),
        ("seq_cl/hidden_list", lambda: o.seq_cl([[0.0]], i32(R), f32(R), 0.5, LT)),
        ("seq_cl/hidden_no_columns", lambda: o.seq_cl(f32(R * LT, 0), i32(R), f32(R), 0.5, LT)),
        ("seq_cl/hidden+length", lambda: o.seq_cl(f32(R * LT), i32(R).long(), f32(R), 0.5, LT)),
        ("seq_cl/length_int64", lambda: o.seq_cl(f32(R * LT, 8), i32(R).long(), f32(R), 0.5, LT)),
        ("seq_cl/length_2d", lambda: o.seq_cl(f32(R * LT, 8), i32(R, 1), f32(R), 0.5, LT)),
        ("seq_cl/length_list", lambda: o.seq_cl(f32(R * LT, 8), [1] * R, f32(R), 0.5, LT)),
        ("seq_cl/length+rows", lambda: o.seq_cl(f32(R * LT - 1, 8), i32(2 * R)[::2], f32(R), 0.5, LT)),
        ("seq_cl/rows_short", lambda: o.seq_cl(f32(R * LT - 1, 8), i32(R), f32(R), 0.5, LT)),
        ("seq_cl/rows_short+lds", lambda: o.seq_cl(f32(1, 36865), i32(R), f32(R), 0.5, 2)),
        ("seq_cl/lds", lambda: o.seq_cl(f32(2, 36865), i32(1), f32(1), 0.5, 2)),
        ("seq_cl/lds+row_v", lambda: o.seq_cl(f32(2, 36865), i32(1), f32(2), 0.5, 2)),
        ("seq_cl/row_v", lambda: o.seq_cl(f32(R * LT, 8), i32(R), f32(R + 1), 0.5, LT)),
        ("seq_cl/row_v_cpu", lambda: o.seq_cl(f32(R * LT, 8), i32(R), f32(R), 0.5, LT)),
        ("seq_cl/cpu", lambda: o.seq_cl(f32(R * LT, 8), i32(R), gpu(f32(R)), 0.5, LT)),
        # ---- check_risk
        ("check_risk/alpha", lambda: o.check_risk(alpha=-1.0)),
        ("check_risk/alpha+length_beta", lambda: o.check_risk(alpha=float("inf"), length_beta=-1.0)),
        ("check_risk/length_beta+margin", lambda: o.check_risk(length_beta="0", margin=-1.0)),
        ("check_risk/margin+risk_weight", lambda: o.check_risk(margin=True, risk_weight=-1.0)),
        ("check_risk/risk_weight+rank_weight", lambda: o.check_risk(risk_weight=float("nan"), rank_weight=-1.0)),
        ("check_risk/rank_weight+source", lambda: o.check_risk(rank_weight=-1.0, source="greedy")),
        ("check_risk/source", lambda: o.check_risk(source="greedy")),
        ("check_risk/source+utility", lambda: o.check_risk(source="greedy", utility="METEOR")),
        ("check_risk/utility", lambda: o.check_risk(utility="METEOR")),
        ("check_risk/utility+k", lambda: o.check_risk(utility="METEOR", k=0)),
        ("check_risk/k_0", lambda: o.check_risk(k=0)),
        ("check_risk/k_17", lambda: o.check_risk(k=17)),
        ("check_risk/k_bool", lambda: o.check_risk(k=True)),
        ("check_risk/k_float", lambda: o.check_risk(k=2.0)),
        ("check_risk/k+cost", lambda: o.check_risk(k=0, cost=adv.float())),
        ("check_risk/cost_f32", lambda: o.check_risk(cost=adv.float())),
        ("check_risk/cost_1d", lambda: o.check_risk(cost=adv[0])),
        ("check_risk/cost_list", lambda: o.check_risk(cost=adv.tolist())),
        ("check_risk/cost_17", lambda: o.check_risk(cost=f64(3, 17))),
        ("check_risk/cost_0", lambda: o.check_risk(cost=f64(3, 0))),
        ("check_risk/cost_against_k", lambda: o.check_risk(k=3, cost=adv)),
        ("check_risk/cost_columns+device", lambda: o.check_risk(k=3, cost=adv, device=CUDA)),
        ("check_risk/cost_other_device", lambda: o.check_risk(cost=adv, device=CUDA)),
        ("check_risk/cost_device+vid_off", lambda: o.check_risk(cost=adv, device=CUDA, vid_off=[1])),
        ("check_risk/vid_off_start", lambda: o.check_risk(vid_off=[1, 2, 3, 4], n_sent=4)),
        ("check_risk/vid_off_falls", lambda: o.check_risk(vid_off=[0, 2, 1, 4], n_sent=4)),
        ("check_risk/vid_off_end", lambda: o.check_risk(vid_off=[0, 5], n_sent=4)),
        ("check_risk/vid_off_empty", lambda: o.check_risk(vid_off=[], n_sent=0)),
        ("check_risk/vid_off_long", lambda: o.check_risk(vid_off=list(range(1, 30)))),
        ("check_risk/vid_off_against_cost", lambda: o.check_risk(cost=gpu(adv), vid_off=[0, 1, 2])),
        ("check_risk/vid_off+cost_cpu", lambda: o.check_risk(cost=adv, vid_off=[0, 1, 2])),
        ("check_risk/cost_cpu", lambda: o.check_risk(cost=adv)),
        # ---- check_pref
        ("check_pref/beta_0", lambda: o.check_pref(beta=0.0)),
        ("check_pref/beta_bool", lambda: o.check_pref(beta=True)),
        ("check_pref/beta_nan", lambda: o.check_pref(beta=float("nan"))),
        ("check_pref/beta+gamma", lambda: o.check_pref(beta=-1.0, gamma=-1.0)),
        ("check_pref/gamma", lambda: o.check_pref(gamma=-1.0)),
        ("check_pref/gamma+length_beta", lambda: o.check_pref(gamma="0", length_beta=-1.0)),
        ("check_pref/length_beta+pref_weight", lambda: o.check_pref(length_beta=float("inf"), pref_weight=-1.0)),
        ("check_pref/pref_weight+label_smoothing", lambda: o.check_pref(pref_weight=-1.0, label_smoothing=0.5)),
        ("check_pref/label_smoothing_half", lambda: o.check_pref(label_smoothing=0.5)),
        ("check_pref/label_smoothing_negative", lambda: o.check_pref(label_smoothing=-0.1)),
        ("check_pref/label_smoothing_bool", lambda: o.check_pref(label_smoothing=True)),
        ("check_pref/label_smoothing_nan", lambda: o.check_pref(label_smoothing=float("nan"))),
        ("check_pref/label_smoothing_str", lambda: o.check_pref(label_smoothing="0.1")),
        ("check_pref/label_smoothing_huge_int", lambda: o.check_pref(label_smoothing=10 ** 400)),
        ("check_pref/label_smoothing+loss_type", lambda: o.check_pref(label_smoothing=0.7, loss_type="dpo")),
        ("check_pref/loss_type", lambda: o.check_pref(loss_type="dpo")),
        ("check_pref/loss_type+pairs", lambda: o.check_pref(loss_type="dpo", pairs="some")),
        ("check_pref/pairs", lambda: o.check_pref(pairs="some")),
        ("check_pref/pairs+smoothing_hinge", lambda: o.check_pref(pairs="some", label_smoothing=0.1, loss_type="hinge")),
        ("check_pref/smoothing_hinge", lambda: o.check_pref(label_smoothing=0.1, loss_type="hinge")),
        ("check_pref/smoothing_ipo+gamma_ipo", lambda: o.check_pref(label_smoothing=0.1, gamma=0.5, loss_type="ipo")),
        ("check_pref/gamma_ipo", lambda: o.check_pref(gamma=0.5, loss_type="ipo")),
        ("check_pref/gamma_ipo+ref_cum", lambda: o.check_pref(gamma=0.5, loss_type="ipo", ref_cum=f64(R))),
        ("check_pref/ref_cum_f64", lambda: o.check_pref(ref_cum=f64(R))),
        ("check_pref/ref_cum_list", lambda: o.check_pref(ref_cum=[0.0] * R, rows=R)),
        ("check_pref/ref_cum_strided", lambda: o.check_pref(ref_cum=f32(2 * R)[::2], rows=R)),
        ("check_pref/ref_cum_rows", lambda: o.check_pref(ref_cum=f32(R + 1), rows=R)),
        ("check_pref/ref_cum_other_device", lambda: o.check_pref(ref_cum=f32(R), rows=R, device=CUDA)),
        ("check_pref/ref_cum_device+k", lambda: o.check_pref(ref_cum=f32(R), rows=R, device=CUDA, k=0)),
        ("check_pref/k_17", lambda: o.check_pref(k=17)),
        ("check_pref/cost_f32", lambda: o.check_pref(cost=adv.float())),
        ("check_pref/cost_against_k", lambda: o.check_pref(k=3, cost=adv)),
        ("check_pref/cost_other_device", lambda: o.check_pref(cost=adv, device=CUDA)),
        ("check_pref/vid_off", lambda: o.check_pref(vid_off=[0, 5], n_sent=4)),
        ("check_pref/source", lambda: o.check_pref(source="greedy")),
        ("check_pref/utility", lambda: o.check_pref(utility="METEOR")),
        ("check_pref/cost_cpu", lambda: o.check_pref(cost=adv)),
        ("check_pref/cost_cpu+ref_cum_cpu", lambda: o.check_pref(cost=adv, ref_cum=f32(R))),
        ("check_pref/ref_cum_cpu", lambda: o.check_pref(ref_cum=f32(R), rows=R)),
        # ---- check_pg / group_advantage
        ("check_pg/clip_lo_1", lambda: o.check_pg(clip_lo=1.0)),
        ("check_pg/clip_lo_negative", lambda: o.check_pg(clip_lo=-1e-9)),
        ("check_pg/clip_lo_nan", lambda: o.check_pg(clip_lo=float("nan"))),
        ("check_pg/clip_lo_str", lambda: o.check_pg(clip_lo="0.2")),
        ("check_pg/clip_lo_bool", lambda: o.check_pg(clip_lo=True)),
        ("check_pg/clip_lo+clip_hi", lambda: o.check_pg(clip_lo=1.5, clip_hi=-1.0)),
        ("check_pg/clip_hi", lambda: o.check_pg(clip_hi=-1e-9)),
        ("check_pg/clip_hi+dual_clip", lambda: o.check_pg(clip_hi=float("inf"), dual_clip=1.0)),
        ("check_pg/dual_clip_1", lambda: o.check_pg(dual_clip=1.0)),
        ("check_pg/dual_clip_negative", lambda: o.check_pg(dual_clip=-3.0)),
        ("check_pg/dual_clip+kl_beta", lambda: o.check_pg(dual_clip=0.5, kl_beta=-1.0)),
        ("check_pg/kl_beta", lambda: o.check_pg(kl_beta=-1.0)),
        ("check_pg/kl_beta+eps", lambda: o.check_pg(kl_beta="1", eps=-1.0)),
        ("check_pg/eps", lambda: o.check_pg(eps=-1.0)),
        ("check_pg/eps+norm", lambda: o.check_pg(eps=True, norm="mean")),
        ("check_pg/norm", lambda: o.check_pg(norm="mean")),
        ("check_pg/norm_int", lambda: o.check_pg(norm=0)),
        ("check_pg/norm+advantage", lambda: o.check_pg(norm="mean", advantage="zscore")),
        ("check_pg/advantage", lambda: o.check_pg(advantage="zscore")),
        ("check_pg/advantage+kl_beta_without_ref", lambda: o.check_pg(advantage=1, kl_beta=0.04, has_ref=False)),
        ("check_pg/kl_beta_without_ref", lambda: o.check_pg(kl_beta=0.04, has_ref=False)),
        ("check_pg/kl_beta_without_ref_step", lambda: o.check_pg(kl_beta=0.04, rows=6, lt=3)),
        ("check_pg/kl_beta_without_ref+old_step", lambda: o.check_pg(kl_beta=0.04, rows=6, lt=3, old_step=st.double())),
        ("check_pg/old_step_f64", lambda: o.check_pg(rows=6, lt=3, old_step=st.double())),
        ("check_pg/old_step_strided", lambda: o.check_pg(rows=3, lt=3, old_step=st[::2])),
        ("check_pg/old_step_size", lambda: o.check_pg(rows=6, lt=3, old_step=st[:, :1])),
        ("check_pg/old_step_list", lambda: o.check_pg(rows=6, lt=3, old_step=st.tolist())),
        ("check_pg/old_step_f64_no_rows", lambda: o.check_pg(old_step=st.double())),
        ("check_pg/ref_step_rows", lambda: o.check_pg(rows=5, lt=3, ref_step=st)),
        ("check_pg/old_step+ref_step", lambda: o.check_pg(rows=5, lt=3, old_step=st, ref_step=st.double())),
        ("check_pg/old_step_other_device", lambda: o.check_pg(rows=6, lt=3, device=CUDA, old_step=st)),
        ("check_pg/ref_step_other_device", lambda: o.check_pg(rows=6, lt=3, device=CUDA, ref_step=st)),
        ("check_pg/ref_step_device+adv", lambda: o.check_pg(rows=6, lt=3, device=CUDA, ref_step=st, adv=adv.float())),
        ("check_pg/adv_f32", lambda: o.check_pg(adv=adv.float())),
        ("check_pg/adv_1d", lambda: o.check_pg(adv=adv[0])),
        ("check_pg/adv_list", lambda: o.check_pg(adv=adv.tolist())),
        ("check_pg/adv_f32+k", lambda: o.check_pg(adv=adv.float(), k=0)),
        ("check_pg/k_0", lambda: o.check_pg(k=0)),
        ("check_pg/k_17", lambda: o.check_pg(k=17)),
        ("check_pg/k_bool", lambda: o.check_pg(k=True)),
        ("check_pg/adv_17", lambda: o.check_pg(adv=f64(3, 17))),
        ("check_pg/adv_0", lambda: o.check_pg(adv=f64(3, 0))),
        ("check_pg/adv_against_k", lambda: o.check_pg(k=3, adv=adv)),
        ("check_pg/adv_other_device", lambda: o.check_pg(adv=adv, device=CUDA)),
        ("check_pg/vid_off_start", lambda: o.check_pg(vid_off=[1, 2, 3, 4], n_sent=4)),
        ("check_pg/vid_off_falls", lambda: o.check_pg(vid_off=[0, 2, 1, 4], n_sent=4)),
        ("check_pg/vid_off_end", lambda: o.check_pg(vid_off=[0, 5], n_sent=4)),
        ("check_pg/vid_off_empty", lambda: o.check_pg(vid_off=[], n_sent=0)),
        ("check_pg/vid_off_against_adv", lambda: o.check_pg(adv=gpu(adv), vid_off=[0, 1, 2])),
        ("check_pg/source", lambda: o.check_pg(source="greedy")),
        ("check_pg/source+utility", lambda: o.check_pg(source="greedy", utility="METEOR")),
        ("check_pg/utility", lambda: o.check_pg(utility="METEOR")),
        ("check_pg/adv_cpu", lambda: o.check_pg(adv=adv)),
        ("check_pg/adv_cpu+old_step_cpu", lambda: o.check_pg(adv=adv, rows=6, lt=3, old_step=st)),
        ("check_pg/old_step_cpu", lambda: o.check_pg(rows=6, lt=3, old_step=st)),
        ("check_pg/ref_step_cpu", lambda: o.check_pg(rows=6, lt=3, ref_step=st)),
        ("group_advantage/reward_f32", lambda: o.group_advantage(adv.float())),
        ("group_advantage/reward_1d", lambda: o.group_advantage(adv[0])),
        ("group_advantage/reward_str", lambda: o.group_advantage("grpo")),
        ("group_advantage/reward_17", lambda: o.group_advantage(f64(2, 17))),
        ("group_advantage/rule", lambda: o.group_advantage(adv, rule="zscore")),
        ("group_advantage/eps", lambda: o.group_advantage(adv, eps=-1.0)),
        ("group_advantage/eps+rule", lambda: o.group_advantage(adv, rule="zscore", eps=-1.0)),
        ("group_advantage/cpu", lambda: o.group_advantage(adv)),
    ]
    return out


def cases():
    """→ [(id, a call without arguments that must raise)]; the ids are unique"""
    out = _wrapper_cases() + _check_cases()
    assert len({i for i, _ in out}) == len(out)
    return out


def refuse_launch(name, *args):
    raise AssertionError("a wrong call reached the kernel library: %s" % name)


def run(call):
    """→ [exception type's name, message]"""
    try:
        call()
    except Exception as e:                # noqa: BLE001 (whatever it raises is the record)
        return [type(e).__name__, str(e)]
    return ["no exception", ""]
