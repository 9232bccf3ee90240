"""What a minimum-risk training step costs next to the plain train step and the self-critical step at the training shape (16 videos × 12
clips, vivt, D = 768, L = 6; bf16x3, eager).  Three legs on the same batch in one process, alternating (``--rounds`` of
``--steps`` steps each):

  train      zero_grad, the model's forward, backward, the fused optimizer: the unchanged path;
  scst_mean  zero_grad, ``SelfCritical.step`` at K = ``--samples`` with the leave-one-out mean baseline, backward, the optimizer: the yardstick;
  risk       zero_grad, ``MinimumRisk.step(source="sample")`` at the same K (risk and rank terms both on), backward, the optimizer.

The risk leg runs the self-critical leg's phases — K samples, K reward calls, the graded pass — with the group kernel and the wider loss
reduction in place of ``scst_weights``.  It is split by device events into decode, rewards, graded forward, backward and optimizer (medians
over the timed steps).  The references the rewards are scored against are the batch's own labels.  Prints one JSON line.

    python tools/bench_risk.py [--steps 5] [--warmup 2] [--rounds 3] [--videos 16] [--samples 4] [--precision bf16x3]
"""
import json
import statistics
import sys

from bench_scst import corpus_of
from eval_tail_bench import alternate, arguments, config5

PHASES = ("decode", "rewards", "graded_forward", "backward", "optimizer")


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    samples = 4
    if "--samples" in argv:
        i = argv.index("--samples")
        samples = int(argv[i + 1])
        del argv[i:i + 2]
    if "--videos" not in argv:
        argv += ["--videos", "16"]
    a = arguments(argv)
    import torch
    from svpc_amd import mrt, ops, scst, synthetic as syn
    from svpc_amd.graph import backward_all
    from svpc_amd.optim import FusedBertAdam
    with config5(a) as (cfg, dev, b, decode):
        tr = decode.translator
        tr.graph = False                            # (the parameters move under the decodes: eager, as a training loop runs them)
        model = tr.model
        model.train()
        model.gumbel_noise = None
        opt = FusedBertAdam(list(model.named_parameters()), lr=1e-5, warmup=0.1, t_total=100000, grad_clip=1.0, ema_decay=-1.0)
        fargs = syn.forward_args(b)
        inputs = syn.translate_inputs(b)
        corpus, videos = corpus_of(cfg, b)
        sc = scst.SelfCritical(tr, corpus)
        mr = mrt.MinimumRisk(tr, corpus)
        splits = []

        def train():
            opt.zero_grad()
            loss = model(*fargs)[0]
            backward_all(model, loss)
            ops.join_side()
            opt.step()

        def critical():
            opt.zero_grad()
            r = sc.step(inputs, videos, num_samples=samples, baseline="mean")
            backward_all(model, r.loss)
            ops.join_side()
            opt.step()

        def risk(record=None):
            opt.zero_grad()
            mr.phase_events = [] if record is not None else None
            r = mr.step(inputs, videos, num_candidates=samples, source="sample", rank_weight=1.0)
            ev = mr.phase_events
            backward_all(model, r.loss)
            ops.join_side()
            if ev is not None:
                mr._stamp()
            opt.step()
            if ev is not None:
                mr._stamp()
                record.append(ev)
            mr.phase_events = None

        legs_fn = (("train", train), ("scst_mean", critical), ("risk", lambda: risk(splits)))
        for _ in range(max(1, a.warmup)):
            train()
            critical()
            risk()
        torch.cuda.synchronize()
        times = alternate(legs_fn, a.rounds, a.steps)
        torch.cuda.synchronize()
        legs = {k: {"ms_per_step_best": 1000.0 * min(v) / a.steps, "ms_per_step_median": 1000.0 * statistics.median(v) / a.steps,
                    "rounds": len(v)} for k, v in times.items()}
        legs["risk"]["phases_ms_median"] = {p: statistics.median(ev[i].elapsed_time(ev[i + 1]) for ev in splits) for i, p in enumerate(PHASES)}
        out = {"metric": "minimum-risk training step against the self-critical step and the plain train step (training shape, eager)",
               "videos": a.videos, "clips": a.clips, "samples": samples, "precision": a.precision, "steps": a.steps,
               "order": ", ".join(k for k, _ in legs_fn) + " alternating", "legs": legs,
               "risk_vs_scst_mean_median": legs["risk"]["ms_per_step_median"] / legs["scst_mean"]["ms_per_step_median"],
               "risk_vs_scst_mean_best": legs["risk"]["ms_per_step_best"] / legs["scst_mean"]["ms_per_step_best"],
               "risk_vs_train_median": legs["risk"]["ms_per_step_median"] / legs["train"]["ms_per_step_median"]}
        print(json.dumps(out))


if __name__ == "__main__":
    main()
