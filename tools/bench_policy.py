"""What clipped policy-gradient training costs at the training shape (16 videos × 12 clips, vivt, D = 768, L = 6; bf16x3, eager; DESIGN
§11.22).  Five legs on the same batch in one process, alternating (``--rounds`` of ``--steps`` steps each):

  risk        zero_grad, ``MinimumRisk.step(source="sample")`` at K = ``--samples``, backward, the optimizer: existing code, the yardstick;
              its decode and reward phases are split off by device events;
  score_own   one stand-alone ``score_captions`` pass of the policy's own translator over the K candidates per sentence, in eval mode
              (the behaviour pass): existing code;
  score_ref   the same pass of a second model (the reference pass): existing code;
  policy      zero_grad, ``PolicyOptimization(reference=the second model).step(source="sample")`` at the same K (GRPO with a KL), backward,
              the optimizer;
  update      a SECOND ``update`` on a rollout collected before: zero_grad, the graded pass, backward, the optimizer — no decode, no rewards,
              no scoring pass.

``policy`` is held against ``risk`` + ``score_own`` + ``score_ref``, ``update`` against ``risk`` minus its decode and reward phases.  The
``policy`` leg is split by device events into decode, rewards, behaviour, reference, graded forward, backward and optimizer (medians over
the timed steps).  The references the rewards are scored against are the batch's own labels.  Prints one JSON line; ``--out PATH`` also
writes it to a file (``profiles/policy_bench.json`` is such a file).

The measurement runs in a child process under a time limit of its own (``--timeout`` seconds; the parent never opens the GPU): a child that
hangs is killed and the tool exits with status 124.  ``--child`` runs the measurement in this process (e.g. under a profiler).

    python tools/bench_policy.py [--steps 5] [--warmup 2] [--rounds 3] [--videos 16] [--samples 4] [--precision bf16x3] [--timeout 600] [--out PATH]
"""
import json
import os
import statistics
import subprocess
import sys

PHASES = ("decode", "rewards", "behaviour", "reference", "collected", "graded_forward", "backward", "optimizer")
RISK_PHASES = ("decode", "rewards", "graded_forward")


def _take(argv, flag, default, kind):
    if flag in argv:
        i = argv.index(flag)
        v = kind(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def measure(argv):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_scst import corpus_of
    from eval_tail_bench import alternate, arguments, config5
    samples = _take(argv, "--samples", 4, int)
    out_path = _take(argv, "--out", None, str)
    if "--videos" not in argv:
        argv += ["--videos", "16"]
    a = arguments(argv)
    import torch
    import bench
    from svpc_amd import mrt, ops, policy, synthetic as syn
    from svpc_amd.graph import backward_all
    from svpc_amd.optim import FusedBertAdam
    from svpc_amd.translator import Translator
    with config5(a) as (cfg, dev, b, decode):
        tr = decode.translator
        tr.graph = False                            # (the parameters move under the decodes: eager, as a training loop runs them)
        model = tr.model
        model.train()
        model.gumbel_noise = None
        opt = FusedBertAdam(list(model.named_parameters()), lr=1e-5, warmup=0.1, t_total=100000, grad_clip=1.0, ema_decay=-1.0)
        # the frozen reference: a second model of the same configuration with a translator of its own
        _, ref_model = bench.build(bench.parse_args([]), dev)
        O = type("O", (), {"cuda": True})
        reference = Translator(O(), {"model_cfg": cfg, "model": ref_model.state_dict()}, model=ref_model, graph=False)
        inputs = syn.translate_inputs(b)
        score_inputs = syn.translate_inputs(b)      # (copies of its own: score_captions blanks the text half in place)
        corpus, videos = corpus_of(cfg, b)
        mr = mrt.MinimumRisk(tr, corpus)
        po = policy.PolicyOptimization(tr, corpus, reference=reference)
        splits, risk_splits = [], []
        fixed = {}

        def finish(loss):
            backward_all(model, loss)
            ops.join_side()

        def risk(record=None):
            opt.zero_grad()
            mr.phase_events = [] if record is not None else None
            r = mr.step(inputs, videos, num_candidates=samples, source="sample", rank_weight=1.0)
            if record is not None:
                record.append(mr.phase_events)
            mr.phase_events = None
            fixed.setdefault("dec", r.dec_seq_list)
            finish(r.loss)
            opt.step()

        def score_own():
            model.eval()
            try:
                with torch.no_grad():
                    tr.score_captions(score_inputs, fixed["dec"])
            finally:
                model.train()

        def score_ref():
            with torch.no_grad():
                reference.score_captions(score_inputs, fixed["dec"])

        def step(record=None):
            opt.zero_grad()
            po.phase_events = [] if record is not None else None
            r = po.step(inputs, videos, num_candidates=samples, source="sample", kl_beta=0.04)
            ev = po.phase_events
            fixed["rollout"] = r.rollout
            finish(r.loss)
            if ev is not None:
                po._stamp()
            opt.step()
            if ev is not None:
                po._stamp()
                record.append(ev)
            po.phase_events = None

        def update():
            opt.zero_grad()
            r = po.update(fixed["rollout"], inputs, kl_beta=0.04)
            finish(r.loss)
            opt.step()

        legs_fn = (("risk", lambda: risk(risk_splits)), ("score_own", score_own), ("score_ref", score_ref), ("policy", lambda: step(splits)),
                   ("update", update))
        for _ in range(max(1, a.warmup)):
            risk()
            score_own()
            score_ref()
            step()
            update()
        torch.cuda.synchronize()
        times = alternate(legs_fn, a.rounds, a.steps)
        torch.cuda.synchronize()
        legs = {k: {"ms_per_step_best": 1000.0 * min(v) / a.steps, "ms_per_step_median": 1000.0 * statistics.median(v) / a.steps,
                    "rounds": len(v)} for k, v in times.items()}
        legs["policy"]["phases_ms_median"] = {p: statistics.median(ev[i].elapsed_time(ev[i + 1]) for ev in splits)
                                              for i, p in enumerate(PHASES) if p != "collected"}
        legs["risk"]["phases_ms_median"] = {p: statistics.median(ev[i].elapsed_time(ev[i + 1]) for ev in risk_splits)
                                            for i, p in enumerate(RISK_PHASES)}
        med = {k: v["ms_per_step_median"] for k, v in legs.items()}
        best = {k: v["ms_per_step_best"] for k, v in legs.items()}
        rp = legs["risk"]["phases_ms_median"]
        tail = med["risk"] - rp["decode"] - rp["rewards"]
        out = {"metric": "clipped policy-gradient training step against the minimum-risk step plus two scoring passes, and a second update "
                         "on one rollout against the minimum-risk step without its decode and rewards (training shape, eager)",
               "videos": a.videos, "clips": a.clips, "samples": samples, "precision": a.precision, "steps": a.steps,
               "order": ", ".join(k for k, _ in legs_fn) + " alternating", "legs": legs,
               "policy_vs_risk_plus_two_scores_median": med["policy"] / (med["risk"] + med["score_own"] + med["score_ref"]),
               "policy_vs_risk_plus_two_scores_best": best["policy"] / (best["risk"] + best["score_own"] + best["score_ref"]),
               "risk_minus_decode_and_rewards_ms_median": tail, "update_vs_risk_minus_decode_and_rewards_median": med["update"] / tail}
        line = json.dumps(out)
        print(line)
        if out_path:
            with open(out_path, "w") as f:
                f.write(line + "\n")


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--child" in argv:
        argv.remove("--child")
        return measure(argv)
    limit = _take(argv, "--timeout", 600, float)
    try:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + argv, timeout=limit)
    except subprocess.TimeoutExpired:
        print("bench_policy: the measurement did not finish within %g s and was killed" % limit, file=sys.stderr)
        return 124
    return done.returncode


if __name__ == "__main__":
    sys.exit(main())
