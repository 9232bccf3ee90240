"""What a preference-optimisation training step costs at the training shape (16 videos × 12 clips, vivt, D = 768, L = 6; bf16x3, eager;
DESIGN §11.21).  Four legs on the same batch in one process, alternating (``--rounds`` of ``--steps`` steps each):

  risk       zero_grad, ``MinimumRisk.step(source="sample")`` at K = ``--samples``, backward, the optimizer: existing code, the yardstick;
  score      one stand-alone ``reference.score_captions`` pass over K candidates per sentence: existing code, the yardstick's second part;
  pref_ref   zero_grad, ``PreferenceOptimization(reference=a second model).step(source="sample")`` at the same K (DPO), backward, the optimizer;
  pref_free  the same step without a reference (SimPO).

``pref_ref`` is held against ``risk`` + ``score``, ``pref_free`` against ``risk`` alone.  The ``pref_ref`` leg is split by device events into
decode, rewards, reference, graded forward, backward and optimizer (medians over the timed steps).  The references the rewards are scored
against are the batch's own labels.  Prints one JSON line.

The measurement runs in a child process under a time limit of its own (``--timeout`` seconds; the parent never opens the GPU): a child that
hangs is killed and the tool exits with status 124.  ``--child`` runs the measurement in this process (e.g. under a profiler).

    python tools/bench_pref.py [--steps 5] [--warmup 2] [--rounds 3] [--videos 16] [--samples 4] [--precision bf16x3] [--timeout 600]
"""
import json
import os
import statistics
import subprocess
import sys

PHASES = ("decode", "rewards", "reference", "graded_forward", "backward", "optimizer")


def _take(argv, flag, default, kind):
    if flag in argv:
        i = argv.index(flag)
        v = kind(argv[i + 1])
        del argv[i:i + 2]
        return v
    return default


def measure(argv):
    from bench_scst import corpus_of
    from eval_tail_bench import alternate, arguments, config5
    samples = _take(argv, "--samples", 4, int)
    if "--videos" not in argv:
        argv += ["--videos", "16"]
    a = arguments(argv)
    import torch
    import bench
    from svpc_amd import mrt, ops, prefopt, synthetic as syn
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
        po = prefopt.PreferenceOptimization(tr, corpus, reference=reference)
        free = prefopt.PreferenceOptimization(tr, corpus)
        splits = []
        fixed = {}

        def finish(loss):
            backward_all(model, loss)
            ops.join_side()

        def risk():
            opt.zero_grad()
            r = mr.step(inputs, videos, num_candidates=samples, source="sample", rank_weight=1.0)
            fixed.setdefault("dec", r.dec_seq_list)
            finish(r.loss)
            opt.step()

        def score():
            with torch.no_grad():
                reference.score_captions(score_inputs, fixed["dec"])

        def pref(record=None):
            opt.zero_grad()
            po.phase_events = [] if record is not None else None
            r = po.step(inputs, videos, num_candidates=samples, source="sample", beta=0.1)
            ev = po.phase_events
            finish(r.loss)
            if ev is not None:
                po._stamp()
            opt.step()
            if ev is not None:
                po._stamp()
                record.append(ev)
            po.phase_events = None

        def pref_free():
            opt.zero_grad()
            r = free.step(inputs, videos, num_candidates=samples, source="sample", beta=2.0, gamma=0.5, length_beta=1.0)
            finish(r.loss)
            opt.step()

        legs_fn = (("risk", risk), ("score", score), ("pref_ref", lambda: pref(splits)), ("pref_free", pref_free))
        for _ in range(max(1, a.warmup)):
            risk()
            score()
            pref()
            pref_free()
        torch.cuda.synchronize()
        times = alternate(legs_fn, a.rounds, a.steps)
        torch.cuda.synchronize()
        legs = {k: {"ms_per_step_best": 1000.0 * min(v) / a.steps, "ms_per_step_median": 1000.0 * statistics.median(v) / a.steps,
                    "rounds": len(v)} for k, v in times.items()}
        legs["pref_ref"]["phases_ms_median"] = {p: statistics.median(ev[i].elapsed_time(ev[i + 1]) for ev in splits)
                                                for i, p in enumerate(PHASES)}
        med = {k: v["ms_per_step_median"] for k, v in legs.items()}
        best = {k: v["ms_per_step_best"] for k, v in legs.items()}
        out = {"metric": "preference-optimisation training step against the minimum-risk step plus one reference scoring pass (training shape, eager)",
               "videos": a.videos, "clips": a.clips, "samples": samples, "precision": a.precision, "steps": a.steps,
               "order": ", ".join(k for k, _ in legs_fn) + " alternating", "legs": legs,
               "pref_ref_vs_risk_plus_score_median": med["pref_ref"] / (med["risk"] + med["score"]),
               "pref_ref_vs_risk_plus_score_best": best["pref_ref"] / (best["risk"] + best["score"]),
               "pref_free_vs_risk_median": med["pref_free"] / med["risk"], "pref_free_vs_risk_best": best["pref_free"] / best["risk"]}
        print(json.dumps(out))


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--child" in argv:
        argv.remove("--child")
        return measure(argv)
    limit = _take(argv, "--timeout", 600, float)
    try:
        done = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + argv, timeout=limit)
    except subprocess.TimeoutExpired:
        print("bench_pref: the measurement did not finish within %g s and was killed" % limit, file=sys.stderr)
        return 124
    return done.returncode


if __name__ == "__main__":
    sys.exit(main())
