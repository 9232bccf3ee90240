"""What the distillation training steps cost next to their parts at the training shape (16 videos × 12 clips, vivt, D = 768, L = 6;
bf16x3, eager).  The legs run on the same batch in one process, alternating (``--rounds`` of ``--steps`` steps each):

  train            zero_grad, the model's forward, backward, the fused optimizer: the unchanged path;
  gold_nll         zero_grad, ``Translator.gold_captions`` and ``scst.sequence_loss`` on them (a constant w), backward, the optimizer: the
                   student's half of a word step, as it cost before this head;
  teacher_mM       the teacher's ``score_captions`` on the gold captions alone, eager, M ∈ {1, 2, 4} members: the teacher's half;
  word_mM          zero_grad, ``Distill.word_step`` against the M-member teacher (``teacher_scores``, the graded pass, ``ops.seq_kd``),
                   backward, the optimizer;
  sequence_m2      zero_grad, ``Distill.sequence_step`` (the 2-member teacher's beam-4 decode, its forced pass, the graded pass), backward,
                   the optimizer.

``word_mM`` is compared with gold_nll + teacher_mM + the larger of the two legs' run-to-run spreads (``over_parts_ms`` ≤ 0: no more than
its parts).  The teacher's members are the student's shape with parameters of other seeds; M = 1 is a plain ``Translator``.  Prints one
JSON line.  ``--profile M`` runs three gold_nll steps and three word steps against the M-member teacher and nothing else (for a kernel trace).

    python tools/bench_distill.py [--steps 5] [--warmup 2] [--rounds 3] [--videos 16] [--precision bf16x3] [--members 1,2,4] [--profile 2]
"""
import json
import statistics
import sys

from eval_tail_bench import alternate, arguments, config5


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--videos" not in argv:
        argv += ["--videos", "16"]
    members, profile = "1,2,4", 0
    for flag in ("--members", "--profile"):
        if flag in argv:
            i = argv.index(flag)
            val = argv[i + 1]
            del argv[i:i + 2]
            if flag == "--members":
                members = val
            else:
                profile = int(val)
    counts = [int(m) for m in members.split(",") if m]
    a = arguments(argv)
    import torch
    import bench
    from svpc_amd import ops, scst, synthetic as syn
    from svpc_amd.distill import Distill
    from svpc_amd.ensemble import EnsembleTranslator
    from svpc_amd.graph import backward_all
    from svpc_amd.optim import FusedBertAdam
    from svpc_amd.translator import Translator
    with config5(a) as (cfg, dev, b, decode):
        tr = decode.translator
        tr.graph = False                            # (the parameters move under the passes: eager, as a training loop runs them)
        model = tr.model
        model.train()
        model.gumbel_noise = None
        others = []
        for m in range(max(counts + [profile, 2])):     # the teacher's members: the student's shape, parameters from other seeds
            other = bench.build(bench.parse_args([]), dev)[1]
            drawn = syn.draw_parameters(list(other.named_parameters()), seed=100 + m)
            with torch.no_grad():
                for n, p in other.named_parameters():
                    p.copy_(drawn[n].to(dev))
            others.append(other)
        O = type("O", (), {"cuda": True})

        def teacher(M):
            if M == 1:
                return Translator(O(), {"model_cfg": cfg, "model": others[0].state_dict()}, model=others[0], graph=False)
            return EnsembleTranslator(O(), [{"model_cfg": cfg, "model": m.state_dict()} for m in others[:M]], others[:M], graph=False)
        opt = FusedBertAdam(list(model.named_parameters()), lr=1e-5, warmup=0.1, t_total=100000, grad_clip=1.0, ema_decay=-1.0)
        fargs = syn.forward_args(b)
        inputs = syn.translate_inputs(b)
        labels = b["input_labels_list"]
        T = sum(int(s) for s in b["batch_step_num"])
        w_gold = torch.full((T, 1), 1.0 / max(1, T * (cfg.max_t_len - 1)), device=dev)
        last = {}

        def finish(loss):
            backward_all(model, loss)
            ops.join_side()
            opt.step()

        def train():
            opt.zero_grad()
            finish(model(*fargs)[0])

        def gold_nll():
            opt.zero_grad()
            gold = [g.unsqueeze(1) for g in tr.gold_captions(labels, b["batch_step_num"])]      # (per call, as word_step forms them)
            finish(scst.sequence_loss(tr, inputs, gold, w_gold).loss)

        def teacher_leg(te):
            def run():
                te.score_captions(syn.translate_inputs(b), tr.gold_captions(labels, b["batch_step_num"]))
            return run

        def word_leg(step):
            def run():
                opt.zero_grad()
                r = step.word_step(inputs, labels, alpha=0.5)
                last["word"] = r
                finish(r.loss)
            return run

        def sequence_leg(step):
            def run():
                opt.zero_grad()
                finish(step.sequence_step(inputs, alpha=0.0, beam_size=4).loss)
            return run

        if profile:
            run = word_leg(Distill(tr, teacher(profile)))
            for _ in range(3):
                gold_nll()                          # (seq_nll's kernels on the same rows, for the comparison in one trace)
                run()
            torch.cuda.synchronize()
            print(json.dumps({"profiled": "three gold_nll steps and three word steps against an M-member teacher (eager)", "members": profile,
                              "videos": a.videos}))
            return
        teachers = {M: teacher(M) for M in counts}
        legs_fn = [("train", train), ("gold_nll", gold_nll)]
        for M in counts:
            legs_fn += [("teacher_m%d" % M, teacher_leg(teachers[M])), ("word_m%d" % M, word_leg(Distill(tr, teachers[M])))]
        legs_fn.append(("sequence_m2", sequence_leg(Distill(tr, teachers[2] if 2 in teachers else teacher(2)))))
        for _ in range(max(1, a.warmup)):
            for _, fn in legs_fn:
                fn()
        torch.cuda.synchronize()
        times = alternate(legs_fn, a.rounds, a.steps)
        torch.cuda.synchronize()
        legs = {k: {"ms_per_step_best": 1000.0 * min(v) / a.steps, "ms_per_step_median": 1000.0 * statistics.median(v) / a.steps,
                    "ms_spread": 1000.0 * (max(v) - min(v)) / a.steps, "rounds": len(v)} for k, v in times.items()}
        med = {k: v["ms_per_step_median"] for k, v in legs.items()}
        compare = {}
        for M in counts:
            spread = max(legs["gold_nll"]["ms_spread"], legs["teacher_m%d" % M]["ms_spread"])
            parts = med["gold_nll"] + med["teacher_m%d" % M]
            compare["word_m%d" % M] = {"ms": med["word_m%d" % M], "parts_ms": parts, "spread_ms": spread,
                                       "over_parts_ms": med["word_m%d" % M] - parts - spread}
        r = last["word"]
        out = {"metric": "distillation training steps against their parts (training shape, eager)", "videos": a.videos, "clips": a.clips,
               "precision": a.precision, "steps": a.steps, "order": ", ".join(k for k, _ in legs_fn) + " alternating", "legs": legs,
               "word_step_against_parts": compare, "sequence_vs_train_median": med["sequence_m2"] / med["train"],
               "last_word_step_kd_minus_ent": float((r.kd - r.ent).double().sum())}
        print(json.dumps(out))


if __name__ == "__main__":
    main()
