"""What a self-critical (CIDEr-reward) training step costs next to the plain train step at the training shape (16 videos × 12 clips, vivt,
D = 768, L = 6; bf16x3, eager).  Three legs on the same batch in one process, alternating (``--rounds`` of ``--steps``
steps each):

  train        zero_grad, the model's forward, backward, the fused optimizer: the unchanged path;
  scst_greedy  zero_grad, ``SelfCritical.step`` at K = ``--samples`` with the greedy baseline, backward, the optimizer;
  scst_mean    the same with the leave-one-out mean baseline (no greedy decode).

The self-critical legs are split by device events into sample, greedy, rewards (the K reward calls and the weights), graded forward,
backward and optimizer (medians over the timed steps); ``reward_share`` is the reward phase's share of the step.  The references the
rewards are scored against are the batch's own labels.  Prints one JSON line.

    python tools/bench_scst.py [--steps 5] [--warmup 2] [--rounds 3] [--videos 16] [--samples 4] [--precision bf16x3]
"""
import json
import statistics
import sys

from eval_tail_bench import alternate, arguments, config5

PHASES = ("sample", "greedy", "rewards", "graded_forward", "backward", "optimizer")


def corpus_of(cfg, b):
    """the batch's labels as every video's one reference paragraph"""
    from svpc_amd.caption_scores import ReferenceCorpus
    from svpc_amd.synthetic import EOS, IGNORE, PAD
    V = cfg.vocab_size
    i2w = ["[PAD]", "[CLS]", "[SEP]", "[VID]", "[BOS]", "[EOS]", "[UNK]"] + ["".join(chr(97 + (i // 26 ** k) % 26) for k in range(3))
                                                                               for i in range(7, V)]
    refs, videos = {}, []
    labels = [t.cpu().tolist() for t in b["input_labels_list"]]
    for v in range(len(b["batch_step_num"])):
        inv = {int(x): k for k, x in b["oov_word_dict"][v].items()}
        sents = [" ".join(i2w[x] if x < V else inv[x] for x in labels[s][v] if x not in (IGNORE, EOS, PAD))
                 for s in range(int(b["batch_step_num"][v]))]
        refs["vid%d" % v] = [" ".join(sents)]
        videos.append(dict(key="vid%d" % v, oov_word_dict=b["oov_word_dict"][v]))
    return ReferenceCorpus(i2w, refs, device=b["video_features_list"][0].device), videos


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
    from svpc_amd import ops, scst, synthetic as syn
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
        splits = {"scst_greedy": [], "scst_mean": []}

        def train():
            opt.zero_grad()
            loss = model(*fargs)[0]
            backward_all(model, loss)
            ops.join_side()
            opt.step()

        def critical(baseline, record=None):
            opt.zero_grad()
            sc.phase_events = [] if record is not None else None
            r = sc.step(inputs, videos, num_samples=samples, baseline=baseline)
            ev = sc.phase_events
            backward_all(model, r.loss)
            ops.join_side()
            if ev is not None:
                sc._stamp()
            opt.step()
            if ev is not None:
                sc._stamp()
                record.append(ev)
            sc.phase_events = None

        legs_fn = (("train", train), ("scst_greedy", lambda: critical("greedy", splits["scst_greedy"])),
                   ("scst_mean", lambda: critical("mean", splits["scst_mean"])))
        for _ in range(max(1, a.warmup)):
            train()
            critical("greedy")
            critical("mean")
        torch.cuda.synchronize()
        times = alternate(legs_fn, a.rounds, a.steps)
        torch.cuda.synchronize()
        legs = {k: {"ms_per_step_best": 1000.0 * min(v) / a.steps, "ms_per_step_median": 1000.0 * statistics.median(v) / a.steps,
                    "rounds": len(v)} for k, v in times.items()}
        for name, recs in splits.items():
            per = {p: statistics.median(ev[i].elapsed_time(ev[i + 1]) for ev in recs) for i, p in enumerate(PHASES)}
            legs[name]["phases_ms_median"] = per
            legs[name]["reward_share"] = per["rewards"] / sum(per.values())
        out = {"metric": "self-critical training step against the plain train step (training shape, eager)", "videos": a.videos,
               "clips": a.clips, "samples": samples, "precision": a.precision, "steps": a.steps,
               "order": ", ".join(k for k, _ in legs_fn) + " alternating", "legs": legs,
               "scst_greedy_vs_train_median": legs["scst_greedy"]["ms_per_step_median"] / legs["train"]["ms_per_step_median"],
               "scst_mean_vs_train_median": legs["scst_mean"]["ms_per_step_median"] / legs["train"]["ms_per_step_median"]}
        print(json.dumps(out))


if __name__ == "__main__":
    main()
