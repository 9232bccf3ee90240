"""What the two unlikelihood training steps cost next to the plain train step at the training shape (16 videos × 12 clips, vivt, D = 768,
L = 6; bf16x3, eager).  Four legs on the same batch in one process, alternating (``--rounds`` of ``--steps`` steps each):

  train          zero_grad, the model's forward, backward, the fused optimizer: the unchanged path;
  gold_nll       zero_grad, ``Translator.gold_captions`` and ``scst.sequence_loss`` on them (a constant w), backward, the optimizer: what
                 the graded pass cost before the unlikelihood head;
  token_step     zero_grad, ``Unlikelihood.token_step`` (the same pass, the same rows; ``ops.ul_negatives`` and ``ops.seq_ul`` as its head),
                 backward, the optimizer;
  sequence_step  zero_grad, ``Unlikelihood.sequence_step`` (a greedy decode, then the pass over it), backward, the optimizer.

``token_vs_gold_nll_median`` is the comparison that isolates the head.  The record also holds the repeat 4-grams (``nrep``) and
penalised positions (``npen``) of the last greedy decode the sequence step made, for the day there is a trained checkpoint to watch them
fall on.  Prints one JSON line.

    python tools/bench_unlikelihood.py [--steps 5] [--warmup 2] [--rounds 3] [--videos 16] [--precision bf16x3]
"""
import json
import statistics
import sys

from eval_tail_bench import alternate, arguments, config5


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    if "--videos" not in argv:
        argv += ["--videos", "16"]
    a = arguments(argv)
    import torch
    from svpc_amd import ops, scst, synthetic as syn
    from svpc_amd.graph import backward_all
    from svpc_amd.optim import FusedBertAdam
    from svpc_amd.unlikelihood import Unlikelihood
    with config5(a) as (cfg, dev, b, decode):
        tr = decode.translator
        tr.graph = False                            # (the parameters move under the decodes: eager, as a training loop runs them)
        model = tr.model
        model.train()
        model.gumbel_noise = None
        opt = FusedBertAdam(list(model.named_parameters()), lr=1e-5, warmup=0.1, t_total=100000, grad_clip=1.0, ema_decay=-1.0)
        fargs = syn.forward_args(b)
        inputs = syn.translate_inputs(b)
        labels = b["input_labels_list"]
        step = Unlikelihood(tr)
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
            gold = [g.unsqueeze(1) for g in tr.gold_captions(labels, b["batch_step_num"])]      # (per call, as token_step forms them)
            finish(scst.sequence_loss(tr, inputs, gold, w_gold).loss)

        def token_step():
            opt.zero_grad()
            finish(step.token_step(inputs, labels, alpha=1.0).loss)

        def sequence_step():
            opt.zero_grad()
            r = step.sequence_step(inputs, alpha=1.0, ngram=4, scope="paragraph")
            last["seq"] = r
            finish(r.loss)

        legs_fn = (("train", train), ("gold_nll", gold_nll), ("token_step", token_step), ("sequence_step", sequence_step))
        for _ in range(max(1, a.warmup)):
            for _, fn in legs_fn:
                fn()
        torch.cuda.synchronize()
        times = alternate(legs_fn, a.rounds, a.steps)
        torch.cuda.synchronize()
        legs = {k: {"ms_per_step_best": 1000.0 * min(v) / a.steps, "ms_per_step_median": 1000.0 * statistics.median(v) / a.steps,
                    "rounds": len(v)} for k, v in times.items()}
        r = last["seq"]
        med = {k: v["ms_per_step_median"] for k, v in legs.items()}
        out = {"metric": "unlikelihood training steps against the plain train step (training shape, eager)", "videos": a.videos,
               "clips": a.clips, "precision": a.precision, "steps": a.steps, "order": ", ".join(k for k, _ in legs_fn) + " alternating",
               "legs": legs, "token_vs_gold_nll_median": med["token_step"] / med["gold_nll"],
               "token_vs_train_median": med["token_step"] / med["train"], "sequence_vs_train_median": med["sequence_step"] / med["train"],
               "greedy_decode_repeat_4grams": int(r.nrep.sum()), "greedy_decode_penalised_positions": int(r.npen.sum())}
        print(json.dumps(out))


if __name__ == "__main__":
    main()
