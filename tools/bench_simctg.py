"""What the contrastive (SimCTG) training step costs next to its likelihood-only leg at the training shape (16 videos × 12 clips, vivt,
D = 768, L = 6; bf16x3, eager).  Three legs on the same batch in one process, alternating (``--rounds`` of ``--steps`` steps):

  train        zero_grad, the model's forward, backward, the fused optimizer: the unchanged path;
  token_nll    zero_grad, ``Unlikelihood.token_step(alpha=0)`` — the graded pass over the gold captions with the likelihood head alone —,
               backward, the optimizer: the yardstick;
  simctg_step  zero_grad, ``SimCTG.step`` (the same pass, the same rows, ``ops.seq_cl`` on the decoder's hidden states as a second head),
               backward, the optimizer.

Allowance = the yardstick's median + the time of the kernels the step adds (``--kernel-stats``: rocprofv3's kernel_stats.csv of a
``--trace`` run of this tool, taken on its own, without counters: seq_cl_fwd, seq_cl_loss, seq_cl_bwd per call and one rows_move call
for the fp32 copy of the hidden rows) + the yardstick's own spread (its slowest minus its fastest round).  The record also holds what the
two kernels move against what they must (R·Lt·D·4 bytes in, the same out) and the batch's mean self-similarity.  Prints one JSON line.

    python tools/bench_simctg.py [--steps 5] [--warmup 2] [--rounds 3] [--videos 16] [--precision bf16x3] [--kernel-stats CSV] [--trace]
"""
import csv
import json
import statistics
import sys

from eval_tail_bench import alternate, arguments, config5

ADDED = ("seq_cl_fwd_kernel", "seq_cl_loss_kernel", "seq_cl_bwd_kernel", "rows_move_kernel")


def kernel_times(path):
    """rocprofv3's kernel_stats.csv → {kernel: average µs per call} for the kernels the step adds"""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            for k in ADDED:
                # (rows_move: the instantiation that writes fp32, kind 0 — the copy out of the activation stream)
                if k in row["Name"] and (k != "rows_move_kernel" or ", 0>(" in row["Name"]):
                    out[k] = float(row["AverageNs"]) / 1000.0
    return out


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    stats = None
    if "--kernel-stats" in argv:
        i = argv.index("--kernel-stats")
        stats = argv[i + 1]
        del argv[i:i + 2]
    trace = "--trace" in argv                       # a short run of the step alone, for rocprofv3 --kernel-trace --stats
    if trace:
        argv.remove("--trace")
    if "--videos" not in argv:
        argv += ["--videos", "16"]
    a = arguments(argv)
    import torch
    from svpc_amd import ops, synthetic as syn
    from svpc_amd.graph import backward_all
    from svpc_amd.optim import FusedBertAdam
    from svpc_amd.simctg import SimCTG
    from svpc_amd.unlikelihood import Unlikelihood
    with config5(a) as (cfg, dev, b, decode):
        tr = decode.translator
        tr.graph = False
        model = tr.model
        model.train()
        model.gumbel_noise = None
        opt = FusedBertAdam(list(model.named_parameters()), lr=1e-5, warmup=0.1, t_total=100000, grad_clip=1.0, ema_decay=-1.0)
        fargs = syn.forward_args(b)
        inputs = syn.translate_inputs(b)
        labels = b["input_labels_list"]
        nll, step = Unlikelihood(tr), SimCTG(tr)
        last = {}

        def finish(loss):
            backward_all(model, loss)
            ops.join_side()
            opt.step()

        def train():
            opt.zero_grad()
            finish(model(*fargs)[0])

        def token_nll():
            opt.zero_grad()
            finish(nll.token_step(inputs, labels, alpha=0.0).loss)

        def simctg_step():
            opt.zero_grad()
            r = step.step(inputs, labels, margin=0.5, cl_weight=1.0)
            last["r"] = r
            finish(r.loss)

        if trace:
            for _ in range(max(1, a.warmup) + a.steps):
                simctg_step()
            torch.cuda.synchronize()
            print(json.dumps({"trace": "simctg_step", "calls": max(1, a.warmup) + a.steps}))
            return
        legs_fn = (("train", train), ("token_nll", token_nll), ("simctg_step", simctg_step))
        for _ in range(max(1, a.warmup)):
            for _, fn in legs_fn:
                fn()
        torch.cuda.synchronize()
        times = alternate(legs_fn, a.rounds, a.steps)
        torch.cuda.synchronize()
        legs = {k: {"ms_per_step_best": 1000.0 * min(v) / a.steps, "ms_per_step_median": 1000.0 * statistics.median(v) / a.steps,
                    "ms_per_step_worst": 1000.0 * max(v) / a.steps, "rounds": len(v)} for k, v in times.items()}
        r = last["r"]
        R, Lt, D = int(r.cl.numel()), cfg.max_t_len, cfg.hidden_size
        must = R * Lt * D * 4
        out = {"metric": "SimCTG training step against its likelihood-only leg (training shape, eager)", "videos": a.videos,
               "clips": a.clips, "precision": a.precision, "steps": a.steps, "order": ", ".join(k for k, _ in legs_fn) + " alternating",
               "legs": legs, "simctg_vs_token_nll_median": legs["simctg_step"]["ms_per_step_median"] / legs["token_nll"]["ms_per_step_median"],
               "simctg_vs_train_median": legs["simctg_step"]["ms_per_step_median"] / legs["train"]["ms_per_step_median"],
               "caption_rows": R, "lt": Lt, "d": D, "bytes_each_kernel_must_read": must, "bytes_the_backward_must_write": must,
               "mean_self_similarity": float(r.sim.double().mean()), "mean_cl": float(r.cl.double().mean()),
               "active_pairs": int(r.nact.sum())}
        if stats is not None:
            k = kernel_times(stats)
            y = legs["token_nll"]
            spread = y["ms_per_step_worst"] - y["ms_per_step_best"]
            added = sum(k.values()) / 1000.0
            out.update({"added_kernels_us": k, "added_kernels_ms": added, "yardstick_spread_ms": spread,
                        "allowance_ms": y["ms_per_step_median"] + added + spread,
                        "inside_allowance": legs["simctg_step"]["ms_per_step_median"] <= y["ms_per_step_median"] + added + spread,
                        "fwd_gb_per_s": must / (k["seq_cl_fwd_kernel"] * 1e3) if "seq_cl_fwd_kernel" in k else None,
                        "bwd_gb_per_s": 2 * must / (k["seq_cl_bwd_kernel"] * 1e3) if "seq_cl_bwd_kernel" in k else None})
        print(json.dumps(out))


if __name__ == "__main__":
    main()
