"""Contrastive search throughput at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3 by default, hipGraph replay): ms per
batch and captions/s of greedy (translate_batch), the width-k beam (translate_batch_beam) and contrastive search at top_k = k, penalty_alpha
= ``--alpha`` (translate_batch_contrastive), for every k of ``--widths``, all on the same batch in the same process.  Every leg is timed
``--reps`` times (``--steps`` batches each): ``ms_per_batch`` is the best repetition, ``ms_spread`` = max − min over the repetitions.  The
yardstick of the contrastive leg at width k is the beam leg at width k: the two run the same decoder passes over the same T·k rows, Lt of
them against Lt − 1, so ``allowance_ms`` = beam ms × Lt / (Lt − 1) + the beam leg's spread, and ``over_allowance_ms`` is what the contrastive
leg takes beyond it (negative: under).  Prints one JSON line.

    python tools/bench_contrastive.py [--steps 10] [--warmup 2] [--reps 3] [--videos 64] [--precision bf16x3] [--widths 4,8] [--alpha 0.6]
                                      [--profile-width K]

With --profile-width K only one replayed beam decode and one replayed contrastive decode at width K run (for rocprofv3 --kernel-trace
--stats: the step kernels' µs per launch side by side)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--clips", type=int, default=12)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3", "fp32"])
    ap.add_argument("--widths", default="4,8")
    ap.add_argument("--alpha", type=float, default=0.6)
    ap.add_argument("--profile-width", type=int, default=0)
    a = ap.parse_args(argv)
    import torch
    import bench
    from svpc_amd import make_batch, ops, synthetic as syn
    from svpc_amd.translator import Translator
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(stream):
        ops.set_precision(a.precision)
        args = bench.parse_args([])
        cfg, model = bench.build(args, dev)
        b = make_batch(cfg, n_videos=a.videos, max_steps=a.clips, n_ingr=10, n_oov=0, seed=2019, full_clips=True)
        b["_ingr_host_lists"] = (b["ingr_input_ids"].tolist(), b["ingr_masks"].tolist(), b["ingr_sep_masks"].tolist())
        for k, v in list(b.items()):
            if isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
                b[k] = [t.to(dev) for t in v]
            elif isinstance(v, torch.Tensor):
                b[k] = v.to(dev)
        O = type("O", (), {"cuda": True})

        def translator():
            return Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=True)

        def call(tr, kind, k):
            if kind == "greedy":
                return tr.translate_batch(syn.translate_inputs(b))
            if kind == "beam":
                return tr.translate_batch_beam(syn.translate_inputs(b), k)
            return tr.translate_batch_contrastive(syn.translate_inputs(b), top_k=k, penalty_alpha=a.alpha)

        if a.profile_width:
            tr = translator()
            for kind in ("beam", "contrastive"):
                call(tr, kind, a.profile_width)        # eager warm-up twice + capture
                torch.cuda.synchronize()
                call(tr, kind, a.profile_width)        # the replayed decode
                torch.cuda.synchronize()
            print(json.dumps({"profiled": "one replayed beam decode and one replayed contrastive decode", "width": a.profile_width,
                              "alpha": a.alpha, "videos": a.videos}))
            return
        sent = a.videos * a.clips
        Lt = cfg.max_t_len
        widths = [int(k) for k in a.widths.split(",") if k]
        legs = {}
        for kind, k in [("greedy", 1)] + [(kind, k) for k in widths for kind in ("beam", "contrastive")]:
            tr = translator()
            for _ in range(max(1, a.warmup)):
                call(tr, kind, k)
            torch.cuda.synchronize()
            times = []
            for _ in range(max(1, a.reps)):
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    call(tr, kind, k)
                torch.cuda.synchronize()
                times.append(1000.0 * (time.perf_counter() - t0) / a.steps)
            legs[kind if kind == "greedy" else "%s%d" % (kind, k)] = {
                "width": k, "ms_per_batch": min(times), "ms_spread": max(times) - min(times), "ms_repetitions": times,
                "captions_per_s": sent * 1000.0 / min(times)}
            del tr
        for k in widths:
            beam, con = legs["beam%d" % k], legs["contrastive%d" % k]
            con["allowance_ms"] = beam["ms_per_batch"] * Lt / (Lt - 1) + beam["ms_spread"]
            con["over_allowance_ms"] = con["ms_per_batch"] - con["allowance_ms"]
        print(json.dumps({"metric": "contrastive search ms per batch and captions/sec (config 5)", "videos": a.videos, "clips": a.clips,
                          "precision": a.precision, "launch": "hipGraph replay per batch structure and setting", "steps": a.steps,
                          "reps": a.reps, "alpha": a.alpha, "iterations": Lt, "legs": legs}))


if __name__ == "__main__":
    main()
