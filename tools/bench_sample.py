"""Random-sampling decode throughput at BASELINE config 5 (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3 by default, hipGraph replay):
captions/s of Translator.translate_batch_sample for R = 1 and R = 4 samples per sentence, against greedy (translate_batch) and the
width-4 beam (translate_batch_beam) on the same batch in the same process, with the encoder-side and per-iteration milliseconds of one
eager call bracketed by HIP events (an upper bound on the replayed phases).  A caption is one sample (R per sentence) or one beam result
(one per sentence).  Prints one JSON line.

    python tools/bench_sample.py [--steps 10] [--warmup 2] [--videos 64] [--precision bf16x3] [--samples 1,4] [--beam 4]
                                 [--temp 1.0] [--topk 0] [--topp 0.0] [--profile-samples R]

With --profile-samples R only one replayed sampling decode of R samples runs (for rocprofv3 --kernel-trace --stats)."""
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
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--clips", type=int, default=12)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3", "fp32"])
    ap.add_argument("--samples", default="1,4")
    ap.add_argument("--beam", type=int, default=4)
    ap.add_argument("--temp", type=float, default=1.0)
    ap.add_argument("--topk", type=int, default=0)
    ap.add_argument("--topp", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--profile-samples", type=int, default=0)
    a = ap.parse_args(argv)
    kw = dict(random_sampling_temp=a.temp, random_sampling_topk=a.topk, random_sampling_topp=a.topp)
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
        tr = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=True)

        def call(tr_, leg):
            kind, n = leg
            if kind == "greedy":
                return tr_.translate_batch(syn.translate_inputs(b))
            if kind == "beam":
                return tr_.translate_batch_beam(syn.translate_inputs(b), n)
            return tr_.translate_batch_sample(syn.translate_inputs(b), n, seed=a.seed, **kw)

        if a.profile_samples:
            leg = ("sample", a.profile_samples)
            call(tr, leg)                              # eager warm-up twice + capture
            torch.cuda.synchronize()
            call(tr, leg)                              # the replayed decode
            torch.cuda.synchronize()
            print(json.dumps({"profiled": "one replayed sampling decode", "samples": a.profile_samples, "videos": a.videos,
                              "settings": kw}))
            return
        legs = {}
        sent = a.videos * a.clips
        runs = [("greedy", 0)] + [("sample", int(r)) for r in a.samples.split(",") if r] + ([("beam", a.beam)] if a.beam else [])
        for leg in runs:
            for _ in range(max(1, a.warmup)):
                call(tr, leg)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call(tr, leg)
            torch.cuda.synchronize()
            el = time.perf_counter() - t0
            tr_e = Translator(O(), {"model_cfg": cfg, "model": model.state_dict()}, model=model, graph=False)
            call(tr_e, leg)
            tr_e.phase_events = []
            call(tr_e, leg)
            torch.cuda.synchronize()
            e = tr_e.phase_events
            n_it = cfg.max_t_len - (1 if leg[0] != "greedy" else 0)
            caps = sent * (leg[1] if leg[0] == "sample" else 1)
            name = "greedy" if leg[0] == "greedy" else "%s%d" % leg
            legs[name] = {"captions_per_s": caps * a.steps / el, "sentences_per_s": sent * a.steps / el, "ms_per_batch": 1000.0 * el / a.steps,
                          "eager_encoder_side_ms": e[0].elapsed_time(e[1]), "eager_iterations": n_it,
                          "eager_ms_per_iteration": e[1].elapsed_time(e[2]) / n_it}
        g = legs["greedy"]["captions_per_s"]
        for v in legs.values():
            v["vs_greedy"] = v["captions_per_s"] / g
        ratios = {}
        if "sample1" in legs:
            ratios["sample1_vs_greedy"] = legs["sample1"]["captions_per_s"] / g
        if "sample%d" % a.beam in legs and "beam%d" % a.beam in legs:
            # the same decoder work (T·B rows), one caption per row for sampling and one per sentence for beam: compare sentences/s
            ratios["sample%d_vs_beam%d" % (a.beam, a.beam)] = legs["sample%d" % a.beam]["sentences_per_s"] / legs["beam%d" % a.beam]["sentences_per_s"]
        print(json.dumps({"metric": "random-sampling decode captions/sec (config 5)", "videos": a.videos, "clips": a.clips,
                          "precision": a.precision, "launch": "hipGraph replay per batch structure and setting", "steps": a.steps,
                          "settings": kw, "seed": a.seed, "legs": legs, "ratios": ratios}))


if __name__ == "__main__":
    main()
