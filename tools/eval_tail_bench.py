"""The scaffold of the evaluation-tail benchmarks (bench_decode_metrics.py, bench_ingredient_f1.py, bench_caption_scores.py,
bench_consensus.py): the
BASELINE config 5 translator and batch (64 videos × 12 clips, vivt, D = 768, L = 6; bf16x3, hipGraph-replayed greedy decode) on the
device, timed legs that alternate, and a leg's statistics."""
import argparse
import contextlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def arguments(argv=None, profile=False):
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--videos", type=int, default=64)
    ap.add_argument("--clips", type=int, default=12)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3", "fp32"])
    if profile:
        ap.add_argument("--profile", action="store_true")
    return ap.parse_args(argv)


@contextlib.contextmanager
def config5(a):
    """On a side stream of device 0: → (cfg, dev, batch on the device, decode) with ``decode()`` = the first element of
    ``Translator.translate_batch`` of that batch (graph=True)."""
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

        def decode():
            return tr.translate_batch(syn.translate_inputs(b))[0]
        decode.translator = tr                     # (bench_consensus.py decodes K samples with the same translator)
        yield cfg, dev, b, decode


def run(fn, steps):
    """seconds of ``steps`` calls of ``fn``, device work included"""
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def alternate(legs, rounds, steps):
    """``legs`` = ((name, fn), …) run A B C A B C …, ``rounds`` of ``steps`` calls each → name → the rounds' seconds"""
    times = {name: [] for name, _ in legs}
    for _ in range(rounds):
        for name, fn in legs:
            times[name].append(run(fn, steps))
    return times


def leg(ts, a):
    sent = a.videos * a.clips
    return {"captions_per_s_best": sent * a.steps / min(ts), "captions_per_s_median": sent * a.steps / statistics.median(ts),
            "ms_per_batch_best": 1000.0 * min(ts) / a.steps, "ms_per_batch_median": 1000.0 * statistics.median(ts) / a.steps,
            "rounds": len(ts)}


def against_decode(prefix, u, d):
    """a leg ``u`` against the decode-only leg ``d`` → the three ``<prefix>_…`` entries of the result line"""
    return {prefix + "_vs_decode_best": u["captions_per_s_best"] / d["captions_per_s_best"],
            prefix + "_vs_decode_median": u["captions_per_s_median"] / d["captions_per_s_median"],
            prefix + "_ms_per_batch": u["ms_per_batch_median"] - d["ms_per_batch_median"]}
