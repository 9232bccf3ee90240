#!/usr/bin/env python
"""Headline benchmark: train steps/sec of the state-aware recurrent transformer (MODEL_TYPE=vivt, batch 16 clip sequences
× 12 clips × 100 frames × 3072 features, D=768, 6+6+6 layers) on N MI355X, one process per GPU, RCCL gradient all-reduce.

A step = {zero_grad, forward, backward, gradient all-reduce (N>1), global clip 1.0, BertAdam} on one synthetic batch that
is already resident in HBM (reference: src/train.py:125-147 without EMA/logging).

  python bench.py --gpus 1 --steps 10 --warmup 3
  python bench.py --gpus N ...            # WORLD_SIZE unset: this process starts N fresh rank processes itself (before any GPU
                                          # call) and relays rank 0's JSON line; non-zero exit if any rank fails
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

Three arithmetic modes exist (svpc_amd.ops.set_precision).  ``value`` is measured in the FASTEST ONE THAT MEETS north_star's parity
bar (loss ≤ 1e-4 relative vs the CPU oracle, greedy ids bit-exact: tests/test_headline_parity.py, tests/test_config5_gpu.py):
``bf16x3`` — three-term split-bf16 products on the bf16 matrix cores.  The other two are timed on the same workload and printed
beside it: ``fastest_mode`` (bf16: bf16 operands and activation streams — faster, but its loss error is > 1e-4; the measured error
is quoted in the line) and ``parity_mode`` (fp32: f32 MFMA).

Prints ONE JSON line on rank 0: metric/value/unit/…/ms_per_step + "config".  A plain run does only what that needs: set up, warm
up, time the steps, write --dump-outputs, print.  ``--full`` adds, all after the timed region: "roofline" (dominant kernel; +
"attention": the clip-encoder attention launches against the HBM roofline — three instrumented eager steps of its own when the step
is replayed from a graph; an eager run brackets its timed steps and prints it either way) + "ragged" + "secondary" (config 5: greedy
decode, with its own roofline) + "fastest_mode" + "parity_mode" + "padded_text_rows" + "ceilings" (vendor GEMM / copy) +
"cpu_baseline"; with N > 1 ranks, exchange.ms_per_step_without_exchange.  ``--no-cpu-baseline`` / ``--no-secondary`` / ``--ragged 0``
trim a --full run.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFLOPS = {"fp32": 157.3, "bf16": 2500.0, "bf16x3": 2500.0}   # MI355X_MICROARCH.md dense peaks (f32-in MFMA; bf16 MFMA)
MFMA_TERMS = {"fp32": 1, "bf16": 1, "bf16x3": 3}      # bf16 MFMA products issued per algorithmic product (three-term split-bf16)
TRAFFIC_FILE = os.path.join(ROOT, "profiles", "dominant_gemm_traffic.json")
TRAFFIC_FILE_X3 = os.path.join(ROOT, "profiles", "dominant_gemm_x3_traffic.json")
PARITY_FILE = os.path.join(ROOT, "profiles", "headline_parity.json")     # written by tests/test_headline_parity.py on the GPU, committed
CONFIG5_PARITY_FILE = os.path.join(ROOT, "profiles", "config5_parity.json")   # tests/test_config5_gpu.py
DOMINANT_SOURCES = {"bf16": ("svpc_amd/csrc/gemm_p8.hip", "svpc_amd/csrc/gemm_common.h", "svpc_amd/csrc/common.h"),
                    "bf16x3": ("svpc_amd/csrc/gemm_p8x3.hip", "svpc_amd/csrc/gemm_common.h", "svpc_amd/csrc/common.h")}
HBM_PEAK_TBPS = 8.0          # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (≈6.3 achievable)
DUMP_MAX_BYTES = 64 << 20    # --dump-outputs: the whole dump
DUMP_SAMPLE, DUMP_SEED = 1 << 22, 0     # --dump-outputs: sampled gradient / weight elements (16 MB each in float32), fixed seed


def dominant_kernel_sha(precision="bf16"):
    h = hashlib.sha256()
    for rel in DOMINANT_SOURCES[precision]:
        with open(os.path.join(ROOT, rel), "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def measured_traffic(precision="bf16"):
    """HBM bytes per launch of the dominant kernel from the rocprofv3 PMC passes recorded in profiles/ (tools/pmc_traffic.py
    writes the file, stamped with the hash of the kernel's sources); None when the sources changed since that measurement."""
    try:
        with open(TRAFFIC_FILE_X3 if precision == "bf16x3" else TRAFFIC_FILE) as f:
            rec = json.load(f)
    except (OSError, ValueError):
        return None, None
    if rec.get("kernel_sources_sha16") != dominant_kernel_sha(precision):
        return None, "stale: %s was measured on other kernel sources" % os.path.basename(TRAFFIC_FILE_X3 if precision == "bf16x3" else TRAFFIC_FILE)
    return rec.get("traffic_bytes_per_launch"), rec.get("source")


def product_sources_sha16():
    """hash of the kernel sources and the host package (the same function as tests/helpers.py: the parity records are stamped with it)"""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "svpc_amd", "csrc", "*.hip")) + glob.glob(os.path.join(ROOT, "svpc_amd", "csrc", "*.h")) +
                   glob.glob(os.path.join(ROOT, "svpc_amd", "csrc", "*.cpp")) + glob.glob(os.path.join(ROOT, "svpc_amd", "*.py")))
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.relpath(f, ROOT).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def _load_record(path):
    """a committed parity record, or (None, reason) when it is missing or was made from other sources than the ones running now"""
    try:
        with open(path) as f:
            rec = json.load(f)
    except (OSError, ValueError):
        return None, "no record"
    sha = rec.pop("_sources_sha16", None)
    if sha != product_sources_sha16():
        return None, "stale: %s was recorded on other sources (%s, now %s) — re-run the GPU parity tests and commit the record" % (
            os.path.basename(path), sha, product_sources_sha16())
    return rec, None


def recorded_parity(precision):
    """worst loss error of the headline-shape parity test (vivt both weight sets, vi, viv) for this mode, from the committed record"""
    rec, why = _load_record(PARITY_FILE)
    if rec is None:
        return {"stale": why}
    rows = [v for k, v in rec.items() if not k.startswith("_") and len(k.split("/")) > 2 and k.split("/")[2] == precision]
    if not rows:
        return None
    flips = [v["gumbel_flips"] for v in rows if "gumbel_flips" in v]
    return {"loss_rel_vs_oracle_worst": max(v["loss_rel"] for v in rows), "argmax_agreement_worst": min(v["argmax_agreement"] for v in rows),
            "gumbel_flips_max": max(flips) if flips else None, "cases": len(rows), "meets_1e-4": max(v["loss_rel"] for v in rows) <= 1e-4,
            "source": "profiles/headline_parity.json (tests/test_headline_parity.py on the MI355X)"}


def recorded_config5(precision):
    rec, why = _load_record(CONFIG5_PARITY_FILE)
    if rec is None:
        return {"stale": why}
    rows = {k: v for k, v in rec.items() if not k.startswith("_") and len(k.split("/")) > 1 and k.split("/")[1] == precision}
    if not rows:
        return None
    ids = {k: v for k, v in rows.items() if isinstance(v, dict) and "token_agreement" in v}      # (8 videos x 12 clips vs the oracle)
    big = {k: v for k, v in rows.items() if isinstance(v, dict) and "equals_8x8" in v}            # (64 videos = 8 decodes of 8, bit for bit)
    if not ids and not big:
        return None
    out = {"source": "profiles/config5_parity.json (tests/test_config5_gpu.py: D=768, L=6, 8 videos x 12 clips vs oracle.greedy_decode; "
                     "64 videos x 12 clips = 8 decodes of 8)"}
    if ids:
        out["token_agreement_vs_oracle"] = {k.split("/")[0] + " weights": v["token_agreement"] for k, v in ids.items()}
        out["bit_exact"] = all(v.get("bit_exact", False) for v in ids.values())
    if big:
        out["64_videos_equal_8x8"] = all(bool(v.get("equals_8x8")) and bool(v.get("chunk_vs_oracle_bit_exact", True)) for v in big.values())
    return out


def parse_args(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--model-type", default="vivt")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--clips", type=int, default=12)
    ap.add_argument("--layers", type=int, default=6)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--heads", type=int, default=12)
    ap.add_argument("--precision", default="bf16x3", choices=["bf16", "bf16x3", "fp32"],
                    help="arithmetic of the GEMM / attention products (accumulation, statistics and parameters are fp32 in all three): "
                         "bf16x3 = three-term split-bf16 (meets the <=1e-4 parity bar; default), bf16 = one-term (fastest), fp32 = f32 MFMA")
    ap.add_argument("--decode", action="store_true", help="only the secondary metric: greedy-decode captions/s (BASELINE config 5: 64 videos)")
    ap.add_argument("--decode-videos", type=int, default=64)
    ap.add_argument("--decode-full", action="store_true", help="decode with the reference-shaped loop (all Lt positions every iteration)")
    ap.add_argument("--decode-eager", action="store_true", help="launch the decode kernels eagerly instead of replaying the batch structure's hipGraph")
    ap.add_argument("--no-graph", action="store_true", help="launch every kernel eagerly instead of replaying a captured hipGraph")
    ap.add_argument("--backend", default="nccl", help="torch.distributed backend (nccl = RCCL; gloo only for single-GPU rehearsals)")
    ap.add_argument("--exchange-dtype", default="fp32", choices=["fp32", "bf16"],
                    help="wire format of the gradient buckets: fp32 (default: N ranks == one process with the N-fold batch, exactly) or "
                         "bf16 (half the xGMI bytes for one 2^-9 rounding per rank; error bounded in tests/test_dp_gloo.py)")
    ap.add_argument("--full", action="store_true",
                    help="also measure everything beyond the headline figure, after the timed region: roofline, ragged legs, config-5 decode, "
                         "the other arithmetic modes, the padded sentence layout, ceilings, the CPU baseline (N=1), the exposed exchange "
                         "time (N>1); --decode: its roofline.  Off by default: a plain run only sets up, warms up, times and prints")
    ap.add_argument("--ragged", type=int, default=20,
                    help="(--full) after the timed region: this many EAGER steps over batches of the structure the reference's loop feeds (S_b ~ U{3..16}, "
                         "E_b ~ U{1..31}, X_b in {0,1,2}), a different structure every step; printed as the `ragged` field (0 = skip)")
    ap.add_argument("--bucket-timeline", action="store_true",
                    help="record per-bucket issue / completion events of the gradient exchange (exchange.bucket_timeline_ms); ON by default "
                         "when more than one rank runs, so that the first multi-GPU record is diagnosable without a second run")
    ap.add_argument("--no-bucket-timeline", action="store_true", help="N > 1: do not record the per-bucket timeline")
    ap.add_argument("--rehearse-dp", action="store_true",
                    help="run the data-parallel code path (process group, three graphs, bucketed all-reduce) even with one rank")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="(--full) skip the CPU baseline")
    ap.add_argument("--no-pack-text", action="store_true",
                    help="run the sentence side over all T x Lt padded rows (default: over the valid tokens only — model.pack_text_rows)")
    ap.add_argument("--no-secondary", action="store_true", help="(--full) skip the ragged / decode / parity-mode / ceilings legs (N=1 only legs)")
    ap.add_argument("--cpu-videos", type=int, default=16, help="videos per CPU-baseline step (16 = the stated configuration)")
    ap.add_argument("--cpu-warmup", type=int, default=3)     # >= 3 warm-up + >= 5 timed steps, median
    ap.add_argument("--cpu-steps", type=int, default=5)
    ap.add_argument("--cpu-threads", type=int, default=0, help="0 = the CPUs this process may use (affinity / cgroup share), capped at the physical cores")
    ap.add_argument("--cpu-alt", action="store_true",
                    help="also time the oracle with one thread per PHYSICAL core of the box when that exceeds this process's CPU share "
                         "(measured on the round-3 box: 128 threads on a 16-CPU share = 59.9 s/step against 7.55 s/step with 16 — oversubscribed, so off by default)")
    ap.add_argument("--parity-steps", type=int, default=5)
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed as DIR/<name>.npy (float32 / float64, "
                         "at most 64 MB): train — loss, global gradient norm, per-parameter gradient and weight norms, a fixed seeded "
                         "sample of the gradients and updated weights; --decode — the greedy token ids")
    ap.add_argument("--dry-run", action="store_true",
                    help="launcher/rendezvous check without a GPU: every rank joins the process group, SUM-all-reduces a small CPU "
                         "gradient arena through GradReducer and rank 0 prints the JSON line (tests/test_bench_launcher.py)")
    ap.add_argument("--dry-run-fail-rank", type=int, default=-1, help="(with --dry-run) this rank exits 3 after the rendezvous")
    return ap.parse_args(argv)


# ------------------------------------------------------------------------------------------------ parent: start N ranks
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch_ranks(args, argv):
    """``--gpus N`` without a launcher: start N fresh rank processes (this process has made no GPU call and makes none), wait for
    all of them, relay rank 0's JSON line.  Exit code = first non-zero rank exit code.  The children never outlive this process:
    each runs in its own session (process group), SIGTERM / SIGINT reaching the parent (the driver's ``timeout``, Ctrl-C) are
    forwarded, and whatever ends the wait loop — a failed rank, a signal, an exception — terminates, then kills, every live child."""
    import signal
    import tempfile
    port = _free_port()
    procs = []
    out0 = tempfile.TemporaryFile(mode="w+")

    def stop_children(grace=5.0):
        live = [p for p in procs if p.poll() is None]
        for p in live:
            try:
                os.killpg(p.pid, signal.SIGTERM)          # the rank and anything it started (start_new_session: pgid == pid)
            except (ProcessLookupError, PermissionError):
                pass
        t_end = time.time() + grace
        while time.time() < t_end and any(p.poll() is None for p in live):
            time.sleep(0.1)
        for p in live:
            if p.poll() is None:
                try:
                    os.killpg(p.pid, signal.SIGKILL)
                except (ProcessLookupError, PermissionError):
                    pass

    class _Stop(Exception):
        pass

    def on_signal(signum, frame):
        raise _Stop(signum)
    old = {sig: signal.signal(sig, on_signal) for sig in (signal.SIGTERM, signal.SIGINT)}
    interrupted = None
    try:
        for r in range(args.gpus):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1",
                       MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
            procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + list(argv), env=env,
                                          stdout=out0 if r == 0 else subprocess.DEVNULL, stderr=None, start_new_session=True))
        # wait for all; a rank that dies must not leave the others blocked in a collective for ever: after the first failure the
        # remaining ranks get 20 s, then exactly these children are stopped
        failed_at = None
        while any(p.poll() is None for p in procs):
            if failed_at is None and any(p.poll() not in (None, 0) for p in procs):
                failed_at = time.time()
            if failed_at is not None and time.time() - failed_at > 20.0:
                stop_children()
            time.sleep(0.2)
    except _Stop as e:
        interrupted = int(e.args[0])
    finally:
        stop_children()
        for sig, h in old.items():
            signal.signal(sig, h)
    if interrupted is not None:
        print("[bench] interrupted by signal %d: ranks stopped" % interrupted, file=sys.stderr)
        sys.exit(128 + interrupted)
    codes = [p.returncode for p in procs]
    out0.seek(0)
    sys.stdout.write(out0.read())
    sys.stdout.flush()
    bad = [(r, c) for r, c in enumerate(codes) if c != 0]
    if bad:
        print("[bench] rank(s) failed: %s" % bad, file=sys.stderr)
        sys.exit(bad[0][1] if bad[0][1] > 0 else 1)


# ------------------------------------------------------------------------------------------------ worker
def build(args, device, model_type=None):
    import torch
    from svpc_amd import StateAwareRecursiveTransformer, make_config
    mt = model_type or args.model_type
    cfg = make_config(model_type=mt, hidden_size=args.hidden, num_hidden_layers=args.layers,
                      num_attention_heads=args.heads)
    torch.manual_seed(2019)
    model = StateAwareRecursiveTransformer(cfg)
    g = torch.Generator().manual_seed(2019)
    glove = 0.4 * torch.randn(cfg.vocab_size, cfg.word_vec_size, generator=g)
    verb = 0.4 * torch.randn(cfg.action_vocab_size, cfg.word_vec_size, generator=g)
    model.ingredient_embeddings.set_pretrained_embedding(glove.clone(), freeze=False)
    model.text_embeddings.set_pretrained_embedding(glove.clone(), freeze=False)
    if mt in ("vivt", "viv"):
        model.reasoner.set_pretrained_embedding(verb.clone(), freeze=False)
    if mt == "vivt":
        model.recipe_reasoner.set_pretrained_embedding(verb.clone(), freeze=False)
    return cfg, model.to(device)


def device_batch(cfg, args, device, seed, n_videos=None):
    import torch
    from svpc_amd import make_batch
    b = make_batch(cfg, n_videos=n_videos or args.batch, max_steps=args.clips, n_ingr=10, n_oov=0, seed=seed, full_clips=True)
    # one (S, N, ...) buffer per per-step list (what svpc_amd.input_pipeline builds on the device): the model consumes them in place
    stacked = ("video_features_list", "input_ids_list", "input_masks_list", "input_labels_list", "token_type_ids_list")
    from svpc_amd import keep_host_copy
    for k in stacked:
        host = b[k]
        buf = torch.stack(host).to(device)
        b[k] = [buf[s] for s in range(buf.shape[0])]
        if k == "input_masks_list":          # the loader's host copy of the masks: the sentence lengths without a read-back (TextPack)
            b[k] = [keep_host_copy(t, h) for t, h in zip(b[k], host)]
    for k, v in list(b.items()):
        if k in stacked:
            continue
        if isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            b[k] = [t.to(device) for t in v]
        elif isinstance(v, torch.Tensor):
            b[k] = v.to(device)
    return b


def host_cpus():
    """(physical cores of the box, logical CPUs, CPUs this process may use: affinity ∩ cgroup quota)"""
    logical = os.cpu_count() or 1
    cores = set()
    try:
        phys = core = None
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("physical id"):
                    phys = line.split(":")[1].strip()
                elif line.startswith("core id"):
                    core = line.split(":")[1].strip()
                elif not line.strip():
                    if phys is not None and core is not None:
                        cores.add((phys, core))
                    phys = core = None
    except OSError:
        pass
    physical = len(cores) or max(1, logical // 2)
    usable = logical
    try:
        usable = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        pass
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            quota, period = f.read().split()[:2]
            if quota != "max":
                usable = min(usable, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return physical, logical, usable


def cpu_baseline(cfg, model, args, threads=None, warmup=None, steps=None):
    """The CPU oracle (a port of the reference path, pinned to it by tests/golden) timed on this host's cores; reported next
    to the GPU number, never the target.  The stated configuration (all 16 videos of a step), BASELINE.md §3's protocol
    (3 warm-up + 5 timed steps, median), as many threads as this process may use (capped at the physical cores)."""
    import torch
    from oracle import svpc_oracle as orc
    from svpc_amd import make_batch, synthetic as syn
    n_vid = args.cpu_videos
    physical, logical, usable = host_cpus()
    if threads is None:
        threads = args.cpu_threads if args.cpu_threads > 0 else min(physical, usable)
    warmup = args.cpu_warmup if warmup is None else warmup
    steps = args.cpu_steps if steps is None else steps
    torch.set_num_threads(max(1, min(threads, logical)))
    b = make_batch(cfg, n_videos=n_vid, max_steps=args.clips, n_ingr=10, n_oov=0, seed=7, full_clips=True)
    P = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    names = [k for k, v in P.items() if v.dtype.is_floating_point and not k.endswith(".pe")]
    state = {}
    wd = {n: (0.0 if any(t in n for t in ("bias", "LayerNorm.bias", "LayerNorm.weight")) else 0.01) for n in names}

    step_no = [0]

    def one_step():
        for n in names:
            P[n].requires_grad_(True)
            P[n].grad = None
        total, _, _, _ = orc.forward(P, cfg, *syn.forward_args(b), training=True)
        total.backward()
        grads = {n: P[n].grad for n in names if P[n].grad is not None}
        with torch.no_grad():
            for n in names:
                P[n].requires_grad_(False)
            # global clip 1.0 → BertAdam (warm-up-linear lr) in the reference's order; pinned by tests/golden/optim.npz
            orc.train_tail_step({n: P[n] for n in grads}, grads, state, None, step_no[0], 1e-4, 0.1, 100000, grad_clip=1.0, wd=wd)
        step_no[0] += 1
    for _ in range(max(0, warmup)):
        one_step()
    times = []
    for _ in range(max(1, steps)):
        t0 = time.time()
        one_step()
        times.append(time.time() - t0)
    dt = sorted(times)[len(times) // 2]
    steps_per_s = (n_vid / float(args.batch)) / dt
    cpu_model = "?"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    cpu_model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    scaled = "" if n_vid == args.batch else ", scaled by %d/%d (a lower bound: the CPU's GEMMs are %dx smaller than at the stated batch)" % (
        n_vid, args.batch, args.batch // max(1, n_vid))
    return {"value": steps_per_s, "unit": "steps/s (16-video steps)", "cores": torch.get_num_threads(), "kind": "port",
            "cpu": "%s: %d physical cores, %d logical cpus on the box, %d usable by this process (affinity / cgroup share)"
                   % (cpu_model, physical, logical, usable),
            "sample": "%d of %d videos per step (S=%d, L=%d, same model and step definition: fwd+bwd+global clip+BertAdam, torch-CPU "
                      "fp32, dropout on), %d warm-up + %d timed steps, median %.2f s/step%s"
                      % (n_vid, args.batch, args.clips, args.layers, warmup, len(times), dt, scaled)}


def _save_outputs(dump_dir, arrays):
    """{name: float32 / float64 ndarray} → dump_dir/<name>.npy"""
    import numpy as np
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_MAX_BYTES, "output dump of %d bytes exceeds %d" % (total, DUMP_MAX_BYTES)
    os.makedirs(dump_dir, exist_ok=True)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        np.save(os.path.join(dump_dir, name + ".npy"), a)


def dump_train_outputs(dump_dir, opt, loss):
    """What the last timed train step hands its caller: the loss, and the gradients and updated parameters it leaves behind.  Every
    trained tensor contributes its gradient and weight norm (float64); the elements themselves as one fixed, seeded sample of
    DUMP_SAMPLE positions.  Tensors are taken in parameter-name order, so the files do not depend on the arena's layout."""
    import numpy as np
    import torch
    arena = opt.ensure_built()
    params = [p for _, p in sorted(zip(arena.names, arena.params), key=lambda e: e[0])]
    with torch.no_grad():
        grads = torch.cat([p.grad.reshape(-1) for p in params])
        weights = torch.cat([p.detach().reshape(-1) for p in params])
        n = grads.numel()
        pick = (np.arange(n) if n <= DUMP_SAMPLE else
                np.unique(np.random.RandomState(DUMP_SEED).randint(0, n, size=DUMP_SAMPLE)))
        pick_d = torch.from_numpy(pick).to(grads.device)
        out = {"loss": np.array([float(loss)], np.float64),
               "grad_global_norm": np.array([float(opt.grad_norm())], np.float64),
               "grad_norms": torch.stack([p.grad.double().norm() for p in params]).cpu().numpy(),
               "weight_norms": torch.stack([p.detach().double().norm() for p in params]).cpu().numpy(),
               "grad_sample": grads[pick_d].float().cpu().numpy(),
               "weight_sample": weights[pick_d].float().cpu().numpy()}
    _save_outputs(dump_dir, out)


def run_decode(cfg, model, args, device, world, rank, dist, steps, warmup, dump_dir=None, roofline=True):
    """captions/s of Translator.translate_batch (greedy) on synthetic clips, videos sharded over ranks (replicas only); ``roofline``:
    also the phase roofline, from two eager calls of its own after the timed region."""
    import torch
    from svpc_amd import make_batch, synthetic as syn
    from svpc_amd.translator import Translator
    n_vid = args.decode_videos
    b = make_batch(cfg, n_videos=n_vid, max_steps=args.clips, n_ingr=10, n_oov=0, seed=2019 + rank, full_clips=True)
    # the three ingredient arrays reach translate_batch as host lists, as the reference's collate hands them (src/translator.py:181-183)
    b["_ingr_host_lists"] = (b["ingr_input_ids"].tolist(), b["ingr_masks"].tolist(), b["ingr_sep_masks"].tolist())
    for k, v in list(b.items()):
        if isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
            b[k] = [t.to(device) for t in v]
        elif isinstance(v, torch.Tensor):
            b[k] = v.to(device)
    tr = Translator(type("O", (), {"cuda": True})(), {"model_cfg": cfg, "model": model.state_dict()}, model=model,
                    incremental=not args.decode_full, graph=not args.decode_eager)
    for _ in range(max(1, warmup)):
        tr.translate_batch(syn.translate_inputs(b))
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        out, _ = tr.translate_batch(syn.translate_inputs(b))
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if dump_dir is not None and rank == 0:
        # the last timed call's greedy ids, one (clips, Lt) block per video in batch order (ids < 2^24: exact in float32)
        _save_outputs(dump_dir, {"decode_ids": torch.cat(out).float().cpu().numpy()})
    caps = world * steps * n_vid * args.clips
    # roofline of the decode, from ONE eager call bracketed with HIP events at its two phase boundaries (after the timed region; the
    # timed calls replay a hipGraph, inside which events cannot be recorded): encoder side (clip encoder over n_vid·S clips, step
    # encoder, simulator, memory) against the MFMA peak, and the Lt decoding iterations (one new token per sentence: weight-streaming
    # GEMVs) against HBM.  Algorithmic work per SURVEY §8(d): encoder side 5.9e10·(L/6) FLOP per video (the train forward's clip
    # encoder + step encoder + simulator), an iteration reads every decoder / head / pointer weight once (fp32 master weights).
    roof = None
    if roofline:
        try:
            from svpc_amd import ops as _ops
            tr_e = Translator(type("O", (), {"cuda": True})(), {"model_cfg": cfg, "model": model.state_dict()}, model=model,
                              incremental=not args.decode_full, graph=False)
            tr_e.translate_batch(syn.translate_inputs(b))
            tr_e.phase_events = []
            tr_e.translate_batch(syn.translate_inputs(b))
            torch.cuda.synchronize()
            e = tr_e.phase_events
            enc_ms, dec_ms = e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2])
            D_, L_, V_, F_, Lv_, Lt_ = cfg.hidden_size, cfg.num_hidden_layers, cfg.vocab_size, cfg.video_feature_size, cfg.max_v_len, cfg.max_t_len
            rows = n_vid * args.clips * Lv_
            enc_flop = 2.0 * rows * F_ * D_ + L_ * rows * (8.0 * D_ * D_ + 4.0 * D_ * cfg.intermediate_size + 4.0 * Lv_ * D_)
            terms = MFMA_TERMS[_ops.get_precision()]
            w_iter = (L_ * 5 * D_ * D_ + 2 * D_ * D_ + D_ * V_ + D_ * D_) * 4.0          # decoder layers (QKV, cross-Q, out) + head + Wing, fp32
            # (frac = the ALGORITHMIC product's FLOP over the peak, as the headline's roofline.frac; the three-term mode ISSUES `terms` × that
            # MFMA work: achieved_issued / frac_issued)
            roof = {"encoder_side": {"ms": enc_ms, "bound": "mfma", "algorithmic_flop": enc_flop, "mfma_terms_per_product": terms,
                                     "achieved": enc_flop / (enc_ms * 1e-3) / 1e12, "peak": MFMA_PEAK_TFLOPS[_ops.get_precision()],
                                     "unit": "TFLOP/s", "frac": enc_flop / (enc_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS[_ops.get_precision()],
                                     "achieved_issued": enc_flop * terms / (enc_ms * 1e-3) / 1e12,
                                     "frac_issued": enc_flop * terms / (enc_ms * 1e-3) / 1e12 / MFMA_PEAK_TFLOPS[_ops.get_precision()]},
                    "decoding_iterations": {"ms": dec_ms, "iterations": Lt_, "ms_per_iteration": dec_ms / Lt_, "bound": "hbm",
                                            "algorithmic_bytes_per_iteration": w_iter,
                                            "achieved": w_iter / (dec_ms / Lt_ * 1e-3) / 1e9, "peak": HBM_PEAK_TBPS * 1e3, "unit": "GB/s",
                                            "frac": w_iter / (dec_ms / Lt_ * 1e-3) / 1e12 / HBM_PEAK_TBPS,
                                            "note": "%d sentences advance one token per iteration through a chain of ~60 dependent launches "
                                                    "of 5-15 us each: the iterations are launch-latency-bound, not byte-bound" % (n_vid * args.clips)},
                    "measured": "one eager call bracketed with HIP events on the launch stream (eager launch overhead included: an upper "
                                "bound on the replayed graph's phase times; eager total %.2f ms vs replayed %.2f ms)"
                                % (enc_ms + dec_ms, 1000.0 * elapsed / steps)}
        except Exception as ex:  # noqa: BLE001
            roof = {"error": "%s: %s" % (type(ex).__name__, str(ex)[:200])}
    from svpc_amd import ops as _ops2
    prec = _ops2.get_precision()
    line = {"metric": "greedy-decode captions/sec (vivt, 64 videos)", "value": caps / elapsed, "unit": "captions/s",
            "n_gpus": world, "steps": steps, "warmup": warmup, "ms_per_step": 1000.0 * elapsed / steps,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": prec, "mode": prec, "parity": recorded_config5(prec), "roofline": roof, "data": "synthetic",
            "config": {"workload": "MODEL_TYPE=%s translate_batch greedy: %d videos/GPU x %d clips, Lt=%d, L=%d; %s, batched "
                                   "over videos, on-device pick"
                                   % (args.model_type, n_vid, args.clips, cfg.max_t_len, cfg.num_hidden_layers,
                                      "full decoder re-run per position (reference loop shape)" if args.decode_full
                                      else "KV-cached incremental decoder (one new token per sentence and iteration)"),
                       "launch": "eager" if args.decode_eager else
                                 ("hipGraph replay per batch structure (inputs copied into the captured buffers)" +
                                  ("; the two halves of the batch as two graphs on two streams (the launch-bound decoding iterations of one "
                                   "half beside the other's)" if (getattr(tr, "two_streams", False) and n_vid >= 2 * getattr(tr, "min_half", 8)) else ""))}}
    if not roofline:
        del line["roofline"]
    return line


def ragged_batches(cfg, args, device, n_structs, seed=4242, shared_features=False):
    """``n_structs`` batches with the structure the reference's loop really feeds (src/train.py:91-132 over
    recursive_caption_dataset.py:528-576): S_b ~ U{3..16} clips per video (the collate pads to the longest), E_b ~ U{1..31} ingredients,
    X_b in {0, 1, 2} out-of-vocabulary ingredient words, 16 videos; resident in HBM like the headline batch.  shared_features: every batch
    reads its frame features from ONE resident (16, N, L, F) buffer (drawn once) — what differs from batch to batch is the STRUCTURE
    (ids, masks, labels, ingredients, step counts), which is what the cold leg measures; a hundred batches then cost seconds to build."""
    import numpy as np
    import torch
    from svpc_amd import keep_host_copy, make_batch
    rng = np.random.RandomState(seed)
    out, clips = [], []
    stacked = ("video_features_list", "input_ids_list", "input_masks_list", "input_labels_list", "token_type_ids_list")
    bank_h = bank_d = None
    if shared_features:
        L_, F_ = cfg.max_v_len + cfg.max_t_len, cfg.video_feature_size
        bank_h = np.zeros((16, args.batch, L_, F_), np.float32)
        bank_h[:, :, 1:cfg.max_v_len - 1] = np.random.RandomState(seed).rand(16, args.batch, cfg.max_v_len - 2, F_).astype(np.float32)
        bank_d = torch.from_numpy(bank_h).to(device)
    for i in range(n_structs):
        S_b = rng.randint(3, 17, size=args.batch).tolist()
        E_b = rng.randint(1, 32, size=args.batch).tolist()
        X_b = [int(min(x, e)) for x, e in zip(rng.randint(0, 3, size=args.batch).tolist(), E_b)]
        b = make_batch(cfg, n_videos=args.batch, max_steps=max(S_b), step_nums=S_b, n_ingr=E_b, n_oov=X_b, seed=seed + 1 + i, full_clips=True,
                       feature_bank=bank_h)
        for k in stacked:
            if k == "video_features_list" and bank_d is not None:
                b[k] = [bank_d[s_] for s_ in range(max(S_b))]
                continue
            buf = torch.stack(b[k]).to(device)
            b[k] = [buf[s_] for s_ in range(buf.shape[0])]
        for k, v in list(b.items()):
            if k in stacked:
                continue
            if isinstance(v, list) and v and isinstance(v[0], torch.Tensor):
                b[k] = [t.to(device) for t in v]
            elif isinstance(v, torch.Tensor):
                b[k] = keep_host_copy(v.to(device), v) if k == "ingr_sep_masks" else v.to(device)     # the loader built it on the host
        out.append(b)
        clips.append(sum(S_b))
    return out, clips


def run_train(args, precision, device, world, rank, dist, steps, warmup, instrument=True, ragged=0, dump_dir=None, full=False):
    """Build model + optimizer in ``precision``, warm up, capture, time ``steps`` steps.  → dict (rank-0 view).  Legs that take steps
    of their own after the timed region (the replayed step's roofline, the exposed exchange time) run only with ``full``."""
    import torch
    from svpc_amd import ops, synthetic as syn
    from svpc_amd.graph import GraphedTrainStep, backward_all
    from svpc_amd.optim import FusedBertAdam, GradReducer
    ops.set_precision(precision)
    cfg, model = build(args, device)
    model.train()
    model.pack_text_rows = not args.no_pack_text
    batch = device_batch(cfg, args, device, seed=2019 + rank)
    fargs = syn.forward_args(batch)
    opt = FusedBertAdam(list(model.named_parameters()), lr=1e-4, warmup=0.1, t_total=100000, grad_clip=1.0, ema_decay=-1.0)
    exchange_on = world > 1 or args.rehearse_dp
    state = {"reducer": None}

    def step():
        if state["reducer"] is not None:
            state["reducer"].mark_step_start()
        opt.zero_grad()
        loss = model(*fargs)[0]
        backward_all(model, loss)
        arena = opt.ensure_built()
        if exchange_on:
            if state["reducer"] is None:
                # graph mode: the exchange runs between captured graphs (no hooks); eager mode: overlapped with backward
                state["reducer"] = GradReducer(arena, overlap=args.no_graph, force=args.rehearse_dp, wire_dtype=args.exchange_dtype,
                                               timeline=(args.bucket_timeline or (world > 1 and not args.no_bucket_timeline)))
                state["reducer"].mark_all_unlaunched()   # first step: hooks were not installed during this backward
            state["reducer"].finish()
        opt.step()
        return loss

    for _ in range(max(warmup, 2)):
        loss = step()
    torch.cuda.synchronize()
    reducer = state["reducer"]

    # ---- capture the step in hipGraphs: ≈600 launches per step would otherwise make it host-bound.  One GPU: one graph
    # (zero_grad → forward → backward → clip+BertAdam).  N GPUs: three graphs with the bucketed RCCL all-reduce issued
    # eagerly in between (svpc_amd/graph.py).  A failed capture is reported in config.degraded, never silently.
    graph, degraded = None, None
    eager_step = step
    if not args.no_graph:
        try:
            loss = None          # drop the last eager autograd graph before capture
            graph = GraphedTrainStep(model, opt, fargs, warmup=2, exchange=reducer if exchange_on else None)
            step = graph
            for _ in range(2):
                step()
            torch.cuda.synchronize()
        except Exception as e:  # noqa: BLE001
            degraded = "hipGraph capture failed (%s: %s)" % (type(e).__name__, str(e)[:200])
            print("[bench] %s - running eagerly" % degraded, file=sys.stderr)
            graph = None
            step = eager_step
            torch.cuda.synchronize()
    # host-side enqueue cost of one step (GPU idle at start, no sync at the end): tells whether the step is launch-bound
    th = time.perf_counter()
    loss = step()
    host_enqueue_ms = 1000.0 * (time.perf_counter() - th)
    torch.cuda.synchronize()
    # roofline leg: HIP events around every launch of the dominant kernel symbol.  Eager mode: inside the timed region.  Graph
    # mode: events cannot be recorded inside a replay, so the same kernels are bracketed in instrumented eager steps right after it.
    rows_enc = args.batch * args.clips * cfg.max_v_len
    bf16_stream = precision != "fp32" and ops.bf16_stream_ok(rows_enc, cfg.hidden_size, cfg.video_feature_size)
    glds = bf16_stream and ops.USE_GLDS      # weights come from the optimizer's bf16 shadow → direct-to-LDS kernel
    want_dt = ((1, 1, 1) if glds else (1, 0, 1)) if bf16_stream else (0, 0, 0)
    if precision == "bf16x3" and bf16_stream:
        want_dt = (2, 2, 2)                  # split operands and output (gemm_p8x3)

    def dom_select(d):
        M_, N_, K_, akc, bkc, adt, bdt, cdt = d
        return akc == 1 and bkc == 1 and (adt, bdt, cdt) == want_dt and M_ == rows_enc
    n_pairs_enc = args.batch * args.clips * cfg.num_attention_heads

    def attn_timer():
        return {"select": lambda n_pairs, mq, mk: n_pairs == n_pairs_enc and mq == cfg.max_v_len and mk == cfg.max_v_len, "fwd": [], "bwd": []}
    # eager steps are bracketed inside the timed region at no extra step; a replayed step needs instrumented eager steps of its own
    instrument = instrument and (graph is None or full)
    if graph is None and instrument:
        ops.GEMM_TIMER = ops.KernelTimer(select=dom_select)
        ops.ATTN_TIMER = attn_timer()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    final_loss = float(loss.item())
    if dump_dir is not None and rank == 0:
        dump_train_outputs(dump_dir, opt, loss)      # before any later leg steps the model again
    # exposed exchange time: the same steps with the all-reduce calls skipped (gradients stay local — timing only, after the
    # timed region); difference of the two = what the exchange adds to a step after overlap
    no_exchange_ms = None
    if full and exchange_on and reducer is not None and world > 1:
        reducer.skip = True
        for _ in range(2):
            step()
        dist.barrier()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(steps):
            step()
        dist.barrier()
        torch.cuda.synchronize()
        no_exchange_ms = 1000.0 * (time.perf_counter() - t1) / steps
        reducer.skip = False
    gsum = None
    if instrument:
        if graph is not None:
            ops.GEMM_TIMER = ops.KernelTimer(select=dom_select)
            ops.ATTN_TIMER = attn_timer()
            with torch.cuda.stream(graph.stream):      # the stream every AccumulateGrad node of this model is bound to
                for _ in range(3):
                    eager_step()
            torch.cuda.synchronize()
        timer, ops.GEMM_TIMER = ops.GEMM_TIMER, None
        atimer, ops.ATTN_TIMER = ops.ATTN_TIMER, None
        gsum = timer.summary()
        # clip-encoder attention against the HBM roofline (north_star: ">= 60 % attention-roofline utilisation"): algorithmic bytes of a
        # launch (Q, K, V, O in their storage types; backward: + dO read, dQ / dK / dV written) over its bracketed duration
        asum = {}
        for which in ("fwd", "bwd"):
            recs = atimer[which]
            if recs:
                ms_a = sum(e0.elapsed_time(e1) for e0, e1, _ in recs) - gsum["event_overhead_ms"] * len(recs)
                by = sum(nb for _, _, nb in recs)
                asum[which] = {"launches": len(recs), "avg_launch_ms": ms_a / len(recs), "algorithmic_bytes_per_launch": by / len(recs),
                               "tbps": by / (ms_a * 1e-3) / 1e12 if ms_a > 0 else 0.0}
        if asum:
            tot_b = sum(v["algorithmic_bytes_per_launch"] * v["launches"] for v in asum.values())
            tot_ms = sum(v["avg_launch_ms"] * v["launches"] for v in asum.values())
            asum["bound"], asum["peak_tbps"] = "hbm", HBM_PEAK_TBPS
            asum["frac_fwd"] = asum["fwd"]["tbps"] / HBM_PEAK_TBPS if "fwd" in asum else None
            asum["frac_bwd"] = asum["bwd"]["tbps"] / HBM_PEAK_TBPS if "bwd" in asum else None
            asum["frac"] = tot_b / (tot_ms * 1e-3) / 1e12 / HBM_PEAK_TBPS if tot_ms > 0 else 0.0
    # ---- the batches the reference's loop really feeds: a different structure every step (no captured plan can be replayed), eager
    # launches, the host-side plan of every batch built inside the timed region (the model's plan caches are cleared each step)
    ragged_res = None
    if ragged > 0 and world == 1:
        try:
            rb, rclips = ragged_batches(cfg, args, device, n_structs=min(8, ragged))
            rargs = [syn.forward_args(b) for b in rb]
            st_r = graph.stream if graph is not None else torch.cuda.current_stream()

            def rstep(k):
                model._plans.clear(); model._ptr_plans.clear(); model._span_cache.clear()
                opt.zero_grad()
                l_ = model(*rargs[k % len(rargs)])[0]
                backward_all(model, l_)
                opt.step()
                return l_

            def rleg():
                with torch.cuda.stream(st_r):
                    tw0 = time.perf_counter()
                    for k in range(max(3, len(rargs))):          # every structure once: allocator and kernel-image warm-up
                        rstep(k)
                    torch.cuda.synchronize()
                    warm = time.perf_counter() - tw0
                    th0 = time.perf_counter()
                    for k in range(ragged):
                        lr_ = rstep(k)
                    host_r = time.perf_counter() - th0
                    torch.cuda.synchronize()
                    el_r = time.perf_counter() - th0
                return dict(steps_per_s=ragged / el_r, ms_per_step=1000.0 * el_r / ragged, host_enqueue_ms_per_step=1000.0 * host_r / ragged,
                            final_loss=float(lr_.item()), warmup_ms_per_step=1000.0 * warm / max(3, len(rargs)))
            avg_clips = sum(rclips[k % len(rclips)] for k in range(ragged)) / float(ragged)
            # (a) everything eager; (b) the clip encoder's forward / backward replayed from hipGraphs captured per clip count T (the only
            # way the batch structure enters it: svpc_amd/clip_graphs.py), the rest of the step eager.  The warm-up passes every structure
            # once, so (b)'s timed steps find their T captured — the steady state of a long run (a few dozen T values exist); what a cold
            # T costs is in `clip_graphs.capture_ms` (warm-up time per step of (b) minus that of (a)).
            from svpc_amd import clip_graphs
            clip_graphs.enable(model, False)
            eager_leg = rleg()
            cg, dg = clip_graphs.enable(model)
            try:
                graph_leg = rleg()
            finally:
                clip_graphs.enable(model, False)
            # (c) COLD: what the first epoch sees — a new structure every step from EMPTY graph caches, every capture inside the timed region
            # (clip counts are bucketed to multiples of 8, so at most 27 captures per family ever happen: svpc_amd/clip_graphs.py)
            cold = None
            n_cold = int(os.environ.get("SVPC_BENCH_COLD_STEPS", "100"))
            if n_cold > 0:
                cb, cclips = ragged_batches(cfg, args, device, n_structs=n_cold, seed=777, shared_features=True)
                cargs = [syn.forward_args(b) for b in cb]
                cg2, dg2 = clip_graphs.enable(model)          # fresh, empty caches
                try:
                    def cstep(k):
                        model._plans.clear(); model._ptr_plans.clear(); model._span_cache.clear()
                        opt.zero_grad()
                        l_ = model(*cargs[k])[0]
                        backward_all(model, l_)
                        opt.step()
                        return l_
                    with torch.cuda.stream(st_r):
                        torch.cuda.synchronize()
                        tc0 = time.perf_counter()
                        for k in range(n_cold):
                            lc_ = cstep(k)
                        host_c = time.perf_counter() - tc0
                        torch.cuda.synchronize()
                        el_c = time.perf_counter() - tc0
                    cold = dict(steps=n_cold, steps_per_s=n_cold / el_c, ms_per_step=1000.0 * el_c / n_cold,
                                host_enqueue_ms_per_step=1000.0 * host_c / n_cold, final_loss=float(lc_.item()),
                                captures=dict(clip_encoder=cg2.stats["captures"], decoder=dg2.stats["captures"]),
                                hits=dict(clip_encoder=cg2.stats["hits"], decoder=dg2.stats["hits"]),
                                distinct_clip_counts=len(set(cclips)), clip_count_buckets=len(set(-(-c // clip_graphs.T_BUCKET) for c in cclips)),
                                avg_clips_per_step=sum(cclips) / float(n_cold),
                                note="100 different structures in a row from empty graph caches, captures inside the timed region")
                finally:
                    clip_graphs.enable(model, False)
                del cb, cargs
            ragged_res = dict(graph_leg)
            ragged_res["cold"] = cold
            ragged_res.update({"steps": ragged, "distinct_structures": len(rargs), "distinct_clip_counts": len(set(rclips)),
                               "avg_clips_per_step": avg_clips, "clips_per_s": avg_clips * ragged_res["steps_per_s"],
                               "launch": "clip encoder and caption decoder: hipGraph replay per clip count T; step encoder, simulators, pointer, "
                                         "losses, optimizer: eager",
                               "clip_graphs": dict(cg.stats, decoder=dict(dg.stats),
                                                   capture_ms=graph_leg["warmup_ms_per_step"] - eager_leg["warmup_ms_per_step"]),
                               "eager_only": eager_leg,
                               "structure": "16 videos, S_b ~ U{3..16} clips, E_b ~ U{1..31} ingredients, X_b in {0,1,2} OOV words, a different "
                                            "structure every step (plan caches cleared: the host-side plan is rebuilt inside the timed region)"})
        except Exception as e:  # noqa: BLE001
            ragged_res = {"error": "%s: %s" % (type(e).__name__, str(e)[:300])}
    ms = 1000.0 * elapsed / steps
    launch = ("hipGraph replay" if not exchange_on else
              "hipGraph replay (fwd + text-side bwd | clip-encoder bwd beside the text-side all-reduce | remaining all-reduce | optimizer)") \
        if graph is not None else ("eager (capture failed: see config.degraded)" if degraded else "eager")
    pk = next(iter(model._pack_cache.values()), None) if getattr(model, "_pack_cache", None) else None
    text_rows = ("valid tokens only: %d of %d sentence rows (text embeddings, decoder, head, pointer mixture, caption loss, Gumbel bag of words)"
                 % (pk.R, len(pk.lens) * cfg.max_t_len)) if pk is not None else "padded: T x Lt sentence rows"
    res = dict(cfg=cfg, model=model, ms=ms, elapsed=elapsed, final_loss=final_loss, host_enqueue_ms=host_enqueue_ms, launch=launch, text_rows=text_rows,
               degraded=degraded, gsum=gsum, asum=(asum if instrument else None), glds=glds, bf16_stream=bf16_stream, rows_enc=rows_enc,
               no_exchange_ms=no_exchange_ms, ragged=ragged_res,
               allreduce_bytes=(reducer.bytes_per_step() if reducer is not None else 0),
               bucket_timeline=(reducer.timeline_ms() if reducer is not None else None),
               n_buckets=(len(reducer.buckets) if reducer is not None else 0))
    return res


def dry_run(args):
    """No GPU: rendezvous + one bucketed SUM all-reduce of a CPU arena through the product's GradReducer (gloo)."""
    import torch
    import torch.distributed as dist
    from svpc_amd.optim import GradArena, GradReducer
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", str(_free_port()))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    if rank == args.dry_run_fail_rank:
        sys.exit(3)
    params = [("w%d" % i, torch.nn.Parameter(torch.zeros(64, 33))) for i in range(5)]
    for i, (_, p) in enumerate(params):
        p.grad = torch.full_like(p, float(rank + 1) * (i + 1))
    arena = GradArena(params)
    red = GradReducer(arena, bucket_bytes=8 << 10, overlap=False)
    red.finish()
    want = sum(r + 1 for r in range(world))
    ok = all(float(p.grad.min()) == float(p.grad.max()) == want * (i + 1) for i, (_, p) in enumerate(params))
    joined = dist.get_world_size()
    dist.barrier()
    if rank == 0:
        print(json.dumps({"metric": "dry-run (launcher + rendezvous + bucketed SUM all-reduce on CPU)", "value": 0.0, "n_gpus": joined,
                          "rccl_ranks": joined, "config": {"gpus_requested": args.gpus, "buckets": len(red.buckets),
                                                            "allreduce_bytes_per_step": red.bytes_per_step(), "sum_ok": ok}}))
    dist.destroy_process_group()
    if not ok:
        sys.exit(4)


def worker(args):
    if args.dry_run:
        return dry_run(args)
    import torch
    from svpc_amd import ops
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    dist = None
    if world > 1 or args.rehearse_dp:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", str(_free_port()))
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        n_dev = torch.cuda.device_count()
        if world > n_dev and args.backend == "nccl":
            # RCCL needs one device per rank; sharing cards is a gloo-only rehearsal (tests) and is reported as such
            print("[bench] %d ranks requested but %d device(s) visible: refusing to share devices over RCCL (use --backend gloo for a "
                  "rehearsal on fewer cards)" % (world, n_dev), file=sys.stderr)
            sys.exit(5)
        dev_index = local_rank % max(1, n_dev)
        torch.cuda.set_device(dev_index)
        if args.backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", dev_index))
        else:
            dist.init_process_group(args.backend)
        joined = dist.get_world_size()
    else:
        dev_index = 0
        torch.cuda.set_device(0)
        joined = 1
    device = torch.device("cuda", dev_index)
    # everything (eager warm-up, capture, instrumented steps) runs on ONE non-default stream: autograd's AccumulateGrad nodes
    # are bound to the stream of the first backward, and a captured graph must not depend on the legacy default stream
    main_stream = torch.cuda.Stream(device=device)
    with torch.cuda.stream(main_stream):
        if args.decode:
            ops.set_precision(args.precision)
            cfg, model = build(args, device)
            out = run_decode(cfg, model, args, device, world, rank, dist if world > 1 else None, args.steps, args.warmup,
                             dump_dir=args.dump_outputs, roofline=args.full)
            if rank == 0:
                print(json.dumps(out))
        else:
            _train_main(args, device, world, rank, dist if (world > 1 or args.rehearse_dp) else None, joined)
    if dist is not None:
        dist.destroy_process_group()


def train_roofline(args, r):
    """the headline's ``roofline`` object: the dominant kernel's launches (and the clip-encoder attention's) bracketed by run_train"""
    precision, cfg, gsum = args.precision, r["cfg"], r["gsum"]
    terms = MFMA_TERMS[precision]
    achieved = terms * gsum["work"] / (gsum["ms"] * 1e-3) / 1e12 if gsum["ms"] > 0 else 0.0
    D_, F_, L_ = cfg.hidden_size, cfg.video_feature_size, cfg.num_hidden_layers
    n_l = max(1, gsum["launches"])
    alg_bytes, alg_flop = gsum["bytes"] / n_l, gsum["work"] / n_l
    default_cfg = (args.batch, args.clips, L_, D_, F_, args.model_type) == (16, 12, 6, 768, 3072, "vivt") and r["bf16_stream"]
    traffic, traffic_src = measured_traffic(precision) if (default_cfg and r["glds"]) else (None, None)
    if precision == "bf16x3" and r["bf16_stream"]:
        kname = ("gemm_p8x3_kernel (split-bf16 three-term product A_lo·B_hi + A_hi·B_hi + A_hi·B_lo on the bf16 matrix cores; operands and "
                 "output stored as two bf16 planes; 256x256 tiles, a staged buffer = hi and lo plane of one 32-deep k-slice of both operands "
                 "(24 MFMAs per 12 fragment reads), 8 phases per pair of buffers, both operands direct-to-LDS, v_mfma_f32_16x16x32_bf16)")
    elif r["glds"]:
        kname = ("gemm_p8_kernel (bf16·bf16→bf16, both operands direct-to-LDS, 256x256x64 tiles, 8 phases per pair of k-tiles, "
                 "v_mfma_f32_16x16x32_bf16)")
    else:
        kname = "gemm_bf16_kernel<128,128,NT,interior,8 waves,%s>" % ("bf16·f32→bf16" if r["bf16_stream"] else "f32")
    return {"bound": "mfma", "kernel": "%s — every forward projection of the clip-encoder activation stream (M=%d rows: "
                      "Q/K/V, attention-out, FFN, video embedding)" % (kname, r["rows_enc"]),
            # `achieved` / `frac`: SURVEY §8(d)'s algorithmic work (2·M·N·K per launch) ÷ the measured launch time — the roofline
            # fraction of the PRODUCT.  The three-term mode issues `mfma_terms_per_product` bf16 MFMA products per algorithmic
            # one: `achieved_issued` / `frac_issued` say how busy the matrix pipe is (its utilisation), not useful throughput.
            "achieved": achieved / terms, "peak": MFMA_PEAK_TFLOPS[precision], "unit": "TFLOP/s",
            "frac": achieved / terms / MFMA_PEAK_TFLOPS[precision],
            "achieved_issued": achieved, "frac_issued": achieved / MFMA_PEAK_TFLOPS[precision],
            "traffic": traffic, "traffic_source": traffic_src,
            "mfma_terms_per_product": terms,
            "algorithmic_flop_per_launch": alg_flop, "issued_mfma_flop_per_launch": alg_flop * terms,
            "algorithmic_bytes_per_launch": alg_bytes,
            "launches": gsum["launches"], "avg_launch_ms": gsum["ms"] / max(1, gsum["launches"]),
            "event_pair_overhead_ms": gsum["event_overhead_ms"],
            "measured": "HIP events on the launch stream (net of the calibrated empty event-pair time), " +
                        ("3 instrumented EAGER steps right after the timed graph replays (events cannot be recorded inside a replay; "
                         "rocprofv3's average over the replays is kept in profiles/ as the cross-check)"
                         if r["launch"].startswith("hipGraph") else "inside the timed region"),
            "attention": r["asum"]}


def _train_main(args, device, world, rank, dist, joined):
    import torch
    from svpc_amd import ops
    r = run_train(args, args.precision, device, world, rank, dist, args.steps, args.warmup,
                  ragged=(args.ragged if (args.full and world == 1 and not args.rehearse_dp and not args.no_secondary) else 0),
                  dump_dir=args.dump_outputs, full=args.full)
    cfg, gsum = r["cfg"], r["gsum"]
    extras = {}
    if args.full and world == 1 and not args.no_secondary and not args.rehearse_dp:
        # N=1-only legs, all after the timed region: config 5 (greedy decode, in the headline mode), the two other arithmetic modes
        # on the same workload, and the two same-box ceilings (vendor GEMM, copy bandwidth)
        try:
            ops.set_precision(args.precision)
            d = run_decode(cfg, r["model"], args, device, 1, 0, None, steps=3, warmup=2)
            extras["secondary"] = {k: d[k] for k in ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "dtype", "mode", "parity",
                                                     "roofline", "config")}
        except Exception as e:  # noqa: BLE001
            extras["secondary"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
        others = [("fastest_mode", "bf16", "bf16 operands (one-term products) and bf16 activation streams: the fastest arithmetic; its loss "
                                           "error exceeds north_star's 1e-4 (see parity), which is why it is not the headline"),
                  ("parity_mode", "fp32", "fp32 (v_mfma_f32_32x32x2_f32 GEMMs, fp32 attention and storage: 1/16 of the bf16 matrix rate)")]
        for key, prec, text in others:
            if prec == args.precision:
                continue
            try:
                p = run_train(args, prec, device, 1, 0, None, args.parity_steps, 2, instrument=False)
                extras[key] = {"precision": text, "mode": prec, "ms_per_step": p["ms"], "steps_per_s": 1000.0 / p["ms"],
                               "steps": args.parity_steps, "launch": p["launch"], "final_loss": p["final_loss"],
                               "degraded": p["degraded"], "parity": recorded_parity(prec)}
                if key == "fastest_mode":
                    try:
                        ops.set_precision(prec)
                        d2 = run_decode(cfg, p["model"], args, device, 1, 0, None, steps=3, warmup=2)
                        extras[key]["secondary"] = {"value": d2["value"], "unit": d2["unit"], "ms_per_step": d2["ms_per_step"],
                                                    "parity": d2["parity"]}
                    except Exception as e:  # noqa: BLE001
                        extras[key]["secondary"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
                del p
            except Exception as e:  # noqa: BLE001
                extras[key] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
        ops.set_precision(args.precision)
        if not args.no_pack_text:
            # the same step over the PADDED sentence layout (every one of the T x Lt rows, as the reference computes them): what the
            # valid-tokens-only run of the headline is worth, measured on this box
            try:
                import copy
                a2 = copy.copy(args)
                a2.no_pack_text = True
                p = run_train(a2, args.precision, device, 1, 0, None, args.parity_steps, 2, instrument=False)
                extras["padded_text_rows"] = {"text_rows": p["text_rows"], "ms_per_step": p["ms"], "steps_per_s": 1000.0 / p["ms"],
                                              "steps": args.parity_steps, "launch": p["launch"], "final_loss": p["final_loss"]}
                del p
            except Exception as e:  # noqa: BLE001
                extras["padded_text_rows"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
        try:
            sys.path.insert(0, os.path.join(ROOT, "tools"))
            import ceilings
            extras["ceilings"] = ceilings.measure(device, quick=True)
        except Exception as e:  # noqa: BLE001
            extras["ceilings"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    if rank != 0:
        return
    ms, elapsed = r["ms"], r["elapsed"]
    precision = args.precision
    dtype = {"bf16": "bf16", "fp32": "f32", "bf16x3": "bf16x3"}[precision]
    arithmetic = {"bf16": "bf16 MFMA operands (one-term products), fp32 accumulate, bf16 activation streams; statistics, losses, master "
                          "weights, optimizer fp32",
                  "fp32": "f32 MFMA, fp32 storage",
                  "bf16x3": "forward: three-term split-bf16 products on the bf16 MFMA (a_lo*b_hi + a_hi*b_lo + a_hi*b_hi), fp32 accumulate, "
                            "activations stored as two bf16 planes (clip encoder) or fp32; backward: bf16 operands (the hi planes); "
                            "statistics, losses, master weights, optimizer fp32"}[precision]
    out = {
        "metric": "train steps/sec (vivt, batch=16, clip_seq=12)", "value": joined * args.steps / elapsed,
        "unit": "steps/s (one step = 16 clip-sequences per GPU; whole-job aggregate)", "n_gpus": joined, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": dtype, "data": "synthetic",
        "config": {"workload": "MODEL_TYPE=%s train step: N=%d videos/GPU x S=%d clips x Lv=%d frames x F=%d, Lt=%d, D=%d, H=%d, "
                               "L=%d (enc+step-enc+dec), V=%d, A=%d, E=10; dropout .1/.1/.4; fwd+bwd+allreduce+clip+BertAdam"
                               % (args.model_type, args.batch, args.clips, cfg.max_v_len, cfg.video_feature_size, cfg.max_t_len,
                                  cfg.hidden_size, cfg.num_attention_heads, cfg.num_hidden_layers, cfg.vocab_size, cfg.action_vocab_size),
                   "mode": precision, "arithmetic": arithmetic, "parity": recorded_parity(precision),
                   "global_batch": args.batch * joined, "parallelism": "dp%d" % joined, "final_loss": r["final_loss"],
                   "host_enqueue_ms_per_step": r["host_enqueue_ms"], "launch": r["launch"], "degraded": r["degraded"],
                   "text_rows": r["text_rows"],
                   "gpus_requested": args.gpus},
    }
    if gsum is not None:
        out["roofline"] = train_roofline(args, r)
    if dist is not None:
        out["rccl_ranks"] = joined
        out["distinct_devices"] = min(joined, torch.cuda.device_count())      # < n_gpus only in a gloo rehearsal that shares cards
        out["exchange"] = {"backend": args.backend, "ranks_joined": joined, "allreduce_bytes_per_step": r["allreduce_bytes"], "buckets": r["n_buckets"],
                           "wire_dtype": args.exchange_dtype,
                           "op": "SUM over the fp32 gradient arena, before the global clip (src/train.py:140-143)",
                           # last step of the run: when each bucket's all-reduce was issued and when the compute stream could pass
                           # its wait, ms since the step's start on the compute stream's clock (diagnosis of an efficiency < 0.9)
                           "bucket_timeline_ms": r["bucket_timeline"],
                           "ms_per_step_without_exchange": r["no_exchange_ms"],
                           "exposed_exchange_ms": (ms - r["no_exchange_ms"]) if r["no_exchange_ms"] is not None else None}
    if r.get("ragged") is not None:
        rg = dict(r["ragged"])
        if "steps_per_s" in rg:
            # the uniform figure the ratio refers to is `value` (192 clips per step); a ragged step carries avg_clips_per_step clips
            rg["vs_uniform_steps_per_s"] = rg["steps_per_s"] / (joined * args.steps / elapsed)
            rg["vs_uniform_clips_per_s"] = rg["clips_per_s"] / (args.batch * args.clips * joined * args.steps / elapsed)
            if rg.get("cold"):
                rg["cold"]["vs_uniform_steps_per_s"] = rg["cold"]["steps_per_s"] / (joined * args.steps / elapsed)
            # the ragged legs run the PADDED sentence layout (the per-clip-count decoder graphs key on T only): like for like is the padded
            # uniform step of this box, when it was measured (`padded_text_rows`)
            pad = extras.get("padded_text_rows") or {}
            if pad.get("steps_per_s"):
                rg["vs_padded_uniform_steps_per_s"] = rg["steps_per_s"] / pad["steps_per_s"]
                if rg.get("cold"):
                    rg["cold"]["vs_padded_uniform_steps_per_s"] = rg["cold"]["steps_per_s"] / pad["steps_per_s"]
        out["ragged"] = rg
    out.update(extras)
    if args.full and world == 1 and not args.no_cpu_baseline and not args.rehearse_dp:
        out["cpu_baseline"] = cpu_baseline(cfg, r["model"], args)
        physical, logical, usable = host_cpus()
        if args.cpu_alt and args.cpu_threads <= 0 and physical > out["cpu_baseline"]["cores"]:
            # the box has more physical cores than this process's share: also time the oracle on all of them (1 + 3 steps)
            try:
                alt = cpu_baseline(cfg, r["model"], args, threads=physical, warmup=1, steps=3)
                out["cpu_baseline"]["all_physical_cores"] = {"value": alt["value"], "cores": alt["cores"], "sample": alt["sample"]}
            except Exception as e:  # noqa: BLE001
                out["cpu_baseline"]["all_physical_cores"] = {"error": "%s: %s" % (type(e).__name__, str(e)[:200])}
    print(json.dumps(out))


def main():
    argv = sys.argv[1:]
    args = parse_args(argv)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return launch_ranks(args, argv)
    worker(args)


if __name__ == "__main__":
    main()
