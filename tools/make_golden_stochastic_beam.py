"""Write tests/golden/stochastic_beam_config5.json: what the fp32 CPU restatement of stochastic beam search
(tests/stochastic_beam_reference.py) decodes at the sampling parity shape — config 5's model (vivt, parameters drawn from seed 7), 8 videos ×
12 clips drawn from seed 2021, W = 4, τ = 0.8, seed 2024.

    python tools/make_golden_stochastic_beam.py [--out tests/golden/stochastic_beam_config5.json]

Only results are recorded: per video the (S_b, 4, Lt) ids, the lengths, cum, G, phi and each sentence's smallest selection margin.  The
GPU test (tests/test_stochastic_beam_gpu.py) builds the same model and batch from the same seeds and compares its decode with these ids,
so the CPU decode — minutes of oracle time — runs here once and not in every run of the suite."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import bench  # noqa: E402
import stochastic_beam_reference as sbr  # noqa: E402
from svpc_amd import synthetic as syn  # noqa: E402

SHAPE = dict(videos=8, clips=12, beam_size=4, random_sampling_temp=0.8, min_length=0, seed=2024, param_seed=7, batch_seed=2021)


def model_and_batch():
    """config 5's model on the CPU with drawn parameters, and the parity batch — both from seeds alone"""
    args = bench.parse_args([])
    cfg, model = bench.build(args, "cpu", model_type="vivt")
    drawn = syn.draw_parameters(list(model.named_parameters()), seed=SHAPE["param_seed"])
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(drawn[n])
    model.eval()
    batch = syn.make_batch(cfg, n_videos=SHAPE["videos"], max_steps=SHAPE["clips"], n_ingr=10, n_oov=0, seed=SHAPE["batch_seed"],
                           full_clips=True)
    return cfg, model, batch


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "stochastic_beam_config5.json"))
    a = ap.parse_args(argv)
    cfg, model, c = model_and_batch()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    P = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ids, cums, lens, Gs, phis, margins = sbr.stochastic_beam_decode(
        P, cfg, c["input_ids_list"], c["video_features_list"], c["input_masks_list"], c["ingr_input_ids"], c["ingr_sep_masks"],
        c["batch_step_num"], c["ingr_id_dict"], c["oov_word_dict"], SHAPE["beam_size"], SHAPE["seed"], temp=SHAPE["random_sampling_temp"],
        min_length=SHAPE["min_length"])
    rec = dict(SHAPE, max_t_len=cfg.max_t_len, vocab_size=cfg.vocab_size, ids=[v.tolist() for v in ids], len=[v.tolist() for v in lens],
               cum=[[[float(x) for x in r] for r in v] for v in cums], G=[v.tolist() for v in Gs], phi=[v.tolist() for v in phis],
               margin=[v.tolist() for v in margins])
    with open(a.out, "w") as f:
        json.dump(rec, f)
    print("wrote %s: %d sentences, smallest margin %.3g" % (a.out, sum(len(v) for v in rec["ids"]), min(min(v) for v in rec["margin"])))


if __name__ == "__main__":
    main()
