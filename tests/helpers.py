"""Shared test helpers: build the product model from a golden fixture; decoded-caption lists for the evaluation metrics' tests; the digests
of the evaluation plans' device-facing tables; the recorder of kernel launches and the recorded training steps of the launch-sequence test."""
import ctypes
import hashlib
import json
import numbers
import os

import numpy as np
import torch

from oracle.cases import case_config_and_batch
from svpc_amd import model as M
from svpc_amd import synthetic as syn
from svpc_amd.model_shapes import parameter_shapes


def build_model(case, mt, golden_dir, device="cpu"):
    z = np.load(os.path.join(golden_dir, "%s_%s.npz" % (case, mt)))
    cfg, batch = case_config_and_batch(case, mt, device=device)
    model = M.StateAwareRecursiveTransformer(cfg)
    V, W, A = cfg.vocab_size, cfg.word_vec_size, cfg.action_vocab_size
    model.ingredient_embeddings.set_pretrained_embedding(torch.zeros(V, W), freeze=False)
    model.text_embeddings.set_pretrained_embedding(torch.zeros(V, W), freeze=False)
    if mt in ("vivt", "viv"):
        model.reasoner.set_pretrained_embedding(torch.zeros(A, W), freeze=False)
    if mt == "vivt":
        model.recipe_reasoner.set_pretrained_embedding(torch.zeros(A, W), freeze=False)
    if case.startswith("tiny"):
        sd = {k[len("param/"):]: torch.from_numpy(z[k]) for k in z.files if k.startswith("param/")}
    else:
        sd = syn.draw_parameters([(n, torch.empty(s)) for n, s in parameter_shapes(cfg, mt).items()], seed=7)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert all(k.endswith(".pe") for k in missing), missing
    model.to(device)
    model.eval()
    noise = [torch.from_numpy(z[k]).to(device) for k in sorted((k for k in z.files if k.startswith("gumbel/")),
                                                              key=lambda s: int(s.split("/")[1]))]
    model.gumbel_noise = noise or None
    return z, cfg, batch, model


def as_views(vids_rows, lt, dtype=torch.int64, device="cuda:0"):
    """per-video lists of id rows → per-video (S_b, lt) tensors that are consecutive views of one device buffer (what a decode returns)"""
    buf = torch.tensor([r for v in vids_rows for r in v], dtype=dtype, device=device).view(-1, lt)
    out, o = [], 0
    for v in vids_rows:
        out.append(buf[o:o + len(v)])
        o += len(v)
    return out


def host_rows(dec, row=None):
    return [(d if row is None else d[:, row]).cpu().tolist() for d in dec]


def _sha(t):
    a = np.ascontiguousarray(t.numpy() if torch.is_tensor(t) else t)
    return hashlib.sha256(("%s%s" % (a.dtype, a.shape)).encode() + a.tobytes()).hexdigest()


def eval_plan_digests(golden_dir):
    """SHA-256 (over dtype, shape and bytes) of every device-facing table the evaluation plans build on the CPU for the batches of
    ingredient_f1.json and caption_scores.json, one lexicon / corpus each, batches planned in file order
    (tests/golden/eval_plan_digests.json records them; tools/make_golden_eval_plan_digests.py)."""
    from svpc_amd.caption_scores import ReferenceCorpus
    from svpc_amd.ingredients import IngredientLexicon

    def plan_digest(plan):
        return dict(buf=_sha(plan.buf), sections=[[k, o, n] for k, (o, n) in plan.sections.items()])
    g = json.load(open(os.path.join(golden_dir, "ingredient_f1.json")))
    lex = IngredientLexicon(g["idx2word"], set(g["all_ingredients"]), device="cpu")
    ingredient = dict(a_bits=_sha(lex.a_bits), batches=[])
    for b in g["batches"]:
        plan = lex.plan([dict(ingredients=v["ingredients"], oov_word_dict=v["oov"], gt_sentences=v["gt_sentences"]) for v in b["videos"]])
        ingredient["batches"].append(dict(plan_digest(plan), n_rows=lex.n_rows, table=_sha(lex.table[:lex.n_rows])))
    g = json.load(open(os.path.join(golden_dir, "caption_scores.json")))
    corpus = ReferenceCorpus(g["idx2word"], g["references"], device="cpu")
    scores = {k: _sha(getattr(corpus, k)) for k in ("voc_off", "voc_tok", "ref_tok", "tab_key", "tab_idf", "gauss")}
    scores["batches"] = [plan_digest(corpus.plan([dict(key=v["key"], oov_word_dict=v["oov"]) for v in b["videos"]])) for b in g["batches"]]
    return dict(ingredient_f1=ingredient, caption_scores=scores)


class LaunchRecorder:
    """``with LaunchRecorder() as rec:`` — every kernel launch made through ``_lib.call`` inside the block is kept in ``rec.launches`` as
    [kernel name, [values of its non-pointer arguments]]: the arguments whose type in ``_lib.declarations()`` is not ``c_void_p`` (shapes,
    strides, flags, table entry counts); addresses and the stream are dropped, so two runs of the same code give the same record."""

    def __enter__(self):
        from svpc_amd import _lib
        decls, keep, inner = _lib.declarations(), {}, _lib.call
        self.launches = []
        self._lib, self._inner = _lib, inner

        def call(name, *args):
            k = keep.get(name)
            if k is None:
                k = keep[name] = [i for i, t in enumerate(decls["svpc_" + name][1]) if t is not ctypes.c_void_p]
            self.launches.append([name, [a if a is None else int(a) if isinstance(a, numbers.Integral) else float(a)
                                         for a in (args[i] for i in k)]])
            return inner(name, *args)
        _lib.call = call
        return self

    def __exit__(self, *exc):
        self._lib.call = self._inner
        return False


TRAIN_LAUNCH_CASES = [("tiny", "fp32"), ("c1", "bf16"), ("c1", "bf16x3")]      # (fixture, precision), model type vivt


def train_launches(case, precision, golden_dir, device="cuda:0", steps=2):
    """The launches of ``steps`` consecutive eager training steps on a golden fixture (forward, backward, ``join_side``, fused optimizer
    step; gradients written straight into the optimizer's arena, which one unrecorded backward builds first) → one
    ``LaunchRecorder.launches`` list per step.  tests/golden/train_launches.json records them (tools/make_golden_train_launches.py)."""
    from svpc_amd import ops
    from svpc_amd.optim import FusedBertAdam
    ops.set_precision(precision)
    try:
        _, _, batch, model = build_model(case, "vivt", golden_dir, device)
        fargs = syn.forward_args(batch)
        opt = FusedBertAdam(list(model.named_parameters()))
        opt.zero_grad(); model(*fargs)[0].backward(); opt.ensure_built()
        out = []
        for _ in range(steps):
            with LaunchRecorder() as rec:
                opt.zero_grad()
                model(*fargs)[0].backward()
                ops.join_side()
                opt.step()
            out.append(rec.launches)
        torch.cuda.synchronize()
        return out
    finally:
        ops.set_precision("fp32")


def product_sources_sha16():
    """hash of everything a parity record depends on: the kernel sources and the host-side package (bench.py recomputes it and refuses
    to quote a record made from other sources)"""
    import glob
    import hashlib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    files = sorted(glob.glob(os.path.join(root, "svpc_amd", "csrc", "*.hip")) + glob.glob(os.path.join(root, "svpc_amd", "csrc", "*.h")) +
                   glob.glob(os.path.join(root, "svpc_amd", "csrc", "*.cpp")) + glob.glob(os.path.join(root, "svpc_amd", "*.py")))
    h = hashlib.sha256()
    for f in files:
        h.update(os.path.relpath(f, root).encode())
        with open(f, "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]
