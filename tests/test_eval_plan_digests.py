"""The device-facing tables of the evaluation plans, pinned byte for byte without a GPU: for every batch of tests/golden/ingredient_f1.json
and caption_scores.json the packed buffer of the plan, its section layout, and the compiler-level tables (the lexicon's predicate bitmap and
``a_bits``; the corpus's ``voc_off``, ``voc_tok``, ``ref_tok``, ``tab_key``, ``tab_idf``, ``gauss``) have the SHA-256 recorded in
tests/golden/eval_plan_digests.json (tools/make_golden_eval_plan_digests.py, run on the commit before the host side was last changed).
The kernels read these bytes by offset: the layout is the contract with them."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from helpers import eval_plan_digests  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_plan_tables_have_the_recorded_bytes():
    want = json.load(open(os.path.join(GOLDEN, "eval_plan_digests.json")))
    got = eval_plan_digests(GOLDEN)
    assert len(want["ingredient_f1"]["batches"]) >= 2 and len(want["caption_scores"]["batches"]) >= 2
    for feature in ("ingredient_f1", "caption_scores"):
        assert sorted(got[feature]) == sorted(want[feature])
        for b, (g, w) in enumerate(zip(got[feature]["batches"], want[feature]["batches"])):
            assert g == w, (feature, b, g, w)
        assert got[feature] == want[feature]
