"""Write tests/golden/eval_plan_digests.json: the SHA-256 of every device-facing table that ``IngredientLexicon`` / ``IngredientPlan`` and
``ReferenceCorpus`` / ``ScorePlan`` build for the batches of tests/golden/ingredient_f1.json and caption_scores.json
(``helpers.eval_plan_digests``).  The layout of these tables is the contract with the kernels, so the record must come from code that is
known to agree with them: run it on a checkout of the commit BEFORE a change to the host side, never on the change under test.

    python tools/make_golden_eval_plan_digests.py --code <checkout whose svpc_amd builds the tables> [--out tests/golden/eval_plan_digests.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "eval_plan_digests.json"))
    a = ap.parse_args(argv)
    sys.path[:0] = [os.path.abspath(a.code), os.path.join(ROOT, "tests")]
    from helpers import eval_plan_digests
    import svpc_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(svpc_amd.__file__))) == os.path.abspath(a.code), svpc_amd.__file__
    with open(a.out, "w") as f:
        json.dump(eval_plan_digests(os.path.join(ROOT, "tests", "golden")), f, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
