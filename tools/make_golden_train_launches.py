"""Write tests/golden/train_launches.json: for each case of ``helpers.TRAIN_LAUNCH_CASES`` the kernel launches of two consecutive eager
training steps — name and non-pointer arguments of every call into the kernel library, in order (``helpers.train_launches``).  The record
pins what the host side launches, so it must come from code that is known to be right: run it (on the GPU) on a checkout of the commit
BEFORE a change to the host side, never on the change under test.  Two runs on the same commit give the same file.

    python tools/make_golden_train_launches.py --code <checkout whose svpc_amd (built) runs the steps> [--out tests/golden/train_launches.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "train_launches.json"))
    a = ap.parse_args(argv)
    sys.path[:0] = [os.path.abspath(a.code), os.path.join(ROOT, "tests")]
    from helpers import TRAIN_LAUNCH_CASES, train_launches
    import svpc_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(svpc_amd.__file__))) == os.path.abspath(a.code), svpc_amd.__file__
    record = {"%s/%s" % cp: train_launches(cp[0], cp[1], os.path.join(ROOT, "tests", "golden")) for cp in TRAIN_LAUNCH_CASES}
    with open(a.out, "w") as f:
        json.dump(record, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
