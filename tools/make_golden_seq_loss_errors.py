"""Write tests/golden/seq_loss_errors.json: under "errors", for every wrong call of tests/seq_loss_error_cases.py the exception's type
and its full message; under "ops_names", the names ``svpc_amd.ops`` holds.  The committed file was taken at commit dba497f ("Add clipped
policy-gradient training (PPO / GRPO) with a per-token KL"), the last one with these bindings inside ops.py.
The record pins the error texts and the order of the host checks of the sequence-loss bindings, so it must come from code
that is known to be right: run it on a checkout of the commit BEFORE a change to those checks, never on the change under test.  It
needs no GPU; two runs on the same commit give the same file.

    python tools/make_golden_seq_loss_errors.py --code <checkout whose svpc_amd is recorded> [--out tests/golden/seq_loss_errors.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--code", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "seq_loss_errors.json"))
    a = ap.parse_args(argv)
    sys.path[:0] = [os.path.abspath(a.code), os.path.join(ROOT, "tests")]
    import svpc_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(svpc_amd.__file__))) == os.path.abspath(a.code), svpc_amd.__file__
    import seq_loss_error_cases as ec
    from svpc_amd import _lib, ops
    _lib.call = ec.refuse_launch
    record = {"errors": {name: ec.run(call) for name, call in ec.cases()},
              "ops_names": sorted(n for n in dir(ops) if not n.startswith("__"))}
    with open(a.out, "w") as f:
        json.dump(record, f, sort_keys=True, indent=0, ensure_ascii=False)
        f.write("\n")


if __name__ == "__main__":
    main()
