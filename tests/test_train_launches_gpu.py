"""What an eager training step launches, pinned launch for launch: for three fixtures (tiny/vivt in fp32, c1/vivt in bf16 and in bf16x3;
gradients written straight into the optimizer's arena, residual sink live) two consecutive steps — forward, backward, ``join_side``, fused
optimizer step — make the calls into the kernel library that tests/golden/train_launches.json records: the same kernels in the same order
with the same non-pointer arguments (shapes, strides, flags, table entry counts).  The record was made by
tools/make_golden_train_launches.py on the commit before the gradient tail moved into svpc_amd/grad_tail.py; two runs there gave
identical files (nothing in the routing depends on an address beyond identity)."""
import json
import os

import pytest

from helpers import TRAIN_LAUNCH_CASES, train_launches

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden(golden_dir):
    return json.load(open(os.path.join(golden_dir, "train_launches.json")))


@pytest.mark.parametrize("case,precision", TRAIN_LAUNCH_CASES)
def test_training_steps_launch_what_the_record_says(golden, golden_dir, case, precision):
    want = golden["%s/%s" % (case, precision)]
    got = train_launches(case, precision, golden_dir)
    assert len(want) == len(got) == 2
    for step, (w, g) in enumerate(zip(want, got)):
        assert len(w) > 100
        for i, (wl, gl) in enumerate(zip(w, g)):
            assert gl == wl, "step %d, launch %d: recorded %r, launched %r (after %r)" % (step, i, wl, gl, [n for n, _ in g[max(0, i - 3):i]])
        assert len(g) == len(w), "step %d: %d launches, %d recorded; first surplus / missing: %r" % (
            step, len(g), len(w), g[len(w)] if len(g) > len(w) else w[len(g)])
