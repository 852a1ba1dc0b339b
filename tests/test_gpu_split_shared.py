"""The fused step kernel's split-fp32 channel mixing (k_step PREC 2) with the LayerNorm-2 operand split once per 48-row chunk in LDS must
compute, bit for bit, what it computed when every wave split every fragment in registers: the three parts are the same, the six terms are
issued in the same order and the k blocks ascend, so each accumulator adds the same sequence of numbers.

tests/golden/split_shared_parent.npz holds the outputs of that earlier form (recorded by tests/golden/make_split_shared_golden.py, whose
`cases()` are replayed here): two CFG loops (TED: the 47 / 48 chunk seam inside the uncond pass and 6 ragged rows; BEAT: R = 72, 8 ragged
rows), the single-pass loop with an odd batch, and one forward of each dataset.  A difference is a wrong row or plane or a read of stale
LDS, never rounding: the comparison is np.array_equal and there is no tolerance."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_split_shared_golden", os.path.join(GOLDEN, "make_split_shared_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "split_shared_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case(golden):
    want = set()
    for name in REC.cases():
        want |= {f"{name}.cond", f"{name}.uncond"} if name.startswith("d_") else {name}
    assert set(golden) == want
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in golden.values())


@pytest.mark.parametrize("name", list(REC.cases()))
def test_bitwise_equal_to_the_in_register_split(golden, name):
    got = REC.flatten(name, REC.cases()[name]())
    for key, arr in got.items():
        ref = golden[key]
        assert arr.shape == ref.shape and arr.dtype == ref.dtype, key
        nbad = int((arr.view(np.uint32) != ref.view(np.uint32)).sum())
        print(f"{key}: {nbad} of {arr.size} values differ, max|d| = {float(np.abs(arr - ref).max()):.3e}")
        assert np.array_equal(arr, ref), key


def test_plain_launches_equal_graph_replay(golden):
    got = REC.loop("ted", 3, 1.5, use_graph=False)
    assert np.array_equal(got, golden["a_ted_b3_cfg"])
