"""The fused step kernel's split-fp32 channel mixing (k_step PREC 2) places a layer's movable vector work beside its bf16 MFMAs: the SiLU
epilogue of a pass's tile runs while the tile after it multiplies, and the bf16 split of chunk 1 is computed into
registers before the mid-layer barrier, with only its stores behind it.  That changes WHEN this work is done, never its terms or their
order, so the results must equal, bit for bit, what the kernel computed with every epilogue after its pass and the split between the
barriers.

tests/golden/layer_overlap_parent.npz and layer_overlap_parent_trace.npz hold the outputs of that earlier form (recorded by
tests/golden/make_layer_overlap_golden.py with a build of the commit before the change; its `cases()` are replayed here).  The shapes are the smallest at which the placement can go wrong:
one layer (nothing follows: early work for a next layer would add temb twice, and the last pass has no MFMAs after it), two layers (one
boundary) and three (a middle layer), each for TED B = 1 with CFG (6 ragged rows: tile 4's lanes are partly masked in the register-staged
split and in the epilogues), TED B = 3 single pass (a paired workgroup and an odd tail) and BEAT B = 2 with CFG (R = 72); one forward at
t = 500 and a 3-step DDPM loop of each, one loop also with plain launches instead of graph replay, and one forward with the layer trace
on (X before every layer must be what it was: work done early for layer l + 1 must not show in the dump after layer l).  A difference is
a wrong, stale or doubled term, never rounding: the comparison is np.array_equal and there is no tolerance."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_layer_overlap_golden", os.path.join(GOLDEN, "make_layer_overlap_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope="module")
def golden():
    out = {}
    for f in (REC.OUT, REC.OUT_TRACE):           # the layer trace lies in a file of its own: each stays under the size limit for a committed file
        with np.load(f) as z:
            out.update({k: z[k] for k in z.files})
    return out


def test_fixture_holds_every_case(golden):
    want = set()
    for name in REC.cases():
        want |= set(REC.keys(name))
    assert set(golden) == want
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in golden.values())
    # the depths of the model are different functions: a fixture that recorded one of them twice would pin nothing
    for shape in REC.SHAPES:
        for la, lb in ((1, 2), (2, 3)):
            assert not np.array_equal(golden[f"L{la}_{shape}_loop"], golden[f"L{lb}_{shape}_loop"]), shape
    shape, layers = REC.TRACE
    tr = golden[f"L{layers}_{shape}_trace.trace"]
    assert tr.shape[1] == layers + 1
    assert all(not np.array_equal(tr[:, i], tr[:, i + 1]) for i in range(layers))


@pytest.mark.parametrize("name", list(REC.cases()))
def test_bitwise_equal_to_the_late_placement(golden, name):
    got = REC.flatten(name, REC.cases()[name]())
    assert list(got) == REC.keys(name)
    for key, arr in got.items():
        ref = golden[key]
        assert arr.shape == ref.shape and arr.dtype == ref.dtype, key
        nbad = int((arr.view(np.uint32) != ref.view(np.uint32)).sum())
        print(f"{key}: {nbad} of {arr.size} values differ, max|d| = {float(np.abs(arr - ref).max()):.3e}")
        assert np.array_equal(arr, ref), key


def test_plain_launches_equal_graph_replay(golden):
    ds, batch, scale = REC.SHAPES["ted_b3_single"]
    got = REC.loop(ds, 3, batch, scale, use_graph=False)
    assert np.array_equal(got, golden["L3_ted_b3_single_loop"])
