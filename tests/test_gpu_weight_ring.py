"""The fused step kernel's split-fp32 channel mixing (k_step PREC 2) streams its weight fragments through a register ring that keeps running
across the pass boundaries of a layer: while a pass multiplies its last k blocks, the first blocks and the bias of the next pass are already
in flight.  That changes WHEN a fragment is fetched, never which fragment multiplies what, so the results must equal, bit for bit, what the
kernel computed when every pass fetched one block ahead inside its own slice.

tests/golden/weight_ring_parent.npz holds the outputs of that earlier form (recorded by tests/golden/make_weight_ring_golden.py with a build
of the commit before the ring; its `cases()` are replayed here).  The shapes are the smallest at which a ring can fetch the wrong thing:
one layer (nothing follows the layer's last pass: a ring that ran on would leave the weight image on every launch) and two layers with
distinct weights (a fetch from the wrong layer's, wave's or channel half's slice multiplies other numbers), each for TED B = 1 and B = 3
with CFG, TED B = 3 single pass (a paired workgroup and an odd tail) and BEAT B = 2 with CFG; one forward at t = 500 and a 3-step DDPM loop
of each.  A difference is a wrong or stale fragment, never rounding: the comparison is np.array_equal and there is no tolerance."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_weight_ring_golden", os.path.join(GOLDEN, "make_weight_ring_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


REC = _recorder()


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "weight_ring_parent.npz")) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_every_case(golden):
    want = set()
    for name in REC.cases():
        want |= {f"{name}.cond", f"{name}.uncond"} if name.endswith("_fwd") else {name}
    assert set(golden) == want
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in golden.values())
    # the two depths of the model are different functions: a fixture that recorded one of them twice would pin nothing
    for shape in REC.SHAPES:
        assert not np.array_equal(golden[f"L1_{shape}_loop"], golden[f"L2_{shape}_loop"]), shape


@pytest.mark.parametrize("name", list(REC.cases()))
def test_bitwise_equal_to_the_one_block_prefetch(golden, name):
    got = REC.flatten(name, REC.cases()[name]())
    for key, arr in got.items():
        ref = golden[key]
        assert arr.shape == ref.shape and arr.dtype == ref.dtype, key
        nbad = int((arr.view(np.uint32) != ref.view(np.uint32)).sum())
        print(f"{key}: {nbad} of {arr.size} values differ, max|d| = {float(np.abs(arr - ref).max()):.3e}")
        assert np.array_equal(arr, ref), key


def test_plain_launches_equal_graph_replay(golden):
    ds, batch, scale = REC.SHAPES["ted_b3_cfg"]
    got = REC.loop(ds, 1, batch, scale, use_graph=False)
    assert np.array_equal(got, golden["L1_ted_b3_cfg_loop"])
