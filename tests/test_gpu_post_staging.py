"""The host half of the two 34-frame post entries (ls_ted_post, ls_beat_post) on the staging the handle-less entry points share
(csrc/ls_staging.h): every output left out in turn and all at once, host against device pointers, and the wrappers' ordering behind
torch's current stream.  B = 2 on the G9 / G10 samples."""
import ctypes
import itertools
import os

import numpy as np
import pytest

from conftest import GOLDEN
from livelyspeaker_amd import _lib, postprocess as pp

pytestmark = pytest.mark.gpu
B = 2
TED_OUTS = (("aligned", (B, 34, 27), np.float32), ("pose", (B, 34, 10, 3), np.float32), ("angle_diff", (B, 34), np.float32),
            ("beat_mask", (B, 34), np.uint8))
BEAT_OUTS = (("decoded", (B, 34, 282), np.float32), ("euler_deg", (B, 34, 141), np.float32))


def _ted_sample():
    return np.ascontiguousarray(np.load(os.path.join(GOLDEN, "ted_golden.npz"))["G5_ddpm1000_final"][:B])


def _beat_sample():
    return np.ascontiguousarray(np.load(os.path.join(GOLDEN, "beat_golden.npz"))["G3_ddpm50_final"][:B])


def _call(entry, sample, outs, keep, on_device):
    """The C entry through ctypes with the outputs named in ``keep`` (the others NULL); returns them as host arrays."""
    import torch
    lib = _lib.load_library()
    src = torch.from_numpy(sample).cuda() if on_device else sample
    m = _lib._Marshal(0, src)
    assert m.on_device == on_device
    got, ptrs = {}, []
    for name, shape, dtype in outs:
        got[name], p = m.out(shape, dtype) if name in keep else (None, None)
        ptrs.append(p)
    p_in = m.f32(src, sample.shape)
    m.ready()
    if entry == "ls_ted_post":
        cfg = pp.ted_post_config()
        rc = lib.ls_ted_post(0, int(on_device), B, ctypes.byref(cfg), p_in, *ptrs)
    else:
        rc = lib.ls_beat_post(0, int(on_device), B, int(sample.shape[1]), p_in, *ptrs)
    assert rc == 0, (entry, sorted(keep), on_device, rc)
    return {k: (v.cpu().numpy() if on_device else v) for k, v in got.items() if v is not None}


@pytest.mark.parametrize("entry,outs,make", [("ls_ted_post", TED_OUTS, _ted_sample), ("ls_beat_post", BEAT_OUTS, _beat_sample)])
def test_every_output_left_out_in_turn_in_both_modes(entry, outs, make):
    sample = make()
    names = [n for n, _, _ in outs]
    full = {dev: _call(entry, sample, outs, set(names), dev) for dev in (False, True)}
    for n, shape, dtype in outs:
        assert full[False][n].shape == shape and full[False][n].dtype == dtype
        assert np.array_equal(full[False][n], full[True][n]), (entry, n)                 # the two modes, bit for bit
    assert full[False][names[0]].any() and full[False][names[-1]].any()
    subsets = [set(names) - {n} for n in names] + [set()]
    for keep, dev in itertools.product(subsets, (False, True)):
        got = _call(entry, sample, outs, keep, dev)
        assert set(got) == keep
        for n in keep:
            assert np.array_equal(got[n], full[False][n]), (entry, n, sorted(keep), dev)


def test_post_wrappers_order_their_input_behind_a_side_stream():
    """ted_postprocess and beat_postprocess call _Marshal.ready(): an input finished late on a non-default torch stream (a long
    matmul chain in front of it) is the one the null-stream kernels read."""
    import torch
    cases = ((pp.ted_postprocess, _ted_sample()), (pp.beat_postprocess, _beat_sample()))
    want = [fn(s) for fn, s in cases]                                                    # host mode: finished copies
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device="cuda")
    true = [torch.from_numpy(s).cuda() for _, s in cases]
    torch.cuda.synchronize()
    for (fn, _), x_true, w in zip(cases, true, want):
        with torch.cuda.stream(side):
            acc = big
            for _ in range(40):                                                          # ~100 ms of queued work in front of the input
                acc = (acc @ big) * 1e-2
            x = torch.zeros_like(x_true)
            x += x_true + 0.0 * acc[:1, :1].sum()                                        # the input exists only after the chain
            got = fn(x)
        for k, v in w.items():
            g = got[k]
            if k == "motion_beat_times":
                assert g == v
            else:
                assert g.is_cuda and np.array_equal(g.cpu().numpy(), v), (fn.__name__, k)
