"""ls_onsets_long, host side: the C-ABI surface, the refusals (every one in front of hipSetDevice) and the Python entry's argument
errors.  Nothing here needs a GPU; the numbers are tests/test_gpu_onsets_long.py's."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from livelyspeaker_amd import _lib, audio_onsets as ao

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_is_declared_exported_and_listed(tmp_path):
    src = tmp_path / "consts.c"
    src.write_text('#include <stdio.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%d %d %d %zu\\n", LS_ABI_VERSION, LS_SCORE_TILE, LS_ONSETS_MAX_FRAMES, sizeof(ls_onsets_args));\n'
                   '    return 0;\n}\n')
    exe = tmp_path / "consts"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [5, ao.SCORE_TILE, ao.MAX_FRAMES, ctypes.sizeof(_lib.LsOnsetsArgs)]
    T = ao.SCORE_TILE
    assert T & (T - 1) == 0 and 1 <= T <= 1024
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    lib = ctypes.CDLL(_lib.library_path())
    name = "ls_onsets_long"
    assert name in _lib.EXPORTS and re.search(rf"\bint {name}\s*\(", hdr) and hasattr(lib, name)
    assert re.fullmatch(r"[a-z_]+", name)
    from livelyspeaker_amd import build
    assert "ls_onsets_long.hip" in build.SOURCES and os.path.exists(os.path.join(build.CSRC, "ls_onsets_frame.h"))


def test_invalid_arguments_are_refused_without_a_launch():
    """Every LS_EINVAL exit sits in front of hipSetDevice: no GPU is needed to be refused.  The frame limit of ls_onsets is not among
    them: the same arguments with 4097 frames are refused there and pass the checks here (device -1 is then no device: LS_EHIP, -3)."""
    lib = _lib.load_library()
    y = np.zeros((1, 2048), np.float32)
    env = np.zeros((1, 5), np.float32)
    out = np.zeros((1, 5), np.float32)

    def args(**kw):
        a = _lib.LsOnsetsArgs()
        a.batch, a.length, a.pad_mode, a.sr, a.sr_pick, a.fmax, a.delta = 1, 2048, 0, 16000.0, 16000.0, 11025.0, 0.07
        a.audio, a.oenv = y.ctypes.data, out.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    def call(**kw):
        return lib.ls_onsets_long(-1, ctypes.byref(args(**kw)))

    assert lib.ls_onsets_long(0, None) == -1
    assert call(audio=None) == -1                                                # no input
    assert call(envelope=env.ctypes.data) == -1                                  # both inputs
    assert call(batch=0) == -1 and call(length=0) == -1
    assert call(pad_mode=1, length=1024) == -1                                   # reflect needs L > 1024
    assert call(pad_mode=2) == -1 and call(pad_mode=-1) == -1
    assert call(fmax=0.0) == -1 and call(fmax=-8000.0) == -1
    assert call(sr=0.0) == -1 and call(sr_pick=0.0) == -1
    assert call(length=2 ** 31 - 2047) == -1                                     # one sample above 2^31 - 2048
    assert call(audio=None, envelope=env.ctypes.data, length=2 ** 31 - 2047) == -1
    assert call(batch=2049, length=2 ** 31 - 2048) == -1                         # 2049 * 4194301 frames: beyond the grid of 4-frame blocks
    given = dict(audio=None, envelope=env.ctypes.data, length=5)
    for name in ("mel_db", "rms", "onset_bt_rms"):                               # a given envelope has no spectrum
        assert call(**given, **{name: out.ctypes.data}) == -1, name
    # what ls_onsets refuses for its frame count alone gets as far as the device here
    assert lib.ls_onsets(-1, ctypes.byref(args(length=512 * 4096))) == -1
    assert call(length=512 * 4096) == -3 and call(audio=None, envelope=env.ctypes.data, length=4097) == -3
    assert call() == -3 and call(batch=2048, length=2 ** 31 - 2048) == -3


def test_source_keeps_every_refusal_ahead_of_the_device():
    src = open(os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_onsets_long.hip")).read()
    body = src[src.index('extern "C" int ls_onsets_long'):]
    assert "LS_EINVAL" not in body[body.index("hipSetDevice"):]


def test_python_surface_refuses_before_the_library_call():
    y = np.zeros((2, 1024), np.float32)
    with pytest.raises(ValueError, match="reflect"):
        ao.audio_onsets_long(y, pad_mode="reflect")
    with pytest.raises(ValueError, match="pad_mode"):
        ao.audio_onsets_long(y, pad_mode="edge")
    with pytest.raises(ValueError, match="either"):
        ao.audio_onsets_long(y, onset_envelope=y)
    with pytest.raises(ValueError, match="either"):
        ao.audio_onsets_long()
    with pytest.raises(ValueError, match="unknown"):
        ao.audio_onsets_long(y, want=("onsets",))
    with pytest.raises(ValueError):
        ao.audio_onsets_long(np.zeros(2048, np.float32))
    with pytest.raises(TypeError):                                               # the ragged form is not part of it
        ao.audio_onsets_long(y, lengths=[1024, 512])
    a, b = inspect.signature(ao.audio_onsets).parameters, inspect.signature(ao.audio_onsets_long).parameters
    assert [(k, v.default, v.kind) for k, v in a.items() if k != "lengths"] == [(k, v.default, v.kind) for k, v in b.items()]
    with pytest.raises(ValueError, match="frames"):                              # the capped entry keeps its limit
        ao.audio_onsets(np.zeros((1, 512 * 4096), np.float32))
