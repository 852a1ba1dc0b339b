"""Host side of the per-clip Philox keys: the key table of a keyed pool's push (``long_form.pool_keys`` -> ls_long_pool_keys) against a
restatement written here and against the C entry through ctypes, on the staggered schedule of tests/test_long_pool_host.py;
tests/pool_keys_main.cpp -- a stand-alone program around the plan's unit -- under the host sanitizers; the refusals of ``row_keys``,
``noise_keys`` and ``join(key=)`` that are raised before an engine exists; and the ABI, which only grew.  No GPU."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from livelyspeaker_amd import _lib, build, long_form, shard, synth
from test_long_form_host import _no_engine, _parts
from test_long_pool_host import AUDIO_LENS, HostPool, ROOT, staggered

TOP = (1 << 48) - 1
KEYS = {"A": 11, "B": (1 << 32) + 5, "C": TOP, "D": 11}        # B above 2^32, C the largest key, D repeats A's


def _restated(keys, ran, wins):
    """The definition, restated: round r holds, ascending, the slots with more than r windows to run; the row of slot s there draws
    at keys[s] + ((ran[s] + r) << 48)."""
    rows = []
    for r in range(max(list(wins) + [0])):
        rows += [int(keys[s]) + ((int(ran[s]) + r) << 48) for s in range(len(wins)) if wins[s] > r]
    return rows


def _c_entry(keys, ran, wins):
    """ls_long_pool_keys through ctypes, the two-call use: (rc, rows)."""
    lib = _lib.load_library()
    S = len(keys)
    k = (ctypes.c_uint64 * S)(*[int(v) for v in keys])
    r = (ctypes.c_int64 * S)(*[int(v) for v in ran])
    w = (ctypes.c_int32 * S)(*[int(v) for v in wins])
    n = ctypes.c_int32(-7)
    rc = lib.ls_long_pool_keys(S, k, r, w, None, 0, ctypes.byref(n))
    if rc != 0:
        return rc, None
    rows = (ctypes.c_uint64 * max(n.value, 1))()
    assert lib.ls_long_pool_keys(S, k, r, w, rows, n.value, ctypes.byref(n)) == 0
    return 0, [int(v) for v in rows[:n.value]]


@pytest.mark.parametrize("AL", AUDIO_LENS)
def test_key_table_of_the_staggered_schedule(AL):
    pool, who, keys, seen = HostPool(4, AL), {}, np.zeros(4, np.uint64), []
    for event, payload in staggered(AL):
        if event == "join":
            s = pool.join(payload[1])
            who[s], keys[s] = payload[0], KEYS[payload[0]]
            continue
        lengths = payload[0] if event == "push" else [0] * 4
        closing = [int(event == "close" or (event == "leave" and who.get(s) == payload[0])) * int(pool.open[s]) for s in range(4)]
        before = pool.ran.copy()
        rounds, _ = pool.push(lengths, closing)
        wins = [sum(s in r for r in rounds) for s in range(4)]
        got = long_form.pool_keys(keys, before, wins)
        assert got.dtype == np.uint64 and got.tolist() == _restated(keys, before, wins) == _c_entry(keys, before, wins)[1]
        # in the plan's row order: row i of round r belongs to slot rounds[r][i]
        flat = [(s, r) for r, slots in enumerate(rounds) for s in slots]
        assert got.tolist() == [KEYS[who[s]] + ((int(before[s]) + r) << 48) for s, r in flat]
        seen += [(who[s], int(before[s]) + r) for s, r in flat]
    # D took over B's slot: it starts at window 0 again, under its own key; every (speaker, window) ran once
    assert seen == [("A", 0), ("A", 1), ("B", 0), ("C", 0), ("C", 1), ("B", 1), ("D", 0), ("C", 2)]


def test_key_table_edges():
    keys = long_form.pool_keys
    assert keys([TOP], [65535], [1]).tolist() == [(1 << 64) - 1]                   # the largest key at the last window: all 64 bits
    assert keys([(1 << 32) + 5, 3], [0, 7], [2, 1]).tolist() == [(1 << 32) + 5, 3 + (7 << 48), (1 << 32) + 5 + (1 << 48)]
    assert keys([5, 1 << 48], [0, 0], [1, 0]).tolist() == [5]                      # an idle slot's key is not looked at
    assert keys([1, 2], [4, 4], [0, 0]).tolist() == []
    with pytest.raises(ValueError):
        keys([1 << 48], [0], [1])                                                  # a key of 2^48
    with pytest.raises(ValueError):
        keys([-1], [0], [1])
    with pytest.raises(ValueError):
        keys([1, 2], [0], [1, 1])                                                  # one entry per slot
    with pytest.raises(_lib.EngineError, match="2\\^16"):
        keys([1], [65536], [1])                                                    # window 2^16
    with pytest.raises(_lib.EngineError, match="2\\^16"):
        keys([1], [65535], [2])
    assert _c_entry([1 << 48], [0], [1])[0] == -1 and _c_entry([1], [65536], [1])[0] == -2      # LS_EINVAL, LS_ESTATE
    # a pool past 2^16 rounds: two clips of 40000 windows each, one after the other in the same slot -- the table never sees the
    # pool's round count, only the clip's own window
    for key in (3, 4):
        rows = keys([key], [0], [40000])
        assert rows.tolist() == _restated([key], [0], [40000]) and int(rows[-1]) == key + (39999 << 48)


def test_random_pools_agree_with_the_restatement():
    rng = np.random.default_rng(20261021)
    for _ in range(200):
        S = int(rng.integers(1, 7))
        keys = [int(k) for k in rng.integers(0, 1 << 48, S, dtype=np.uint64)]
        ran = rng.integers(0, 60000, S)
        wins = rng.integers(0, 4, S)
        assert long_form.pool_keys(keys, ran, wins).tolist() == _restated(keys, ran, wins) == _c_entry(keys, ran, wins)[1]


def test_pool_keys_on_its_edges_under_asan_and_ubsan(tmp_path):
    """tests/pool_keys_main.cpp with the plan's unit, as plain C++ with the host sanitizers linked statically: a child process of its
    own, nothing preloaded, nothing inside Python, no GPU."""
    exe = str(tmp_path / "pool_keys")
    made = subprocess.run([build.hipcc_path(), "-x", "c++", "-std=c++17", "-O1", "-g", "-fno-gpu-sanitize", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "pool_keys_main.cpp"),
                           os.path.join(ROOT, "livelyspeaker_amd", "csrc", "ls_chain_plan.cpp"), "-o", exe], capture_output=True, text=True)
    assert made.returncode == 0, made.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    assert run.stderr == "", run.stderr


@pytest.mark.parametrize("ds", ["ted", "beat"])
def test_refusals_come_before_any_engine(ds, monkeypatch):
    _no_engine(monkeypatch)
    cfg, model, diffusion = _parts(ds)
    y = synth.make_long_cond(cfg, 2, 2)
    shape = (2, cfg.njoints, cfg.nfeats, 34)
    kw = dict(model_kwargs={"y": {}}, skip_timesteps=0, init_image=None, progress=False, dump_steps=None, noise=None, const_noise=False)
    assert diffusion.row_keys is None
    try:
        # ---- layer 1: diffusion.row_keys
        diffusion.row_keys = [3, 17]
        for source in ("torch_cpu", "torch_device"):                        # any other noise source
            diffusion.noise_source = source
            for loop in (diffusion.ddim_sample_loop, diffusion.p_sample_loop):
                with pytest.raises(ValueError, match="philox"):
                    loop(model, shape, **kw)
        diffusion.noise_source = "philox"
        for bad in ([3], [3, 17, 42], np.arange(3), []):                     # a wrong length
            diffusion.row_keys = bad
            for loop in (diffusion.ddim_sample_loop, diffusion.p_sample_loop):
                with pytest.raises(ValueError, match="row_keys holds"):
                    loop(model, shape, **kw)
        diffusion.row_keys = [3, 1 << 64]
        with pytest.raises(ValueError, match="2\\^64"):
            diffusion.ddim_sample_loop(model, shape, **kw)
        diffusion.row_keys = np.array([3, 17], np.int64)
        diffusion.sample_offset = 5                                         # a nonzero sample_offset at the same time
        for loop in (diffusion.ddim_sample_loop, diffusion.p_sample_loop):
            with pytest.raises(ValueError, match="sample_offset"):
                loop(model, shape, **kw)
        diffusion.sample_offset = 0
        with pytest.raises(ValueError, match="shard"):                      # sharded sampling
            shard.sample_sharded(diffusion.ddim_sample_loop, model, shape, {}, diffusion=diffusion)
        with pytest.raises(ValueError, match="shard"):
            shard.sample_sharded(diffusion.p_sample_loop, model, shape, {})
        # what may refuse does, and says so
        with pytest.raises(NotImplementedError, match="row_keys"):
            diffusion.plms_sample_loop(model, shape, model_kwargs={"y": {}})
        with pytest.raises(NotImplementedError, match="row_keys"):
            diffusion.calc_bpd_loop(model, np.zeros(shape, np.float32), model_kwargs={"y": {}})
        emo = {"emo": y["emo"]} if ds == "beat" else {}
        with pytest.raises(NotImplementedError, match="row_keys"):
            long_form.sample_long(diffusion, model, y["audio"], y["seed_poses"], y["vid_indices"], y["scale"], **emo)
        with pytest.raises(NotImplementedError, match="row_keys"):
            long_form.open_stream(diffusion, model, y["seed_poses"], y["vid_indices"], y["scale"], emo=None if ds == "ted" else y["emo"][:, 0])
        with pytest.raises(NotImplementedError, match="row_keys"):
            long_form.open_pool(diffusion, model, 4, noise_keys="clip")
        diffusion.row_keys = None
        # ---- layer 2: open_pool(noise_keys=) and join(key=)
        with pytest.raises(ValueError, match="noise_keys"):
            long_form.open_pool(diffusion, model, 4, noise_keys="slot")     # an unknown value
        diffusion.noise_source = "torch_cpu"
        with pytest.raises(ValueError, match="philox"):
            long_form.open_pool(diffusion, model, 4, noise_keys="clip")     # keys are Philox keys
        one_emo = {"emo": int(y["emo"][0, 0])} if ds == "beat" else {}
        plain = long_form.open_pool(diffusion, model, 4)
        assert "key" not in plain.slots
        with pytest.raises(ValueError, match="keyed pool"):
            plain.join(y["seed_poses"][0], 1, 1.0, key=3, **one_emo)        # join(key=) on a pool that is not keyed
        diffusion.noise_source = "philox"
        plain = long_form.open_pool(diffusion, model, 4)
        with pytest.raises(ValueError, match="keyed pool"):
            plain.join(y["seed_poses"][0], 1, 1.0, key=3, **one_emo)
        diffusion.sample_offset = 1 << 48
        with pytest.raises(ValueError, match="sample_offset"):
            long_form.open_pool(diffusion, model, 4, noise_keys="clip")
        diffusion.sample_offset = 0
        keyed = long_form.open_pool(diffusion, model, 4, noise_keys="clip")     # opening touches no engine
        assert keyed.slots["key"].dtype == np.uint64 and keyed.slots["key"].tolist() == [0, 0, 0, 0]
        for bad in (1 << 48, -1, 2.0, "7", True):
            with pytest.raises(ValueError, match="key must be"):
                keyed.join(y["seed_poses"][0], 1, 1.0, key=bad, **one_emo)
    finally:
        diffusion.noise_source, diffusion.row_keys, diffusion.sample_offset = "torch_cpu", None, 0


NEW_EXPORTS = ("ls_set_row_keys", "ls_long_pool_keyed", "ls_long_pool_set_key", "ls_long_pool_keys")


def test_the_abi_only_grew(tmp_path):
    lib = _lib.load_library()
    assert lib.ls_abi_version() == 5
    hdr = open(os.path.join(ROOT, "include", "ls_hip.h")).read()
    for name in NEW_EXPORTS:
        assert name in _lib.EXPORTS and f"int {name}(" in hdr and hasattr(lib, name), name
    for name in ("long_pool_keyed", "long_pool_set_key"):
        assert hasattr(_lib.Engine, name)
    assert hasattr(_lib, "long_pool_keys") and "Philox keyed by (slot, window)" not in hdr
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "ls_hip.h"\nint main(void) {\n'
                   '    printf("%zu %zu %zu %zu %d\\n", sizeof(ls_sample_args), sizeof(ls_long_sample_args), sizeof(ls_long_pool_join_args),\n'
                   '           sizeof(ls_long_pool_push_args), LS_ABI_VERSION);\n    return 0;\n}\n')
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [ctypes.sizeof(_lib.LsSampleArgs), 104, ctypes.sizeof(_lib.LsLongPoolJoinArgs), ctypes.sizeof(_lib.LsLongPoolPushArgs), 5]
    # the structs themselves: git's record of them is the pin -- the ctypes mirrors the existing host tests check field by field
    assert "reserved" in [n for n, _ in _lib.LsLongPoolPushArgs._fields_]
