"""CPU: the sampling handle's weight images (csrc/ls_weights.cpp) byte for byte.  tests/weight_images_main.cpp is compiled with the
project's hipcc into a host-only program, run for four configurations, and every file it writes is compared by SHA-256 with
tests/golden/weight_images.json, which was recorded from the code before the images moved into ls_weights.cpp
(profiles/r15_weight_images.md).  The resolver's two faults go through the same program."""
import hashlib
import json
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from livelyspeaker_amd import build

with open(os.path.join(GOLDEN, "weight_images.json")) as _f:
    DIGESTS = json.load(_f)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("weight_images") / "weight_images")
    cmd = [build.hipcc_path(), "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC,
           os.path.join(ROOT, "tests", "weight_images_main.cpp"), os.path.join(build.CSRC, "ls_weights.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return exe


@pytest.mark.parametrize("config", ["ted", "beat", "beat150", "ted200"])
def test_weight_images_equal_the_recorded_ones(driver, tmp_path, config):
    res = subprocess.run([driver, config, str(tmp_path)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    want = DIGESTS[config]
    got = {}
    for name in os.listdir(tmp_path):
        with open(tmp_path / name, "rb") as f:
            got[name] = hashlib.sha256(f.read()).hexdigest()
    assert sorted(got) == sorted(want)                  # the groups this model has, no more
    assert [n for n in sorted(want) if got[n] != want[n]] == []


def test_the_groups_follow_the_model():
    names = {c: set(DIGESTS[c]) for c in DIGESTS}
    assert "lw_wtp.bin" not in names["ted200"] and "lw_wcf.bin" not in names["ted200"] and "tokpad.txt" not in names["ted200"]
    assert "lw_wtp.bin" in names["ted"] and not [n for n in names["ted"] if n.startswith("mx_w")] and "emo_emb.bin" not in names["ted"]
    assert {"mx_wtok.bin", "mx_wch.bin", "mx_wpose.bin"} <= names["beat150"] and "wch_img.bin" not in names["beat150"]
    assert {"wch_img.bin", "wch_lo2_img.bin", "wtok1_hi_img.bin", "emo_emb.bin"} <= names["beat"]


@pytest.mark.parametrize("fault,key,message", [
    ("drop", "backbone.mlps.1.block1.0.beta", "missing weight 'backbone.mlps.1.block1.0.beta'"),
    ("drop", "input_mapping.bias", "missing weight 'input_mapping.bias'"),
    ("resize", "speaker_mu.bias", "weight 'speaker_mu.bias' has 513 elements, expected 512"),
])
def test_resolver_names_the_faulty_key(driver, tmp_path, fault, key, message):
    res = subprocess.run([driver, "ted", str(tmp_path), fault, key], capture_output=True, text=True)
    assert res.returncode == 2 and res.stdout.strip() == message, res.stdout + res.stderr
    assert os.listdir(tmp_path) == []                   # nothing is built once a key is faulty
