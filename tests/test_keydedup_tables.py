"""The per-call key tables of the exact verify (bn254_amd/csrc/bn254_keydedup.h, run by bn254_keydedup.hip): the raw twist-point walk plus
the per-line scaling equal, word for word, what g2_line_table + fp_canon gives (the table registration stores and the keyed Miller kernel's
bound proof assumes: canonical limbs) — for the generator, random subgroup keys and points on the twist outside the subgroup, in the pair
layout's host emulation, plain and under the interval tracker (-DBN_TRACK_BOUNDS aborts on a violated limb / value bound)."""
import json
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_keydedup.cpp")

DRIVER = r'''
import ctypes, json, sys
lib, keys = sys.argv[1], json.loads(open(sys.argv[2]).read())
L = ctypes.CDLL(lib)
W = 87 * 4 * 9
for hexkey in keys:
    ref, kd = (ctypes.c_int32 * W)(), (ctypes.c_int32 * W)()
    rc = L.hk_tables(bytes.fromhex(hexkey), ref, kd)
    assert rc == 0, (hexkey, rc)
    assert list(ref) == list(kd), hexkey
print("ok", len(keys))
'''


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    out = tmp_path_factory.mktemp("hk")
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libhk_%s.so" % name))
        procs[name] = (so, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + ["-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                                                                                       "-o", so, SRC], stderr=subprocess.PIPE, text=True))
    for name, (so, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: so for name, (so, _) in procs.items()}


@pytest.fixture(scope="module")
def keys():
    from oracle import bn254_model as M
    with open(os.path.join(ROOT, "tests", "golden", "derived_vectors.json")) as f:
        d = json.load(f)
    rnd = random.Random(7)
    pts = [M.G2_GEN] + [M.g2_mul(M.G2_GEN, rnd.randrange(1, M.R)) for _ in range(4)]
    enc = [M.g2_to_uncompressed(p).hex() for p in pts]
    off = bytes.fromhex(d["g2_not_in_subgroup"])
    off_pt = M.g2_from_uncompressed(off, subgroup_check=False)
    assert not M.g2_in_subgroup(off_pt)
    enc += [off.hex()] + [M.g2_to_uncompressed(M.g2_mul(off_pt, k)).hex() for k in (2, 3, 12345)]
    return enc


@pytest.mark.parametrize("build", ["plain", "bounds"])
def test_key_tables_equal_registration(libs, keys, build, tmp_path):
    kf = tmp_path / "keys.json"
    kf.write_text(json.dumps(keys))
    p = subprocess.run([sys.executable, "-c", DRIVER, libs[build], str(kf)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and p.stdout.startswith("ok"), (p.stdout[-500:], p.stderr[-2000:])
