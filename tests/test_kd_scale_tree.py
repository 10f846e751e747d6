"""The scaling pass of the key dedup's table builder with one inversion per key (bn254_keydedup.h: kd_scale_tree, the host form of the tree
k_kd_scale runs on the device) against kd_scale_line and g2_line_table + fp_canon, word for word, on the raw lines of the builder's level
program: generator, subgroup keys, points outside G2 and of the twist's small order 10069 — in the pair layout's host emulation, plain and
under the interval tracker (-DBN_TRACK_BOUNDS aborts on a violated limb or value bound)."""
import json
import os
import subprocess
import sys

import pytest

from tests.test_kd_builder import keys  # noqa: F401  (the key set of the builder's own test)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_kd_tree.cpp")

DRIVER = r'''
import ctypes, json, sys
lib, keys = sys.argv[1], json.loads(open(sys.argv[2]).read())
L = ctypes.CDLL(lib)
W = 87 * 4 * 9
flags = []
for hexkey in keys:
    ref, line, tree = (ctypes.c_int32 * W)(), (ctypes.c_int32 * W)(), (ctypes.c_int32 * W)()
    rc = L.kt_tables(bytes.fromhex(hexkey), ref, line, tree)
    assert rc in (0, 1), (hexkey, rc)
    assert list(ref) == list(line), hexkey
    if rc == 0:
        assert list(tree) == list(line), hexkey
    flags.append(rc)
print("ok", json.dumps(flags))
'''


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    out = tmp_path_factory.mktemp("kt")
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libkt_%s.so" % name))
        procs[name] = (so, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + ["-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                                                                                       "-o", so, SRC], stderr=subprocess.PIPE, text=True))
    for name, (so, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: so for name, (so, _) in procs.items()}


@pytest.mark.parametrize("build", ["plain", "bounds"])
def test_tree_equals_line_by_line_scaling(libs, keys, build, tmp_path):  # noqa: F811
    kf = tmp_path / "keys.json"
    kf.write_text(json.dumps(keys))
    p = subprocess.run([sys.executable, "-c", DRIVER, libs[build], str(kf)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and p.stdout.startswith("ok"), (p.stdout[-500:], p.stderr[-2000:])
    flags = json.loads(p.stdout.split(None, 1)[1])
    assert len(flags) == len(keys) >= 14 and flags.count(0) >= 7          # the tree was compared for the subgroup keys at least
