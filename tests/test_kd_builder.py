"""The key-table builder of the exact verify's key dedup (bn254_amd/csrc/bn254_kdlines.h, run by k_kd_lines in bn254_keydedup.hip): the lane
machine's level program for one key, its raw lines through kd_scale_line, equals word for word what g2_line_table + fp_canon gives (the table
registration stores), flags a line with c2 = 0 exactly when g2_line_table does, and its raw lines are those of kd_walk_raw_lines as field
elements — for the generator, random subgroup keys, points on the twist outside the subgroup (random ones, the golden one and its multiples,
points of the twist's small order 10069), in the pair layout's host emulation, plain and under the interval tracker (-DBN_TRACK_BOUNDS aborts
on a violated limb / value bound)."""
import json
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_kd_builder.cpp")

DRIVER = r'''
import ctypes, json, sys
lib, keys, raw = sys.argv[1], json.loads(open(sys.argv[2]).read()), sys.argv[3] == "1"
L = ctypes.CDLL(lib)
W = 87 * 4 * 9
flags = []
for hexkey in keys:
    ref, kd = (ctypes.c_int32 * W)(), (ctypes.c_int32 * W)()
    rc = L.kb_tables(bytes.fromhex(hexkey), ref, kd)
    assert rc in (0, 1), (hexkey, rc)
    assert list(ref) == list(kd), hexkey
    flags.append(rc)
    if raw:
        a, b = (ctypes.c_int32 * (87 * 6 * 9))(), (ctypes.c_int32 * (87 * 6 * 9))()
        assert L.kb_raw(bytes.fromhex(hexkey), a, b) == 0, hexkey
        assert list(a) == list(b), hexkey
print("ok", json.dumps(flags))
'''

TWIST_SMALL_ORDER = 10069          # #E'(Fq2) = r * 10069 * (a 241-bit prime)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    out = tmp_path_factory.mktemp("kb")
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libkb_%s.so" % name))
        procs[name] = (so, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + ["-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas",
                                                                                       "-o", so, SRC], stderr=subprocess.PIPE, text=True))
    for name, (so, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: so for name, (so, _) in procs.items()}


def _random_twist_point(M, rnd):
    while True:
        x = (rnd.randrange(M.Q), rnd.randrange(M.Q))
        y = M.f2_sqrt(M.f2_add(M.f2_mul(M.f2_mul(x, x), x), M.B2))
        if y is not None:
            return (x, y)


@pytest.fixture(scope="module")
def keys():
    from oracle import bn254_model as M
    with open(os.path.join(ROOT, "tests", "golden", "derived_vectors.json")) as f:
        d = json.load(f)
    rnd = random.Random(11)
    pts = [M.G2_GEN] + [M.g2_mul(M.G2_GEN, rnd.randrange(1, M.R)) for _ in range(6)]
    off = bytes.fromhex(d["g2_not_in_subgroup"])
    off_pt = M.g2_from_uncompressed(off, subgroup_check=False)
    assert not M.g2_in_subgroup(off_pt)
    pts += [off_pt] + [M.g2_mul(off_pt, k) for k in (2, 3, 12345, M.R)]
    cof = (2 * M.Q - M.R) // TWIST_SMALL_ORDER
    small = 0
    for _ in range(4):
        p = _random_twist_point(M, rnd)
        assert not M.g2_in_subgroup(p)
        pts.append(p)
        s = M.g2_mul(p, M.R * cof)                       # order 10069 (or the identity)
        if s is not None:
            assert M.g2_mul(s, TWIST_SMALL_ORDER) is None
            pts += [s, M.g2_mul(s, 2)]
            small += 1
    assert small >= 1
    return [M.g2_to_uncompressed(p).hex() for p in pts if p is not None]


@pytest.mark.parametrize("build", ["plain", "bounds"])
def test_builder_tables_equal_registration(libs, keys, build, tmp_path):
    kf = tmp_path / "keys.json"
    kf.write_text(json.dumps(keys))
    p = subprocess.run([sys.executable, "-c", DRIVER, libs[build], str(kf), "1" if build == "plain" else "0"], capture_output=True, text=True,
                       timeout=900)
    assert p.returncode == 0 and p.stdout.startswith("ok"), (p.stdout[-500:], p.stderr[-2000:])
    flags = json.loads(p.stdout.split(None, 1)[1])
    assert flags[0] == 0 and flags[1:7] == [0] * 6                # subgroup keys: no line with c2 = 0


def test_builder_level_table_is_well_formed():
    """the builder's own level (LM_KD_ADD0): within the level no slot is written twice, no product reads a product output of the level, and
    it computes wave T's level 0 of an addition (LM_T_ADD[0]) unchanged"""
    text = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_kdlines.h")).read()
    tables = re.findall(r"LM_TABLE (LM_\w+)\[(\d+)\]\[9\] = \{(.*?)\};", text, re.S)
    assert [t[0] for t in tables] == ["LM_KD_ADD0"]
    body = tables[0][2]
    muls = re.findall(r"lm_mul\((LS_\w+), (LS_\w+), (LS_\w+)\)", body)
    lins = re.findall(r"lm_lin\((LS_\w+),", body)
    outs = [m[0] for m in muls]
    assert len(set(outs)) == len(outs) and len(set(lins)) == len(lins) and not set(outs) & set(lins)
    for out, a, b in muls:
        assert a not in outs and b not in outs, out
    lm = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_lmachine.h")).read()
    t_add = re.search(r"LM_TABLE LM_T_ADD\[3\]\[9\] = \{\s*\{(.*?)\},\s*\{", lm, re.S).group(1)
    for entry in re.findall(r"LM_E\(lm_mul\([^)]*\), lm_lin\([^)]*\)\)", t_add):
        assert entry in body, entry
