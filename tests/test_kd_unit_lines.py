"""The keyed Miller loop on UNIT LINES (BN254_OPT_KEY_DEDUP_FOLD = 2; bn254_amd/csrc/bn254_pairing.h: miller_loop_keyed_unit,
bn254_field.h: fp12_mul_unit_line) in the pair layout's host emulation, plain and under the interval tracker (-DBN_TRACK_BOUNDS aborts on
a violated limb / value bound):
- miller_loop_keyed_unit gives the Fq12 element of miller_loop_keyed, its twelve coefficients word for word after canonicalisation: two
  valid tuples, a wrong signature, every skip combination (pair A by its point, by a refused key and by the identity key, pair B, both),
  a key outside G2;
- products per lane: 2 307 dual and 348 single — 64 squarings less the peeled one (63 x 12), the first line pair assigned from its
  three-product line product, the 86 others as two unit lines of 9 products each (86 x 18), four scalings per line pair (87 x 4) —
  against miller_loop_keyed's 2 508 and 348."""
import json
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_kd_unit.cpp")

DRIVER = r'''
import ctypes, json, sys
lib, job = sys.argv[1], json.loads(open(sys.argv[2]).read())
L = ctypes.CDLL(lib)
i32 = ctypes.c_int32
assert 63 * 12 + 3 + 86 * 18 == 2307 and 87 * 4 == 348
n = 0
for h, sig, pk, key_inf in job["tuples"]:
    a, b, cnt = (i32 * 108)(), (i32 * 108)(), (ctypes.c_ulonglong * 4)()
    assert L.hu_miller_both(bytes.fromhex(h), bytes.fromhex(sig), bytes.fromhex(pk), key_inf, a, b, cnt) == 0
    assert all(0 <= w < 1 << 29 for w in a), "not canonical"
    assert list(a) == list(b), (h[:8], sig[:8], pk[:8], key_inf)
    assert list(cnt) == [2508, 348, 2307, 348], list(cnt)
    n += 1
print("ok", n, "first digit", L.hu_first_digit())
'''


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    out = tmp_path_factory.mktemp("ku")
    # the compile lines of libhostsim_pair.so / libhostsim_pair_bounds.so (tests/hostsim/Makefile)
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-g", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libku_%s.so" % name))
        procs[name] = (so, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + ["-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas",
                                                                                       "-Wno-unused-function", "-o", so, SRC], stderr=subprocess.PIPE, text=True))
    for name, (so, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: so for name, (so, _) in procs.items()}


@pytest.fixture(scope="module")
def job(derived):
    from oracle import bn254_model as M
    from oracle import c_oracle as c
    off = bytes.fromhex(derived["g2_not_in_subgroup"])
    assert not M.g2_in_subgroup(M.g2_from_uncompressed(off, subgroup_check=False))
    cases = [v for v in derived["verify_cases"] if v["status"] in (0, 9) and bytes.fromhex(v["pk"]) != bytes(128)
             and bytes.fromhex(v["sig"]) != bytes(64)]
    valid = [v for v in cases if v["status"] == 0][:2]
    wrong = [v for v in cases if v["status"] == 9][:1]
    assert len(valid) == 2 and len(wrong) == 1
    tuples = []
    for v in valid + wrong:
        st, h, _ = c.hash_to_g1(bytes.fromhex(v["message_hex"]))
        assert st == 0
        tuples.append([h.hex(), v["sig"], v["pk"], 0])
    h, sig, pk, _ = tuples[0]
    zero1, zero2 = bytes(64).hex(), bytes(128).hex()
    tuples += [[zero1, sig, pk, 0],          # pair A skipped by its G1 point
               [h, sig, pk, 1],              # ... by a refused key (generator table, as the device builds it)
               [h, sig, zero2, 0],           # ... by the identity key
               [h, zero1, pk, 0],            # pair B skipped
               [zero1, zero1, pk, 0],        # both
               [h, zero1, pk, 1]]
    tuples.append([h, sig, off.hex(), 0])    # a key outside G2 (flags = 0 does not test the subgroup)
    return {"tuples": tuples}


@pytest.mark.parametrize("build", ["plain", "bounds"])
def test_unit_line_loop(libs, job, build, tmp_path):
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    p = subprocess.run([sys.executable, "-c", DRIVER, libs[build], str(jf)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and p.stdout.startswith("ok"), (p.stdout[-500:], p.stderr[-3000:])
