"""The FOLDED ROWS of the key dedup (BN254_OPT_KEY_DEDUP_FOLD; bn254_amd/csrc/bn254_keydedup.h: kd_fold_lines, bn254_pairing.h:
miller_loop_keyed_fold, bn254_constants.h: C_NEG_G2_FOLD) in the pair layout's host emulation, plain and under the interval tracker
(-DBN_TRACK_BOUNDS aborts on a violated limb / value bound):
- a key's 22 folded rows satisfy the identity they stand for, evaluated with big integers at random points: the product of the two table
  lines of the row equals (K0 y^2 + xi) + K1 xy w + K2 x^2 w^2 + K3 y w^3 + K4 x w^4 — generator, random subgroup keys, points outside G2;
- C_NEG_G2_FOLD is the fold of C_NEG_G2_LINES;
- miller_loop_keyed_fold gives the Fq12 element of miller_loop_keyed, coefficient by coefficient after canonicalisation: valid tuples, a
  wrong signature, every skip combination (pair A by its point and by its key, pair B, both);
- products per lane: 2 376 dual (132 below miller_loop_keyed's 2 508) and 398 single (43 x 4 + 22 x 10 scalings + the six monomials x^2,
  xy, y^2 of the two G1 points, which every lane of a pair computes for itself)."""
import json
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_kd_fold.cpp")

DRIVER = r'''
import ctypes, json, random, sys
lib, job = sys.argv[1], json.loads(open(sys.argv[2]).read())
L = ctypes.CDLL(lib)
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
RINV = pow(1 << 261, -1, Q)
XI = (9, 1)
i32 = ctypes.c_int32

def fq(words):                      # 9 canonical limbs, Montgomery form -> integer
    assert all(0 <= w < 1 << 29 for w in words), words
    v = sum(w << (29 * k) for k, w in enumerate(words))
    assert v < Q
    return v * RINV % Q
def fq2(words): return (fq(words[:9]), fq(words[9:18]))
def add(a, b): return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)
def mul(a, b): return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)
def smul(a, k): return (a[0] * k % Q, a[1] * k % Q)
def wmul(a, b):                     # polynomials in w over Fq2, w^6 = xi
    r = [(0, 0)] * 11
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            r[i + j] = add(r[i + j], mul(x, y))
    return [add(r[k], mul(r[k + 6], XI)) if k + 6 < 11 else r[k] for k in range(6)]
def line(c0, c1, x, y): return [smul(c0, y), smul(c1, x), (0, 0), (1, 0), (0, 0), (0, 0)]
def folded(K, x, y):
    return [add(smul(K[0], y * y % Q), XI), smul(K[1], x * y % Q), smul(K[2], x * x % Q), smul(K[3], y), smul(K[4], x), (0, 0)]

def check_rows(plain, rows, first, rnd, what):
    for r in range(22):
        i = first[r]
        c = [fq2(plain[(i + e // 2) * 36 + (e % 2) * 18:][:18]) for e in range(4)]      # c0, c1, c0', c1'
        K = [fq2(rows[(r * 5 + e) * 18:][:18]) for e in range(5)]
        assert K[0] == mul(c[0], c[2]) and K[2] == mul(c[1], c[3]) and K[3] == add(c[0], c[2]) and K[4] == add(c[1], c[3]), (what, r)
        assert K[1] == add(mul(c[0], c[3]), mul(c[1], c[2])), (what, r)
        x, y = rnd.randrange(Q), rnd.randrange(Q)
        assert wmul(line(c[0], c[1], x, y), line(c[2], c[3], x, y)) == folded(K, x, y), (what, r)

rnd = random.Random(11)
lines, fold, const, first, naf = (i32 * (87 * 36))(), (i32 * (22 * 90))(), (i32 * (22 * 90))(), (i32 * 22)(), (i32 * 64)()
L.hf_neg_g2(lines, fold, const, first, naf)
first, naf = list(first), list(naf)
# folded row r = the doubling and the addition line of the r-th nonzero digit; the last one = the two closing lines
want, idx = [], 0
for d in naf:
    if d: want.append(idx)
    idx += 2 if d else 1
assert first == want + [idx] and idx + 2 == 87 and len(first) == 22
assert list(fold) == list(const), "C_NEG_G2_FOLD is not the fold of C_NEG_G2_LINES"
check_rows(list(lines), list(const), first, rnd, "-G2")
for hexkey in job["keys"]:
    plain, rows = (i32 * (87 * 36))(), (i32 * (22 * 90))()
    assert L.hf_fold_rows(bytes.fromhex(hexkey), plain, rows) == 0, hexkey
    check_rows(list(plain), list(rows), first, rnd, hexkey[:16])
n = 0
for h, sig, pk, key_inf in job["tuples"]:
    a, b, cnt = (i32 * 108)(), (i32 * 108)(), (ctypes.c_ulonglong * 4)()
    assert L.hf_miller_both(bytes.fromhex(h), bytes.fromhex(sig), bytes.fromhex(pk), key_inf, a, b, cnt) == 0
    assert list(a) == list(b), (h[:8], sig[:8], pk[:8], key_inf)
    assert list(cnt) == [2508, 348, 2376, 398] and cnt[0] - cnt[2] == 132, list(cnt)
    n += 1
print("ok", len(job["keys"]), n)
'''


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    out = tmp_path_factory.mktemp("kf")
    # the compile lines of libhostsim_pair.so / libhostsim_pair_bounds.so (tests/hostsim/Makefile)
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-g", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libkf_%s.so" % name))
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
    rnd = random.Random(7)
    pts = [M.G2_GEN] + [M.g2_mul(M.G2_GEN, rnd.randrange(1, M.R)) for _ in range(3)]
    keys = [M.g2_to_uncompressed(p).hex() for p in pts]
    off = bytes.fromhex(derived["g2_not_in_subgroup"])
    off_pt = M.g2_from_uncompressed(off, subgroup_check=False)
    assert not M.g2_in_subgroup(off_pt)
    keys += [off.hex()] + [M.g2_to_uncompressed(M.g2_mul(off_pt, k)).hex() for k in (2, 12345)]
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
               [h, sig, pk, 1],              # ... by a refused key (generator tables, as the device builds them)
               [h, sig, zero2, 0],           # ... by the identity key
               [h, zero1, pk, 0],            # pair B skipped
               [zero1, zero1, pk, 0],        # both
               [h, zero1, pk, 1]]
    tuples.append([h, sig, keys[4], 0])      # a key outside G2 (flags = 0 does not test the subgroup)
    return {"keys": keys, "tuples": tuples}


@pytest.mark.parametrize("build", ["plain", "bounds"])
def test_folded_rows_and_loop(libs, job, build, tmp_path):
    jf = tmp_path / "job.json"
    jf.write_text(json.dumps(job))
    p = subprocess.run([sys.executable, "-c", DRIVER, libs[build], str(jf)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and p.stdout.startswith("ok"), (p.stdout[-500:], p.stderr[-3000:])
