"""Aggregates over distinct messages against registered keys, the parts that need no GPU:
- the two entry points are declared, exported with the header's arity and bound in INTEGRATION.md's extern block;
- the Python mirror refuses mismatched lengths before it touches a device;
- -G2's lines in the key-table format (what registration appends behind the keys) equal C_NEG_G2_LINES[.][0..1] word for word;
- the slot loop of the keyed kernel (tests/hostsim/hostsim_aggd_keyed.cpp, pair-layout emulation) at width 1 and 2, on aggregates of
  k = 0..6 with random keys, identity keys, identity H(m) and sigma: its verdict equals the oracle's pairing_check and its value the
  product of per-pair miller_loop_keyed values — plain and under the bound tracker (-DBN_TRACK_BOUNDS aborts on a violated bound)."""
import ctypes
import os
import random
import re

import pytest

from bn254_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254_batch_aggregate_verify_distinct_keyed", "bn254_batch_aggregate_verify_distinct_keyed_device"]
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_aggd_keyed.cpp")
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
N_LINES, LIMBS = 87, 9


def _arity(decl):
    return len([a for a in decl.split(",") if a.strip()])


def _header_decls():
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {name: re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr) for name in NAMES}


def test_declared_and_registered():
    decls = _header_decls()
    for name in NAMES:
        assert decls[name], name
        assert name in _native.EXPORTED_SYMBOLS
    assert _arity(decls[NAMES[0]].group(1)) == 10 and _arity(decls[NAMES[1]].group(1)) == 11
    assert "const uint32_t *key_idx" in decls[NAMES[0]].group(1) and "const uint32_t *d_key_idx" in decls[NAMES[1]].group(1)


def test_exported_by_the_library():
    _native.build()
    lib = _native.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == _arity(_header_decls()[name].group(1))


def test_integration_extern_block_matches_header():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    decls = _header_decls()
    for name in NAMES:
        m = re.search(r"\bfn\s+%s\s*\(([^)]*)\)\s*->\s*c_int;" % name, doc)
        assert m, name
        assert _arity(m.group(1)) == _arity(decls[name].group(1)), name


def test_api_rejects_mismatched_lengths_before_the_device(monkeypatch):
    from bn254_amd import api, engine

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(engine, "default_engine", no_device)
    sig = api.Signature(bytes(64))
    with pytest.raises(api.Error) as e:
        api.ECDSA.aggregate_verify_keyed([b"a", b"b"], sig, [0])
    assert e.value.kind == api.ErrorKind.InvalidLength
    with pytest.raises(api.Error) as e:
        api.ECDSA.batch_aggregate_verify_distinct_keyed([([b"a"], sig, [0]), ([b"a", b"b"], sig, [1])])
    assert e.value.kind == api.ErrorKind.InvalidLength


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """the harness with the flags of the Makefile's libhostsim_pair.so and libhostsim_pair_bounds.so, built side by side"""
    import subprocess
    out = tmp_path_factory.mktemp("hak")
    common = ["-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libhak_%s.so" % name))
        procs[name] = (so, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + common + ["-o", so, SRC], stderr=subprocess.PIPE, text=True))
    for name, (so, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: so for name, (so, _) in procs.items()}


def _neg_g2_lines_from_header():
    text = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_constants.h")).read()
    m = re.search(r"C_NEG_G2_LINES\[BN_N_FIXED_LINES\]\[3\]\[2\]\[BN_LIMBS\]\s*=\s*\{(.*?)\};", text, flags=re.S)
    assert m
    words = [int(x, 0) for x in re.findall(r"-?(?:0x[0-9a-fA-F]+|\d+)", re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S))]
    assert len(words) == N_LINES * 3 * 2 * LIMBS
    return words


def test_neg_g2_key_table_is_the_constant_table(libs):
    """registration's -G2 entry ([line][c0 / c1][re / im][limb]) is C_NEG_G2_LINES[line][0 / 1], word for word"""
    const = _neg_g2_lines_from_header()
    lib = ctypes.CDLL(libs["plain"])
    out = (ctypes.c_int32 * (N_LINES * 4 * LIMBS))()
    lib.hak_neg_g2_table(out)
    for idx in range(N_LINES):
        want = const[idx * 54:idx * 54 + 36]                # coefficients 0 and 1 of the 3 x 2 x 9 words of the line
        assert list(out[idx * 36:idx * 36 + 36]) == want, idx


@pytest.fixture(scope="module")
def cases():
    """aggregates (hs, pks, sigma, oracle verdict): k = 0..6 valid and with sigma off by the generator; identity keys (their pair is
    one), an identity H(m) (ditto), an identity sigma (the empty aggregate is then valid)"""
    from oracle import c_oracle as c
    rnd = random.Random(20261016)
    g1, g2 = c.g1_generator(), c.g2_generator()
    neg_g2 = c.g2_mul(g2, (R - 1).to_bytes(32, "big"))

    def agg(k, tag, ident_keys=(), ident_h=(), bad_sigma=False):
        sks = [rnd.randrange(1, R) for _ in range(k)]
        hs, pks, sigma = [], [], bytes(64)
        for j in range(k):
            st, h, _ = c.hash_to_g1(b"aggdk/host/%s/%d" % (tag.encode(), j))
            assert st == 0
            if j in ident_h:
                h = bytes(64)
            pk = bytes(128) if j in ident_keys else c.g2_mul(g2, sks[j].to_bytes(32, "big"))
            if j not in ident_keys and j not in ident_h:
                sigma = c.g1_add(sigma, c.g1_mul(h, sks[j].to_bytes(32, "big")))
            hs.append(h)
            pks.append(pk)
        if bad_sigma:
            sigma = c.g1_add(sigma, g1)
        verdict = c.pairing_check(b"".join(hs) + sigma, b"".join(pks) + neg_g2, k + 1)
        return hs, pks, sigma, verdict

    out = []
    for k in range(7):
        out.append(agg(k, "v%d" % k))
        out.append(agg(k, "b%d" % k, bad_sigma=True))
    out.append(agg(3, "ik", ident_keys=(1,)))
    out.append(agg(4, "ik2", ident_keys=(0, 3), bad_sigma=True))
    out.append(agg(2, "ih", ident_h=(0,)))
    out.append(agg(5, "ih2", ident_h=(4,), ident_keys=(2,)))
    assert [x[3] for x in out[:14]] == [0, 9] * 7 and [x[3] for x in out[14:]] == [0, 9, 0, 0]
    return out


@pytest.mark.parametrize("build", ["plain", "bounds"])
@pytest.mark.parametrize("width", [1, 2])
def test_slot_loop_against_the_oracle(libs, cases, build, width):
    lib = ctypes.CDLL(libs[build])
    for i, (hs, pks, sigma, verdict) in enumerate(cases):
        got = lib.hak_aggregate(len(hs), b"".join(hs) or bytes(64), b"".join(pks) or bytes(128), sigma, width)
        assert got == verdict, (i, len(hs), got, verdict)
