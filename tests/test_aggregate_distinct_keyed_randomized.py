"""Randomised batch verification of keyed aggregates over distinct messages, the parts that need no GPU:
- the two entry points and the debug hook are declared, exported with the header's arity and bound in INTEGRATION.md's extern block;
- the two options are mirrored in bn254_amd.engine, and the defaults the tests restore are in bn254_ws.h;
- the Python mirror refuses mismatched lengths and a bad seed before it touches a device;
- the G1 side and the group checks (tests/hostsim/hostsim_aggd_rand.cpp: bn254_aggrand.h compiled for the host, the slot loop and the final
  exponentiation) against a model of the header's rule built from the oracle (g1_mul, g1_add, pairing_check) and hashlib for r_i: the scaled
  points, the (group, key) bucket sums and S_g, and the group verdicts, in 128-bit, RAND64 and GLV modes — plain and under the bound tracker
  (-DBN_TRACK_BOUNDS aborts on a violated bound)."""
import ctypes
import hashlib
import os
import random
import re

import pytest

from bn254_amd import _native
from tests import aggr_model as AM
from tests.aggr_model import LAMBDA, R, model, r_model  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_aggd_rand.cpp")
NAMES = ["bn254_batch_aggregate_verify_distinct_keyed_randomized", "bn254_batch_aggregate_verify_distinct_keyed_randomized_device"]


def _arity(decl):
    return len([a for a in decl.split(",") if a.strip()])


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bn254_hip.h")).read(), flags=re.S)


def _decl(name):
    return re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, _header())


def test_declared_and_registered():
    for name in NAMES + ["bn254_debug_agg_rand_last", "bn254_debug_agg_rand_sums"]:
        assert _decl(name), name
        assert name in _native.EXPORTED_SYMBOLS, name
    host, dev = _decl(NAMES[0]).group(1), _decl(NAMES[1]).group(1)
    assert _arity(host) == 11 and _arity(dev) == 12
    assert "const uint8_t *seed32" in host and "const uint8_t *seed32" in dev and "const uint32_t *d_key_idx" in dev
    assert _arity(_decl("bn254_debug_agg_rand_last").group(1)) == 2
    assert _arity(_decl("bn254_debug_agg_rand_sums").group(1)) == 10


def test_exported_by_the_library():
    _native.build()
    lib = _native.load()
    for name in NAMES + ["bn254_debug_agg_rand_last", "bn254_debug_agg_rand_sums"]:
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == _arity(_decl(name).group(1)), name


def test_integration_extern_block_matches_header():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        m = re.search(r"\bfn\s+%s\s*\(([^)]*)\)\s*->\s*c_int;" % name, doc)
        assert m, name
        assert _arity(m.group(1)) == _arity(_decl(name).group(1)), name


def test_options_mirrored_with_defaults():
    from bn254_amd import engine
    text = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    for opt in ("AGG_RAND_MIN_PAIRS", "AGG_RAND_GROUP_PAIRS"):
        m = re.search(r"#define BN254_OPT_%s (\d+)" % opt, text)
        assert m and getattr(engine, "OPT_" + opt) == int(m.group(1)), opt
    ws = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    for d in ("AGG_RAND_MIN_PAIRS_DEFAULT", "AGG_RAND_GROUP_PAIRS_DEFAULT"):
        assert re.search(r"#define\s+%s\s+\d+" % d, ws), d


def test_api_rejects_bad_input_before_the_device(monkeypatch):
    from bn254_amd import api, engine

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(engine, "default_engine", no_device)
    sig = api.Signature(bytes(64))
    with pytest.raises(api.Error) as e:
        api.ECDSA.batch_aggregate_verify_distinct_keyed_randomized([([b"a"], sig, [0]), ([b"a", b"b"], sig, [1])])
    assert e.value.kind == api.ErrorKind.InvalidLength
    with pytest.raises(ValueError):
        api.ECDSA.batch_aggregate_verify_distinct_keyed_randomized([([b"a"], sig, [0])], seed=bytes(31))


# ---- the G1 side and the group checks against the oracle ---------------------------------------------------------------------------------
MODES = [(0, "rand128"), (1, "rand64"), (2, "glv")]


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """the harness with the flags of the Makefile's libhostsim_pair.so and libhostsim_pair_bounds.so, built side by side"""
    import subprocess
    out = tmp_path_factory.mktemp("har")
    common = ["-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libhar_%s.so" % name))
        procs[name] = (so, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + common + ["-o", so, SRC], stderr=subprocess.PIPE, text=True))
    for name, (so, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: ctypes.CDLL(so) for name, (so, _) in procs.items()}


def test_rand_scalar_model():
    """r_i as documented: 0 -> 1 never hides a zero of the GLV form, which is k1 + k2 lambda with k1 = 1 only when both halves are zero"""
    seed = bytes(range(32))
    assert r_model(seed, 5, 1) == int.from_bytes(hashlib.sha256(seed + (5).to_bytes(8, "little")).digest()[:8], "little")
    assert r_model(seed, 5, 0) % (1 << 64) == r_model(seed, 5, 1)


@pytest.mark.parametrize("build", ["plain", "bounds"])
def test_scaled_points_against_the_oracle(libs, build):
    """aggr_scale: r_i H for several aggregate indices (0, 1, a large one) in every mode, r = 1 for a group of one, the identity stays"""
    from oracle import c_oracle as c
    lib = libs[build]
    seed = hashlib.sha256(b"aggdr/scale").digest()
    out = ctypes.create_string_buffer(64)
    pts = [c.hash_to_g1(b"aggdr/scale/%d" % j)[1] for j in range(3)] + [bytes(64)]
    for i in (0, 1, 7, (1 << 32) + 3):
        for mode, name in MODES:
            for p in pts:
                lib.har_scale(p, seed, ctypes.c_uint64(i), mode, 0, out)
                want = c.g1_mul(p, (r_model(seed, i, mode) % R).to_bytes(32, "big")) if p != bytes(64) else bytes(64)
                assert out.raw == want, (i, name)
                lib.har_scale(p, seed, ctypes.c_uint64(i), mode, 1, out)
                assert out.raw == p, (i, name)


@pytest.fixture(scope="module")
def batch():
    """5 keys and the identity key (index 5); with groups of 16 messages: group 0 = aggregates 0-4 (repeated keys, an identity-key pair,
    an empty aggregate, aggregate 2 with a wrong sigma: the group fails), group 2 = aggregates 5-7 (an identity H, a bucket of one: key 4,
    valid), group 3 = aggregate 8 alone (300 messages over one key: a bucket of 300, r = 1, valid), the other groups empty."""
    from oracle import c_oracle as c
    rnd = random.Random(20261017)
    g2 = c.g2_generator()
    sks = [rnd.randrange(1, R) for _ in range(5)]
    pks = [c.g2_mul(g2, s.to_bytes(32, "big")) for s in sks] + [bytes(128)]
    plan = [[0, 1, 0, 2], [3, 3, 5], [1, 0, 1, 2, 0], [], [0, 1] * 10, [0, 1, 2, 3, 0, 1], [4], [3] * 10, [2] * 300]
    hs, kidx, sigs, off = [], [], [], [0]
    for a, keys in enumerate(plan):
        sigma = bytes(64)
        for j, key in enumerate(keys):
            st, h, _ = c.hash_to_g1(b"aggdr/batch/%d/%d" % (a, j))
            assert st == 0
            if (a, j) == (5, 2):
                h = bytes(64)                                           # an identity H(m): its pair contributes one
            if key < 5:
                sigma = c.g1_add(sigma, c.g1_mul(h, sks[key].to_bytes(32, "big")))
            hs.append(h)
            kidx.append(key)
        if a == 2:
            sigma = c.g1_add(sigma, c.g1_generator())
        sigs.append(sigma)
        off.append(off[-1] + len(keys))
    return pks, hs, kidx, sigs, off


@pytest.mark.parametrize("build", ["plain", "bounds"])
@pytest.mark.parametrize("mode,name", MODES)
def test_buckets_and_group_verdicts_against_the_oracle(libs, batch, build, mode, name):
    """bucket sums (repeated keys, identity key, identity H, a bucket of one, a bucket of 300), S_g and the verdicts of groups of several
    aggregates, of one (r = 1) and of none; two group sizes"""
    from oracle import c_oracle as c
    lib = libs[build]
    pks, hs, kidx, sigs, off = batch
    K, m, n = len(pks), len(hs), len(sigs)
    seed = hashlib.sha256(b"aggdr/groups/%d" % mode).digest()
    for gp in ((16, 1024) if build == "plain" else (16,)):
        G = max(gp, K)
        ng = m // G + 1
        buckets, verdict, tp = ctypes.create_string_buffer(64 * ng * (K + 1)), ctypes.create_string_buffer(ng), ctypes.c_uint64()
        rc = lib.har_groups(ctypes.c_size_t(K), b"".join(pks), ctypes.c_size_t(m), b"".join(hs), (ctypes.c_uint32 * m)(*kidx), ctypes.c_size_t(n),
                            (ctypes.c_uint64 * (n + 1))(*off), b"".join(sigs), seed, mode, ctypes.c_uint64(gp), buckets, verdict, ctypes.byref(tp))
        assert rc == 0
        sums, want, pairs = model(c, pks, hs, kidx, sigs, off, seed, mode, gp)
        got = [buckets.raw[64 * b:64 * b + 64] for b in range(ng * (K + 1))]
        assert got == sums, (gp, [b for b in range(len(sums)) if got[b] != sums[b]])
        assert list(verdict.raw) == want and tp.value == pairs, (gp, list(verdict.raw), want)
        if gp == 16:
            assert want[:4] == [9, 255, 0, 0] and set(want[4:]) == {255}, want
            assert off[8] // G == 3 and off[7] // G == 2 and off[9] - off[8] == 300
        else:
            assert want == [9], want                                    # one group: the wrong sigma fails it


def test_grouping_model_against_the_harness(libs, batch):
    """tests/aggr_model.py: grouping() — what bn254_debug_agg_rand_last must report — against the harness' table pairs and group verdicts
    on the batch above (aggregate 2 is the only wrong one), two group sizes; and with aggregates taken off the check, against model()"""
    from oracle import c_oracle as c
    lib = libs["plain"]
    pks, hs, kidx, sigs, off = batch
    K, m, n = len(pks), len(hs), len(sigs)
    sizes = [off[i + 1] - off[i] for i in range(n)]
    key_inf = [p == bytes(128) for p in pks]
    seed = hashlib.sha256(b"aggdr/grouping").digest()
    for gp, want in ((16, dict(groups=3, failed_groups=1, rechecked=5, single_groups=1)), (1024, dict(groups=1, failed_groups=1, rechecked=9, single_groups=0))):
        ng = m // max(gp, K) + 1
        buckets, verdict, tp = ctypes.create_string_buffer(64 * ng * (K + 1)), ctypes.create_string_buffer(ng), ctypes.c_uint64()
        rc = lib.har_groups(ctypes.c_size_t(K), b"".join(pks), ctypes.c_size_t(m), b"".join(hs), (ctypes.c_uint32 * m)(*kidx), ctypes.c_size_t(n),
                            (ctypes.c_uint64 * (n + 1))(*off), b"".join(sigs), seed, 0, ctypes.c_uint64(gp), buckets, verdict, ctypes.byref(tp))
        assert rc == 0
        got = AM.grouping(sizes, [True] * n, [i == 2 for i in range(n)], kidx, key_inf, K, gp)
        members = AM.groups_of(sizes, [True] * n, K, gp)
        assert got["table_pairs"] == tp.value and got["groups"] == len([v for v in verdict.raw if v != 255]), (gp, got)
        assert got["failed_groups"] == len([g for g, a in members.items() if len(a) >= 2 and verdict.raw[g] == 9]), (gp, got)
        assert got["rechecked"] == sum(len(a) for g, a in members.items() if len(a) >= 2 and verdict.raw[g] == 9), (gp, got)
        assert {k: got[k] for k in want} == want, (gp, got)
    # aggregates 1 and 6 off the check: group 0 loses key 3's bucket, group 2 keeps 5 and 7; model() with at_check counts the same pairs
    at = [i not in (1, 6) for i in range(n)]
    got = AM.grouping(sizes, at, [i == 2 for i in range(n)], kidx, key_inf, K, 16)
    sums, verdict, pairs = model(c, pks, hs, kidx, sigs, off, seed, 0, 16, at_check=at)
    assert got == dict(groups=3, table_pairs=pairs, failed_groups=1, rechecked=4, single_groups=1), (got, pairs)
    assert verdict[:4] == [9, 255, 0, 0] and sums[0 * (K + 1) + 3] == bytes(64) and sums[2 * (K + 1) + 4] == bytes(64)


def test_gpu_batch_plans_meet_their_conditions():
    """the batches of tests/test_gpu_aggregate_distinct_keyed_randomized_groups.py: in every 'passing' one at least half of the counted
    groups hold two or more aggregates at the check; in the interleaved one a quarter of the aggregates are off the check and a quarter of
    the passing groups contain one; the localised failures fail some groups and not all; the run lengths meet every edge of a workgroup"""
    from tests.conftest import ws_default
    AM.check_runs(ws_default("AGGR_SUM_WG"))
    assert sorted(set(len([k for k in a.kidx if k != AM.KIDX_IDENT]) for a in AM.ragged_plan())) == AM.SIZES
    for gp in AM.GROUP_PAIRS:
        AM.check_passing(AM.ragged_plan(), gp)
        AM.check_passing(AM.runs_plan(), gp)
        AM.check_passing(AM.interleaved_plan(), gp, interleaved=True)
        AM.check_passing(AM.interleaved_plan(), gp, interleaved=True, reject_identity=True)
        for plan in (AM.failing_plan(gp),) + ((AM.cancelling_plan(gp),) if gp != 4096 else ()):   # 4 096: one group
            w = AM.plan_grouping(plan, gp)
            assert 1 <= w["failed_groups"] and (gp == 4096 or w["failed_groups"] < w["groups"] - w["single_groups"]), (gp, w)
    assert AM.plan_grouping(AM.cancelling_plan(1), 1)["failed_groups"] == 2
    for G in (AM.N_KEYS, 200):
        plan = AM.edges_plan(G)
        sizes = [len(a.msgs) for a in plan]
        assert sum(sizes) == 6 * G and sizes[-3:] == [0, 0, 0]
        assert sorted(AM.groups_of(sizes, [True] * len(plan), AM.N_KEYS, G)) == [0, 1, 3, 4, 5, 6]
        AM.check_passing(plan, G)
    for nb in (False, True):
        plan = AM.repeated_plan([2, 3, 4, 255, 256, 257, 513], nb)
        w = AM.plan_grouping(plan, 1)
        assert w["groups"] == 7 and w["single_groups"] == (0 if nb else 7), w
