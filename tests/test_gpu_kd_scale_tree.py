"""k_kd_scale (bn254_keydedup.hip): one inversion per key — a product tree over the key's 87 c2 values — instead of one per line.  The per-call
tables must stay those of registration and the route decision what it was: for pools of 1, 2, 5, 256 and 1 024 keys with refused, identity
and off-subgroup keys among them, the device tables read back (bn254_debug_key_tables) equal registration's word for word, and the status
bytes of the dedup route equal those of the forced generic route, of the keyed verify on the
REGISTERED tables of the same keys and (one pool) of the oracle; with a key of the twist's order-10 069 subgroup in the pool the
KD_DEGENERATE decision is the one the host's g2_line_table gives for the same keys."""
import random

import pytest

from tests.soak_gpu import twist_small_order_key
from tests.test_gpu_key_dedup import make_batch, verify_device

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    e = bn254_amd.Engine(0)
    from bn254_amd import engine as E
    e.set_option(E.OPT_KEY_DEDUP_MIN_MULT, 1)
    return e


@pytest.mark.parametrize("pool", [1, 2, 5, 256, 1024])
def test_tables_of_the_call_are_those_of_registration(eng, derived, pool):
    n = 16385
    msgs, sigs, pks = make_batch(eng, n, pool, derived)          # pools of 8 keys and more carry four invalid keys
    keyed = verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP_MIN_MULT=1)
    r = verify_device.route
    assert (r["ran"], r["keys"], r["flags"], r["keyed_n"], r["generic_n"]) == (1, pool, 0, n, 0), r
    # the tables the call built, word for word those of registration (g2_line_table + fp_canon) for every key both sides accept
    words, rep, st_kd, inf_kd = eng.debug_key_tables(0, 0, pool)
    assert sorted(r % pool for r in rep) == list(range(pool))
    st_reg = eng.register_keys(b"".join(pks[128 * r:128 * r + 128] for r in rep), flags=0)
    words_reg, _, _, inf_reg = eng.debug_key_tables(1, 0, pool)
    per_key, same = 87 * 36, 0
    for k in range(pool):
        if st_kd[k] == 0 and st_reg[k] == 0 and not inf_kd[k] and not inf_reg[k]:
            assert words[k * per_key:(k + 1) * per_key] == words_reg[k * per_key:(k + 1) * per_key], (pool, k, rep[k])
            same += 1
    assert same >= pool - 4 and same >= 1                         # all but make_batch's four invalid keys
    generic = verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP_FORCE_GENERIC=1)
    assert (verify_device.route["keyed_n"], verify_device.route["generic_n"]) == (0, n)
    assert keyed == generic, pool
    assert keyed.count(0) > 0 and keyed.count(9) > 0
    st_keys = eng.register_keys(pks[:128 * pool], flags=0)       # the same keys through g2_line_table
    registered = eng.batch_verify_keyed(msgs, sigs, [i % pool for i in range(n)], flags=0)
    altered = {1, 2, 3, 4} if pool >= 8 else set()              # make_batch's invalid keys: compared with the generic route above
    checked = 0
    for i in range(n):
        if st_keys[i % pool] == 0 and i % pool not in altered:
            assert keyed[i] == registered[i], (pool, i)
            checked += 1
    assert checked >= n // 2
    if pool == 256:
        from oracle import c_oracle
        want, _ = c_oracle.batch_verify(msgs, sigs, pks, flags=0, nthreads=16)
        assert keyed == want


@pytest.fixture(scope="module")
def host_degenerate(tmp_path_factory):
    """key bytes -> does g2_line_table (the host build of the device headers, tests/hostsim/hostsim_kd_builder.cpp) meet a line with c2 = 0?
    The expectation for the device's KD_DEGENERATE flag, computed without the device."""
    import ctypes
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = str(tmp_path_factory.mktemp("kb") / "libkb.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-o", so,
                           os.path.join(root, "tests", "hostsim", "hostsim_kd_builder.cpp")], timeout=900)
    lib = ctypes.CDLL(so)

    def degenerate(key):
        words = 87 * 4 * 9
        ref, kd = (ctypes.c_int32 * words)(), (ctypes.c_int32 * words)()
        rc = lib.kb_tables(bytes(key), ref, kd)
        assert rc in (0, 1), rc
        return rc == 1
    return degenerate


@pytest.mark.parametrize("pool", [2, 256])
def test_small_order_twist_key_keeps_its_decision(eng, derived, host_degenerate, pool):
    """a key of the twist's subgroup of order 10 069 in the pool (and, at 256 keys, make_batch's off-subgroup key): KD_DEGENERATE is set exactly
    when the host's g2_line_table meets a line with c2 = 0 for one of the keys that get a table of their own, and the call then takes the
    generic loop; either way the statuses are the generic route's"""
    n = 16385
    msgs, sigs, pks = make_batch(eng, n, pool, derived)
    bad = twist_small_order_key(random.Random(5))
    pks = bytearray(pks)
    for i in range(pool - 1, n, pool):                           # the pool's last key
        pks[128 * i:128 * i + 128] = bad
    pks = bytes(pks)
    expect = host_degenerate(bad) or (pool >= 8 and host_degenerate(bytes.fromhex(derived["g2_not_in_subgroup"])))
    got = verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP_MIN_MULT=1)
    r = verify_device.route
    assert r["ran"] == 1 and r["keys"] == pool and r["flags"] == (2 if expect else 0), (r, expect)
    assert (r["keyed_n"], r["generic_n"]) == ((0, n) if expect else (n, 0)), r
    assert got == verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP=0)
    assert got == verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP_FORCE_GENERIC=1)
