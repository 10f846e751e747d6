"""The folded rows of the key dedup on the device (BN254_OPT_KEY_DEDUP_FOLD; bn254_keydedup.hip: the tail of k_kd_scale, bn254_pair.hip:
k_miller_verify_keyed_fold_pair) at the first lane-pair size, 16 385 items — the smallest batch that reaches the route.  Statuses against
the generic loop forced on the device (KEY_DEDUP_FORCE_GENERIC = 1), against the line-by-line keyed kernel (the option at 0) and against the
oracle; the folded rows read back through bn254_debug_key_fold_tables against the host's kd_fold_lines, word for word (the host library is
built here from tests/hostsim/hostsim_kd_fold.cpp); what a second call and a call that drops the cache build."""
import ctypes
import os
import subprocess

import pytest

from tests.test_gpu_key_cache import Dev, N, batch_over, cache, eng, gen, keyed, odd_keys, opt, reference  # noqa: F401  (eng, gen: fixtures)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAIN, FOLD = 87 * 36, 22 * 90


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("kf") / "libkf.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function",
                           "-o", so, os.path.join(ROOT, "tests", "hostsim", "hostsim_kd_fold.cpp")])
    return ctypes.CDLL(so)


def with_identity_signatures(batch):
    """every 89th signature becomes the identity (64 zero bytes), beside the wrong (every 61st) and malformed (every 97th) ones of batch_over"""
    msgs, sigs, pks = batch
    sigs = bytearray(sigs)
    for i in range(88, len(msgs), 89):
        sigs[64 * i:64 * i + 64] = bytes(64)
    return msgs, bytes(sigs), pks


def rows_equal_host(e, host, batch, keys):
    """plain and folded rows of the last call's keys against the host's g2_line_table / kd_fold_lines on the same key bytes; a refused key
    and the identity have the generator's rows (their pair A is skipped).  Returns how many keys were compared on their own bytes."""
    from oracle import c_oracle
    pks = batch[2]
    plain, rep, st, inf = e.debug_key_tables(0, 0, keys)
    fold = e.debug_key_fold_tables(0, keys)
    assert len(fold) == keys * FOLD
    own = 0
    for k in range(keys):
        raw = pks[128 * rep[k]:128 * rep[k] + 128]
        real = st[k] == 0 and not inf[k]
        hp, hf = (ctypes.c_int32 * PLAIN)(), (ctypes.c_int32 * FOLD)()
        assert host.hf_fold_rows(raw if real else c_oracle.g2_generator(), hp, hf) == 0, (k, rep[k])
        assert plain[k * PLAIN:(k + 1) * PLAIN] == list(hp), (k, rep[k])
        assert fold[k * FOLD:(k + 1) * FOLD] == list(hf), (k, rep[k])
        own += real
    return own


@pytest.mark.parametrize("pool", [1, 5, 256])
def test_fold_statuses_and_rows(eng, gen, derived, host, pool):
    from oracle import c_oracle
    ids = list(range(pool))
    batch = with_identity_signatures(batch_over(gen, N, ids, odd_keys(gen, derived, ids)))
    want, _ = c_oracle.batch_verify(*batch, flags=0, nthreads=16)
    dev = Dev(batch)
    opt(eng, "KEY_DEDUP_FOLD", 1)
    for call in (0, 1):                                   # the second call builds nothing and gives the same statuses
        st, rep, route = dev.run(eng)
        cache(rep, pool, pool if call else 0, 0 if call else pool)
        keyed(route, N, pool)
        assert st == want, (pool, call)
        assert rows_equal_host(eng, host, batch, pool) == (pool if pool < 5 else pool - 3)   # (refused twice and the identity: generator rows)
    opt(eng, "KEY_DEDUP_FOLD", 0)                         # the line-by-line keyed kernel on the same cached rows
    st, rep, route = dev.run(eng)
    cache(rep, pool, pool, 0)
    keyed(route, N, pool)
    assert st == want
    opt(eng, "KEY_DEDUP_FOLD", 1)
    opt(eng, "KEY_DEDUP_FORCE_GENERIC", 1)                # the generic loop, decided on the device
    st, rep, route = dev.run(eng)
    assert (route["ran"], route["keyed_n"], route["generic_n"]) == (1, 0, N), route
    assert st == want
    # (a pool of five has ONE ordinary key: its items alone are valid, a fifth of the batch)
    assert want.count(0) > (N // 8 if pool == 5 else N // 2) and want.count(9) > 0 and want.count(6) > 0
    if pool >= 5:
        assert want.count(4) > 0                          # the off-curve key and identity signatures


def test_dropped_cache_rebuilds_the_folded_rows(eng, gen, host):
    """KEY_DEDUP_MAX_KEYS = 8 rows: the second call's new keys do not fit beside the first call's, the cache is dropped and every key of
    the call is built into rows other keys held before — folded rows included; then a reset by the option"""
    opt(eng, "KEY_DEDUP_MAX_KEYS", 8)
    a, b = batch_over(gen, N, list(range(0, 5))), batch_over(gen, N, list(range(3, 9)))
    st, rep, route = Dev(a).run(eng)
    cache(rep, 5, 0, 5)
    assert rows_equal_host(eng, host, a, 5) == 5
    want_a = reference(gen, a)
    assert st == want_a
    st, rep, route = Dev(b).run(eng)
    cache(rep, 6, 0, 6, True)
    keyed(route, N, 6)
    assert rows_equal_host(eng, host, b, 6) == 6
    opt(eng, "KEY_DEDUP_FOLD", 0)
    st0, rep, route = Dev(b).run(eng)
    cache(rep, 6, 6, 0)
    assert st0 == st == reference(gen, b) and st.count(0) > N // 2
    opt(eng, "KEY_DEDUP_FOLD", 1)
    opt(eng, "KEY_CACHE", 0)                              # emptied before the call: all built again
    st, rep, route = Dev(a).run(eng)
    cache(rep, 5, 0, 5)
    assert rep["dropped"] & 2
    keyed(route, N, 5)
    assert st == want_a
    assert rows_equal_host(eng, host, a, 5) == 5
