"""Randomised batch verification of keyed aggregates over distinct messages (include/bn254_hip.h:
bn254_batch_aggregate_verify_distinct_keyed_randomized[_device]) on the GPU.  The defining identity: the same status bytes as the exact
keyed call on the same inputs.  Every case forces the randomised route (BN254_OPT_AGG_RAND_MIN_PAIRS = 0) and, where small batches should
still form many groups, a small BN254_OPT_AGG_RAND_GROUP_PAIRS.  Run on the MI355X box: -m gpu."""
import ctypes
import os

import pytest

from bn254_amd import engine as E
from tests.aggr_model import HOOK_FIELDS, KEY_INF, grouping, grouping_from_statuses
from tests.conftest import ws_default
from tests.datagen import D
from tests.test_gpu_aggregate_distinct import g1_sum, sign_all
from tests.test_gpu_aggregate_distinct_keyed import (KIDX_IDENT, N_GOOD, build, c, eng, flat, keyed, keyset, reg_set,  # noqa: F401
                                                     shared_inputs)

pytestmark = pytest.mark.gpu

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SEEDS = [bytes(range(32)), bytes([0xA5] * 31) + b"\x01"]
MODES = [("rand128", 0), ("rand64", E.FLAG_RAND64), ("glv", E.FLAG_RAND_GLV)]


@pytest.fixture(autouse=True)
def randomised(eng):
    eng.set_option(E.OPT_AGG_RAND_MIN_PAIRS, 0)
    yield
    eng.set_option(E.OPT_AGG_RAND_MIN_PAIRS, ws_default("AGG_RAND_MIN_PAIRS_DEFAULT"))
    eng.set_option(E.OPT_AGG_RAND_GROUP_PAIRS, ws_default("AGG_RAND_GROUP_PAIRS_DEFAULT"))


def rand(eng, aggs, seed=SEEDS[0], flags=0):
    msgs, idx, sigs, sizes = flat(aggs)
    return eng.batch_aggregate_verify_distinct_keyed_randomized(msgs, idx, sigs, sizes, seed, flags=flags)


@pytest.fixture(scope="module")
def ragged70(eng, c, keyset):  # noqa: F811
    return build(eng, c, keyset, [0, 1, 2, 3, 4, 5, 8, 13, 21, 34, 55, 70], "rand70")


def diff(got, want):
    return [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]


def test_ragged_same_bytes_as_the_exact_call(eng, c, keyset, ragged70):  # noqa: F811
    """sizes 0..70, every corruption of the keyed tests: two seeds, three scalar modes, sigma flags 0 / 1, groups of 1 .. many aggregates"""
    reg_set(eng, keyset)
    for f in (0, 1):
        want = keyed(eng, ragged70, f)
        assert want.count(0) >= 20 and want.count(9) >= 20 and {2, 4, 6} <= set(want)
        for gp in (1, 200, 4096):                                       # G = max(gp, 68 keys): many groups, a few, one
            eng.set_option(E.OPT_AGG_RAND_GROUP_PAIRS, gp)
            for seed in SEEDS:
                for name, mf in MODES:
                    got = rand(eng, ragged70, seed, f | mf)
                    assert got == want, (f, gp, name, diff(got, want))
                    h = eng.debug_agg_rand_last()
                    assert h["ran"] == 1
                    model = grouping_from_statuses(ragged70, want, KEY_INF, gp)      # the counters from the header's rule
                    assert {k: h[k] for k in HOOK_FIELDS} == model, (f, gp, name, h, model)


def test_reject_identity_and_hash_failures(eng, c, keyset, ragged70):  # noqa: F811
    """REJECT_IDENTITY at registration (the identity key -> 4) and HashToPointError (OPT_HASH_MAX_TRIES = 3): the exact call's bytes"""
    eng.set_option(E.OPT_AGG_RAND_GROUP_PAIRS, 100)
    try:
        reg = reg_set(eng, keyset, flags=2)
        assert reg[KIDX_IDENT] == 4
        for f in (2, 3):
            assert rand(eng, ragged70, flags=f) == keyed(eng, ragged70, f), f
        reg_set(eng, keyset)
        eng.set_option(E.OPT_HASH_MAX_TRIES, 3)
        want = keyed(eng, ragged70)
        assert 7 in want or 3 in want or len(set(want)) >= 4
        assert rand(eng, ragged70) == want
    finally:
        eng.set_option(E.OPT_HASH_MAX_TRIES, 0)
        reg_set(eng, keyset)


def test_fallbacks_give_the_same_bytes(eng, keyset, ragged70):  # noqa: F811
    """no keys, pair lanes off, m below the threshold: the exact keyed route (the hook says so)"""
    reg_set(eng, keyset)
    want = keyed(eng, ragged70)
    try:
        eng.set_option(E.OPT_AGG_RAND_MIN_PAIRS, 1 << 30)
        assert rand(eng, ragged70) == want and eng.debug_agg_rand_last()["ran"] == 0
        eng.set_option(E.OPT_AGG_RAND_MIN_PAIRS, 0)
        eng.set_option(E.OPT_PAIR_LANES, 0)
        assert rand(eng, ragged70) == want and eng.debug_agg_rand_last()["ran"] == 0
        eng.set_option(E.OPT_PAIR_LANES, 1)
        eng.register_keys(b"")
        assert rand(eng, ragged70) == keyed(eng, ragged70) and eng.debug_agg_rand_last()["ran"] == 0
    finally:
        eng.set_option(E.OPT_PAIR_LANES, 1)
        reg_set(eng, keyset)


def test_weights_are_there(eng, c, keyset):  # noqa: F811
    """two aggregates of one group with sigma_a + D and sigma_b - D: an unweighted sum would pass both; both are 9, the group failed and
    both aggregates were re-checked"""
    reg_set(eng, keyset)
    sks, pks, _ = keyset
    aggs = []
    for a in range(2):
        msgs = [D("aggdr/weights/%d" % a, j) for j in range(3)]
        kidx = [(5 * a + 3 * j) % N_GOOD for j in range(3)]
        aggs.append([msgs, g1_sum(eng, sign_all(eng, msgs, [sks[x] for x in kidx])), kidx])
    d = c.g1_mul(c.g1_generator(), (12345).to_bytes(32, "big"))
    minus_d = c.g1_mul(c.g1_generator(), (R - 12345).to_bytes(32, "big"))
    assert keyed(eng, aggs) == bytes(2) and rand(eng, aggs) == bytes(2)
    aggs[0][1] = c.g1_add(aggs[0][1], d)
    aggs[1][1] = c.g1_add(aggs[1][1], minus_d)
    for name, mf in MODES:
        assert rand(eng, aggs, flags=mf) == bytes([9, 9]), name
        h = eng.debug_agg_rand_last()
        assert (h["ran"], h["groups"], h["failed_groups"], h["rechecked"], h["single_groups"]) == (1, 1, 1, 2, 0), (name, h)


def aggregate_sigmas(eng, sigs, k, n):
    off = (ctypes.c_uint64 * (n + 1))(*[i * k for i in range(n + 1)])
    out, st = eng.batch_g1_sum(sigs, off)
    assert st == bytes(n)
    return [out[64 * i:64 * i + 64] for i in range(n)]


def test_merging_is_there(eng):
    """4 096 x 16 over 256 keys, all valid: 0 everywhere; the group checks' table pairs = sum over groups of (distinct keys + 1); no group
    failed, nothing re-checked.  The same batch with every 64th aggregate corrupted: the exact bytes"""
    sks, pks, msgs, kidx, sigs = shared_inputs(eng, 256, "rand_merge")
    eng.register_keys(b"".join(pks))
    m, k = len(msgs), 16
    n = m // k
    sigma = aggregate_sigmas(eng, sigs, k, n)
    eng.set_option(E.OPT_AGG_RAND_GROUP_PAIRS, 4096)
    assert ws_default("AGG_RAND_GROUP_PAIRS_DEFAULT") <= 4096
    got = eng.batch_aggregate_verify_distinct_keyed_randomized(msgs, kidx, b"".join(sigma), [k] * n, SEEDS[1])
    assert got == bytes(n)
    h = eng.debug_agg_rand_last()
    groups = {}
    for i in range(n):
        groups.setdefault(i * k // 4096, set()).update(kidx[i * k:(i + 1) * k])
    assert h["groups"] == len(groups) and h["table_pairs"] == sum(len(s) + 1 for s in groups.values()), h
    assert h["failed_groups"] == 0 and h["rechecked"] == 0 and h["single_groups"] == 0, h
    ms = msgs[:]
    for a in range(0, n, 64):
        ms[a * k], ms[a * k + 1] = ms[a * k + 1], ms[a * k]
    want = eng.batch_aggregate_verify_distinct_keyed(ms, kidx, b"".join(sigma), [k] * n)
    assert want.count(9) == n // 64
    assert eng.batch_aggregate_verify_distinct_keyed_randomized(ms, kidx, b"".join(sigma), [k] * n, SEEDS[0]) == want
    h = eng.debug_agg_rand_last()
    assert h["failed_groups"] == len(groups) and h["rechecked"] == n, h


def test_single_aggregate_groups_are_exact(eng):
    """one aggregate of 2^18 messages over 256 keys: 0 valid, 9 with one message swapped — one group of one (r = 1), nothing re-checked"""
    from tests.datagen import sk_bytes
    n_keys, m = 256, 1 << 18
    sks = [sk_bytes(20000 + j) for j in range(n_keys)]
    out, st = eng.batch_g2_mul(None, b"".join(sks), n_keys, reduce_scalar=True)
    assert st == bytes(n_keys)
    eng.register_keys(out)
    msgs = [D("aggdr/one", j) for j in range(m)]
    kidx = [(j * 7) % n_keys for j in range(m)]
    sigs, st = eng.batch_sign(msgs, b"".join(sks[x] for x in kidx))
    assert st == bytes(m)
    sigma = aggregate_sigmas(eng, sigs, m, 1)[0]
    for ms, want in ((msgs, 0), ([msgs[1], msgs[0]] + msgs[2:], 9)):
        assert eng.batch_aggregate_verify_distinct_keyed_randomized(ms, kidx, sigma, [m], SEEDS[0]) == bytes([want])
        h = eng.debug_agg_rand_last()
        assert (h["ran"], h["groups"], h["single_groups"], h["failed_groups"], h["rechecked"]) == (1, 1, 1, 0, 0), h
        assert h["table_pairs"] == n_keys + 1, h


def test_k1_equals_batch_verify_keyed(eng):
    """k = 1 everywhere at 65 536 tuples, every 8th mutated: byte for byte the statuses of bn254_batch_verify_keyed"""
    sks, pks, msgs, kidx, sigs = shared_inputs(eng, 256, "k1")
    n = len(msgs)
    eng.register_keys(b"".join(pks + [bytes(128)]))
    kidx = kidx[:]
    S = [sigs[64 * i:64 * i + 64] for i in range(n)]
    for i in range(0, n, 8):
        r = (i // 8) % 5
        if r == 0:
            S[i] = S[i + 1]
        elif r == 1:
            kidx[i] = (kidx[i] + 3) % 256
        elif r == 2:
            kidx[i] = 256 + 1 + (i % 3)
        elif r == 3:
            s = bytearray(S[i]); s[40] ^= 4; S[i] = bytes(s)
        else:
            kidx[i] = 256
    sig = b"".join(S)
    want = eng.batch_verify_keyed(msgs, sig, kidx, flags=0)
    assert len(set(want)) >= 3
    for gp in (256, 4096):
        eng.set_option(E.OPT_AGG_RAND_GROUP_PAIRS, gp)
        got = eng.batch_aggregate_verify_distinct_keyed_randomized(msgs, kidx, sig, [1] * n, SEEDS[0])
        assert got == want, (gp, diff(got, want))
        h = eng.debug_agg_rand_last()
        model = grouping([1] * n, [s in (0, 9) for s in want], [s == 9 for s in want], kidx, [False] * 256 + [True], 257, gp)
        assert h["ran"] == 1 and {k: h[k] for k in HOOK_FIELDS} == model, (gp, h, model)


def test_device_form(eng, keyset):  # noqa: F811
    """the _device form on a caller's stream: reversed / overlapping agg_off give 2; expect_msgs_len bounds the message spans;
    a misaligned pointer is refused; two calls enqueued back to back without a synchronise in between"""
    from tests.hip_ctypes import DevBuf, Stream
    from bn254_amd.engine import NativeError, pack_messages
    reg_set(eng, keyset)
    sks, pks, _ = keyset
    sizes = [2, 3, 1, 4]
    m = sum(sizes)
    msgs = [D("aggdr/dev", j) for j in range(m)]
    sigs = sign_all(eng, msgs, [sks[j] for j in range(m)])
    sigmas, pos = [], 0
    for k in sizes:
        sigmas.append(g1_sum(eng, sigs[pos:pos + k]))
        pos += k
    blob, off = pack_messages(msgs)
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    st_dev = Stream()
    bufs = []
    eng.set_option(E.OPT_AGG_RAND_GROUP_PAIRS, 1)
    try:
        def dev(data):
            b = DevBuf(len(data), data=data)
            bufs.append(b)
            return b

        d_msgs, d_off, d_sigs = dev(blob), dev(u64(off)), dev(b"".join(sigmas))
        d_idx = dev(u32(range(m)))
        d_st = [DevBuf(8, fill=0xEE), DevBuf(8, fill=0xEE)]
        bufs += d_st

        def enqueue(agg, which=0, sigs_ptr=None):
            d_agg = dev(u64(agg))
            eng.batch_aggregate_verify_distinct_keyed_randomized_device(d_msgs.ptr, d_off.ptr, d_idx.ptr, m, sigs_ptr or d_sigs.ptr, d_agg.ptr,
                                                                         len(sizes), SEEDS[0], d_st[which].ptr, stream=st_dev.handle)

        def run(agg):
            enqueue(agg)
            st_dev.synchronize()
            return list(d_st[0].download(len(sizes)))

        assert run([0, 2, 5, 6, 10]) == [0, 0, 0, 0]
        assert run([0, 2, 1, 6, 10]) == [0, 2, 2, 0]
        assert run([0, 3, 5, 6, 10]) == [9, 9, 0, 0]
        enqueue([0, 3, 5, 6, 10], 0)                                    # two calls, one synchronise
        enqueue([0, 2, 5, 6, 10], 1)
        st_dev.synchronize()
        assert list(d_st[0].download(4)) == [9, 9, 0, 0] and list(d_st[1].download(4)) == [0, 0, 0, 0]
        eng.expect_msgs_len(off[m] - 1)                                 # the last message runs past the declared buffer: 5
        assert run([0, 2, 5, 6, 10]) == [0, 0, 0, 5]
        assert run([0, 2, 5, 6, 10]) == [0, 0, 0, 0]                    # the declaration is consumed by one call
        with pytest.raises(NativeError) as e:
            enqueue([0, 2, 5, 6, 10], 0, sigs_ptr=d_sigs.ptr + 1)
        assert e.value.rc == -10002
    finally:
        st_dev.synchronize()
        for b in bufs:
            b.free()
        st_dev.destroy()


def test_python_api(eng, keyset):  # noqa: F811
    """ECDSA.batch_aggregate_verify_distinct_keyed_randomized: None, VerificationFailed, IndexOutOfBounds; InvalidLength before the device"""
    from bn254_amd.api import ECDSA, Error, ErrorKind, PrivateKey, PublicKey
    from tests.datagen import sk_bytes
    sk = [PrivateKey(int.from_bytes(sk_bytes(j), "big")) for j in range(3)]
    pk = [PublicKey.from_private_key(s) for s in sk]
    assert ECDSA.register_keys(pk, engine=eng) == [None, None, None]
    msgs = [b"round 10 validator 0", b"round 10 validator 1", b"round 10 validator 2"]
    sigs = [ECDSA.sign(m, s) for m, s in zip(msgs, sk)]
    sigma = sigs[0] + sigs[1] + sigs[2]
    try:
        batch = [(msgs, sigma, [0, 1, 2]), (msgs[:2], sigs[0] + sigs[1], [0, 1]), (msgs[:2], sigma, [0, 3]), (msgs, sigma, [1, 0, 2])]
        want = [None, None, Error(ErrorKind.IndexOutOfBounds), Error(ErrorKind.VerificationFailed)]
        assert ECDSA.batch_aggregate_verify_distinct_keyed_randomized(batch, engine=eng) == want
        assert ECDSA.batch_aggregate_verify_distinct_keyed_randomized(batch, seed=SEEDS[1], engine=eng, rand64=True) == want
        with pytest.raises(Error) as e:
            ECDSA.batch_aggregate_verify_distinct_keyed_randomized([(msgs, sigma, [0, 1])], engine=eng)
        assert e.value.kind == ErrorKind.InvalidLength
    finally:
        reg_set(eng, keyset)


def test_cpp_example(tmp_path):
    """host/aggregate_distinct_keyed_randomized_example.cpp builds with -Wall -Werror against the library and prints success"""
    import subprocess
    from bn254_amd import _native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "aggregate_distinct_keyed_randomized_example")
    host = os.path.join(root, "bn254_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-I", host,
                           os.path.join(host, "aggregate_distinct_keyed_randomized_example.cpp"), "-o", exe, _native.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "keyed aggregates over distinct messages, randomised: ok" in out.stdout
