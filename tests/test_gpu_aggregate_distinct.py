"""Aggregate verification over DISTINCT messages (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct[_device]) on the GPU,
against statuses composed from the oracle's g1_validate / g2_validate / hash_to_g1 / pairing_check by the header's rule, and against
bn254_batch_verify for aggregates of one pair.  Run on the MI355X box: -m gpu."""
import ctypes
import os
import subprocess

import pytest

from tests.conftest import ws_default
from tests.datagen import D, sk_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
W = ws_default("AGGD_WG_PAIRS")          # pairs one workgroup of the segmented Miller kernel reduces
FLAGS = [0, 1, 2, 3]                      # BN254_FLAG_G2_SUBGROUP_CHECK | BN254_FLAG_REJECT_IDENTITY


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


@pytest.fixture(scope="module")
def keys(eng):
    """64 key pairs: secret keys and their public keys (GPU key derivation, oracle-pinned elsewhere)"""
    sks = [sk_bytes(j) for j in range(64)]
    pks, st = eng.batch_g2_mul(None, b"".join(sks), 64, reduce_scalar=True)
    assert st == bytes(64)
    return sks, [pks[128 * j:128 * j + 128] for j in range(64)]


def neg_g2(c):
    return c.g2_mul(c.g2_generator(), (R - 1).to_bytes(32, "big"))


def expected(c, msgs, pks, sks, sig, flags):
    """the header's rule, from the oracle: sigma's decode status, the first failing key, the first failing message, the pairing check.
    The oracle's pairing_check takes at most 16 pairs: a longer aggregate is checked as e(sum_j sk_j H(m_j), G2) * e(sigma, -G2) == 1,
    the same product by bilinearity (pk_j = sk_j G2, the keys' secret scalars are known)"""
    st = c.g1_validate(sig, flags)
    if st:
        return st
    for pk in pks:
        st = c.g2_validate(pk, flags)
        if st:
            return st
    hs = []
    for m in msgs:
        st, pt, _ = c.hash_to_g1(m)
        if st:
            return 1
        hs.append(pt)
    if len(msgs) + 1 <= 16:
        return c.pairing_check(b"".join(hs) + sig, b"".join(pks) + neg_g2(c), len(msgs) + 1)
    acc = bytes(64)
    for h, sk in zip(hs, sks):
        acc = c.g1_add(acc, c.g1_mul(h, sk))
    return c.pairing_check(acc + sig, c.g2_generator() + neg_g2(c), 2)


def sign_all(eng, msgs, sks):
    sigs, st = eng.batch_sign(msgs, b"".join(sks))
    assert st == bytes(len(msgs))
    return [sigs[64 * i:64 * i + 64] for i in range(len(msgs))]


def g1_sum(eng, sigs):
    if not sigs:
        return bytes(64)
    off = (ctypes.c_uint64 * 2)(0, len(sigs))
    out, st = eng.batch_g1_sum(b"".join(sigs), off)
    assert st == b"\x00"
    return out


def flat(aggs):
    msgs = [m for a in aggs for m in a[0]]
    pks = b"".join(p for a in aggs for p in a[2])
    return msgs, pks, b"".join(a[1] for a in aggs), [len(a[0]) for a in aggs]


def ragged_batch(eng, c, keys):
    """aggregate sizes 0..3 and every workgroup boundary -1 / 0 / +1, each valid and mutated (one key swapped, messages permuted between two
    keys, sigma + the generator, an undecodable key late in the aggregate); sizes placed so that aggregates straddle workgroups"""
    sks, pks = keys
    sizes = [0, 1, 2, 3, W - 1, W, W + 1, 2 * W - 1, 2 * W, 2 * W + 1, 5, 129]
    g1 = c.g1_generator()
    aggs, t = [], 0
    for si, k in enumerate(sizes):
        for variant in range(5):
            msgs = [D("aggd/ragged/%d/%d" % (si, variant), j) for j in range(k)]
            kidx = [(t + j) % 64 for j in range(k)]
            t += k + 1
            sigs = sign_all(eng, msgs, [sks[x] for x in kidx]) if k else []
            sigma = g1_sum(eng, sigs)
            apks = [pks[x] for x in kidx]
            asks = [sks[x] for x in kidx]
            if variant == 1 and k:
                apks[k // 2] = pks[(kidx[k // 2] + 1) % 64]                 # one key swapped
                asks[k // 2] = sks[(kidx[k // 2] + 1) % 64]
            elif variant == 2 and k >= 2:
                msgs[0], msgs[1] = msgs[1], msgs[0]                        # messages permuted between two keys
            elif variant == 3:
                sigma = c.g1_add(sigma, g1) if sigma != bytes(64) else g1  # sigma + the generator
            elif variant == 4 and k:
                bad = bytearray(apks[k - 1]); bad[70] ^= 1; apks[k - 1] = bytes(bad)   # off the twist, late in the aggregate
            aggs.append((msgs, sigma, apks, asks))
    return aggs


def valid_aggregate(eng, keys, k, tag):
    sks, pks = keys
    msgs = [D(tag, j) for j in range(k)]
    sigs, st = eng.batch_sign(msgs, b"".join(sks[j % 64] for j in range(k)))
    assert st == bytes(k)
    sigma, st = eng.batch_g1_sum(sigs, (ctypes.c_uint64 * 2)(0, k))
    assert st == b"\x00"
    return msgs, sigma, [pks[j % 64] for j in range(k)], [sks[j % 64] for j in range(k)]


@pytest.fixture(scope="module")
def ragged(eng, c, keys):
    """the ragged batch (one Miller loop per pair: fewer than AGGD_TWO_PER_PAIR_MIN_M pairs) and the same with a valid aggregate appended
    that takes the whole batch past that threshold (the segmented two-pair Miller kernel); the long aggregate is valid by construction
    (batch_sign + batch_g1_sum, both oracle-pinned)"""
    aggs = ragged_batch(eng, c, keys)
    want = {f: bytes(expected(c, a[0], a[2], a[3], a[1], f) for a in aggs) for f in (0, 1)}
    long_agg = valid_aggregate(eng, keys, ws_default("AGGD_TWO_PER_PAIR_MIN_M"), "aggd/ragged/long")
    return aggs, want, aggs + [long_agg], {f: want[f] + b"\x00" for f in want}


def test_single_pair_aggregates_equal_batch_verify(eng, keys, derived):
    """(a) k = 1: byte for byte the statuses of bn254_batch_verify on ~4096 mutated tuples, with and without each flag, and with hash failures"""
    from bn254_amd.engine import OPT_HASH_MAX_TRIES
    sks, pks = keys
    n = 4096
    msgs = [D("aggd/k1", i) for i in range(n)]
    sigs = sign_all(eng, msgs, [sks[i % 64] for i in range(n)])
    kp = [pks[i % 64] for i in range(n)]
    off_sub = bytes.fromhex(derived["g2_not_in_subgroup"])
    for i in range(n):
        if i % 16 == 15:
            sigs[i] = sigs[i - 1]                                         # wrong signature: 9
        elif i % 16 == 3:
            s = bytearray(sigs[i]); s[40] ^= 4; sigs[i] = bytes(s)         # off the curve
        elif i % 16 == 5:
            p = bytearray(kp[i]); p[100] ^= 2; kp[i] = bytes(p)           # off the twist
        elif i % 16 == 7:
            kp[i] = off_sub                                               # outside the order-r subgroup
        elif i % 16 == 9:
            sigs[i] = bytes(64)                                           # identity signature
        elif i % 16 == 11:
            kp[i] = bytes(128)                                            # identity key
        elif i % 16 == 13:
            s = bytearray(sigs[i]); s[0] = 0xFF; sigs[i] = bytes(s)        # coordinate >= q
    S, P = b"".join(sigs), b"".join(kp)
    try:
        for tries in (0, 3):                                              # 3: messages that need more counters fail to hash
            eng.set_option(OPT_HASH_MAX_TRIES, tries)
            for f in FLAGS:
                got = eng.batch_aggregate_verify_distinct(msgs, P, S, [1] * n, flags=f)
                want = eng.batch_verify(msgs, S, P, flags=f)
                assert got == want, (tries, f)
                assert len(set(want)) >= 4
    finally:
        eng.set_option(OPT_HASH_MAX_TRIES, 0)


def test_ragged_batch_against_oracle(eng, ragged):
    """(b) ragged aggregates (sizes 0..3, the workgroup boundaries -1 / 0 / +1, straddling workgroups), valid and mutated"""
    aggs, want, aggs2, want2 = ragged
    for batch, w in ((aggs, want), (aggs2, want2)):                       # one pair per lane pair, then two (the segmented Miller kernel)
        msgs, pks, sigs, sizes = flat(batch)
        assert len(msgs) > ws_default("LM_MAX_BATCH_DEFAULT")             # the lane-pair routes
        for f in (0, 1):
            got = eng.batch_aggregate_verify_distinct(msgs, pks, sigs, sizes, flags=f)
            assert got == w[f], [(i, g, x, sizes[i]) for i, (g, x) in enumerate(zip(got, w[f])) if g != x][:8]
    assert want[0].count(0) >= 12 and want[0].count(9) >= 20 and set(want[0]) - {0, 9}


def test_routes_agree(eng, ragged):
    """(d) lane pairs, one lane per pairing (BN254_OPT_PAIR_LANES 0) and the lane-machine route for small m give identical statuses"""
    from bn254_amd.engine import OPT_LM_MAX_BATCH, OPT_PAIR_LANES
    aggs, want, aggs2, want2 = ragged
    msgs, pks, sigs, sizes = flat(aggs2)
    try:
        eng.set_option(OPT_PAIR_LANES, 0)
        assert eng.batch_aggregate_verify_distinct(msgs, pks, sigs, sizes, flags=1) == want2[1]
        eng.set_option(OPT_PAIR_LANES, 1)
        msgs, pks, sigs, sizes = flat(aggs)
        eng.set_option(OPT_LM_MAX_BATCH, len(msgs))                       # every pair through the lane machine
        assert eng.batch_aggregate_verify_distinct(msgs, pks, sigs, sizes, flags=1) == want[1]
        small = aggs[:20]                                                 # sizes 0..3 and W - 1: the default small-m route
        m, p, s, z = flat(small)
        eng.set_option(OPT_LM_MAX_BATCH, ws_default("LM_MAX_BATCH_DEFAULT"))
        assert len(m) <= ws_default("LM_MAX_BATCH_DEFAULT")
        assert eng.batch_aggregate_verify_distinct(m, p, s, z, flags=1) == want[1][:20]
    finally:
        eng.set_option(OPT_PAIR_LANES, 1)
        eng.set_option(OPT_LM_MAX_BATCH, ws_default("LM_MAX_BATCH_DEFAULT"))


@pytest.mark.parametrize("k", [W * W + 1, 1 << 20])
def test_multi_level_reduction(eng, keys, k):
    """(c) one aggregate beyond one level of partials, and one of 2^20 pairs: valid -> 0, one key replaced -> 9 (sigma from batch_sign +
    batch_g1_sum, both oracle-pinned); a small aggregate on either side checks that the neighbours are untouched"""
    sks, pks = keys
    msgs = [D("aggd/big/%d" % k, j) for j in range(k)]
    sigs, st = eng.batch_sign(msgs, b"".join(sks[j % 64] for j in range(k)))
    assert st == bytes(k)
    off = (ctypes.c_uint64 * 2)(0, k)
    sigma, st = eng.batch_g1_sum(sigs, off)
    assert st == b"\x00"
    kp = b"".join(pks[j % 64] for j in range(k))
    small_m = [D("aggd/big/side", j) for j in range(3)]
    small_s = g1_sum(eng, sign_all(eng, small_m, sks[:3]))
    small_p = b"".join(pks[:3])
    got = eng.batch_aggregate_verify_distinct(small_m + msgs + small_m, small_p + kp + small_p, small_s + sigma + small_s, [3, k, 3])
    assert got == bytes([0, 0, 0])
    j = k - 5
    bad = kp[:128 * j] + pks[(j + 1) % 64] + kp[128 * (j + 1):]
    got = eng.batch_aggregate_verify_distinct(msgs, bad, sigma, [k])
    assert got == bytes([9])


def test_device_form_offsets(eng, keys):
    """(e) the _device form on a caller stream: a decreasing agg_off pair gives 2 to that aggregate, a reversed message offset gives 5 to
    its aggregate only"""
    from tests.hip_ctypes import DevBuf, Stream
    from bn254_amd.engine import pack_messages
    sks, pks = keys
    sizes = [2, 3, 1, 4]
    m = sum(sizes)
    msgs = [D("aggd/dev", j) for j in range(m)]
    sigs = sign_all(eng, msgs, [sks[j] for j in range(m)])
    sigmas, pos = [], 0
    for k in sizes:
        sigmas.append(g1_sum(eng, sigs[pos:pos + k]))
        pos += k
    blob, off = pack_messages(msgs)
    off = list(off)
    off_bad = off[:]
    off_bad[7] = off[6] - 1                                               # message 6 reversed, message 7 longer (both in aggregate 3: pairs 6..9)
    agg_ok = [0, 2, 5, 6, 10]
    agg_bad = [0, 2, 1, 6, 10]                                            # aggregate 1: [2, 1) reversed; aggregate 2: [1, 6) starts before 2
    st_dev = Stream()
    bufs = []
    try:
        def dev(data):
            b = DevBuf(len(data), data=data)
            bufs.append(b)
            return b

        d_msgs, d_pks, d_sigs = dev(blob), dev(b"".join(pks[:m])), dev(b"".join(sigmas))
        u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
        d_status = DevBuf(8, fill=0xEE)
        bufs.append(d_status)
        cases = [(off, agg_ok, [0, 0, 0, 0]), (off_bad, agg_ok, [0, 0, 0, 5]), (off, agg_bad, [0, 2, 2, 0])]
        for o, a, want in cases:
            d_off, d_agg = dev(u64(o)), dev(u64(a))
            eng.batch_aggregate_verify_distinct_device(d_msgs.ptr, d_off.ptr, d_pks.ptr, m, d_sigs.ptr, d_agg.ptr, len(sizes), d_status.ptr,
                                                       stream=st_dev.handle)
            st_dev.synchronize()
            assert list(d_status.download(len(sizes))) == want, (o, a)
    finally:
        for b in bufs:
            b.free()
        st_dev.destroy()


def test_python_api_end_to_end(eng):
    """(f) ECDSA.aggregate_verify / batch_aggregate_verify_distinct: None for a valid aggregate, Error(VerificationFailed) for a swapped pair"""
    from bn254_amd.api import ECDSA, Error, ErrorKind, PrivateKey, PublicKey
    sk = [PrivateKey(int.from_bytes(sk_bytes(j), "big")) for j in range(3)]
    pk = [PublicKey.from_private_key(s) for s in sk]
    msgs = [b"block 7 tx 0", b"block 7 tx 1", b"block 7 tx 2"]
    sigs = [ECDSA.sign(m, s) for m, s in zip(msgs, sk)]
    sigma = sigs[0] + sigs[1] + sigs[2]
    assert ECDSA.aggregate_verify(msgs, sigma, pk, engine=eng) is None
    with pytest.raises(Error) as e:
        ECDSA.aggregate_verify([msgs[1], msgs[0], msgs[2]], sigma, pk, engine=eng)
    assert e.value.kind == ErrorKind.VerificationFailed
    res = ECDSA.batch_aggregate_verify_distinct([(msgs, sigma, pk), (msgs[:2], sigs[0] + sigs[1], pk[:2]), (msgs[:2], sigma, pk[:2])], engine=eng)
    assert res == [None, None, Error(ErrorKind.VerificationFailed)]


def test_cpp_example(tmp_path):
    """(f) host/aggregate_distinct_example.cpp builds with -Wall -Werror against the library and prints success"""
    from bn254_amd import _native
    exe = str(tmp_path / "aggregate_distinct_example")
    host = os.path.join(ROOT, "bn254_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", host,
                           os.path.join(host, "aggregate_distinct_example.cpp"), "-o", exe, _native.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "aggregate over distinct messages: ok" in out.stdout
