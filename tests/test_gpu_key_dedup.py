"""Key deduplication of the exact verify (bn254_keydedup.hip, BN254_OPT_KEY_DEDUP): bn254_batch_verify_device on lane pairs finds the batch's
distinct keys, tabulates their lines once and runs the keyed Miller loop when the thresholds hold.  Every status byte must equal the generic
route's (KEY_DEDUP = 0, already checked against the oracle elsewhere) and, at the smallest size, the oracle's — for repeated and distinct keys,
invalid keys (off the curve, >= q, identity, outside G2) under every flag, bad signatures beside a repeated key, the fallback forced through the
developer hook, and distinct keys forced into one hash bucket (full 128-byte compare, probe overflow)."""
import pytest

from tests.datagen import D, sk_bytes

pytestmark = pytest.mark.gpu

Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


_KEYS = {}


def key_pool(eng, size):
    if size not in _KEYS:
        sks = [sk_bytes(9000 + j) for j in range(size)]
        pk, st = eng.batch_g2_mul(None, b"".join(sks), size, reduce_scalar=True)
        assert st == bytes(size)
        _KEYS[size] = (sks, pk)
    return _KEYS[size]


def make_batch(eng, n, pool, derived=None):
    """n items over `pool` keys (item i uses key i % pool): every 61st signature is its neighbour's (status 9), every 97th malformed
    (x >= q: status 6); with `derived`, four keys of the pool are replaced by invalid ones (outside G2, x >= q, off the curve, identity)"""
    sks, pk = key_pool(eng, pool)
    msgs = [D("kdedup", i) for i in range(n)]
    sigs, st = eng.batch_sign(msgs, b"".join(sks[i % pool] for i in range(n)))
    assert st == bytes(n)
    sigs = bytearray(sigs)
    good = bytes(sigs)
    for i in range(60, n, 61):
        sigs[64 * i:64 * i + 64] = good[64 * (i - 1):64 * i]
    for i in range(96, n, 97):
        sigs[64 * i:64 * i + 32] = Q.to_bytes(32, "big")
    keys = [bytearray(pk[128 * j:128 * j + 128]) for j in range(pool)]
    if derived is not None and pool >= 8:
        keys[1] = bytearray(bytes.fromhex(derived["g2_not_in_subgroup"]))
        keys[2][0:32] = Q.to_bytes(32, "big")
        keys[3][127] ^= 1
        keys[4] = bytearray(128)
    pks = b"".join(bytes(keys[i % pool]) for i in range(n))
    return msgs, bytes(sigs), pks


def verify_device(eng, msgs, sigs, pks, flags, stream=None, sync=True, **opts):
    """bn254_batch_verify_device on the batch (messages of any length), with the options `opts` set for this call only; returns the status
    bytes and leaves the key dedup's decision in verify_device.route.  stream: a torch.cuda.Stream or tests.hip_ctypes.Stream to enqueue on
    (None: the context's own); sync=False: returns collect() instead, which waits for that stream, then reads the statuses and the route —
    the inputs stay alive until then, and with a stream nothing waits on the host between the call and collect(), so calls can queue up"""
    import torch
    from bn254_amd import engine as E
    n = len(msgs)
    for k, v in opts.items():
        eng.set_option(getattr(E, "OPT_" + k), v)
    try:
        offs = [0]
        for m in msgs:
            offs.append(offs[-1] + len(m))
        d_msgs = torch.frombuffer(bytearray(b"".join(msgs) or b"\0"), dtype=torch.uint8).to("cuda:0")
        d_off = torch.tensor(offs, dtype=torch.int64, device="cuda:0")
        d_sigs = torch.frombuffer(bytearray(sigs), dtype=torch.uint8).to("cuda:0")
        d_pks = torch.frombuffer(bytearray(pks), dtype=torch.uint8).to("cuda:0")
        d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda:0")
        handle = None if stream is None else getattr(stream, "cuda_stream", None) or stream.handle
        if stream is None:
            torch.cuda.synchronize()
        else:                                          # the uploads ordered before the call on the device: no host sync between calls
            s = stream if isinstance(stream, torch.cuda.Stream) else torch.cuda.ExternalStream(handle, device="cuda:0")
            s.wait_stream(torch.cuda.current_stream())
        eng.batch_verify_device(d_msgs.data_ptr(), d_off.data_ptr(), d_sigs.data_ptr(), d_pks.data_ptr(), n, d_st.data_ptr(), flags=flags,
                                stream=handle)

        def collect(keep=(d_msgs, d_off, d_sigs, d_pks)):
            if stream is not None:
                stream.synchronize()
            eng.synchronize()
            verify_device.route = eng.debug_key_dedup_last()
            return bytes(d_st.cpu().numpy())
        return collect() if sync else collect
    finally:
        from tests.conftest import ws_default
        defaults = {"KEY_DEDUP": 1, "KEY_DEDUP_FORCE_GENERIC": 0, "KEY_DEDUP_HASH_BITS": 0,
                    "KEY_DEDUP_MAX_KEYS": ws_default("KEY_DEDUP_MAX_KEYS_DEFAULT"), "KEY_DEDUP_MIN_MULT": ws_default("KEY_DEDUP_MIN_MULT_DEFAULT"),
                    "MAX_CHUNK": 0, "ASSUME_FREE_MB": 0, "SPLIT_MILLER": 0, "PAIR_LANES": 1}
        for k in opts:
            eng.set_option(getattr(E, "OPT_" + k), defaults[k])


def test_small_vs_oracle_mixed_keys(eng, derived):
    """n = 16 385 (the first lane-pair size) over 256 keys with invalid ones among them, every flag: oracle == dedup == generic"""
    from oracle import c_oracle
    n = 16385
    msgs, sigs, pks = make_batch(eng, n, 256, derived)
    for flags in (0, 1, 2, 3):
        want, _ = c_oracle.batch_verify(msgs, sigs, pks, flags=flags, nthreads=16)
        got = verify_device(eng, msgs, sigs, pks, flags)
        assert got == want, flags
        assert verify_device.route == dict(ran=1, keys=256, flags=0, keyed_n=n, generic_n=0), (flags, verify_device.route)   # the tables ran
        assert verify_device(eng, msgs, sigs, pks, flags, KEY_DEDUP=0) == want, flags
        assert verify_device.route["ran"] == 0
    assert want.count(9) > 0 and want.count(6) > 0 and want.count(0) > 0


@pytest.mark.parametrize("n", [16385, 65536, 262144])
@pytest.mark.parametrize("pool", [1, 256, 4096, None])
def test_dedup_matches_generic(eng, derived, n, pool):
    pool = pool or n
    msgs, sigs, pks = make_batch(eng, n, pool, derived)
    for flags in ((0, 1) if pool == 256 else (0,)):
        generic = verify_device(eng, msgs, sigs, pks, flags, KEY_DEDUP=0)
        assert verify_device.route["ran"] == 0
        assert verify_device(eng, msgs, sigs, pks, flags) == generic, (n, pool, flags)
        r = verify_device.route
        assert r["ran"] == 1 and r["keys"] == pool and r["flags"] == 0, r
        keyed = pool <= 1024 and n >= 16 * pool                          # the default thresholds (bn254_ws.h)
        assert (r["keyed_n"], r["generic_n"]) == ((n, 0) if keyed else (0, n)), (n, pool, r)
        assert verify_device(eng, msgs, sigs, pks, flags, KEY_DEDUP_FORCE_GENERIC=1) == generic, (n, pool, flags)
        assert (verify_device.route["keyed_n"], verify_device.route["generic_n"]) == (0, n)
        if pool <= 1024:
            # every key in one hash bucket: one key groups by the full 128-byte compare (keyed route); 256 keys overflow the probe bound
            assert verify_device(eng, msgs, sigs, pks, flags, KEY_DEDUP_HASH_BITS=1) == generic, (n, pool, flags)
            r = verify_device.route
            if pool == 1:
                assert r["keys"] == 1 and r["flags"] == 0 and r["keyed_n"] == n, r
            else:
                assert r["flags"] & 1 and (r["keyed_n"], r["generic_n"]) == (0, n), r
        # thresholds that admit every batch: the tables of up to 4096 keys at any multiplicity
        if pool <= 4096:
            assert verify_device(eng, msgs, sigs, pks, flags, KEY_DEDUP_MAX_KEYS=4096, KEY_DEDUP_MIN_MULT=1) == generic, (n, pool, flags)
            assert verify_device.route["keyed_n"] == n, verify_device.route
    if pool == 256:
        ok = generic.count(0)
        assert ok > n // 2 and generic.count(9) > 0


def test_colliding_keys_grouped_by_bytes(eng):
    """32 distinct keys forced into two hash buckets: the probe sequences stay within the bound, so the keyed route runs on keys that share
    a hash — only the full 128-byte compare keeps them apart"""
    n = 16385
    msgs, sigs, pks = make_batch(eng, n, 32)
    generic = verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP=0)
    assert verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP_HASH_BITS=1) == generic
    assert verify_device.route == dict(ran=1, keys=32, flags=0, keyed_n=n, generic_n=0), verify_device.route
    assert generic.count(0) > n // 2
