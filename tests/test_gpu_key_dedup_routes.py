"""The key dedup of bn254_batch_verify_device (bn254_keydedup.hip) beyond one default call on the context's stream: random key defects and
ragged messages at dedup sizes, slices inside one call (BN254_OPT_MAX_CHUNK and the automatic rule), a caller's stream with several calls and
a buffer growth between syncs, the other entry points that reach the route (the randomised verify below its threshold, the multi-context
layer) or must not (split A/B layout, one lane per verify), and the device-side thresholds at their boundaries.  Every case compares status
bytes with the generic route (KEY_DEDUP = 0 or KEY_DEDUP_FORCE_GENERIC) and, where affordable, the oracle, and asserts from
debug_key_dedup_last which route ran — with KEY_DEDUP = 0 every route assertion of a keyed case fails."""
import random

import pytest

from tests.conftest import ws_default
from tests.soak_gpu import dedup_batch, twist_small_order_key
from tests.test_gpu_key_dedup import make_batch, verify_device

pytestmark = pytest.mark.gpu

N_FIRST = 16385                 # the first lane-pair size of the routing table (bn254_ws.h: TRIO_MAX_BATCH_DEFAULT + 1)
MAX_KEYS = ws_default("KEY_DEDUP_MAX_KEYS_DEFAULT")
MIN_MULT = ws_default("KEY_DEDUP_MIN_MULT_DEFAULT")
MAX_KEYS_LIMIT = ws_default("KEY_DEDUP_MAX_KEYS_LIMIT")


def _kd_max_probes():
    import os
    import re
    from tests.conftest import ROOT
    text = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    m = re.search(r"#define\s+KD_MAX_PROBES\s+(\d+)u?", text)
    assert m
    return int(m.group(1))


KD_MAX_PROBES = _kd_max_probes()


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def keyed(n, keys=None):
    """the route of a call whose whole batch took the keyed Miller loop"""
    r = verify_device.route
    ok = r["ran"] == 1 and r["flags"] == 0 and (r["keyed_n"], r["generic_n"]) == (n, 0) and (keys is None or r["keys"] == keys)
    assert ok, (n, keys, r)


def generic(n):
    r = verify_device.route
    assert r["ran"] == 1 and (r["keyed_n"], r["generic_n"]) == (0, n), (n, r)


@pytest.fixture(scope="module")
def soak_keys(eng, derived):
    from tests.datagen import sk_bytes
    sks = [sk_bytes(j) for j in range(64)]
    pk_pool, st = eng.batch_g2_mul(None, b"".join(sks), 64, reduce_scalar=True)
    assert st == bytes(64)
    odd = [bytes(128), bytes.fromhex(derived["g2_not_in_subgroup"]), twist_small_order_key(random.Random(7))]
    return sks, pk_pool, odd


# ---- 1. random key defects at dedup sizes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N_FIRST, 19997])
def test_random_defects_vs_oracle(eng, c, soak_keys, n):
    """64 keys and 3 - 4 mutated variants of each (bit flips, x >= q in every field, random bytes, identity, outside G2, order 10 069),
    the soak's signature defects and ragged messages, flags 0 - 3: dedup == oracle == generic"""
    sks, pk_pool, odd = soak_keys
    rnd = random.Random(n)
    msgs, sigs, pks, kinds = dedup_batch(eng, rnd, n, sks, pk_pool, odd, b"kd-routes-%d" % n)
    assert {"flip", "q0", "q1", "q2", "q3", "rand", "odd"} <= kinds, kinds
    assert {len(m) for m in msgs} == {0, 1, 31, 55, 56, 64, 119, 120, 160}
    distinct = len({pks[128 * i:128 * i + 128] for i in range(n)})
    assert distinct <= MAX_KEYS and distinct * MIN_MULT <= n
    for flags in (0, 1, 2, 3):
        want, _ = c.batch_verify(msgs, sigs, pks, flags=flags, nthreads=16)
        assert verify_device(eng, msgs, sigs, pks, flags) == want, flags
        keyed(n, distinct)
        assert verify_device(eng, msgs, sigs, pks, flags, KEY_DEDUP=0) == want, flags
        assert verify_device.route["ran"] == 0
        assert len(set(want)) >= 4, sorted(set(want))


# ---- 2. slices of one call -----------------------------------------------------------------------------------------------------------
def _switching_pools(eng, n, at):
    """n items: item i < at over 256 keys, the rest over 96 other keys — consecutive slices build different tables"""
    msgs, sigs, pks = make_batch(eng, n, 256)
    m2, s2, p2 = make_batch(eng, n, 96)
    return msgs[:at] + m2[at:], sigs[:64 * at] + s2[64 * at:], pks[:128 * at] + p2[128 * at:]


def test_max_chunk_slices_on_the_dedup_route(eng, c):
    """BN254_OPT_MAX_CHUNK = 20 000: every full slice runs the dedup on one stream with no host sync between slices, the key pool changes
    inside the second slice; the last slice of 65 543 is a small-batch layout (no dedup), the last of 60 000 a keyed one over the new pool"""
    n = 65536 + 7
    msgs, sigs, pks = _switching_pools(eng, n, 30011)
    want, _ = c.batch_verify(msgs, sigs, pks, flags=0, nthreads=16)
    assert verify_device(eng, msgs, sigs, pks, 0, MAX_CHUNK=20000) == want
    assert verify_device.route["ran"] == 0                                    # the last slice: 5 543 items, below the lane-pair row
    assert verify_device(eng, msgs, sigs, pks, 0, MAX_CHUNK=20000, KEY_DEDUP=0) == want
    m = 60000
    got = verify_device(eng, msgs[:m], sigs[:64 * m], pks[:128 * m], 0, MAX_CHUNK=20000)
    keyed(20000, 96)                                                          # the third slice: keyed over the second pool
    assert got == want[:m]
    assert want.count(0) > n // 2 and want.count(9) > 0 and want.count(6) > 0


@pytest.mark.parametrize("free_mb", [16, 64])
def test_automatic_slicing_prices_the_key_tables(eng, c, free_mb):
    """the automatic rule (ws_chunk_for) priced through BN254_OPT_ASSUME_FREE_MB on a fresh context (nothing reserved: the inputs are made
    on another one): at 16 MB the default key tables alone (1 024 x KD_BYTES_PER_KEY, about 19 MB) do not fit — the batch must still be
    sliced, as it is with KEY_DEDUP = 0; at 64 MB slices that hold the tables run the dedup"""
    import bn254_amd
    n = 65536
    msgs, sigs, pks = make_batch(eng, n, 256)
    want, _ = c.batch_verify(msgs, sigs, pks, flags=0, nthreads=16)
    e = bn254_amd.Engine(0)
    try:
        got = verify_device(e, msgs, sigs, pks, 0, ASSUME_FREE_MB=free_mb)
        r = verify_device.route
        assert r["ran"] == 0 or r["keyed_n"] + r["generic_n"] < n, (free_mb, r)     # sliced: the last decision saw fewer than n items
        if free_mb == 64:
            assert r["ran"] == 1 and r["keyed_n"] > 0 and r["keyed_n"] < n, r      # ... by slices large enough for the keyed loop
        assert got == want, free_mb
    finally:
        e.close()


# ---- 3. a caller's stream ------------------------------------------------------------------------------------------------------------
def test_back_to_back_calls_on_a_caller_stream(eng):
    """three calls on one torch stream, one sync at the end: 256 keys (keyed), 8 keys (keyed), all-distinct keys (generic) — the
    second and third calls reset the hash table while the previous keyed Miller loop may still read the dedup buffers"""
    import torch
    n = N_FIRST
    batches = [make_batch(eng, n, 256), make_batch(eng, n, 8), make_batch(eng, n, n)]
    alone = []
    for b, k in zip(batches, (256, 8, None)):
        alone.append(verify_device(eng, *b, 0))
        if k:
            keyed(n, k)
        else:
            generic(n)
    s = torch.cuda.Stream(device="cuda:0")
    pending = [verify_device(eng, *b, 0, stream=s, sync=False) for b in batches]
    got = [p() for p in pending]
    generic(n)
    assert got == alone
    assert all(a.count(0) > n // 2 for a in alone)


def test_buffer_growth_between_calls_on_a_caller_stream(c):
    """a keyed call on a hip stream, no sync, KEY_DEDUP_MAX_KEYS raised to 4 096, a second call on the same stream whose larger batch and key
    count grow the dedup buffers (kd_reserve quiesces the context, then frees them): both results correct"""
    import bn254_amd
    from bn254_amd.engine import OPT_KEY_DEDUP_MAX_KEYS
    from tests.hip_ctypes import Stream
    e = bn254_amd.Engine(0)
    s = Stream()
    try:
        b1, b2 = make_batch(e, N_FIRST, 256), make_batch(e, 65536, 2048)
        want1, _ = c.batch_verify(*b1, flags=0, nthreads=16)
        first = verify_device(e, *b1, 0, stream=s, sync=False)
        e.set_option(OPT_KEY_DEDUP_MAX_KEYS, 4096)
        second = verify_device(e, *b2, 0, stream=s, sync=False)
        got1, got2 = first(), second()
        keyed(65536, 2048)
        assert got1 == want1
        e.set_option(OPT_KEY_DEDUP_MAX_KEYS, MAX_KEYS)
        assert got2 == verify_device(e, *b2, 0, KEY_DEDUP=0)
        assert got2.count(0) > 65536 // 2
    finally:
        e.set_option(OPT_KEY_DEDUP_MAX_KEYS, MAX_KEYS)
        s.synchronize()
        s.destroy()
        e.close()


# ---- 4. other entry points -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [N_FIRST, 65536])
def test_randomized_device_below_its_threshold(eng, n):
    """bn254_batch_verify_randomized_device below RAND_MIN_BATCH takes the exact verify with the flags masked: the keyed loop runs, and the
    statuses and group verdicts equal the generic route's"""
    import torch
    from bn254_amd.engine import OPT_KEY_DEDUP
    assert n < ws_default("RAND_MIN_BATCH_DEFAULT")
    msgs, sigs, pks = make_batch(eng, n, 256)
    d_msgs = torch.frombuffer(bytearray(b"".join(msgs)), dtype=torch.uint8).to("cuda:0")
    d_off = torch.tensor([32 * i for i in range(n + 1)], dtype=torch.int64, device="cuda:0")
    d_sigs = torch.frombuffer(bytearray(sigs), dtype=torch.uint8).to("cuda:0")
    d_pks = torch.frombuffer(bytearray(pks), dtype=torch.uint8).to("cuda:0")
    groups = (n + 63) // 64
    out = {}
    for kd in (1, 0):
        eng.set_option(OPT_KEY_DEDUP, kd)
        try:
            d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda:0")
            d_ok = torch.full((groups,), 0xEE, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            eng.batch_verify_randomized_device(d_msgs.data_ptr(), d_off.data_ptr(), d_sigs.data_ptr(), d_pks.data_ptr(), n, bytes(range(32)),
                                               d_st.data_ptr(), d_ok.data_ptr(), flags=0x200)
            eng.synchronize()
            out[kd] = (bytes(d_st.cpu().numpy()), bytes(d_ok.cpu().numpy()), eng.debug_key_dedup_last())
        finally:
            eng.set_option(OPT_KEY_DEDUP, 1)
    assert out[1][2] == dict(ran=1, keys=256, flags=0, keyed_n=n, generic_n=0), out[1][2]
    assert out[0][2]["ran"] == 0
    assert out[1][:2] == out[0][:2]
    st, ok = out[1][:2]
    assert st.count(0) > n // 2 and st.count(9) > 0
    assert set(ok) == {0, 1} and all(ok[g] == (9 not in st[64 * g:64 * g + 64]) for g in range(groups))   # 1 iff no item failed the pairing check


@pytest.fixture(scope="module")
def mg4():
    import bn254_amd
    m = bn254_amd.MultiEngine([0, 0, 0, 0])
    yield m
    m.close()


def test_multi_context_shards_run_their_own_dedup(eng, c, mg4):
    """MultiEngine over [0, 0, 0, 0]: every context runs the dedup on its shard of more than 16 384 items; all four gathered status
    buffers equal the single-context call's and the oracle's, and the same with KEY_DEDUP = 0 on every context"""
    import torch
    from bn254_amd.engine import OPT_KEY_DEDUP
    from tests.test_mgpu import _device_shards
    n = 4 * N_FIRST + 3
    msgs, sigs, pks = make_batch(eng, n, 256)
    want, _ = c.batch_verify(msgs, sigs, pks, flags=0, nthreads=16)
    assert verify_device(eng, msgs, sigs, pks, 0) == want
    dev = torch.device("cuda", 0)
    keep, d_msgs, d_off, d_sigs, d_pks = _device_shards(torch, mg4, msgs, sigs, pks, n, dev)
    L = mg4.gathered_len(n)
    for kd in (1, 0):
        for g in range(4):
            mg4.engine(g).set_option(OPT_KEY_DEDUP, kd)
        try:
            alls = [torch.full((L,), 0xEE, dtype=torch.uint8, device=dev) for _ in range(4)]
            torch.cuda.synchronize()
            mg4.batch_verify_device(d_msgs, d_off, d_sigs, d_pks, n, [a.data_ptr() for a in alls])
            mg4.synchronize()
            torch.cuda.synchronize()
            for g in range(4):
                lo, hi = mg4.shard_range(n, g)
                r = mg4.engine(g).debug_key_dedup_last()
                if kd:
                    assert hi - lo > 16384 and r == dict(ran=1, keys=256, flags=0, keyed_n=hi - lo, generic_n=0), (g, r)
                else:
                    assert r["ran"] == 0, (g, r)
                assert bytes(alls[g][:n].cpu().numpy()) == want, (kd, g)
        finally:
            for g in range(4):
                mg4.engine(g).set_option(OPT_KEY_DEDUP, 1)


@pytest.mark.parametrize("opt", ["SPLIT_MILLER", "PAIR_LANES"])
def test_layouts_without_the_dedup(eng, opt):
    """the split A/B layout (SPLIT_MILLER = 1, n <= BN_SPLIT_MAX_N) and one lane per verify (PAIR_LANES = 0) never run the dedup; their
    statuses equal the default (keyed) call's"""
    n = 65536
    msgs, sigs, pks = make_batch(eng, n, 256)
    default = verify_device(eng, msgs, sigs, pks, 0)
    keyed(n, 256)
    assert verify_device(eng, msgs, sigs, pks, 0, **{opt: 1 if opt == "SPLIT_MILLER" else 0}) == default
    assert verify_device.route["ran"] == 0, verify_device.route


# ---- 5. boundaries of the device-side decision ---------------------------------------------------------------------------------------
def test_max_keys_boundary(eng):
    """D = MAX_KEYS is keyed, D = MAX_KEYS + 1 generic (MIN_MULT = 1: only that threshold in play)"""
    mk = 40
    for d, want_keyed in ((mk, True), (mk + 1, False)):
        msgs, sigs, pks = make_batch(eng, N_FIRST, d)
        ref = verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP_FORCE_GENERIC=1)
        assert verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP_MAX_KEYS=mk, KEY_DEDUP_MIN_MULT=1) == ref, d
        r = verify_device.route
        assert r["keys"] == d and r["flags"] == 0, r
        keyed(N_FIRST, d) if want_keyed else generic(N_FIRST)


def test_min_mult_boundary(eng):
    """n = D * MIN_MULT is keyed, n - 1 generic (D = 1 100 under MAX_KEYS = 2 048; both n on the lane-pair row)"""
    d = 1100
    for n, want_keyed in ((d * MIN_MULT, True), (d * MIN_MULT - 1, False)):
        assert n > 16384
        msgs, sigs, pks = make_batch(eng, n, d)
        ref = verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP=0)
        assert verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP_MAX_KEYS=2048) == ref, n
        assert verify_device.route["keys"] == d and verify_device.route["flags"] == 0, verify_device.route
        keyed(n, d) if want_keyed else generic(n)


def test_probe_bound_with_two_buckets(eng):
    """KEY_DEDUP_HASH_BITS = 1: every key hashes to slot 0 or 1 and linear probing walks one cluster.  KD_MAX_PROBES keys always fit (a key
    sits at most KD_MAX_PROBES - 1 slots past its home); KD_MAX_PROBES + 2 never do (only slots 0 .. KD_MAX_PROBES are reachable)"""
    for d, want_keyed in ((KD_MAX_PROBES, True), (KD_MAX_PROBES + 2, False)):
        msgs, sigs, pks = make_batch(eng, N_FIRST, d)
        ref = verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP=0)
        assert verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP_HASH_BITS=1) == ref, d
        if want_keyed:
            keyed(N_FIRST, d)
        else:
            assert verify_device.route["flags"] & 1, verify_device.route
            generic(N_FIRST)


@pytest.mark.parametrize("d", [3, 96, 1023])
def test_full_last_builder_wave(eng, derived, d):
    """pools of D = 0 (mod 3) keys: k_kd_lines' last wave holds three live keys; an invalid key in that wave and in the first"""
    from tests.test_gpu_key_dedup import Q
    msgs, sigs, pks = make_batch(eng, N_FIRST, d)
    if d > 3:
        keys = [bytearray(pks[128 * j:128 * j + 128]) for j in range(d)]
        keys[d - 1] = bytearray(bytes.fromhex(derived["g2_not_in_subgroup"]))
        keys[d - 2][32:64] = Q.to_bytes(32, "big")
        keys[1] = bytearray(128)
        pks = b"".join(bytes(keys[i % d]) for i in range(N_FIRST))
    for flags in (0, 1):
        ref = verify_device(eng, msgs, sigs, pks, flags, KEY_DEDUP_FORCE_GENERIC=1)
        assert verify_device(eng, msgs, sigs, pks, flags) == ref, (d, flags)
        keyed(N_FIRST, d)
    assert ref.count(0) > N_FIRST // 2


def test_max_keys_at_its_limit(eng, c):
    """KEY_DEDUP_MAX_KEYS = KEY_DEDUP_MAX_KEYS_LIMIT, 16 384 distinct valid keys, n = 262 144: the largest builder and scaling grids the
    option allows run the keyed loop; statuses equal the generic route's, and the oracle's on the first 16 385 items"""
    d, n = MAX_KEYS_LIMIT, MAX_KEYS_LIMIT * MIN_MULT
    msgs, sigs, pks = make_batch(eng, n, d)
    got = verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP_MAX_KEYS=d)
    keyed(n, d)
    assert got == verify_device(eng, msgs, sigs, pks, 0, KEY_DEDUP_FORCE_GENERIC=1)
    m = N_FIRST
    want, _ = c.batch_verify(msgs[:m], sigs[:64 * m], pks[:128 * m], flags=0, nthreads=16)
    assert got[:m] == want
    assert got.count(0) > n // 2
