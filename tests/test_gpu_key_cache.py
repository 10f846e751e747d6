"""The key cache of the exact verify's key dedup (BN254_OPT_KEY_CACHE, bn254_keydedup.hip: k_kd_match): the line tables stay in the context
between calls, found again by the key's 128 bytes, and a call builds only the keys it has not seen.  Every case runs at the first lane-pair
sizes (16 385 .. 20 000 items), compares the status bytes with a context that runs the generic loop (KEY_DEDUP = 0) and — where the keys or
flags matter — with the oracle, and asserts from bn254_debug_key_cache_last what the call found and built.  Tables read back through
bn254_debug_key_tables must equal registration's word for word whether the call built them or found them."""
import random

import pytest

from tests.datagen import D
from tests.soak_gpu import twist_small_order_key
from tests.test_gpu_kd_scale_tree import host_degenerate  # noqa: F401  (fixture: the host's prediction of a degenerate line)
from tests.test_gpu_key_dedup import Q, key_pool

pytestmark = pytest.mark.gpu

N = 16385                      # the first lane-pair size
POOL = 512                     # the keys every batch of this file draws from, by index
PER_KEY = 87 * 36


@pytest.fixture(scope="module")
def gen():
    """makes keys and signatures, and gives the reference statuses: the generic loop, no dedup at all"""
    import bn254_amd
    from bn254_amd import engine as E
    e = bn254_amd.Engine(0)
    e.set_option(E.OPT_KEY_DEDUP, 0)
    yield e
    e.close()


@pytest.fixture()
def eng():
    """a context of its own per test: the cache starts empty"""
    import bn254_amd
    e = bn254_amd.Engine(0)
    yield e
    e.close()


def opt(e, name, value):
    from bn254_amd import engine as E
    e.set_option(getattr(E, "OPT_" + name), value)


_BASE = {}


def batch_over(gen, n, ids, odd=None):
    """n items, item i under key ids[i % len(ids)] of the pool; every 61st signature is its neighbour's (status 9), every 97th malformed
    (status 6).  odd: {position in ids: 128 key bytes} replaces the key bytes at those positions (the signatures stay the valid key's)."""
    sks, pk = key_pool(gen, POOL)
    if n not in _BASE:
        _BASE[n] = [D("kcache", i) for i in range(n)]
    msgs = _BASE[n]
    sigs, st = gen.batch_sign(msgs, b"".join(sks[ids[i % len(ids)]] for i in range(n)))
    assert st == bytes(n)
    sigs = bytearray(sigs)
    good = bytes(sigs)
    for i in range(60, n, 61):
        sigs[64 * i:64 * i + 64] = good[64 * (i - 1):64 * i]
    for i in range(96, n, 97):
        sigs[64 * i:64 * i + 32] = Q.to_bytes(32, "big")
    keys = [pk[128 * j:128 * j + 128] for j in ids]
    for pos, raw in (odd or {}).items():
        keys[pos] = bytes(raw)
    return msgs, bytes(sigs), b"".join(keys[i % len(ids)] for i in range(n))


class Dev:
    """a batch resident on the device; the key buffer can be overwritten in place"""

    def __init__(self, batch):
        import torch
        msgs, sigs, pks = batch
        self.batch, self.n = batch, len(msgs)
        offs = [0]
        for m in msgs:
            offs.append(offs[-1] + len(m))
        up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to("cuda:0")
        self.msgs, self.sigs, self.pks = up(b"".join(msgs)), up(sigs), up(pks)
        self.off = torch.tensor(offs, dtype=torch.int64, device="cuda:0")
        self.st = torch.full((self.n,), 0xEE, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()

    def set_keys(self, pks):
        import torch
        assert len(pks) == 128 * self.n
        self.pks.copy_(torch.frombuffer(bytearray(pks), dtype=torch.uint8))          # same address, same n
        self.batch = (self.batch[0], self.batch[1], pks)
        torch.cuda.synchronize()

    def enqueue(self, e, flags=0, stream=None):
        self.st.fill_(0xEE)
        import torch
        torch.cuda.synchronize()
        e.batch_verify_device(self.msgs.data_ptr(), self.off.data_ptr(), self.sigs.data_ptr(), self.pks.data_ptr(), self.n, self.st.data_ptr(),
                              flags=flags, stream=None if stream is None else stream.cuda_stream)

    def status(self):
        import torch
        torch.cuda.synchronize()
        return bytes(self.st.cpu().numpy())

    def run(self, e, flags=0):
        """-> (status bytes, cache report, route report)"""
        self.enqueue(e, flags)
        e.synchronize()
        return self.status(), e.debug_key_cache_last(), e.debug_key_dedup_last()


_REF = {}


def reference(gen, batch, flags=0):
    """the generic loop's statuses of the batch (computed once per batch and flags)"""
    key = (id(batch[0]), batch[1], batch[2], flags)
    if key not in _REF:
        st, _, route = Dev(batch).run(gen, flags)
        assert route["ran"] == 0
        _REF[key] = st
    return _REF[key]


def cache(report, keys, hits, built, capacity_drop=False):
    assert (report["ran"], report["keys"], report["hits"], report["built"], report["dropped"] & 1) == (1, keys, hits, built, int(capacity_drop)), report


def keyed(route, n, keys):
    assert route == dict(ran=1, keys=keys, flags=0, keyed_n=n, generic_n=0), route


def tables_equal_registration(e, gen, batch, keys):
    """the tables of the last call's keys, read back by key id, against bn254_ctx_register_keys on the same bytes: word for word for every
    key both sides accept; returns how many were compared"""
    pks = batch[2]
    words, rep, st_kd, inf_kd = e.debug_key_tables(0, 0, keys)
    assert len({pks[128 * r:128 * r + 128] for r in rep}) == keys                  # one representative per distinct key
    st_reg = gen.register_keys(b"".join(pks[128 * r:128 * r + 128] for r in rep), flags=0)
    words_reg, _, _, inf_reg = gen.debug_key_tables(1, 0, keys)
    same = 0
    for k in range(keys):
        if st_kd[k] == 0 and st_reg[k] == 0 and not inf_kd[k] and not inf_reg[k]:
            assert words[k * PER_KEY:(k + 1) * PER_KEY] == words_reg[k * PER_KEY:(k + 1) * PER_KEY], (k, rep[k])
            same += 1
    return same


def odd_keys(gen, derived, ids):
    """refused, identity, off-curve and off-subgroup keys at positions 1 .. 4 (pools of five keys and more), as tests/test_gpu_kd_builder.py
    builds them"""
    if len(ids) < 5:
        return {}
    _, pk = key_pool(gen, POOL)
    big = bytearray(pk[128 * ids[2]:128 * ids[2] + 128])
    big[0:32] = Q.to_bytes(32, "big")
    curve = bytearray(pk[128 * ids[3]:128 * ids[3] + 128])
    curve[127] ^= 1
    return {1: bytes.fromhex(derived["g2_not_in_subgroup"]), 2: bytes(big), 3: bytes(curve), 4: bytes(128)}


@pytest.mark.parametrize("pool", [1, 5, 256])
def test_repeat(eng, gen, derived, pool):
    """the same call twice: the second finds every key and builds none; statuses equal on both calls, the generic loop's and the oracle's;
    the tables are registration's after both"""
    from oracle import c_oracle
    ids = list(range(pool))
    batch = batch_over(gen, N, ids, odd_keys(gen, derived, ids))
    want, _ = c_oracle.batch_verify(*batch, flags=0, nthreads=16)
    assert reference(gen, batch) == want
    dev = Dev(batch)
    for call in (0, 1):
        st, rep, route = dev.run(eng)
        cache(rep, pool, pool if call else 0, 0 if call else pool)
        keyed(route, N, pool)
        assert st == want, (pool, call)
        assert tables_equal_registration(eng, gen, batch, pool) >= max(pool - 4, 1)
    assert want.count(0) > 0 and want.count(9) > 0 and want.count(6) > 0


def test_partial_overlap(eng, gen):
    """the second call keeps half of the first call's keys and adds as many new ones: only those are built, old and new rows are right"""
    a, b = batch_over(gen, N, list(range(16))), batch_over(gen, N, list(range(8, 24)))
    st, rep, route = Dev(a).run(eng)
    cache(rep, 16, 0, 16)
    assert st == reference(gen, a)
    st, rep, route = Dev(b).run(eng)
    cache(rep, 16, 8, 8)
    keyed(route, N, 16)
    assert st == reference(gen, b)
    assert tables_equal_registration(eng, gen, b, 16) == 16
    st, rep, route = Dev(a).run(eng)                                             # the first call's keys are all still there
    cache(rep, 16, 16, 0)
    assert st == reference(gen, a)
    assert tables_equal_registration(eng, gen, a, 16) == 16


def test_other_order(eng, gen):
    """the same keys in another order of first appearance: the call's key ids differ from the cache's rows"""
    ids = list(range(40))
    a, b = batch_over(gen, N, ids), batch_over(gen, N, ids[::-1])
    st, rep, _ = Dev(a).run(eng)
    cache(rep, 40, 0, 40)
    assert st == reference(gen, a)
    st, rep, route = Dev(b).run(eng)
    cache(rep, 40, 40, 0)
    keyed(route, N, 40)
    assert st == reference(gen, b)
    assert tables_equal_registration(eng, gen, b, 40) == 40
    assert st.count(0) > N // 2


def test_bytes_not_pointers(eng, gen):
    """the caller overwrites its key buffer in place with other keys between two calls (same addresses, same n): statuses follow the new
    keys — the signatures are still the old keys', so every pairing check of a changed item now fails"""
    ids = list(range(16))
    a = batch_over(gen, N, ids)
    other = batch_over(gen, N, [j + 100 for j in ids])
    dev = Dev(a)
    st, rep, _ = dev.run(eng)
    cache(rep, 16, 0, 16)
    assert st == reference(gen, a) and st.count(0) > N // 2
    dev.set_keys(other[2])
    mixed = (a[0], a[1], other[2])
    st, rep, route = dev.run(eng)
    cache(rep, 16, 0, 16)
    keyed(route, N, 16)
    assert st == reference(gen, mixed)
    assert st.count(0) == 0 and st.count(9) > N // 2
    dev.set_keys(a[2])                                                            # and back: both sets are cached by now
    st, rep, _ = dev.run(eng)
    cache(rep, 16, 16, 0)
    assert st == reference(gen, a)


@pytest.mark.parametrize("order", [(0, 1), (1, 0), (0, 2), (2, 0), (3, 0)])
def test_flags(gen, derived, order):
    """the same key bytes under other decode flags (1 = subgroup check, 2 = reject the identity): a row built under one set of flags is not
    read under another; statuses are those of a context that never saw the other call (the generic loop's and the oracle's)"""
    import bn254_amd
    from oracle import c_oracle
    ids = list(range(8))
    batch = batch_over(gen, N, ids, odd_keys(gen, derived, ids))
    dev = Dev(batch)
    e = bn254_amd.Engine(0)
    try:
        for call, flags in enumerate(order + order[:1]):
            want, _ = c_oracle.batch_verify(*batch, flags=flags, nthreads=16)
            assert reference(gen, batch, flags) == want
            st, rep, route = dev.run(e, flags)
            cache(rep, 8, 0, 8)                                                   # every change of flags starts from an empty cache
            assert rep["dropped"] & 2
            keyed(route, N, 8)
            assert st == want, (order, call, flags)
        st, rep, _ = dev.run(e, order[0])
        cache(rep, 8, 8, 0)
        assert st == want
    finally:
        e.close()
    by_flags = {f: reference(gen, batch, f) for f in (0, 1, 2, 3)}
    assert len(set(by_flags.values())) == 4                                       # the flags do change these statuses


def test_generic_route_calls_leave_the_cache(eng, gen):
    """between two cached calls, calls the thresholds refuse — too many keys (D > MAX_KEYS), too few items per key (D x MIN_MULT > n): they
    look nothing up, and the call after them still finds its keys"""
    opt(eng, "KEY_DEDUP_MAX_KEYS", 400)
    a = batch_over(gen, N, list(range(16)))
    many = batch_over(gen, N, list(range(401)))                                  # 401 keys: 401 x 16 <= n, but more than MAX_KEYS
    st, rep, _ = Dev(a).run(eng)
    cache(rep, 16, 0, 16)
    st, rep, route = Dev(many).run(eng)
    cache(rep, 401, 0, 0)
    assert (route["keyed_n"], route["generic_n"]) == (0, N), route
    assert st == reference(gen, many)
    from bn254_amd.engine import NativeError
    with pytest.raises(NativeError) as refused:                                  # such a call has no tables to read back
        eng.debug_key_tables(0, 0, 4)
    assert refused.value.rc == -10001
    st, rep, route = Dev(a).run(eng)
    cache(rep, 16, 16, 0)
    keyed(route, N, 16)
    assert st == reference(gen, a)
    opt(eng, "KEY_DEDUP_MIN_MULT", 64)                                            # not part of a row's identity: the cache stays
    thin = batch_over(gen, N, list(range(300)))                                  # 300 <= MAX_KEYS, 300 x 64 > n
    st, rep, route = Dev(thin).run(eng)
    cache(rep, 300, 0, 0)
    assert (route["keyed_n"], route["generic_n"]) == (0, N), route
    assert st == reference(gen, thin)
    st, rep, route = Dev(a).run(eng)
    cache(rep, 16, 16, 0)
    keyed(route, N, 16)
    assert st == reference(gen, a)


def test_small_order_twist_key_beside_the_cache(eng, gen, host_degenerate):
    """a batch with a key of the twist's order-10 069 subgroup beside cached and new keys.  Whether the builder meets a line with c2 = 0 for it
    is predicted WITHOUT the device, by the host build of g2_line_table (host_degenerate, the fixture of tests/test_gpu_kd_scale_tree.py).
    As things stand the prediction is "no": no key bytes that reach a degenerate line of this loop are known — no prefix of 6u + 2 is 0 or
    +-1 mod 10 069 —, so this key is an ordinary key outside G2, takes the keyed route and is cached like any other.  Were the prediction
    "yes", the call would have to take the generic loop and cache nothing from itself; that decision is pinned, with the builder's report
    forced, by test_degenerate_line_is_never_cached.  Statuses are the generic loop's either way."""
    bad = twist_small_order_key(random.Random(5))
    degenerate = host_degenerate(bad)
    a = batch_over(gen, N, list(range(8)))
    ids_b = list(range(4, 8)) + list(range(30, 35))                              # four cached keys, four new ones, and the odd key's slot
    b = batch_over(gen, N, ids_b, {8: bad})
    c = batch_over(gen, N, ids_b[:8])
    st, rep, _ = Dev(a).run(eng)
    cache(rep, 8, 0, 8)
    st, rep, route = Dev(b).run(eng)
    cache(rep, 9, 4, 5)
    assert st == reference(gen, b)
    assert route["flags"] == (2 if degenerate else 0), (route, degenerate)
    assert (route["keyed_n"], route["generic_n"]) == ((0, N) if degenerate else (N, 0)), route
    st, rep, route = Dev(c).run(eng)
    cache(rep, 8, 4, 4) if degenerate else cache(rep, 8, 8, 0)                    # a degenerate call keeps none of its four new good keys
    keyed(route, N, 8)
    assert st == reference(gen, c)
    st, rep, route = Dev(b).run(eng)
    cache(rep, 9, 8, 1) if degenerate else cache(rep, 9, 9, 0)
    assert route["flags"] == (2 if degenerate else 0), route
    assert st == reference(gen, b)
    st, rep, route = Dev(a).run(eng)
    cache(rep, 8, 8, 0)
    assert st == reference(gen, a)
    assert tables_equal_registration(eng, gen, a, 8) == 8


def test_degenerate_line_is_never_cached(eng, gen):
    """KEY_DEDUP_FORCE_GENERIC = 2: the builder reports a degenerate line (KD_DEGENERATE, route flags = 2) for the keys it builds, and the
    device decides as it does for such a key: the call takes the generic loop and caches nothing from itself, neither cached keys' rows
    change nor do the keys built beside the flagged one become findable.  A call that builds nothing is not touched by the report."""
    a, b = batch_over(gen, N, list(range(8))), batch_over(gen, N, list(range(4, 8)) + list(range(30, 34)))
    st, rep, _ = Dev(a).run(eng)
    cache(rep, 8, 0, 8)
    opt(eng, "KEY_DEDUP_FORCE_GENERIC", 2)
    st, rep, route = Dev(b).run(eng)
    cache(rep, 8, 4, 4)
    assert route == dict(ran=1, keys=8, flags=2, keyed_n=0, generic_n=N), route
    assert st == reference(gen, b)
    st, rep, route = Dev(a).run(eng)                                             # all cached: nothing built, nothing reported
    cache(rep, 8, 8, 0)
    keyed(route, N, 8)
    assert st == reference(gen, a)
    opt(eng, "KEY_DEDUP_FORCE_GENERIC", 0)
    st, rep, route = Dev(b).run(eng)                                             # the degenerate call kept none of its four new keys
    cache(rep, 8, 4, 4)
    keyed(route, N, 8)
    assert st == reference(gen, b)
    assert tables_equal_registration(eng, gen, b, 8) == 8
    st, rep, route = Dev(b).run(eng)
    cache(rep, 8, 8, 0)
    st, rep, route = Dev(a).run(eng)
    cache(rep, 8, 8, 0)
    assert st == reference(gen, a)
    assert tables_equal_registration(eng, gen, a, 8) == 8


def test_forced_generic_call_commits_nothing(eng, gen):
    """KEY_DEDUP_FORCE_GENERIC: the call looks its keys up and builds the missing ones, but takes the generic loop — the path of a call with
    a degenerate line, decided by the host's switch instead of the builder's report — and commits nothing: the next call builds the same keys again, into the same free rows"""
    a, b = batch_over(gen, N, list(range(8))), batch_over(gen, N, list(range(4, 12)))
    st, rep, _ = Dev(a).run(eng)
    cache(rep, 8, 0, 8)
    opt(eng, "KEY_DEDUP_FORCE_GENERIC", 1)
    st, rep, route = Dev(b).run(eng)
    cache(rep, 8, 4, 4)
    assert (route["keyed_n"], route["generic_n"]) == (0, N), route
    assert st == reference(gen, b)
    opt(eng, "KEY_DEDUP_FORCE_GENERIC", 0)
    st, rep, route = Dev(b).run(eng)
    cache(rep, 8, 4, 4)
    keyed(route, N, 8)
    assert st == reference(gen, b)
    assert tables_equal_registration(eng, gen, b, 8) == 8
    st, rep, route = Dev(b).run(eng)
    cache(rep, 8, 8, 0)
    st, rep, route = Dev(a).run(eng)
    cache(rep, 8, 8, 0)
    assert st == reference(gen, a)
    assert tables_equal_registration(eng, gen, a, 8) == 8


def test_capacity_drops_the_cache(eng, gen):
    """KEY_DEDUP_MAX_KEYS = 8 rows, more distinct keys over three calls than fit: the call whose new keys do not fit drops the cache and
    builds all its keys; statuses right throughout"""
    opt(eng, "KEY_DEDUP_MAX_KEYS", 8)
    calls = [(list(range(0, 5)), 0, 5, False),        # five rows in use
             (list(range(3, 9)), 0, 6, True),         # two hits, four misses: 5 + 4 > 8 -> dropped, all six built
             (list(range(7, 9)), 2, 0, False),        # both found among the six
             (list(range(0, 5)), 0, 5, True),         # 6 + 5 > 8
             (list(range(0, 5)), 5, 0, False)]
    for ids, hits, built, drop in calls:
        batch = batch_over(gen, N, ids)
        st, rep, route = Dev(batch).run(eng)
        cache(rep, len(ids), hits, built, drop)
        keyed(route, N, len(ids))
        assert st == reference(gen, batch), ids
        assert tables_equal_registration(eng, gen, batch, len(ids)) == len(ids)


def test_growth_of_the_buffers(eng, gen):
    """n = 16 385, then a size that makes the dedup buffers grow (and move), then 16 385 again: the grown call starts from an empty cache"""
    ids = list(range(16))
    small, large = batch_over(gen, N, ids), batch_over(gen, 19997, ids)
    st, rep, _ = Dev(small).run(eng)
    cache(rep, 16, 0, 16)
    assert st == reference(gen, small)
    st, rep, route = Dev(large).run(eng)
    cache(rep, 16, 0, 16)
    assert rep["dropped"] & 2
    keyed(route, 19997, 16)
    assert st == reference(gen, large)
    st, rep, route = Dev(small).run(eng)
    cache(rep, 16, 16, 0)
    keyed(route, N, 16)
    assert st == reference(gen, small)
    assert tables_equal_registration(eng, gen, small, 16) == 16


def test_two_caller_streams(eng, gen):
    """call A on one caller stream, call B on another, no host synchronisation in between; B's keys are all A's: B waits on the device for
    A's tables and finds them"""
    import torch
    a, b = batch_over(gen, N, list(range(24))), batch_over(gen, N, list(range(23, 7, -1)))
    da, db = Dev(a), Dev(b)
    s1, s2 = torch.cuda.Stream(device="cuda:0"), torch.cuda.Stream(device="cuda:0")
    torch.cuda.synchronize()
    eng.batch_verify_device(da.msgs.data_ptr(), da.off.data_ptr(), da.sigs.data_ptr(), da.pks.data_ptr(), N, da.st.data_ptr(), flags=0,
                            stream=s1.cuda_stream)
    eng.batch_verify_device(db.msgs.data_ptr(), db.off.data_ptr(), db.sigs.data_ptr(), db.pks.data_ptr(), N, db.st.data_ptr(), flags=0,
                            stream=s2.cuda_stream)
    s2.synchronize()
    s1.synchronize()
    eng.synchronize()
    rep, route = eng.debug_key_cache_last(), eng.debug_key_dedup_last()
    cache(rep, 16, 16, 0)
    keyed(route, N, 16)
    assert db.status() == reference(gen, b)
    assert da.status() == reference(gen, a)
    assert tables_equal_registration(eng, gen, b, 16) == 16


def test_option_off_and_on_again(eng, gen):
    """KEY_CACHE = 0: every call builds all its keys (the parent's behaviour); back at 1 the first call builds all, the next one none"""
    batch = batch_over(gen, N, list(range(16)))
    want = reference(gen, batch)
    dev = Dev(batch)
    st, rep, _ = dev.run(eng)
    cache(rep, 16, 0, 16)
    opt(eng, "KEY_CACHE", 0)
    for _ in range(2):
        st, rep, route = dev.run(eng)
        cache(rep, 16, 0, 16)
        keyed(route, N, 16)
        assert st == want
    assert tables_equal_registration(eng, gen, batch, 16) == 16
    opt(eng, "KEY_CACHE", 1)
    for call in (0, 1):
        st, rep, route = dev.run(eng)
        cache(rep, 16, 16 if call else 0, 0 if call else 16)
        keyed(route, N, 16)
        assert st == want
    assert want.count(0) > N // 2


def test_slices_hit(eng, gen):
    """two slices forced with BN254_OPT_MAX_CHUNK: the second slice finds the keys the first one built"""
    n = 2 * N
    batch = batch_over(gen, n, list(range(16)))
    opt(eng, "MAX_CHUNK", N)
    st, rep, route = Dev(batch).run(eng)
    cache(rep, 16, 16, 0)
    keyed(route, N, 16)
    assert st == reference(gen, batch)
    assert st.count(0) > n // 2
