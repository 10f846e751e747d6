"""bn254_batch_collect_keyed_bitmap_randomized[_device] on the GPU (include/bn254_hip.h): every output byte for byte that of
the exact collect on the same context, and of tests/collect_model.py plus the oracle's g1_add; the groups of 64 shares per key as the debug
hook counts them; a pair of errors that cancels in the plain sum; the weights' index rule under slicing (a forged pair that cancels exactly
when the weights are those of the caller's indices); the routes to the exact call; the _device form's range rule.  The route is forced with
options 38 = 0 and 39 = 0 and restored afterwards.  Key set, case set and helpers: tests/test_gpu_collect_keyed_bitmap.py.
Run on the MI355X box: -m gpu."""
import hashlib

import pytest

from bn254_amd import engine as E
from tests.aggr_model import r_model
from tests.test_gpu_collect_keyed_bitmap import (BM, K_IDENT, N_GOOD, N_KEYS, SIZES, build, c, collect, eng, expected, flat,   # noqa: F401
                                                 keyed, keyset, reg_set, sign)

pytestmark = pytest.mark.gpu

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SEEDS = [hashlib.sha256(b"collect-rand/seed/%d" % j).digest() for j in range(3)]
FORCE = {E.OPT_COLLECT_RAND_MIN_SHARES: 0, E.OPT_COLLECT_RAND_MIN_PER_KEY: 0}
DEFAULTS = {E.OPT_COLLECT_RAND_MIN_SHARES: E.COLLECT_RAND_MIN_SHARES_DEFAULT, E.OPT_COLLECT_RAND_MIN_PER_KEY: E.COLLECT_RAND_MIN_PER_KEY_DEFAULT,
            E.OPT_MAX_CHUNK: 0, E.OPT_HASH_MAX_TRIES: 0}


def with_options(eng, opts, fn):
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            eng.set_option(k, DEFAULTS[k])


def rand_collect(eng, tuples, seed, flags=0, bm_words=BM, opts=FORCE):
    """-> (the five outputs, the hook's counters)"""
    msgs, shares, keys, sizes = flat(tuples)

    def call():
        out = eng.batch_collect_keyed_bitmap_randomized(msgs, b"".join(shares), keys, sizes, bm_words, seed, flags=flags, want_counts=True)
        return out, eng.debug_collect_rand_last()
    return with_options(eng, opts, call)


def n_shares_of(tuples):
    return sum(len(t[1]) for t in tuples)


@pytest.fixture(scope="module")
def cases(eng, c, keyset):
    return build(eng, c, keyset, "rand-cases")


def test_parity_on_the_mixed_case_set(eng, c, keyset, cases):
    """tuples of 0 .. 130 shares plus the special tuples: all five outputs equal the exact call's and the model's, with 128-bit, 64-bit and
    GLV weights under two seeds; identity 1 and the closed loop (identity 2) hold"""
    reg_set(eng, keyset)
    assert [len(t[1]) for t in cases[:len(SIZES)]] == SIZES
    exact = collect(eng, cases)
    assert eng.debug_collect_rand_last() == dict(slices=0, groups=0, failed_groups=0, rechecked=0)
    share_st, tuple_st, agg, bits, counts = exact
    assert share_st == keyed(eng, cases) and {0, 2, 4, 6, 9} <= set(share_st) and tuple_st == bytes(len(cases))
    assert (bits, counts, agg) == expected(c, cases, share_st, tuple_st)
    at_check = sum(1 for s in share_st if s in (0, 9))
    for flags in (0, E.FLAG_RAND64, E.FLAG_RAND_GLV):
        for seed in SEEDS[:2]:
            got, hook = rand_collect(eng, cases, seed, flags)
            assert got[0] == exact[0], (flags, [(i, a, b) for i, (a, b) in enumerate(zip(got[0], exact[0])) if a != b][:8])
            assert got == exact, flags
            # every key's run is padded to whole groups; the wrong shares make groups fail, and every share of a failed group is re-checked
            assert hook["slices"] == 1 and at_check / 64 <= hook["groups"] <= at_check // 64 + N_KEYS, hook
            assert 1 <= hook["failed_groups"] <= share_st.count(9) and share_st.count(9) <= hook["rechecked"] <= 64 * hook["failed_groups"], hook
    # flags = REJECT_IDENTITY reach the shares' decode on this route as on the exact one
    got, _ = rand_collect(eng, cases, SEEDS[0], 2 | E.FLAG_RAND64)
    assert got == collect(eng, cases, 2) and got[0] != exact[0]
    assert eng.batch_verify_keyed_bitmap([t[0] for t in cases], agg, bits, BM) == bytes(len(cases))
    # the exact call, and the keyed randomised call the route shares its kernels with, behind a randomised collect: no stale state
    assert collect(eng, cases) == exact


@pytest.mark.parametrize("cnt", [63, 64, 65, 129])
def test_group_boundaries(eng, c, keyset, cnt):
    """one key with exactly cnt participating shares, duplicates of a valid share across three tuples: ceil(cnt / 64) groups, none failed,
    none re-checked.  129 with one wrong share: the groups hold 64, 64 and 1 shares in the order the scatter's atomics land, so the share
    (from the middle of the call) sits in a full group — one failed group, its 64 shares re-checked, only that share reads 9"""
    sks, _ = keyset
    reg_set(eng, keyset)
    key = 7
    msgs = [b"collect-rand/boundary/%d/%d" % (cnt, i) for i in range(3)]
    sigs = sign(eng, [(m, sks[key]) for m in msgs])
    sizes = [cnt // 3, cnt // 3, cnt - 2 * (cnt // 3)]
    tuples = [(m, [(sg, key)] * k) for m, sg, k in zip(msgs, sigs, sizes)]
    exact = collect(eng, tuples)
    assert exact[0] == bytes(cnt) and exact[4] == [1, 1, 1] and exact[2] == b"".join(sigs)
    got, hook = rand_collect(eng, tuples, SEEDS[0])
    assert got == exact
    assert hook == dict(slices=1, groups=(cnt + 63) // 64, failed_groups=0, rechecked=0)
    if cnt == 129:
        s_bad = 100
        assert sizes[0] + sizes[1] <= s_bad                               # it lies in the last tuple
        t, k = 2, s_bad - sizes[0] - sizes[1]
        tuples[t][1][k] = (c.g1_add(sigs[t], c.g1_generator()), key)
        exact = collect(eng, tuples)
        assert list(exact[0]) == [9 if s == s_bad else 0 for s in range(cnt)]
        got, hook = rand_collect(eng, tuples, SEEDS[1])
        assert got == exact
        assert hook == dict(slices=1, groups=3, failed_groups=1, rechecked=64)


def test_cancelling_pair(eng, c, keyset):
    """sigma_1 + G1 and sigma_2 - G1 by one key in two tuples: the plain sum of the two is right, the weighted one is not — both read 9,
    neither bit is set, the outputs are the exact call's"""
    sks, _ = keyset
    reg_set(eng, keyset)
    g1 = c.g1_generator()
    neg_g1 = c.g1_mul(g1, (R - 1).to_bytes(32, "big"))
    tuples = build(eng, c, keyset, "rand-cancel", sizes=[6, 7, 5], extras=False)
    msgs = [t[0] for t in tuples]
    key = 33
    s1, s2 = sign(eng, [(msgs[0], sks[key]), (msgs[2], sks[key])])
    assert c.g1_add(c.g1_add(s1, g1), c.g1_add(s2, neg_g1)) == c.g1_add(s1, s2)
    tuples[0][1].append((c.g1_add(s1, g1), key))
    tuples[2][1].insert(0, (c.g1_add(s2, neg_g1), key))
    at1, at2 = len(tuples[0][1]) - 1, len(tuples[0][1]) + len(tuples[1][1])
    exact = collect(eng, tuples)
    assert exact[0][at1] == 9 and exact[0][at2] == 9
    for flags in (0, E.FLAG_RAND64, E.FLAG_RAND_GLV):
        got, hook = rand_collect(eng, tuples, SEEDS[0], flags)
        assert got == exact, flags
        assert got[0][at1] == 9 and got[0][at2] == 9 and hook["failed_groups"] >= 1
        assert not (got[3][0 * BM + key // 32] >> (key % 32)) & 1 and not (got[3][2 * BM + key // 32] >> (key % 32)) & 1


def test_index_rule_under_slicing(eng, c, keyset, cases):
    """BN254_OPT_MAX_CHUNK = 37: the mixed case set in a dozen slices gives the unsliced and the exact bytes.  Then the known-seed probe, on
    six all-valid tuples of 20 shares in four slices: two shares of key 0 inside the second slice are replaced by sigma_1 + r(s_2) D and
    sigma_2 - r(s_1) D, D = G1.  The forged pair cancels in the group's sum exactly when the weights are those of the caller's indices —
    both read 0 and no group fails; under another seed both read 9.  (Which is also why the seed must be secret.)"""
    sks, _ = keyset
    reg_set(eng, keyset)
    chunk = 37
    sliced = dict(FORCE)
    sliced[E.OPT_MAX_CHUNK] = chunk
    exact = collect(eng, cases)
    whole, hook1 = rand_collect(eng, cases, SEEDS[0])
    got, hook = rand_collect(eng, cases, SEEDS[0], opts=sliced)
    n_sh = n_shares_of(cases)
    assert hook1["slices"] == 1 and hook["slices"] == (n_sh + chunk - 1) // chunk >= 3
    assert got == whole == exact
    # the probe
    msgs = [b"collect-rand/probe/%d" % i for i in range(6)]
    plan = [(i, t) for i in range(6) for t in range(20)]                   # share t of every tuple is by key t
    sigs = sign(eng, [(msgs[i], sks[t]) for i, t in plan])
    s1, s2 = 40, 60                                                        # tuples 2 and 3, key 0, both inside the slice [37, 74)
    assert plan[s1][1] == plan[s2][1] == 0 and chunk <= s1 < s2 < 2 * chunk
    seed = SEEDS[2]
    r1, r2 = r_model(seed, s1, 0), r_model(seed, s2, 0)
    mult, st = eng.batch_g1_mul(None, r2.to_bytes(32, "big") + (R - r1).to_bytes(32, "big"), 2)
    assert st == bytes(2)
    forged = list(sigs)
    forged[s1] = c.g1_add(sigs[s1], mult[:64])
    forged[s2] = c.g1_add(sigs[s2], mult[64:])
    tuples = [(msgs[i], [(forged[20 * i + t], t) for t in range(20)]) for i in range(6)]
    exact = collect(eng, tuples)
    assert list(exact[0]) == [9 if s in (s1, s2) else 0 for s in range(120)]
    got, hook = rand_collect(eng, tuples, seed, opts=sliced)
    assert hook["slices"] == 4 and hook["failed_groups"] == 0 and hook["rechecked"] == 0, hook
    assert got[0] == bytes(120) and got[1] == bytes(6)
    got, hook = rand_collect(eng, tuples, SEEDS[0], opts=sliced)
    assert got == exact and hook["failed_groups"] == 1 and hook["slices"] == 4, hook


def test_routes_to_the_exact_call(eng, c, keyset, cases):
    """no keys registered; option 38 above n_shares; option 39 above n_shares // n_keys: 0 randomised slices, the exact call's outputs.
    One below either bound the route is taken."""
    n_sh = n_shares_of(cases)
    try:
        eng.register_keys(b"")
        exact = collect(eng, cases, bm_words=0)
        got, hook = rand_collect(eng, cases, SEEDS[0], bm_words=0)
        assert got == exact and 0 not in got[0] and 2 in got[0] and hook == dict(slices=0, groups=0, failed_groups=0, rechecked=0)
    finally:
        reg_set(eng, keyset)
    exact = collect(eng, cases)
    for opts, want_slices in (({E.OPT_COLLECT_RAND_MIN_SHARES: n_sh + 1, E.OPT_COLLECT_RAND_MIN_PER_KEY: 0}, 0),
                              ({E.OPT_COLLECT_RAND_MIN_SHARES: n_sh, E.OPT_COLLECT_RAND_MIN_PER_KEY: 0}, 1),
                              ({E.OPT_COLLECT_RAND_MIN_SHARES: 0, E.OPT_COLLECT_RAND_MIN_PER_KEY: n_sh // N_KEYS + 1}, 0),
                              ({E.OPT_COLLECT_RAND_MIN_SHARES: 0, E.OPT_COLLECT_RAND_MIN_PER_KEY: n_sh // N_KEYS}, 1)):
        got, hook = rand_collect(eng, cases, SEEDS[1], opts=opts)
        assert got == exact, opts
        assert hook["slices"] == want_slices and (hook["groups"] > 0) == bool(want_slices), (opts, hook)
    # the defaults: a call of a few hundred shares is below both of them
    assert n_sh < E.COLLECT_RAND_MIN_SHARES_DEFAULT
    got, hook = rand_collect(eng, cases, SEEDS[1], opts={})
    assert got == exact and hook["slices"] == 0


def test_device_form(eng, c, keyset, cases):
    """the _device form on a caller's stream against the exact _device call: the plain case, a reversed share range, one past n_shares, one
    starting before an earlier offset, and messages whose hash fails under BN254_OPT_HASH_MAX_TRIES — tuple_status, the fill of
    share_status with 2, the empty rows and everything else are the same bytes"""
    from tests.hip_ctypes import DevBuf, Stream
    from bn254_amd.engine import pack_messages
    reg_set(eng, keyset)
    tuples = [t for t in cases if 0 < len(t[1]) <= 17][:9]
    msgs, shares, keys, sizes = flat(tuples)
    n, n_shares = len(tuples), len(keys)
    blob, off = pack_messages(msgs)
    off = list(off)
    soff = [sum(sizes[:i]) for i in range(n + 1)]
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_msgs, d_shares, d_keys, d_moff = dev(bytes(blob)), dev(b"".join(shares)), dev(u32(keys) + bytes(4)), dev(u64(off))
        outs = [dev(nbytes=k) for k in (n_shares, n, 64 * n, 4 * BM * n, 4 * n)]

        def run(share_off, seed):
            for b, k in zip(outs, (n_shares, n, 64 * n, 4 * BM * n, 4 * n)):
                b.upload(b"\xEE" * k)
            d_soff = dev(u64(share_off))
            head = (d_msgs.ptr, d_moff.ptr, d_shares.ptr, d_keys.ptr, d_soff.ptr, n_shares, n, BM)
            if seed is None:
                eng.batch_collect_keyed_bitmap_device(*head, *(b.ptr for b in outs), stream=stream.handle)
            else:
                eng.batch_collect_keyed_bitmap_randomized_device(*head, seed, *(b.ptr for b in outs), stream=stream.handle)
            stream.synchronize()
            hook = eng.debug_collect_rand_last()
            return tuple(b.download(k) for b, k in zip(outs, (n_shares, n, 64 * n, 4 * BM * n, 4 * n))), hook

        def both(share_off):
            exact, hook0 = run(share_off, None)
            got, hook = with_options(eng, FORCE, lambda: run(share_off, SEEDS[0]))
            assert hook0["slices"] == 0 and hook["slices"] == 1
            assert got == exact
            return got
        host = collect(eng, tuples)
        g = both(soff)
        assert g[0] == host[0] and g[1] == host[1] and g[2] == host[2]
        i = 3
        rev = soff[:]
        rev[i + 1] = soff[i] - 1                     # tuple i reversed; tuple i + 1 then starts before the earlier offset soff[i]
        g = both(rev)
        assert g[1][i] == 2 and g[1][i + 1] == 2 and all(g[0][s] == 2 for s in range(soff[i], soff[i + 2]))
        assert g[2][64 * i:64 * (i + 2)] == bytes(128) and g[3][4 * BM * i:4 * BM * (i + 2)] == bytes(8 * BM) and g[4][4 * i:4 * (i + 2)] == bytes(8)
        past = soff[:]
        past[n] = n_shares + 1                       # the last tuple runs past n_shares
        g = both(past)
        assert g[1][n - 1] == 2 and all(g[0][s] == 2 for s in range(soff[n - 1], n_shares)) and g[0][:soff[n - 1]] == host[0][:soff[n - 1]]
        lap = soff[:]
        lap[i + 1] = soff[i + 2]                     # tuple i swallows tuple i + 1; tuple i + 2 then starts before an earlier offset
        lap[i + 2] = soff[i + 1]
        g = both(lap)
        assert g[1][i] == 0 and g[1][i + 1] == 2 and g[1][i + 2] == 2 and all(g[0][s] == 2 for s in range(soff[i + 2], soff[i + 3]))
        # one counter per message: the messages that need a second one fail to hash (1), their shares read 1 behind decode and key
        g = with_options(eng, {E.OPT_HASH_MAX_TRIES: 1}, lambda: both(soff))
        assert 1 in g[1] and 0 in g[1], list(g[1])
        for t in range(n):
            if g[1][t] == 1:
                assert all(g[0][s] == (1 if host[0][s] in (0, 9) else host[0][s]) for s in range(soff[t], soff[t + 1])), t
                assert g[2][64 * t:64 * t + 64] == bytes(64) and g[4][4 * t:4 * t + 4] == bytes(4)
        with pytest.raises(E.NativeError) as e:
            eng.batch_collect_keyed_bitmap_randomized_device(d_msgs.ptr, d_moff.ptr, d_shares.ptr, d_keys.ptr + 1, dev(u64(soff)).ptr, n_shares, n, BM,
                                                             SEEDS[0], *(b.ptr for b in outs), stream=stream.handle)
        assert e.value.rc == -10002                    # BN254_E_MISALIGNED
        with pytest.raises(E.NativeError) as e:
            eng.batch_collect_keyed_bitmap_randomized_device(d_msgs.ptr, d_moff.ptr, d_shares.ptr, d_keys.ptr, dev(u64(soff)).ptr, n_shares, n, BM - 1,
                                                             SEEDS[0], *(b.ptr for b in outs), stream=stream.handle)
        assert e.value.rc == -10001                    # BN254_E_BAD_ARGUMENT: the bitmap cannot hold key 45
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


def test_python_mirror(eng, keyset):
    """ECDSA.aggregate_keyed_signers_randomized gives the exact mirror's triple and round-trips into ECDSA.verify_keyed_signers"""
    from bn254_amd.api import ECDSA, PrivateKey, PublicKey
    from tests.datagen import sk_bytes
    sk = [PrivateKey(int.from_bytes(sk_bytes(j), "big")) for j in range(4)]
    pk = [PublicKey.from_private_key(s) for s in sk]
    try:
        assert ECDSA.register_keys(pk, engine=eng) == [None] * 4
        msg = b"round 11"
        sigs = [ECDSA.sign(msg, s) for s in sk]
        args = (msg, [sigs[2], sigs[0], sigs[1], sigs[2], sigs[3]], [2, 0, 3, 2, 9])
        want = ECDSA.aggregate_keyed_signers(*args, engine=eng)

        def call():
            out = [ECDSA.aggregate_keyed_signers_randomized(*args, engine=eng), ECDSA.aggregate_keyed_signers_randomized(*args, seed=SEEDS[0], engine=eng, rand64=True)]
            return out, eng.debug_collect_rand_last()
        (a, b), hook = with_options(eng, FORCE, call)
        assert hook["slices"] == 1 and hook["failed_groups"] == 1
        for got in (a, b):
            assert got[0].raw == want[0].raw and got[1] == want[1] == [0, 2] and got[2] == want[2]
        assert ECDSA.verify_keyed_signers(msg, a[0], a[1], engine=eng) is None
        res = with_options(eng, FORCE, lambda: ECDSA.batch_aggregate_keyed_signers_randomized([(msg, sigs, [0, 1, 2, 3]), (b"other", [], [])], engine=eng))
        assert res[0][1] == [0, 1, 2, 3] and res[1][1] == [] and res[1][0].raw == bytes(64)
    finally:
        reg_set(eng, keyset)
