"""Same-message aggregates as signer bitmaps over registered keys (include/bn254_hip.h: bn254_batch_verify_keyed_bitmap[_device]) on the GPU.
The defining identity: the status bytes equal those of bn254_batch_aggregate_verify_distinct_keyed with the same flags on aggregates that
repeat the tuple's message once per set bit, key_idx = the set bits in ascending order.  Every route is compared byte for byte (subset
tables, key by key, over the key limit, pair lanes off, every row of the routing table, slices, host and _device forms), a dozen tuples are
anchored on the oracle alone, and a re-registration must not meet stale tables.  Run on the MI355X box: -m gpu."""
import random

import pytest

from bn254_amd import engine as E
from tests.datagen import D, sk_bytes

pytestmark = pytest.mark.gpu

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
N_GOOD = 40


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def derive(eng, sks):
    out, st = eng.batch_g2_mul(None, b"".join(s.to_bytes(32, "big") for s in sks), len(sks), reduce_scalar=True)
    assert st == bytes(len(sks))
    return [out[128 * j:128 * j + 128] for j in range(len(sks))]


@pytest.fixture(scope="module")
def keyset(eng, derived):
    """40 good keys, then: off the twist (4), outside the subgroup (4), a coordinate >= q (6), the identity, key 0 AGAIN (doubling) and the
    NEGATION of key 1.  Returns (secret keys as integers — 0 for keys that contribute nothing —, encodings, registration statuses)."""
    sks = [int.from_bytes(sk_bytes(500 + j), "big") % R for j in range(N_GOOD)]
    pks = derive(eng, sks)
    off_twist = bytearray(pks[3]); off_twist[100] ^= 2
    big = bytearray(pks[5]); big[0] = 0xFF
    neg1 = derive(eng, [R - sks[1]])[0]
    pks += [bytes(off_twist), bytes.fromhex(derived["g2_not_in_subgroup"]), bytes(big), bytes(128), pks[0], neg1]
    sks += [0, 0, 0, 0, sks[0], R - sks[1]]
    reg = eng.register_keys(b"".join(pks))
    assert list(reg) == [0] * N_GOOD + [4, 4, 6, 0, 0, 0], reg[N_GOOD:]
    return sks, pks, reg


K_OFF_TWIST, K_OFF_SUB, K_BIG, K_IDENT, K_DUP0, K_NEG1 = range(N_GOOD, N_GOOD + 6)
N_KEYS = N_GOOD + 6


def reg_set(eng, keyset, flags=0):
    return eng.register_keys(b"".join(keyset[1]), flags=flags)


def sign_sum(eng, msgs, sk_sums):
    """sigma_i = (sum of the signers' secret keys) * H(m_i); a zero sum is the identity"""
    sigs, st = eng.batch_sign(msgs, b"".join((s % R or 1).to_bytes(32, "big") for s in sk_sums))
    assert st == bytes(len(msgs))
    return [bytes(64) if s % R == 0 else sigs[64 * i:64 * i + 64] for i, s in enumerate(sk_sums)]


def to_words(bits, bm_words):
    w = [0] * bm_words
    for j in bits:
        if j // 32 < bm_words:
            w[j // 32] |= 1 << (j % 32)
    return w


def bitmap_call(eng, tuples, bm_words, flags=0):
    words = [x for t in tuples for x in to_words(t[2], bm_words)]
    return eng.batch_verify_keyed_bitmap([t[0] for t in tuples], b"".join(t[1] for t in tuples), words, bm_words, flags=flags)


def identity_call(eng, tuples, bm_words, flags=0):
    """the defining identity: the distinct-message keyed call with the message repeated once per set bit (bits the bitmap cannot hold are
    absent), key_idx = the set bits in ascending order"""
    msgs, idx, sizes = [], [], []
    for m, _, bits in tuples:
        held = sorted(j for j in set(bits) if j // 32 < bm_words)
        msgs += [m] * len(held)
        idx += held
        sizes.append(len(held))
    return eng.batch_aggregate_verify_distinct_keyed(msgs, idx, b"".join(t[1] for t in tuples), sizes, flags=flags)


def build(eng, c, keyset, tag, n_rounds=2, seed=1):
    """tuples (message, sigma, set bits): popcounts 0, 1, 2, 8, 9 and all; valid, sigma wrong, sigma undecodable, sigma the identity; refused
    keys, bits at and above n_keys, the identity key, key 0 twice, key 1 and its negation"""
    sks, pks, reg = keyset
    rnd = random.Random(seed)
    g1 = c.g1_generator()
    sets = []
    for r in range(n_rounds):
        for pop in (0, 1, 2, 8, 9, N_GOOD):
            sets.append(sorted(rnd.sample(range(N_GOOD), pop)))
        sets += [[0, K_DUP0], [0, 9, K_DUP0, 17], [1, K_NEG1], [1, 2, K_NEG1], [K_IDENT], [4, K_IDENT, 30], [K_NEG1], list(range(N_KEYS - 6)) + [K_IDENT, K_DUP0, K_NEG1]]
        sets += [[2, K_OFF_TWIST], [K_OFF_SUB, 3, K_BIG], [K_BIG], [5, N_KEYS], [N_KEYS + 20], [6, K_BIG, N_KEYS + 1], [7, 63], [64 + r], [8, 95]]
    msgs = [D("bm/%s" % tag, i) for i in range(len(sets))]
    sigma = sign_sum(eng, msgs, [sum(sks[j] for j in s if j < N_KEYS) for s in sets])
    out = []
    for i, s in enumerate(sets):
        out.append((msgs[i], sigma[i], s))
        out.append((msgs[i], c.g1_add(sigma[i], g1), s))                  # sigma wrong
        bad = bytearray(sigma[i] if sigma[i] != bytes(64) else g1); bad[40] ^= 4
        out.append((msgs[i], bytes(bad), s))                               # sigma off the curve
        out.append((msgs[i], bytes(64), s))                                # sigma the identity
    return out


@pytest.fixture(scope="module")
def cases(eng, c, keyset):
    return build(eng, c, keyset, "cases")


def with_options(eng, opts, fn):
    defaults = {E.OPT_BITMAP_ROUTE: 0, E.OPT_BITMAP_TABLE_MAX_KEYS: 4096, E.OPT_PAIR_LANES: 1, E.OPT_MAX_CHUNK: 0}
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            eng.set_option(k, defaults[k])


ROUTES = [("tables", {}), ("keys", {E.OPT_BITMAP_ROUTE: 2}), ("over_limit", {E.OPT_BITMAP_TABLE_MAX_KEYS: N_KEYS - 1}), ("option_zero", {E.OPT_BITMAP_TABLE_MAX_KEYS: 0}),
          ("forced_tables", {E.OPT_BITMAP_ROUTE: 1, E.OPT_BITMAP_TABLE_MAX_KEYS: 0}), ("pair_lanes_off", {E.OPT_PAIR_LANES: 0}),
          ("pair_lanes_off_keys", {E.OPT_PAIR_LANES: 0, E.OPT_BITMAP_ROUTE: 2}), ("sliced", {E.OPT_MAX_CHUNK: 37})]


def diff(got, want, tuples):
    return [(i, g, w, tuples[i][2][:6]) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]


def test_defining_identity_every_route(eng, c, keyset, cases):
    """every case, flags 0 and REJECT_IDENTITY, bitmaps of 2 words (exact), 3 and 4 (too large, bits above n_keys) and 1 (too small: keys 32..
    absent), on every route: the bytes of the distinct-message keyed call"""
    reg_set(eng, keyset)
    for bm_words in (2, 4, 1, 3):
        for f in (0, 2):
            want = identity_call(eng, cases, bm_words, f)
            if bm_words == 4:
                assert {0, 2, 4, 6, 9} <= set(want) and want.count(0) >= 16 and want.count(9) >= 16, set(want)
            for name, opts in (ROUTES if bm_words in (2, 4) else ROUTES[:2]):
                got = with_options(eng, opts, lambda: bitmap_call(eng, cases, bm_words, f))
                assert got == want, (name, bm_words, f, diff(got, want, cases))
    # bm_words = 0: every bitmap is empty — e(sigma, -G2) == 1
    got = eng.batch_verify_keyed_bitmap([t[0] for t in cases], b"".join(t[1] for t in cases), [], 0)
    assert got == identity_call(eng, cases, 0)
    assert all(g == 0 for g, t in zip(got, cases) if t[1] == bytes(64)) and 9 in got


def test_reject_identity_at_registration(eng, c, keyset, cases):
    """REJECT_IDENTITY given at registration refuses the identity key (4): its tuples follow rule 2; stale tables would say 0"""
    try:
        assert bitmap_call(eng, cases, 2, 0) == identity_call(eng, cases, 2, 0)       # tables of the plain registration are in place
        reg = reg_set(eng, keyset, flags=2)
        assert reg[K_IDENT] == 4
        for f in (0, 2):
            want = identity_call(eng, cases, 2, f)
            for name, opts in ROUTES[:3]:
                got = with_options(eng, opts, lambda: bitmap_call(eng, cases, 2, f))
                assert got == want, (name, f, diff(got, want, cases))
        assert 4 in bitmap_call(eng, [t for t in cases if t[2] == [K_IDENT]], 2, 0)
    finally:
        reg_set(eng, keyset)


def test_no_keys_registered(eng, c, keyset, cases):
    """an empty key set: any set bit gives 2 behind sigma's decode status; empty bitmaps check e(sigma, -G2) == 1"""
    try:
        eng.register_keys(b"")
        for bm_words in (2, 0):
            got = bitmap_call(eng, cases, bm_words, 0)
            for i, (m, sigma, bits) in enumerate(cases):
                st = c.g1_validate(sigma, 0)
                held = [j for j in bits if j // 32 < bm_words]
                want = st if st else (2 if held else (0 if sigma == bytes(64) else 9))
                assert got[i] == want, (i, bm_words)
            assert got == identity_call(eng, cases, bm_words, 0)
    finally:
        reg_set(eng, keyset)


def test_oracle_anchor(eng, c, keyset):
    """a dozen tuples whose expected status comes from the oracle alone: g2_add over the set bits, hash_to_g1, pairing_check"""
    sks, pks, reg = keyset
    reg_set(eng, keyset)
    rnd = random.Random(5)
    g2 = c.g2_generator()
    neg_g2 = c.g2_mul(g2, (R - 1).to_bytes(32, "big"))
    sets = [sorted(rnd.sample(range(N_GOOD), p)) for p in (1, 2, 3, 8, 9, 17)] + [[0, K_DUP0], [1, K_NEG1], [3, K_IDENT, 4], [], [1, 5, K_NEG1], [0, 1, 2]]
    msgs = [D("bm/anchor", i) for i in range(len(sets))]
    sigma = sign_sum(eng, msgs, [sum(sks[j] for j in s) for s in sets])
    sigma[-1] = c.g1_add(sigma[-1], c.g1_generator())
    want = []
    for m, sg, s in zip(msgs, sigma, sets):
        apk = bytes(128)
        for j in s:
            apk = c.g2_add(apk, pks[j])
        st, h, _ = c.hash_to_g1(m)
        assert st == 0
        want.append(c.pairing_check(h + sg, apk + neg_g2, 2))
    assert want == [0] * 11 + [9]
    tuples = list(zip(msgs, sigma, sets))
    for name, opts in ROUTES:
        assert list(with_options(eng, opts, lambda: bitmap_call(eng, tuples, 2))) == want, name


@pytest.fixture(scope="module")
def many(eng, c, keyset):
    """enough tuples for the last row of the routing table: popcounts 1..3 over the good keys, every 5th sigma wrong, every 11th a refused key"""
    sks, pks, reg = keyset
    top = max(r[0] for r in eng.route_table()[:-1]) + 2
    rnd = random.Random(11)
    sets = [sorted(rnd.sample(range(N_GOOD), 1 + i % 3)) for i in range(top)]
    msgs = [D("bm/many", i) for i in range(top)]
    sk_sums = [sum(sks[j] for j in s) + (1 if i % 5 == 0 else 0) for i, s in enumerate(sets)]
    sigma = sign_sum(eng, msgs, sk_sums)
    for i in range(0, top, 11):
        sets[i] = sets[i] + [K_OFF_TWIST + (i // 11) % 3]
    return list(zip(msgs, sigma, sets))


def test_both_sides_of_every_routing_row(eng, keyset, many):
    reg_set(eng, keyset)
    rows = eng.route_table()
    assert len(rows) >= 2
    sizes = sorted({n for r in rows[:-1] for n in (r[0], r[0] + 1)} | {1, 2, 63, 64, 65})
    for n in sizes:
        t = many[:n]
        want = identity_call(eng, t, 2)
        assert bitmap_call(eng, t, 2) == want, (n, diff(bitmap_call(eng, t, 2), want, t))
        if n >= 63:
            assert {0, 4, 9} <= set(want)
    n = sizes[-1]
    want = identity_call(eng, many[:n], 2)
    for opts in ({E.OPT_MAX_CHUNK: 1000}, {E.OPT_BITMAP_ROUTE: 2}, {E.OPT_PAIR_LANES: 0, E.OPT_MAX_CHUNK: 4096}):
        assert with_options(eng, opts, lambda: bitmap_call(eng, many[:n], 2)) == want, opts


def test_device_form_and_reregistration(eng, c, keyset, cases):
    """the _device form on a caller's stream gives the host form's bytes; a reversed offset pair gives 5; bn254_ctx_expect_msgs_len bounds
    the spans; a misaligned bitmap is refused; a set registered between two calls takes effect (no stale tables)"""
    from tests.hip_ctypes import DevBuf, Stream
    from bn254_amd.engine import pack_messages
    sks, pks, reg = keyset
    reg_set(eng, keyset)
    tuples = [t for t in cases if t[2]][:96]
    n = len(tuples)
    blob, off = pack_messages([t[0] for t in tuples])
    off = list(off)
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    bits = u32([x for t in tuples for x in to_words(t[2], 2)])
    st_dev = Stream()
    bufs = []
    try:
        def dev(data):
            b = DevBuf(len(data), data=data)
            bufs.append(b)
            return b
        d_msgs, d_sigs, d_bits = dev(bytes(blob)), dev(b"".join(t[1] for t in tuples)), dev(bits + bytes(4))
        d_status = DevBuf(n, fill=0xEE)
        bufs.append(d_status)

        def run(offsets, flags=0, msgs_len=None, bits_ptr=None):
            d_off = dev(u64(offsets))
            if msgs_len is not None:
                eng.expect_msgs_len(msgs_len)
            eng.batch_verify_keyed_bitmap_device(d_msgs.ptr, d_off.ptr, d_sigs.ptr, bits_ptr or d_bits.ptr, 2, n, d_status.ptr, flags=flags, stream=st_dev.handle)
            st_dev.synchronize()
            return d_status.download(n)

        for f in (0, 2):
            want = bitmap_call(eng, tuples, 2, f)
            assert run(off, f) == want == identity_call(eng, tuples, 2, f)
            assert with_options(eng, {E.OPT_BITMAP_ROUTE: 2}, lambda: run(off, f)) == want
            assert with_options(eng, {E.OPT_MAX_CHUNK: 10}, lambda: run(off, f)) == want
        want = bitmap_call(eng, tuples, 2, 0)
        i = next(k for k in range(1, n - 1) if want[k] in (0, 9) and off[k + 1] > off[k])
        rev = off[:]
        rev[i + 1] = off[i] - 1                                             # tuple i reversed (tuple i + 1 grows: another message)
        got = run(rev)
        assert got[i] == 5 and got[:i] == want[:i] and got[i + 2:] == want[i + 2:]
        got = run(off, msgs_len=off[n] - 1)                                 # the last message runs past the declared buffer
        last = n - 1
        assert got[:last] == want[:last] and got[last] == (5 if want[last] in (0, 9) else want[last])
        assert run(off) == want                                             # the declaration was consumed
        with pytest.raises(Exception):
            run(off, bits_ptr=d_bits.ptr + 1)                               # BN254_E_MISALIGNED
        # re-registration: set B = the good keys rotated by one -> a valid tuple of set A fails under B, and B's own tuples pass
        rot = pks[1:N_GOOD] + pks[:1] + pks[N_GOOD:]
        eng.register_keys(b"".join(rot))
        got_b = run(off)
        assert got_b == identity_call(eng, tuples, 2) and got_b != want
        valid_a = [k for k in range(n) if want[k] == 0 and tuples[k][1] != bytes(64) and all(j < N_GOOD for j in tuples[k][2])]
        assert valid_a and all(got_b[k] == 9 for k in valid_a if len(tuples[k][2]) < N_GOOD)
        eng.register_keys(b"".join(pks[:8]))                                # a smaller set: bits 8.. are out of range now
        got_c = run(off)
        assert got_c == identity_call(eng, tuples, 2)
        assert all(got_c[k] == 2 for k in valid_a if max(tuples[k][2]) >= 8)
    finally:
        for b in bufs:
            b.free()
        st_dev.destroy()
        reg_set(eng, keyset)


def test_large_key_set_two_thirds(eng, keyset):
    """1 040 keys (not a multiple of 32, one refused, one identity), 2 048 tuples with random two-thirds bitmaps, every 7th sigma wrong:
    tables, key by key and over the limit against the distinct-message keyed call"""
    n_keys, n = 1040, 2048
    rnd = random.Random(3)
    sks = [int.from_bytes(sk_bytes(3000 + j), "big") % R for j in range(n_keys)]
    pks = derive(eng, sks)
    bad = bytearray(pks[700]); bad[100] ^= 2
    pks[700], sks[700] = bytes(bad), 0
    pks[33], sks[33] = bytes(128), 0
    try:
        reg = eng.register_keys(b"".join(pks))
        assert reg[700] == 4 and reg.count(0) == n_keys - 1
        sets = [[j for j in range(n_keys) if (i % 64 == 0 if j == 700 else rnd.random() < 2 / 3)] for i in range(n)]
        msgs = [D("bm/large", i) for i in range(n)]
        sigma = sign_sum(eng, msgs, [sum(sks[j] for j in s) + (1 if i % 7 == 0 else 0) for i, s in enumerate(sets)])
        tuples = list(zip(msgs, sigma, sets))
        bm_words = (n_keys + 31) // 32
        want = identity_call(eng, tuples, bm_words)
        assert want.count(0) > n // 2 and want.count(9) >= n // 8 and want.count(4) == n // 64
        for name, opts in (("tables", {}), ("keys", {E.OPT_BITMAP_ROUTE: 2}), ("over_limit", {E.OPT_BITMAP_TABLE_MAX_KEYS: 1024})):
            got = with_options(eng, opts, lambda: bitmap_call(eng, tuples, bm_words))
            assert got == want, (name, diff(got, want, tuples))
    finally:
        reg_set(eng, keyset)


def test_python_api(eng, keyset):
    """ECDSA.verify_keyed_signers / batch_verify_keyed_signers: None for a valid aggregate, VerificationFailed for a missing signer,
    IndexOutOfBounds outside the set"""
    from bn254_amd.api import ECDSA, Error, ErrorKind, PrivateKey, PublicKey
    sk = [PrivateKey(int.from_bytes(sk_bytes(j), "big")) for j in range(3)]
    pk = [PublicKey.from_private_key(s) for s in sk]
    try:
        assert ECDSA.register_keys(pk, engine=eng) == [None, None, None]
        msg = b"round 9"
        sigs = [ECDSA.sign(msg, s) for s in sk]
        sigma = sigs[0] + sigs[1] + sigs[2]
        assert ECDSA.verify_keyed_signers(msg, sigma, [0, 1, 2], engine=eng) is None
        with pytest.raises(Error) as e:
            ECDSA.verify_keyed_signers(msg, sigma, [0, 2], engine=eng)
        assert e.value.kind == ErrorKind.VerificationFailed
        res = ECDSA.batch_verify_keyed_signers([(msg, sigma, [2, 1, 0]), (msg, sigs[0] + sigs[2], [0, 2]), (msg, sigma, [0, 1, 2, 3]),
                                                (msg, sigma, [0, 1, 2, 1 << 40])], engine=eng)
        assert res == [None, None, Error(ErrorKind.IndexOutOfBounds), Error(ErrorKind.IndexOutOfBounds)]
    finally:
        reg_set(eng, keyset)
