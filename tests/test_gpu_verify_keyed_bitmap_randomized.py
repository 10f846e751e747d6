"""bn254_batch_verify_keyed_bitmap_randomized[_device] on the GPU (include/bn254_hip.h): the status bytes are the exact bitmap
call's byte for byte — mixed plan, three scalar modes, two seeds, several group sizes, host and _device forms, every bitmap width, slices,
fallbacks — and, since a wrong G1 side only makes a group fail and fall back to the exact re-check, the counters of
bn254_debug_bitmap_rand_last are compared field by field with tests/bitmap_rand_model.py: a batch that should pass has no failed group and
nothing re-checked.  Run on the MI355X box: -m gpu."""
import pytest

from bn254_amd import engine as E
from tests import bitmap_rand_model as BM
from tests.conftest import ws_default
from tests.datagen import D, sk_bytes

pytestmark = pytest.mark.gpu

R = BM.R
N_GOOD, N_KEYS = BM.N_GOOD, BM.N_KEYS
K_OFF_TWIST, K_OFF_SUB, K_BIG, K_IDENT, K_DUP0, K_NEG1 = range(N_GOOD, N_GOOD + 6)
KEY_INF = [False] * N_KEYS
KEY_INF[K_IDENT] = True
MODES = [("rand128", 0), ("rand64", E.FLAG_RAND64), ("glv", E.FLAG_RAND_GLV)]
SEEDS = [bytes(range(32)), bytes(range(7, 39))]


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
    """the 46 keys of tests/test_gpu_verify_keyed_bitmap.py: 40 good ones, off the twist, outside the subgroup, a coordinate >= q, the
    identity, key 0 again and the negation of key 1"""
    sks = [int.from_bytes(sk_bytes(500 + j), "big") % R for j in range(N_GOOD)]
    pks = derive(eng, sks)
    off_twist = bytearray(pks[3]); off_twist[100] ^= 2
    big = bytearray(pks[5]); big[0] = 0xFF
    neg1 = derive(eng, [R - sks[1]])[0]
    pks += [bytes(off_twist), bytes.fromhex(derived["g2_not_in_subgroup"]), bytes(big), bytes(128), pks[0], neg1]
    sks += [0, 0, 0, 0, sks[0], R - sks[1]]
    return sks, pks


def reg_set(eng, keyset, flags=0):
    return eng.register_keys(b"".join(keyset[1]), flags=flags)


@pytest.fixture(autouse=True)
def randomised(eng, keyset):
    reg_set(eng, keyset)
    eng.set_option(E.OPT_BITMAP_RAND_MIN_TUPLES, 1)
    eng.set_option(E.OPT_BITMAP_RAND_MAX_KEYS, 1 << 20)
    yield
    eng.set_option(E.OPT_BITMAP_RAND_MAX_KEYS, ws_default("BITMAP_RAND_MAX_KEYS_DEFAULT"))
    eng.set_option(E.OPT_BITMAP_RAND_MIN_TUPLES, ws_default("BITMAP_RAND_MIN_TUPLES_DEFAULT"))
    eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, ws_default("BITMAP_RAND_GROUP_TUPLES_DEFAULT"))
    eng.set_option(E.OPT_MAX_CHUNK, 0)
    eng.set_option(E.OPT_PAIR_LANES, 1)


def sign_sum(eng, msgs, sk_sums):
    sigs, st = eng.batch_sign(msgs, b"".join((s % R or 1).to_bytes(32, "big") for s in sk_sums))
    assert st == bytes(len(msgs))
    return [bytes(64) if s % R == 0 else sigs[64 * i:64 * i + 64] for i, s in enumerate(sk_sums)]


def to_words(bits, bm_words):
    w = [0] * bm_words
    for j in bits:
        if j // 32 < bm_words:
            w[j // 32] |= 1 << (j % 32)
    return w


def words_of(tuples, bm_words):
    return [x for t in tuples for x in to_words(t[2], bm_words)]


def exact(eng, tuples, bm_words, flags=0):
    return eng.batch_verify_keyed_bitmap([t[0] for t in tuples], b"".join(t[1] for t in tuples), words_of(tuples, bm_words), bm_words, flags=flags)


def rand(eng, tuples, bm_words, seed, flags=0):
    return eng.batch_verify_keyed_bitmap_randomized([t[0] for t in tuples], b"".join(t[1] for t in tuples), words_of(tuples, bm_words), bm_words, seed,
                                                    flags=flags)


def diff(got, want):
    return [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]


def hook(eng):
    h = eng.debug_bitmap_rand_last()
    assert h.pop("ran") == 1, h
    return h


def mixed(eng, c, keyset, tag, n_rounds=2):
    """the mixed plan of the exact call's tests: popcounts 0 / 1 / 2 / 8 / 9 / all; valid, wrong, undecodable and identity sigma; refused and
    out-of-range bits, the identity key, key 0 twice, key 1 and its negation"""
    import random
    sks = keyset[0]
    rnd = random.Random(1)
    g1 = c.g1_generator()
    sets = []
    for r in range(n_rounds):
        for pop in (0, 1, 2, 8, 9, N_GOOD):
            sets.append(sorted(rnd.sample(range(N_GOOD), pop)))
        sets += [[0, K_DUP0], [0, 9, K_DUP0, 17], [1, K_NEG1], [1, 2, K_NEG1], [K_IDENT], [4, K_IDENT, 30], [K_NEG1], list(range(N_GOOD)) + [K_IDENT, K_DUP0, K_NEG1]]
        sets += [[2, K_OFF_TWIST], [K_OFF_SUB, 3, K_BIG], [K_BIG], [5, N_KEYS], [N_KEYS + 20], [6, K_BIG, N_KEYS + 1], [7, 63], [64 + r], [8, 95]]
    msgs = [D("bmr/%s" % tag, i) for i in range(len(sets))]
    sigma = sign_sum(eng, msgs, [sum(sks[j] for j in s if j < N_KEYS) for s in sets])
    out = []
    for i, s in enumerate(sets):
        out.append((msgs[i], sigma[i], s))
        out.append((msgs[i], c.g1_add(sigma[i], g1), s))
        bad = bytearray(sigma[i] if sigma[i] != bytes(64) else g1); bad[40] ^= 4
        out.append((msgs[i], bytes(bad), s))
        out.append((msgs[i], bytes(64), s))
    return out


def valid(eng, keyset, tag, sets, msgs=None):
    """valid tuples (message, sigma, set bits) over the good keys, the identity key, the doubled key and the negation"""
    sks = keyset[0]
    msgs = msgs or [D("bmr/%s" % tag, i) for i in range(len(sets))]
    sigma = sign_sum(eng, msgs, [sum(sks[j] for j in s) for s in sets])
    return [(m, sg, s) for m, sg, s in zip(msgs, sigma, sets)]


passing_sets = BM.passing_sets


@pytest.fixture(scope="module")
def cases(eng, c, keyset):
    reg_set(eng, keyset)
    return mixed(eng, c, keyset, "cases")


@pytest.fixture(scope="module")
def good(eng, keyset):
    reg_set(eng, keyset)
    return valid(eng, keyset, "good", passing_sets(301))


def test_parity_with_the_exact_call(eng, keyset, cases):
    """the mixed plan: the exact call's bytes in three scalar modes, two seeds, groups of 7, 64 and the whole batch; REJECT_IDENTITY too;
    bitmaps of 0, 1, 2, 3 and 4 words"""
    n = len(cases)
    for bm_words, f in ((2, 0), (2, 2), (4, 0), (1, 0), (3, 2), (0, 0)):
        want = exact(eng, cases, bm_words, f)
        if bm_words == 4:
            assert {0, 2, 4, 6, 9} <= set(want)
        for G in (7, 64, n):
            eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, G)
            for seed in (SEEDS if bm_words == 2 and f == 0 else SEEDS[:1]):
                for name, mf in MODES:
                    got = rand(eng, cases, bm_words, seed, f | mf)
                    assert got == want, (bm_words, f, G, name, diff(got, want))
                    h = hook(eng)
                    at = [s in (0, 9) for s in want]
                    w = BM.grouping([t[2] for t in cases], at, [s == 9 for s in want], KEY_INF, G, bm_words)
                    assert h == w, (bm_words, f, G, name, h, w)


def test_device_form_on_a_stream(eng, keyset, cases):
    from tests.hip_ctypes import DevBuf, Stream
    from bn254_amd.engine import pack_messages
    n, bm_words = len(cases), 2
    want = exact(eng, cases, bm_words, 0)
    blob, moff = pack_messages([t[0] for t in cases])
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    st_dev, bufs = Stream(), []
    try:
        def dev(data):
            b = DevBuf(len(data), data=data)
            bufs.append(b)
            return b
        d_msgs, d_off, d_sigs, d_bits = dev(blob), dev(u64(moff)), dev(b"".join(t[1] for t in cases)), dev(u32(words_of(cases, bm_words)))
        d_st = DevBuf(n, fill=0xEE)
        bufs.append(d_st)
        eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, 64)
        for name, mf in MODES:
            eng.batch_verify_keyed_bitmap_randomized_device(d_msgs.ptr, d_off.ptr, d_sigs.ptr, d_bits.ptr, bm_words, n, SEEDS[0], d_st.ptr, flags=mf,
                                                            stream=st_dev.handle)
            st_dev.synchronize()
            got = bytes(d_st.download(n))
            assert got == want, (name, diff(got, want))
            assert hook(eng)["groups"] >= 2
    finally:
        st_dev.synchronize()
        for b in bufs:
            b.free()
        st_dev.destroy()


def test_passing_batch_needs_no_recheck(eng, keyset, good):
    """301 valid tuples: every group passes its combined check — the counters are exactly the model's, no failed group, nothing re-checked.
    This is the test that catches a wrong sum, fold or r_i."""
    n = len(good)
    for G in (7, 64, 512):
        eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, G)
        w = BM.grouping([t[2] for t in good], [True] * n, [False] * n, KEY_INF, G, 2)
        assert w["groups"] == -(-n // G) and w["failed_groups"] == 0 and w["rechecked"] == 0
        for seed in SEEDS:
            for name, mf in MODES:
                got = rand(eng, good, 2, seed, mf)
                assert got == bytes(n), (G, name, diff(got, bytes(n)))
                assert hook(eng) == w, (G, name, hook(eng), w)


def test_localised_failure_and_cancelling_pair(eng, c, keyset, good):
    """one wrong sigma in groups 1 and 3 of 64: exactly those fail, their tuples are re-checked, 9 on the planned tuples alone; sigma_a + D
    and sigma_b - D in one group and across two groups: both get 9"""
    n, G = len(good), 64
    eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, G)
    g1 = c.g1_generator()
    d, minus_d = c.g1_mul(g1, (12345).to_bytes(32, "big")), c.g1_mul(g1, (R - 12345).to_bytes(32, "big"))
    for bad_at in ({70: g1, 200: g1}, {70: d, 71: minus_d}, {70: d, 140: minus_d}):
        tuples = [(m, c.g1_add(s, bad_at[i]) if i in bad_at else s, b) for i, (m, s, b) in enumerate(good)]
        want = bytes(9 if i in bad_at else 0 for i in range(n))
        assert exact(eng, tuples, 2) == want
        for name, mf in MODES:
            got = rand(eng, tuples, 2, SEEDS[0], mf)
            assert got == want, (name, diff(got, want))
            h = hook(eng)
            groups = {i // G for i in bad_at}
            assert h["failed_groups"] == len(groups) and h["rechecked"] == sum(min(G, n - g * G) for g in groups), h
            sums = eng.debug_bitmap_rand_sums()
            assert sorted(g for g, s in enumerate(sums) if s["verdict"] == 9) == sorted(groups)


def test_equal_messages(eng, keyset):
    """tuples that share one message, with equal and with complementary bitmaps: equal (and, through the negated key, opposite) points at
    every level of the sums; 513 tuples with one bitmap: one bucket across the workgroups of the sums"""
    half_a, half_b = list(range(0, N_GOOD, 2)), list(range(1, N_GOOD, 2)) + [K_NEG1]
    for count in (2, 64, 65, 257, 513):
        for sets in ([half_a] * count, [half_a if i % 2 else half_b for i in range(count)]):
            tuples = valid(eng, keyset, "eq", sets, msgs=[D("bmr/eq", 0)] * count)
            for G in (64, 1024):
                eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, G)
                w = BM.grouping(sets, [True] * count, [False] * count, KEY_INF, G, 2)
                got = rand(eng, tuples, 2, SEEDS[0])
                assert got == bytes(count), (count, G, diff(got, bytes(count)))
                assert hook(eng) == w, (count, G, hook(eng), w)
    sets = [list(range(N_GOOD))] * 513
    tuples = valid(eng, keyset, "eq", sets, msgs=[D("bmr/eq", 1)] * 513)
    for cut in (255, 256, 257, 511, 512, 513):
        eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, 1024)
        got = rand(eng, tuples[:cut], 2, SEEDS[1], E.FLAG_RAND64)
        assert got == bytes(cut) and hook(eng) == BM.grouping(sets[:cut], [True] * cut, [False] * cut, KEY_INF, 1024, 2), cut


def test_key_set_shapes(eng, keyset):
    """1, 8, 9, 46 and 257 registered keys (window edges); a group whose tuples are all empty bitmaps; a group with none at the check"""
    sks = [int.from_bytes(sk_bytes(900 + j), "big") % R for j in range(257)]
    pks = derive(eng, sks)
    import random
    rnd = random.Random(9)
    for K in (1, 8, 9, 257):
        assert eng.register_keys(b"".join(pks[:K])) == bytes(K)
        bm_words = (K + 31) // 32
        sets = [sorted(rnd.sample(range(K), rnd.randint(0, K))) for _ in range(40)] + [list(range(K)), [K - 1], [0]]
        msgs = [D("bmr/shape/%d" % K, i) for i in range(len(sets))]
        sigma = sign_sum(eng, msgs, [sum(sks[j] for j in s) for s in sets])
        tuples = list(zip(msgs, sigma, sets))
        for G in (5, 64):
            eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, G)
            got = rand(eng, tuples, bm_words, SEEDS[0])
            assert got == bytes(len(sets)), (K, G, diff(got, bytes(len(sets))))
            assert hook(eng) == BM.grouping(sets, [True] * len(sets), [False] * len(sets), [False] * K, G, bm_words), (K, G)
    reg_set(eng, keyset)
    # groups of 4: group 1 holds empty bitmaps only (sigma = O), group 2 nobody at the check
    sets = [[1, 2], [3], [4, 5], [6]] + [[]] * 4 + [[K_BIG]] * 4 + [[7], [8, 9]]
    tuples = valid(eng, keyset, "empty", [[j for j in s if j < N_GOOD] for s in sets])
    tuples = [(m, s, b) for (m, s, _), b in zip(tuples, sets)]
    eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, 4)
    want = exact(eng, tuples, 2)
    assert want == bytes([0] * 8 + [6] * 4 + [0] * 2)
    assert rand(eng, tuples, 2, SEEDS[0]) == want
    assert hook(eng) == dict(groups=3, table_pairs=(6 + 1) + 1 + (3 + 1), failed_groups=0, rechecked=0, single_groups=0)
    sums = eng.debug_bitmap_rand_sums()
    assert [s["nagg"] for s in sums] == [4, 4, 0, 2] and sums[1]["pairs"] == [] and sums[1]["s"] == bytes(64) and sums[2]["pairs"] == []


def test_fallbacks_and_reregistration(eng, keyset, cases, good):
    """no registered keys, pair lanes off and n below the minimum: the exact bytes, ran = 0; a re-registration between two calls"""
    want = exact(eng, cases, 2)
    eng.set_option(E.OPT_BITMAP_RAND_MIN_TUPLES, len(cases) + 1)
    assert rand(eng, cases, 2, SEEDS[0]) == want and eng.debug_bitmap_rand_last()["ran"] == 0
    eng.set_option(E.OPT_BITMAP_RAND_MIN_TUPLES, 1)
    eng.set_option(E.OPT_PAIR_LANES, 0)
    assert rand(eng, cases, 2, SEEDS[0]) == want and eng.debug_bitmap_rand_last()["ran"] == 0
    eng.set_option(E.OPT_PAIR_LANES, 1)
    assert rand(eng, cases, 2, SEEDS[0]) == want and eng.debug_bitmap_rand_last()["ran"] == 1
    eng.register_keys(b"")
    none = exact(eng, cases, 2)
    assert rand(eng, cases, 2, SEEDS[0]) == none and eng.debug_bitmap_rand_last()["ran"] == 0 and 2 in none
    # keys 0 and 1 swapped: a tuple that names one of them fails now, with fresh tables and a fresh bad-bit vector
    sks, pks = keyset
    eng.register_keys(b"".join([pks[1], pks[0]] + pks[2:]))
    eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, 64)
    want = exact(eng, good, 2)
    assert 9 in want and 0 in want
    assert rand(eng, good, 2, SEEDS[0]) == want
    reg_set(eng, keyset, flags=2)
    want = exact(eng, good, 2)
    assert 4 in want and rand(eng, good, 2, SEEDS[0]) == want


def test_slices(eng, keyset, cases, good):
    """BN254_OPT_MAX_CHUNK forcing three slices: the same statuses; r_i keeps the caller's numbering"""
    eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, 16)
    for tuples in (cases, good):
        want = exact(eng, tuples, 2)
        eng.set_option(E.OPT_MAX_CHUNK, (len(tuples) + 2) // 3)
        for name, mf in MODES:
            assert rand(eng, tuples, 2, SEEDS[0], mf) == want, name
        h = hook(eng)
        assert h["groups"] >= 2 and (tuples is cases or h["failed_groups"] == 0)
        eng.set_option(E.OPT_MAX_CHUNK, 0)
