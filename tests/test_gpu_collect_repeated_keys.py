"""A registered key set that REPEATS keys, through bn254_batch_collect_keyed_bitmap[_randomized] and bn254_batch_verify_keyed_bitmap on the
GPU: indices 0 .. 127 hold one key pk_A, 128 .. 191 its negation, 192 .. 255 the 64 distinct keys B_j (tests/collect_repeat_cases.py).  On
it the additions of equal and of opposite points are the normal path of k_cl_sum_wave's tree (cl_tree_level: in LDS, output aliasing the
first input, under a wave vote inside `t < stride`), of a lane's own stride (cl_step), and of the bitmap verify's subset tables
(bn254_bitmap.h: bm_subset_entry, jac_accumulate_from).
Nothing expected comes from the device: the share statuses are planted (0 for a valid share, 9 for sigma + G1), the rows and counts are
tests/collect_model.py's, the aggregates the oracle's g1_add over the planted points and, again, its g1_mul of sigma by the net multiple.
Helpers: tests/test_gpu_collect_keyed_bitmap.py, tests/test_gpu_collect_keyed_bitmap_randomized.py, tests/test_gpu_verify_keyed_bitmap.py.
Run on the MI355X box: -m gpu."""
import pytest

from bn254_amd import engine as E
from tests import collect_model
from tests import collect_repeat_cases as rc
from tests.datagen import D, sk_bytes
from tests.test_gpu_collect_keyed_bitmap import ROUTES, c, collect, derive, eng, keyed, sign, with_options   # noqa: F401
from tests.test_gpu_collect_keyed_bitmap_randomized import FORCE, SEEDS, rand_collect
from tests.test_gpu_verify_keyed_bitmap import bitmap_call, identity_call

pytestmark = pytest.mark.gpu

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
BM = rc.BM
TABLE_ROUTES = [("tables", 4096), ("key_by_key", 0)]               # BN254_OPT_BITMAP_TABLE_MAX_KEYS: its default, and 0 = keys added one by one


@pytest.fixture(scope="module")
def keys(eng):
    """-> (a, [b_j], the 256 encodings); registered"""
    a = int.from_bytes(sk_bytes(900), "big") % R
    b = [int.from_bytes(sk_bytes(901 + j), "big") % R for j in range(rc.N_B)]
    pk = derive(eng, [a, R - a] + b)
    pks = [pk[0]] * rc.N_A + [pk[1]] * rc.N_NEG + pk[2:]
    assert len(pks) == rc.N_KEYS and len(set(pks)) == 2 + rc.N_B
    assert eng.register_keys(b"".join(pks)) == bytes(rc.N_KEYS)
    return a, b, pks


@pytest.fixture(scope="module")
def planted(eng, c, keys):
    """the case set signed, each tuple under a message of its own -> dict(names, msgs, tuples, sigma, bsh, status, bits, counts, agg)"""
    a, b, _ = keys
    cases = rc.shapes()
    msgs = [D("collect/repeated", i) for i in range(len(cases))]
    pairs, at = [], []
    for i, (_, sh) in enumerate(cases):
        at.append(len(pairs))
        pairs += [(msgs[i], a), (msgs[i], R - a)] + [(msgs[i], b[k - rc.K_B]) for kind, k in sh if kind == "B"]
    sigs = sign(eng, pairs)
    g1 = c.g1_generator()
    sigma, bsh = [], []
    for i, (_, sh) in enumerate(cases):
        s, neg = sigs[at[i]], sigs[at[i] + 1]
        assert c.g1_add(s, neg) == bytes(64) and s != bytes(64)            # the share of an index in 128 .. 191 is -sigma
        sigma.append(s)
        bsh.append(dict(zip([k for kind, k in sh if kind == "B"], sigs[at[i] + 2:])))
    wrong = [c.g1_add(s, g1) for s in sigma]
    neg = [sigs[k + 1] for k in at]
    shares, share_keys, sizes, status = rc.plant(cases, lambda i, kind, key: {"A": sigma[i], "N": neg[i], "W": wrong[i]}.get(kind) or bsh[i][key])
    tuples, k = [], 0
    for m, size in zip(msgs, sizes):
        tuples.append((m, list(zip(shares[k:k + size], share_keys[k:k + size]))))
        k += size
    rows, counts, chosen = collect_model.select(share_keys, status, sizes, bytes(len(cases)), BM)
    agg = collect_model.aggregates(c, shares, chosen)
    # ... and every aggregate a second way: (the net multiple) sigma + the B shares
    for i, (name, sh) in enumerate(cases):
        m, bs, count = rc.net(sh)
        point = c.g1_mul(sigma[i], (m % R).to_bytes(32, "big")) if m % R else bytes(64)
        for j in bs:
            point = c.g1_add(point, bsh[i][rc.K_B + j])
        assert agg[i] == point and counts[i] == count, name
    return dict(names=[name for name, _ in cases], msgs=msgs, tuples=tuples, sigma=sigma, status=bytes(status),
                bits=[w for r in rows for w in r], counts=counts, agg=b"".join(agg), cases=cases)


def names_of(p, got_agg):
    return " ".join(p["names"][i] for i in range(len(p["names"])) if got_agg[64 * i:64 * i + 64] != p["agg"][64 * i:64 * i + 64])


def test_every_route(eng, c, keys, planted):
    """identity 1 with the planted statuses; statuses, rows, counts and aggregates on every route; the two sum layouts give the same bytes"""
    p = planted
    n = len(p["tuples"])
    assert keyed(eng, p["tuples"]) == p["status"] and p["status"].count(9) > n and p["status"].count(0) > 20 * n
    i64, i2, i0 = p["names"].index("double_every_level"), p["names"].index("double_at_16"), p["names"].index("cancel_at_4+1")
    assert p["agg"][64 * i64:64 * i64 + 64] == c.g1_mul(p["sigma"][i64], (64).to_bytes(32, "big")) and p["counts"][i64] == 64
    assert p["agg"][64 * i2:64 * i2 + 64] == c.g1_add(p["sigma"][i2], p["sigma"][i2]) and p["counts"][i2] == 2
    assert p["agg"][64 * i0:64 * i0 + 64] == bytes(64) and p["counts"][i0] == 2 and sum(bin(w).count("1") for w in p["bits"][BM * i0:BM * i0 + BM]) == 2
    seen = {}
    for name, opts in ROUTES:
        share_st, tuple_st, agg, bits, counts = with_options(eng, opts, lambda: collect(eng, p["tuples"], bm_words=BM))
        assert share_st == p["status"], (name, [(s, a, b) for s, (a, b) in enumerate(zip(share_st, p["status"])) if a != b][:8])
        assert tuple_st == bytes(n), name
        assert bits == p["bits"] and counts == p["counts"], name
        assert agg == p["agg"], "%s: %s" % (name, names_of(p, agg))
        seen[name] = agg
    assert seen["all_waves"] == seen["all_lanes"]


@pytest.mark.parametrize("flags", [0, E.FLAG_RAND64, E.FLAG_RAND_GLV], ids=["rand128", "rand64", "glv"])
def test_randomized(eng, keys, planted, flags):
    """bn254_batch_collect_keyed_bitmap_randomized, options 38 and 39 forced to 0: the planted outputs, which are the exact call's, in one slice"""
    p = planted
    assert FORCE == {E.OPT_COLLECT_RAND_MIN_SHARES: 0, E.OPT_COLLECT_RAND_MIN_PER_KEY: 0}
    got, hook = rand_collect(eng, p["tuples"], SEEDS[0], flags, bm_words=BM)
    assert hook["slices"] == 1, hook
    assert got[2] == p["agg"], names_of(p, got[2])
    assert got == (p["status"], bytes(len(p["tuples"])), p["agg"], p["bits"], p["counts"])
    assert got == collect(eng, p["tuples"], bm_words=BM)


def bitmap_routes(eng, fn):
    out = {}
    try:
        for name, value in TABLE_ROUTES:
            eng.set_option(E.OPT_BITMAP_TABLE_MAX_KEYS, value)
            out[name] = fn()
    finally:
        eng.set_option(E.OPT_BITMAP_TABLE_MAX_KEYS, 4096)
    return out


def test_bitmap_verify_of_the_aggregates(eng, c, keys, planted):
    """identity 2 over equal and opposite keys inside one 8-key window: the model's rows with the oracle's aggregates read 0, with the subset
    tables and key by key; three tuples anchored on the oracle alone (g2_add over the set bits, hash_to_g1, pairing_check)"""
    _, _, pks = keys
    p = planted
    n = len(p["msgs"])
    neg_g2 = c.g2_mul(c.g2_generator(), (R - 1).to_bytes(32, "big"))
    for name in ("double_every_level", "mixed_vote", "cancel_first_level"):
        i = p["names"].index(name)
        apk = bytes(128)
        for j in range(rc.N_KEYS):
            if (p["bits"][BM * i + j // 32] >> (j % 32)) & 1:
                apk = c.g2_add(apk, pks[j])
        st, h, _ = c.hash_to_g1(p["msgs"][i])
        assert st == 0
        assert c.pairing_check(h + p["agg"][64 * i:64 * i + 64], apk + neg_g2, 2) == 0, name
        if name == "double_every_level":
            assert apk == c.g2_mul(pks[0], (64).to_bytes(32, "big"))               # 64 copies of pk_A
        if name == "cancel_first_level":
            assert apk == bytes(128) and p["agg"][64 * i:64 * i + 64] == bytes(64)
    got = bitmap_routes(eng, lambda: eng.batch_verify_keyed_bitmap(p["msgs"], p["agg"], p["bits"], BM))
    for name, _ in TABLE_ROUTES:
        assert got[name] == bytes(n), (name, [p["names"][i] for i in range(n) if got[name][i]])


def test_hand_made_bitmaps(eng, c, keys):
    """no collect in front: bits {0, 1}, a full window of equal keys, a key beside its negation across two windows, a window of negations;
    with the right sigma (0), with sigma + G1 (9) and with the sigma of one signer more (9), against the distinct-message keyed call on the
    message repeated"""
    a, _, _ = keys
    sets = [[0, 1], list(range(8)), [127, 128], list(range(128, 136)), [0, 1, 127, 128, 129], [5, 6, 7, 8, 9, 200]]
    msgs = [D("bm/repeated", i) for i in range(len(sets))]
    sig = sign(eng, [(m, a) for m in msgs] + [(msgs[5], keys[1][200 - rc.K_B])])
    g1 = c.g1_generator()
    tuples, want = [], []
    for i, s in enumerate(sets):
        m = sum(1 if j < rc.K_NEG else -1 for j in s if j < rc.K_B)
        sigma = c.g1_mul(sig[i], (m % R).to_bytes(32, "big")) if m % R else bytes(64)
        if i == 5:
            sigma = c.g1_add(sigma, sig[len(sets)])
        tuples += [(msgs[i], sigma, s), (msgs[i], c.g1_add(sigma, g1), s), (msgs[i], c.g1_add(sigma, sig[i]), s)]
        want += [0, 9, 9]
    got = bitmap_routes(eng, lambda: (bitmap_call(eng, tuples, BM), identity_call(eng, tuples, BM)))
    for name, _ in TABLE_ROUTES:
        assert list(got[name][0]) == want == list(got[name][1]), name
