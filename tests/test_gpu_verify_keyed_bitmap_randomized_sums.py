"""bn254_debug_bitmap_rand_sums against tests/bitmap_rand_model.py on the GPU: per group the tuples at the check, S_g and the
(key index, T_{g,j}) pairs, byte for byte — r_i from hashlib, points and sums from the oracle's g1_mul / g1_add.  A ragged plan with members
off the check in between, three scalar modes, two seeds; once more after a localised failure (the sums survive the re-check).
Run on the MI355X box: -m gpu."""
import pytest

from bn254_amd import engine as E
from tests import bitmap_rand_model as BM
from tests.test_gpu_verify_keyed_bitmap_randomized import (KEY_INF, K_BIG, K_DUP0, K_IDENT, K_NEG1, MODES, N_GOOD, N_KEYS, SEEDS, c, eng, exact, keyset,  # noqa: F401
                                                           rand, randomised, valid)

pytestmark = pytest.mark.gpu


def ragged(eng, c, keyset):  # noqa: F811
    """the ragged plan of tests/bitmap_rand_model.py, signed: members off the check in between"""
    plan = BM.ragged_sets()
    tuples = valid(eng, keyset, "sums", [s for s, _ in plan])
    out = []
    for (m, s, b), (_, k) in zip(tuples, plan):
        if k == "refused":
            b = b + [K_BIG]
        elif k == "oob":
            b = b + [N_KEYS + 3]
        elif k == "curve":
            s = bytearray(s if s != bytes(64) else c.g1_generator()); s[40] ^= 4; s = bytes(s)
        out.append((m, s, b))
    return out


def check(eng, c, tuples, want, seed, mode, G, bm_words=2):  # noqa: F811
    at = [s in (0, 9) for s in want]
    hs = [c.hash_to_g1(t[0])[1] if a else None for t, a in zip(tuples, at)]
    w = BM.model(c, hs, [t[1] for t in tuples], [t[2] for t in tuples], at, KEY_INF, seed, mode, G, bm_words)
    got = eng.debug_bitmap_rand_sums()
    assert len(got) == len(w)
    for g, (d, m) in enumerate(zip(got, w)):
        assert d["nagg"] == m["nagg"] and d["s"] == m["s"], (g, mode)
        assert d["pairs"] == m["pairs"], (g, mode, [k for k, _ in d["pairs"]], [k for k, _ in m["pairs"]])
    return got


def test_sums_against_the_model(eng, c, keyset):  # noqa: F811
    tuples = ragged(eng, c, keyset)
    want = exact(eng, tuples, 2)
    assert 9 not in want and {0, 2, 4, 6} <= set(want) and want.count(0) >= 70, set(want)   # out of range 2, sigma off the curve 4, refused key 6
    for G in (7, 32):
        eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, G)
        for seed in SEEDS:
            for mode, (name, mf) in enumerate(MODES):
                assert rand(eng, tuples, 2, seed, mf) == want, (G, name)
                got = check(eng, c, tuples, want, seed, mode, G)
                assert all(d["verdict"] == 0 for d in got if d["nagg"])
                h = eng.debug_bitmap_rand_last()
                assert h["failed_groups"] == 0 and h["rechecked"] == 0


def test_sums_survive_the_recheck(eng, c, keyset):  # noqa: F811
    tuples = ragged(eng, c, keyset)
    m, s, b = tuples[40]
    tuples[40] = (m, c.g1_add(s, c.g1_generator()), b)
    want = exact(eng, tuples, 2)
    assert want[40] == 9 and want.count(9) == 1
    eng.set_option(E.OPT_BITMAP_RAND_GROUP_TUPLES, 16)
    assert rand(eng, tuples, 2, SEEDS[0]) == want
    got = check(eng, c, tuples, want, SEEDS[0], 0, 16)
    assert [g for g, d in enumerate(got) if d["nagg"] and d["verdict"] == 9] == [40 // 16]
