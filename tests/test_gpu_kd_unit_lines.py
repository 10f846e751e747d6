"""The keyed Miller loop on unit lines on the device (BN254_OPT_KEY_DEDUP_FOLD = 2; bn254_pair.hip: k_miller_verify_keyed_unit_pair,
bn254_pairing.h: miller_loop_keyed_unit) at the first lane-pair size, 16 385 items — the smallest batch that reaches the route — over pools
of 1, 5 and 256 keys: wrong, malformed and identity signatures; refused, identity and off-curve keys.  Statuses with the option at 2
against the oracle, against the folded rows (1), the line pairs (0) and the generic loop forced on the device; the route report says the
keyed kernel ran; a second call, on a warm key cache, gives the same statuses."""
import pytest

from tests.test_gpu_kd_fold import with_identity_signatures
from tests.test_gpu_key_cache import Dev, N, batch_over, cache, eng, gen, keyed, odd_keys, opt  # noqa: F401  (eng, gen: fixtures)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("pool", [1, 5, 256])
def test_unit_line_statuses(eng, gen, derived, pool):
    from oracle import c_oracle
    ids = list(range(pool))
    batch = with_identity_signatures(batch_over(gen, N, ids, odd_keys(gen, derived, ids)))
    want, _ = c_oracle.batch_verify(*batch, flags=0, nthreads=16)
    dev = Dev(batch)
    opt(eng, "KEY_DEDUP_FOLD", 2)
    for call in (0, 1):                                   # the second call finds every key in the cache and builds none
        st, rep, route = dev.run(eng)
        cache(rep, pool, pool if call else 0, 0 if call else pool)
        keyed(route, N, pool)                             # bn254_debug_key_dedup_last: every item took the keyed kernel
        assert st == want, (pool, call)
    for other in (1, 0):                                  # the folded rows, then the line pairs, on the same cached rows
        opt(eng, "KEY_DEDUP_FOLD", other)
        st, rep, route = dev.run(eng)
        cache(rep, pool, pool, 0)
        keyed(route, N, pool)
        assert st == want, (pool, other)
    opt(eng, "KEY_DEDUP_FOLD", 2)
    opt(eng, "KEY_DEDUP_FORCE_GENERIC", 1)                # the generic loop, decided on the device
    st, rep, route = dev.run(eng)
    assert (route["ran"], route["keyed_n"], route["generic_n"]) == (1, 0, N), route
    assert st == want
    # (a pool of five has ONE ordinary key: its items alone are valid, a fifth of the batch)
    assert want.count(0) > (N // 8 if pool == 5 else N // 2) and want.count(9) > 0 and want.count(6) > 0
    if pool >= 5:
        assert want.count(4) > 0                          # the off-curve key and identity signatures


def test_option_range(eng):
    from bn254_amd import engine as E
    for value in (0, 1, 2):
        eng.set_option(E.OPT_KEY_DEDUP_FOLD, value)
    for value in (-1, 3):
        with pytest.raises(Exception):
            eng.set_option(E.OPT_KEY_DEDUP_FOLD, value)
