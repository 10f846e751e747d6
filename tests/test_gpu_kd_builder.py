"""The key-table builder of the exact verify's key dedup (k_kd_lines: the lane machine's wave-T program, three keys per wave) on the device:
for pools of 1 and 2 keys, a pool whose last wave is partly empty, 256 and 1 024 keys (KEY_DEDUP_MAX_KEYS), with refused keys (x >= q, off
the curve), identity keys and keys outside G2 mixed in, the dedup route runs the keyed Miller loop and every status byte equals the generic
route's (KEY_DEDUP_FORCE_GENERIC) and the oracle's."""
import pytest

from tests.test_gpu_key_dedup import Q, key_pool, make_batch, verify_device

pytestmark = pytest.mark.gpu

N = 16385                      # the first lane-pair size; 1 024 keys x the default minimum multiplicity 16 <= N


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


def mixed_batch(eng, derived, kinds):
    """N items over len(kinds) keys (item i uses key i % len(kinds)); key j is a valid key or, by kinds[j], one outside G2 ("off", "off3": its triple), one
    with x >= q ("big"), one off the curve ("curve") or the identity ("inf")"""
    pool = len(kinds)
    msgs, sigs, pks = make_batch(eng, N, pool)
    _, pk = key_pool(eng, pool)
    keys = [bytearray(pk[128 * j:128 * j + 128]) for j in range(pool)]
    for j, k in enumerate(kinds):
        if k == "off":
            keys[j] = bytearray(bytes.fromhex(derived["g2_not_in_subgroup"]))
        elif k == "off3":
            from oracle import bn254_model as M
            off = M.g2_from_uncompressed(bytes.fromhex(derived["g2_not_in_subgroup"]), subgroup_check=False)
            keys[j] = bytearray(M.g2_to_uncompressed(M.g2_mul(off, 3)))
        elif k == "big":
            keys[j][0:32] = Q.to_bytes(32, "big")
        elif k == "curve":
            keys[j][127] ^= 1
        elif k == "inf":
            keys[j] = bytearray(128)
    return msgs, sigs, b"".join(bytes(keys[i % pool]) for i in range(N))


POOLS = {
    "1_ok": ["ok"],
    "1_inf": ["inf"],
    "1_off": ["off"],
    "2": ["ok", "off"],
    "5_partial_wave": ["ok", "big", "ok", "inf", "curve"],
    "256": ["ok"] * 256,
    "1024": ["ok"] * 1024,
}


@pytest.mark.parametrize("name", list(POOLS))
def test_builder_pools_vs_generic_and_oracle(eng, derived, name):
    from oracle import c_oracle
    kinds = list(POOLS[name])
    if len(kinds) >= 256:                               # invalid keys of every kind among the valid ones, one of them in the last wave
        for j, k in zip((1, 2, 3, 4, len(kinds) - 1), ("off", "big", "curve", "inf", "off3")):
            kinds[j] = k
    msgs, sigs, pks = mixed_batch(eng, derived, kinds)
    for flags in (0, 1):
        got = verify_device(eng, msgs, sigs, pks, flags)
        assert verify_device.route == dict(ran=1, keys=len(kinds), flags=0, keyed_n=N, generic_n=0), (name, flags, verify_device.route)
        generic = verify_device(eng, msgs, sigs, pks, flags, KEY_DEDUP_FORCE_GENERIC=1)
        assert (verify_device.route["keyed_n"], verify_device.route["generic_n"]) == (0, N)
        assert got == generic, (name, flags)
        if flags == 0:
            want, _ = c_oracle.batch_verify(msgs, sigs, pks, flags=flags, nthreads=16)
            assert got == want, name
    if "ok" in kinds:
        assert got.count(0) > 0 and got.count(9) > 0
