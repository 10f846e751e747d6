"""Registering a validator set together with its proofs of possession (include/bn254_hip.h: bn254_ctx_register_keys_pop,
bn254_mgpu_register_keys_pop) on the GPU.  The defining identity: key_status[j] = what bn254_ctx_register_keys reports for key j if that is
non-zero, else what bn254_batch_pop_verify reports for (pk_j, pop_j) under flags & REJECT_IDENTITY — on the mixed 46-key set of
tests/test_gpu_verify_keyed_bitmap.py with good proofs and every planted bad one, on all three branches of the keyed route, at the sizes
around a wave; and that byte IS the registration status: a key whose proof failed reads 9 in the keyed verify, the bitmap verify (the
lowest bad bit), a collect tuple, a merge tuple and a distinct-message keyed aggregate, while the proven keys verify.  The rogue-key attack
end to end: it forges under plain registration and is refused under this one.  Run on the MI355X box: -m gpu."""
import pytest

from bn254_amd import engine as E
from tests import pop_cases as pc
from tests.conftest import ws_default
from tests.datagen import D, sk_bytes

pytestmark = pytest.mark.gpu

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
TAG = E.POP_TAG
N_GOOD = 40
K_OFF_TWIST, K_OFF_SUB, K_BIG, K_IDENT, K_DUP0, K_NEG1 = range(N_GOOD, N_GOOD + 6)
N_KEYS = N_GOOD + 6


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


def split(b, size):
    return [b[i:i + size] for i in range(0, len(b), size)]


def prove(eng, sks):
    """sks: integers -> (sk bytes list, pk list, pop list)"""
    skb = [int(s).to_bytes(32, "big") for s in sks]
    pks, pops, st = eng.batch_pop_prove(b"".join(skb))
    assert st == bytes(len(sks))
    return skb, split(pks, 128), split(pops, 64)


def sign(eng, msgs, sks):
    sigs, st = eng.batch_sign(msgs, b"".join(int(s).to_bytes(32, "big") for s in sks))
    assert st == bytes(len(msgs))
    return split(sigs, 64)


@pytest.fixture(scope="module")
def mixed(eng, derived):
    """the 46-key set of the bitmap verify's tests — 40 good keys, then off the twist (4), outside the subgroup (4), a coordinate >= q (6),
    the identity, key 0 again and the negation of key 1 — with a good proof for every key that can have one: (sks, pks, pops)"""
    sks = [int.from_bytes(sk_bytes(500 + j), "big") % R for j in range(N_GOOD)]
    _, pks, pops = prove(eng, sks)
    off_twist = bytearray(pks[3]); off_twist[100] ^= 2
    big = bytearray(pks[5]); big[0] = 0xFF
    _, neg_pk, neg_pop = prove(eng, [R - sks[1]])
    pks = pks + [bytes(off_twist), bytes.fromhex(derived["g2_not_in_subgroup"]), bytes(big), bytes(128), pks[0], neg_pk[0]]
    # the refused keys come with the proof of the key they were made from; the identity key with the identity
    pops = pops + [pops[3], pops[4], pops[5], bytes(64), pops[0], neg_pop[0]]
    sks = sks + [0, 0, 0, 0, sks[0], R - sks[1]]
    assert list(eng.register_keys(b"".join(pks))) == [0] * N_GOOD + [4, 4, 6, 0, 0, 0]
    return sks, pks, pops


def identity(eng, pks, pops, flags):
    """key_status as the header defines it, from the two existing calls"""
    reg = eng.register_keys(b"".join(pks), flags=flags)
    ver = eng.batch_pop_verify(b"".join(pks), b"".join(pops), flags=flags & E.FLAG_REJECT_IDENTITY)
    return bytes(r if r else v for r, v in zip(reg, ver))


def bad_proofs(eng, mixed):
    """the mixed set's proofs with every planted bad proof on good keys, and a non-identity proof on the identity key"""
    sks, pks, pops = mixed
    untagged = sign(eng, [pks[10]], [sks[10]])[0]
    out = list(pops)
    out[7] = pops[8]                                   # another key's proof
    out[10] = untagged                                 # the signature on the key bytes without the tag
    out[12] = pc.off_curve(pops[12])
    out[13] = pc.coord(pops[13], 0, int.from_bytes(pops[13][:32], "big") + pc.Q)
    out[14] = bytes(64)                                # the identity proof
    out[15] = pc.neg(pops[15])
    out[K_IDENT] = pops[2]
    out[K_DUP0] = pops[1]                              # key 0 again, with key 1's proof: index 0 proven, index K_DUP0 not
    out[K_OFF_TWIST] = pc.off_curve(pops[3])           # both bad: the registration status wins
    return out


def test_key_status_is_the_defining_identity_on_the_mixed_set(eng, mixed):
    sks, pks, pops = mixed
    bad = bad_proofs(eng, mixed)
    for f in (0, E.FLAG_REJECT_IDENTITY):
        ident = 4 if f else 0
        want = identity(eng, pks, pops, f)
        assert list(want) == [0] * N_GOOD + [4, 4, 6, ident, 0, 0]
        assert eng.register_keys_pop(b"".join(pks), b"".join(pops), flags=f) == want and eng.n_registered_keys == N_KEYS
        want = identity(eng, pks, bad, f)
        exp = [0] * N_GOOD + [4, 4, 6, 4 if f else 9, 9, 0]
        exp[7], exp[10], exp[12], exp[13], exp[14], exp[15] = 9, 9, 4, 6, 4 if f else 9, 9
        assert list(want) == exp
        assert eng.register_keys_pop(b"".join(pks), b"".join(bad), flags=f) == want
        # the subgroup flag is not looked at, as in the plain call
        assert eng.register_keys_pop(b"".join(pks), b"".join(bad), flags=f | E.FLAG_G2_SUBGROUP_CHECK) == want


def route_at(eng, n):
    return next(r[1] for r in eng.route_table() if r[0] >= n)


def test_all_three_branches_of_the_keyed_route_at_65_keys(eng, mixed):
    sks, pks, pops = mixed
    bad = bad_proofs(eng, mixed)
    _, more_pks, more_pops = prove(eng, [int.from_bytes(sk_bytes(560 + j), "big") for j in range(65 - N_KEYS)])
    k, p = pks + more_pks, bad + more_pops
    assert len(k) == 65
    want = {f: identity(eng, k, p, f) for f in (0, 2)}
    seen = []
    try:
        for lm, trio in ((None, None), (0, None), (0, 0)):
            if lm is not None:
                eng.set_option(E.OPT_LM_MAX_BATCH, lm)
            if trio is not None:
                eng.set_option(E.OPT_TRIO_MAX_BATCH, trio)
            seen.append(route_at(eng, 65))
            for f in (0, 2):
                assert eng.register_keys_pop(b"".join(k), b"".join(p), flags=f) == want[f], (lm, trio, f)
    finally:
        eng.set_option(E.OPT_LM_MAX_BATCH, ws_default("LM_MAX_BATCH_DEFAULT"))
        eng.set_option(E.OPT_TRIO_MAX_BATCH, ws_default("TRIO_MAX_BATCH_DEFAULT"))
    assert seen[0] == 0 and seen[1] not in (0, 2) and seen[2] == 2, seen      # lane machine, small-batch kernels on expanded keys, lane pairs


def test_sizes_capacity_null_status_and_argument_errors(eng, mixed):
    sks, pks, pops = mixed
    lib, h = eng._lib, eng._h
    _, more_pks, more_pops = prove(eng, [int.from_bytes(sk_bytes(600 + j), "big") for j in range(90)])
    k, p = pks[:N_GOOD] + more_pks, pops[:N_GOOD] + more_pops
    p[0], p[63], p[64] = p[1], p[62], p[65]                                    # an unproven key at both ends of the first wave, and behind it
    for n in (1, 64, 65, 0):
        want = identity(eng, k[:n], p[:n], 2)
        assert eng.register_keys_pop(b"".join(k[:n]), b"".join(p[:n]), flags=2) == want and eng.n_registered_keys == n
        assert list(want) == [9 if j in (0, 63, 64) else 0 for j in range(n)]
    # nothing registered: every keyed item is out of range
    msgs = [D("pop/none", i) for i in range(3)]
    assert eng.batch_verify_keyed(msgs, b"".join(sign(eng, msgs, sks[:3])), [0, 1, 2]) == b"\x02\x02\x02"
    # a registration that grows the tables: a fresh context holds none, then 3 keys, then 130
    import bn254_amd
    fresh = bn254_amd.Engine(0)
    try:
        assert fresh.register_keys_pop(b"".join(k[:3]), b"".join(p[:3]), flags=2) == b"\x09\x00\x00"
        assert fresh.register_keys_pop(b"".join(k), b"".join(p), flags=2) == identity(eng, k, p, 2)
        m130 = [D("pop/grow", i) for i in range(len(k))]
        s130 = b"".join(sign(eng, m130, [int.from_bytes(sk_bytes(500 + j), "big") % R for j in range(N_GOOD)] +
                             [int.from_bytes(sk_bytes(600 + j), "big") for j in range(90)]))
        got = fresh.batch_verify_keyed(m130, s130, list(range(len(k))))
        assert list(got) == [9 if j in (0, 63, 64) else 0 for j in range(len(k))]
    finally:
        fresh.close()
    # key_status = NULL
    assert eng.register_keys_pop(b"".join(k[:5]), b"".join(p[:5]), flags=2) == b"\x09\x00\x00\x00\x00"
    assert lib.bn254_ctx_register_keys_pop(h, b"".join(k[:4]), b"".join(p[:4]), 4, 2, None) == 0
    m4 = [D("pop/null", i) for i in range(5)]
    s4 = b"".join(sign(eng, m4, sks[:5]))
    assert eng.batch_verify_keyed(m4, s4, [0, 1, 2, 3, 4]) == b"\x09\x00\x00\x00\x02"       # four keys stand, the first unproven
    # pops = NULL (and pks = NULL): BN254_E_BAD_ARGUMENT before anything is touched — the previous set stays
    assert lib.bn254_ctx_register_keys_pop(h, b"".join(k[:2]), None, 2, 2, None) == -10001
    assert lib.bn254_ctx_register_keys_pop(h, None, b"".join(p[:2]), 2, 2, None) == -10001
    assert lib.bn254_ctx_register_keys_pop(None, b"".join(k[:2]), b"".join(p[:2]), 2, 2, None) == -10001
    assert eng.batch_verify_keyed(m4, s4, [0, 1, 2, 3, 4]) == b"\x09\x00\x00\x00\x02"


def words(bits, bm_words=1):
    w = [0] * bm_words
    for j in bits:
        w[j // 32] |= 1 << (j % 32)
    return w


def g1_sum(eng, sigs):
    out, st = eng.batch_g1_sum(b"".join(sigs), [0, len(sigs)])
    assert st == b"\x00"
    return out


def test_an_unproven_key_is_refused_by_every_keyed_call(eng, mixed):
    sks, pks, pops = mixed
    # keys: good, good, GOOD KEY WITH ANOTHER KEY'S PROOF, off the twist, good
    k = [pks[0], pks[1], pks[2], pks[K_OFF_TWIST], pks[4]]
    p = [pops[0], pops[1], pops[9], pops[3], pops[4]]
    s = [sks[0], sks[1], sks[2], 0, sks[4]]
    assert eng.register_keys_pop(b"".join(k), b"".join(p), flags=2) == b"\x00\x00\x09\x04\x00"
    m = D("pop/downstream", 0)
    share = sign(eng, [m] * 5, [x or 1 for x in s])
    # keyed verify
    assert eng.batch_verify_keyed([m] * 5, b"".join(share), [0, 1, 2, 3, 4]) == b"\x00\x00\x09\x04\x00"
    # bitmap verify: the lowest bad bit
    tuples = [([0, 1, 4], [0, 1, 4]), ([1, 2, 4], [1, 2, 4]), ([2, 3], [2]), ([3], [4]), ([3, 4], [4]), ([2], [2])]
    sig = b"".join(g1_sum(eng, [share[j] for j in signers]) for _, signers in tuples)
    bits = [x for b, _ in tuples for x in words(b)]
    assert eng.batch_verify_keyed_bitmap([m] * len(tuples), sig, bits, 1) == b"\x00\x09\x09\x04\x04\x09"
    assert eng.batch_verify_keyed_bitmap_randomized([m] * len(tuples), sig, bits, 1, bytes(range(32))) == b"\x00\x09\x09\x04\x04\x09"
    # one collect tuple: the shares of keys 0, 1, 2, 4
    share_st, tuple_st, agg, rows = eng.batch_collect_keyed_bitmap([m], b"".join(share[j] for j in (0, 1, 2, 4)), [0, 1, 2, 4], [4], 1)
    assert (share_st, tuple_st, rows) == (b"\x00\x00\x09\x00", b"\x00", words([0, 1, 4]))
    assert agg == g1_sum(eng, [share[0], share[1], share[4]])
    # one merge tuple: partials {0, 1}, {2}, {4}
    parts = [g1_sum(eng, [share[0], share[1]]), share[2], share[4]]
    part_st, taken, tuple_st, agg, rows = eng.merge_keyed_bitmap([m], b"".join(parts), words([0, 1]) + words([2]) + words([4]), [3], 1)
    assert (part_st, taken, tuple_st, rows) == (b"\x00\x09\x00", b"\x01\x00\x01", b"\x00", words([0, 1, 4]))
    # one distinct-message keyed aggregate with the unproven key, one without
    dm = [D("pop/distinct", i) for i in range(5)]
    ds = sign(eng, dm, [x or 1 for x in s])
    aggs = g1_sum(eng, [ds[0], ds[1], ds[2]]) + g1_sum(eng, [ds[0], ds[1], ds[4]])
    assert eng.batch_aggregate_verify_distinct_keyed(dm[:3] + [dm[0], dm[1], dm[4]], [0, 1, 2, 0, 1, 4], aggs, [3, 3]) == b"\x09\x00"


def test_no_stale_state_across_registrations(eng, mixed):
    sks, pks, pops = mixed
    k, p = pks[:6], pops[:6]
    m = D("pop/stale", 0)
    share = sign(eng, [m] * 6, sks[:6])
    tuples = [[0, 1, 2], [3, 4, 5], [2, 3]]
    sig = b"".join(g1_sum(eng, [share[j] for j in t]) for t in tuples)
    bits = [x for t in tuples for x in words(t)]
    assert eng.register_keys_pop(b"".join(k), b"".join(p), flags=2) == bytes(6)
    assert eng.batch_verify_keyed_bitmap([m] * 3, sig, bits, 1) == b"\x00\x00\x00"      # builds the bad-bit vector and the subset tables
    swapped = list(p)
    swapped[4] = p[5]
    assert eng.register_keys_pop(b"".join(k), b"".join(swapped), flags=2) == b"\x00\x00\x00\x00\x09\x00"
    assert eng.batch_verify_keyed_bitmap([m] * 3, sig, bits, 1) == b"\x00\x09\x00"      # the vector followed
    assert eng.register_keys(b"".join(k)) == bytes(6)                                     # plain registration accepts the key again
    assert eng.batch_verify_keyed_bitmap([m] * 3, sig, bits, 1) == b"\x00\x00\x00"


def test_the_rogue_key_attack_end_to_end(eng):
    """pk* = a G2 - pk_v: under plain registration a H(m) verifies as "victim and attacker signed m"; registered with proofs the attacker's
    key is refused — its holder knows no secret for it, the best available proof a H(TAG || pk*) does not verify"""
    sk_v, a = int.from_bytes(sk_bytes(9001), "big"), int.from_bytes(sk_bytes(9002), "big")
    _, (pk_v,), (pop_v,) = prove(eng, [sk_v])
    a_g2, st = eng.batch_g2_mul(None, a.to_bytes(32, "big"), 1, reduce_scalar=True)
    assert st == b"\x00"
    rogue, st = eng.batch_g2_add(a_g2, pc.neg(pk_v), 1)
    assert st == b"\x00" and rogue not in (pk_v, a_g2, bytes(128))
    keys = pk_v + rogue
    m = b"transfer everything to the attacker"
    forged, honest = sign(eng, [m, m], [a, sk_v])
    both, victim = words([0, 1]), words([0])
    # today's behaviour, which states the hole
    assert eng.register_keys(keys) == b"\x00\x00"
    assert eng.batch_verify_keyed_bitmap([m], forged, both, 1) == b"\x00"
    # with proofs
    best = sign(eng, [TAG + rogue], [a])[0]
    assert eng.register_keys_pop(keys, pop_v + best, flags=2) == b"\x00\x09"
    assert eng.batch_verify_keyed_bitmap([m, m], forged + honest, both + victim, 1) == b"\x09\x00"
    assert eng.batch_verify_keyed_bitmap([m], forged, words([1]), 1) == b"\x09"


def test_mgpu_registers_on_every_device(eng, mixed):
    import bn254_amd
    sks, pks, pops = mixed
    bad = bad_proofs(eng, mixed)
    mg = bn254_amd.MultiEngine([0, 0, 0, 0])
    try:
        for f in (0, 2):
            want = eng.register_keys_pop(b"".join(pks), b"".join(bad), flags=f)
            assert mg.register_keys_pop(b"".join(pks), b"".join(bad), flags=f) == want
        n = 4 * N_GOOD                                   # every device's shard meets proven and unproven keys
        msgs = [D("pop/mgpu", i) for i in range(n)]
        idx = [i % N_GOOD for i in range(n)]
        sigs = b"".join(sign(eng, msgs, [sks[j] for j in idx]))
        got = mg.batch_verify_keyed(msgs, sigs, idx)
        assert got == eng.batch_verify_keyed(msgs, sigs, idx)
        assert list(got) == [{7: 9, 10: 9, 12: 4, 13: 6, 14: 4, 15: 9}.get(j, 0) for j in idx]
        assert eng._lib.bn254_mgpu_register_keys_pop(mg._h, b"".join(pks), None, N_KEYS, 0, None) == -10001
    finally:
        mg.close()


def test_python_mirrors(eng):
    from bn254_amd.api import ECDSA, Error, ErrorKind, PrivateKey, PublicKey, Signature
    ks = [PrivateKey.try_from(sk_bytes(9100 + j)) for j in range(3)]
    pks = [PublicKey.from_private_key(k) for k in ks]
    proofs = [k.prove_possession() for k in ks]
    for k, pk, proof in zip(ks, pks, proofs):
        assert isinstance(proof, Signature) and proof.raw == ECDSA.sign(TAG + pk.raw, k).raw
        assert pk.verify_possession(proof) is None
    with pytest.raises(Error) as e:
        pks[0].verify_possession(proofs[1])
    assert e.value.kind == ErrorKind.VerificationFailed
    with pytest.raises(Error) as e:
        pks[0].verify_possession(Signature(bytes(64)))
    assert e.value.kind == ErrorKind.InvalidGroupPoint
    with pytest.raises(Error) as e:
        PublicKey(bytes(128)).verify_possession(Signature(bytes(64)))
    assert e.value.kind == ErrorKind.InvalidGroupPoint
    bad = Signature(pc.coord(proofs[2].raw, 0, int.from_bytes(proofs[2].raw[:32], "big") + pc.Q))
    assert ECDSA.batch_verify_possession(pks, [proofs[0], proofs[0], bad], engine=eng) == [None, Error(ErrorKind.VerificationFailed), Error(ErrorKind.NotMemberError)]
    with pytest.raises(Error) as e:
        ECDSA.batch_verify_possession(pks, proofs[:2], engine=eng)
    assert e.value.kind == ErrorKind.InvalidLength
    assert ECDSA.register_keys_proven(pks, proofs, engine=eng) == [None, None, None]
    assert ECDSA.register_keys_proven(pks, [proofs[0], proofs[2], proofs[2]], engine=eng) == [None, Error(ErrorKind.VerificationFailed), None]
    m = [D("pop/api", i) for i in range(3)]
    sigs = [ECDSA.sign(m[i], ks[i]) for i in range(3)]
    assert ECDSA.batch_verify_keyed(m, sigs, [0, 1, 2], engine=eng) == [None, Error(ErrorKind.VerificationFailed), None]
    with pytest.raises(Error) as e:
        ECDSA.register_keys_proven(pks, proofs[:2], engine=eng)
    assert e.value.kind == ErrorKind.InvalidLength


def test_cpp_example(tmp_path):
    """host/pop_example.cpp builds with -Wall -Werror against the library and prints success"""
    import os
    import subprocess
    from bn254_amd import _native
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "pop_example")
    host = os.path.join(root, "bn254_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "include"), "-I", host,
                           os.path.join(host, "pop_example.cpp"), "-o", exe, _native.LIB_PATH, "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "proofs of possession: ok" in out.stdout
