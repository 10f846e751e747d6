"""Proofs of possession on the GPU (include/bn254_hip.h: bn254_batch_pop_prove[_device], bn254_batch_pop_verify[_device]).
prove: byte for byte the composition of bn254_batch_g2_mul(NULL, sks, reduce) and bn254_batch_sign on TAG || pk, the oracle's bytes on the
golden vectors and on 16 random keys, the pinned results for sk == 0 (mod r) and sk >= r.  verify: byte for byte bn254_batch_verify on
host-composed messages with the subgroup flag forced — at n = 1, 63, 64, 65 and on both sides of every row of the default routing table,
with the planted faults of tests/pop_cases.py tiled through the batch; 18 items anchored on the oracle alone; host and _device forms; a
pending bn254_ctx_expect_msgs_len is neither consumed nor applied.  Run on the MI355X box: -m gpu."""
import json
import os

import pytest

from bn254_amd import engine as E
from tests import pop_cases as pc
from tests.datagen import sk_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
TAG = E.POP_TAG
N_MAX = 16385                                         # one past the last finite row of the default routing table


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def split(b, size):
    return [b[i:i + size] for i in range(0, len(b), size)]


@pytest.fixture(scope="module")
def proven(eng):
    """N_MAX keys with their proofs, made once on the device: (sks, pk list, pop list)"""
    sks = b"".join(sk_bytes(7000 + j) for j in range(N_MAX))
    pks, pops, st = eng.batch_pop_prove(sks)
    assert st == bytes(N_MAX)
    return sks, split(pks, 128), split(pops, 64)


@pytest.fixture(scope="module")
def planted(eng, proven, derived):
    sks, pks, pops = proven
    untagged, st = eng.batch_sign([pks[0]], sks[:32])
    assert st == bytes(1)
    return pc.planted(pks, pops, [untagged], bytes.fromhex(derived["g2_not_in_subgroup"]))


def test_prove_is_the_composition_of_key_derivation_and_sign(eng, proven):
    sks, pks, pops = proven
    n = 300                                            # several waves, not a multiple of one
    want_pks, st = eng.batch_g2_mul(None, sks[:32 * n], n, reduce_scalar=True)
    assert st == bytes(n) and b"".join(pks[:n]) == want_pks
    want_pops, st = eng.batch_sign([TAG + pk for pk in pks[:n]], sks[:32 * n])
    assert st == bytes(n) and b"".join(pops[:n]) == want_pops
    for k in (0, 1, 63, 64, 65):                       # the sizes of their own, n = 0 included
        got = eng.batch_pop_prove(sks[:32 * k])
        assert got == (b"".join(pks[:k]), b"".join(pops[:k]), bytes(k))


def test_prove_equals_the_oracle(eng, c):
    vs = json.load(open(os.path.join(ROOT, "tests", "golden", "pop_vectors.json")))["vectors"]
    sks = [bytes.fromhex(v["sk"]) for v in vs] + [sk_bytes(7100000 + j) for j in range(16)]
    pks, pops, st = eng.batch_pop_prove(b"".join(sks))
    assert st == bytes(len(sks))
    pks, pops = split(pks, 128), split(pops, 64)
    for v, pk, pop in zip(vs, pks, pops):
        assert pk.hex() == v["pk"] and pop.hex() == v["pop"]
    for sk, pk, pop in zip(sks, pks, pops):
        assert pk == c.public_key_g2(sk) and pop == c.sign(TAG + pk, sk)


def test_prove_pinned_scalars(eng, proven):
    """sk == 0 (mod r): the identity twice, status 0; sk >= r: the bytes of sk mod r (include/bn254_hip.h)"""
    sks, pks, pops = proven
    k = int.from_bytes(sks[:32], "big")
    assert k + R < 1 << 256
    got = eng.batch_pop_prove(bytes(32) + R.to_bytes(32, "big") + (k + R).to_bytes(32, "big") + (2 * R).to_bytes(32, "big"))
    assert got == (bytes(128) * 2 + pks[0] + bytes(128), bytes(64) * 2 + pops[0] + bytes(64), bytes(4))
    assert eng.batch_pop_verify(bytes(128), bytes(64), flags=0) == b"\x00"
    assert eng.batch_pop_verify(bytes(128), bytes(64), flags=E.FLAG_REJECT_IDENTITY) == b"\x04"


def test_planted_faults_anchored_on_the_oracle(eng, c, planted):
    """18 oracle verifies: every planted case with the subgroup check on, the identity cases also with the identity refused"""
    assert {cs.name for cs in planted} == set(pc.EXPECT)
    want0 = bytes(c.verify(pc.message(cs.pk), cs.pop, cs.pk, 1) for cs in planted)
    assert want0 == pc.expected(planted, 0), list(zip([cs.name for cs in planted], want0))
    ident = [cs for cs in planted if "identity" in cs.name]
    assert len(planted) + len(ident) == 18
    want2 = bytes(c.verify(pc.message(cs.pk), cs.pop, cs.pk, 3) for cs in ident)
    assert want2 == pc.expected(ident, 2)
    for f in (0, 2):
        got = eng.batch_pop_verify(b"".join(cs.pk for cs in planted), b"".join(cs.pop for cs in planted), flags=f)
        assert got == pc.expected(planted, f), (f, list(zip([cs.name for cs in planted], got)))


def route_sizes(eng):
    rows = [r[0] for r in eng.route_table() if r[0] < 1 << 63]
    assert rows == [1024, 1536, 3072, 16384], rows   # the default table (tests/test_abi.py::test_routing_table_rows)
    return [1, 63, 64, 65] + [n for r in rows for n in (r - 1, r, r + 1)]


def test_verify_equals_batch_verify_on_composed_messages(eng, proven, planted):
    _, pks, pops = proven
    for n in route_sizes(eng):
        k, p, at = pc.tile(planted, pks[:n], pops[:n], every=5 if n > 64 else 3)
        for f in ((0, 2) if n <= 1025 else (0,)):
            want = eng.batch_verify([TAG + x for x in k], b"".join(p), b"".join(k), flags=f | E.FLAG_G2_SUBGROUP_CHECK)
            got = eng.batch_pop_verify(b"".join(k), b"".join(p), flags=f)
            assert got == want, (n, f, [(i, got[i], want[i]) for i in range(n) if got[i] != want[i]][:8])
            assert all(got[i] == pc.EXPECT[cs.name][1 if f else 0] for i, cs in at.items()), (n, f)
            assert all(got[i] == 0 for i in range(n) if i not in at), (n, f)
            if f == 0:
                assert eng.batch_pop_verify(b"".join(k), b"".join(p), flags=E.FLAG_G2_SUBGROUP_CHECK) == want      # the flag is forced anyway


def test_verify_sliced(eng, proven, planted):
    _, pks, pops = proven
    n = 300
    k, p, _ = pc.tile(planted, pks[:n], pops[:n])
    want = eng.batch_pop_verify(b"".join(k), b"".join(p), flags=2)
    try:
        eng.set_option(E.OPT_MAX_CHUNK, 37)
        assert eng.batch_pop_verify(b"".join(k), b"".join(p), flags=2) == want
        sks = proven[0][:32 * n]
        assert eng.batch_pop_prove(sks) == (b"".join(pks[:n]), b"".join(pops[:n]), bytes(n))
    finally:
        eng.set_option(E.OPT_MAX_CHUNK, 0)


def test_device_forms_and_a_pending_msgs_len(eng, proven, planted):
    from bn254_amd.engine import pack_messages
    from tests.hip_ctypes import DevBuf, Stream
    sks, pks, pops = proven
    n = 130
    k, p, _ = pc.tile(planted, pks[:n], pops[:n])
    want = eng.batch_pop_verify(b"".join(k), b"".join(p), flags=2)
    assert set(want) >= {0, 4, 6, 9}
    stream, bufs = Stream(), []
    try:
        def dev(data=None, nbytes=None):
            b = DevBuf(len(data) if data is not None else nbytes, data=data, fill=None if data is not None else 0xEE)
            bufs.append(b)
            return b
        d_pks, d_pops, d_status = dev(b"".join(k)), dev(b"".join(p)), dev(nbytes=n)
        eng.batch_pop_verify_device(d_pks.ptr, d_pops.ptr, n, d_status.ptr, flags=2, stream=stream.handle)
        stream.synchronize()
        assert d_status.download(n) == want
        eng.batch_pop_verify_device(d_pks.ptr, d_pops.ptr, n, d_status.ptr, flags=2)          # the context's own stream
        eng.synchronize()
        assert d_status.download(n) == want
        with pytest.raises(Exception):
            eng.batch_pop_verify_device(d_pks.ptr + 1, d_pops.ptr, n, d_status.ptr)             # BN254_E_MISALIGNED
        # prove, device form
        d_sks, d_out_pks, d_out_pops, d_st = dev(sks[:32 * n]), dev(nbytes=128 * n), dev(nbytes=64 * n), dev(nbytes=n)
        eng.batch_pop_prove_device(d_sks.ptr, n, d_out_pks.ptr, d_out_pops.ptr, d_st.ptr, stream=stream.handle)
        stream.synchronize()
        assert (d_out_pks.download(128 * n), d_out_pops.download(64 * n), d_st.download(n)) == (b"".join(pks[:n]), b"".join(pops[:n]), bytes(n))
        # a declaration of ONE byte is pending: the proof calls neither apply nor consume it ...
        eng.expect_msgs_len(1)
        assert eng.batch_pop_verify(b"".join(k), b"".join(p), flags=2) == want
        eng.batch_pop_verify_device(d_pks.ptr, d_pops.ptr, n, d_status.ptr, flags=2, stream=stream.handle)
        stream.synchronize()
        assert d_status.download(n) == want
        eng.batch_pop_prove_device(d_sks.ptr, n, d_out_pks.ptr, d_out_pops.ptr, d_st.ptr, stream=stream.handle)
        stream.synchronize()
        assert d_st.download(n) == bytes(n) and d_out_pops.download(64 * n) == b"".join(pops[:n])
        # ... and it still bounds the caller's next hashing call: every message of 144 bytes runs past one byte
        blob, off = pack_messages([TAG + x for x in k])
        d_msgs, d_off = dev(bytes(blob)), dev(b"".join(int(x).to_bytes(8, "little") for x in off))
        eng.batch_verify_device(d_msgs.ptr, d_off.ptr, d_pops.ptr, d_pks.ptr, n, d_status.ptr, flags=3, stream=stream.handle)
        stream.synchronize()
        got = d_status.download(n)
        assert all(g == (5 if w in (0, 9) else w) for g, w in zip(got, want)), list(zip(got, want))[:12]
        assert got.count(5) >= n // 2
        eng.batch_verify_device(d_msgs.ptr, d_off.ptr, d_pops.ptr, d_pks.ptr, n, d_status.ptr, flags=3, stream=stream.handle)   # consumed
        stream.synchronize()
        assert d_status.download(n) == want
    finally:
        for b in bufs:
            b.free()
        stream.destroy()
