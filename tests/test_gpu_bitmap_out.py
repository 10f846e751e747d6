"""What the signer-bitmap calls return besides a status byte (include/bn254_hip.h: bn254_batch_aggregate_keys_bitmap[_device],
bn254_batch_verify_keyed_bitmap_export[_device], bn254_ctx_set_key_weights, bn254_batch_bitmap_weights[_device]) on the GPU, over the case
set of tests/bitmap_out_cases.py.  Aggregate keys and hashes are checked against the oracle's g2_add and hash_to_g1 and against the
defining identity with bn254_batch_g2_sum, on every route of the sum; the export call's status bytes against the plain bitmap verify at
every boundary of the routing table; the weights against Python integers.  Run on the MI355X box: -m gpu."""
import os
import random
import struct
import subprocess

import pytest

from bn254_amd import engine as E
from tests import bitmap_out_cases as B
from tests.conftest import ws_default
from tests.datagen import D, sk_bytes

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, MISALIGNED = -10001, -10002


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    return B.oracle()


@pytest.fixture(scope="module")
def keyset(derived):
    return B.keyset(derived["g2_not_in_subgroup"])


@pytest.fixture()
def registered(eng, keyset):
    """the case set's keys registered (every test starts from them, whatever the one before left)"""
    assert list(eng.register_keys(b"".join(keyset[1]))) == B.REG_STATUS
    return keyset


DEFAULTS = {E.OPT_BITMAP_ROUTE: 0, E.OPT_BITMAP_TABLE_MAX_KEYS: ws_default("BITMAP_TABLE_MAX_KEYS_DEFAULT"), E.OPT_PAIR_LANES: 1, E.OPT_MAX_CHUNK: 0,
            E.OPT_HASH_MAX_TRIES: 0}
# the four routes of the sum, then the size rule on its far side and slices
ROUTES = [("tables_pair", {E.OPT_BITMAP_ROUTE: 1}), ("keys_pair", {E.OPT_BITMAP_ROUTE: 2}), ("tables_lane", {E.OPT_BITMAP_ROUTE: 1, E.OPT_PAIR_LANES: 0}),
          ("keys_lane", {E.OPT_BITMAP_ROUTE: 2, E.OPT_PAIR_LANES: 0}), ("over_limit", {E.OPT_BITMAP_TABLE_MAX_KEYS: B.N_KEYS - 1}), ("default", {}),
          ("sliced", {E.OPT_MAX_CHUNK: 7})]


def with_options(eng, opts, fn):
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            eng.set_option(k, DEFAULTS[k])


def words(rows, bm_words):
    return [x for bits in rows for x in B.to_words(bits, bm_words)]


def u32(v):
    return struct.pack("<%dI" % len(v), *v)


def rc_of(fn):
    with pytest.raises(E.NativeError) as e:
        fn()
    return e.value.rc


class Dev:
    """device buffers and a caller's stream, freed together"""

    def __init__(self):
        from tests.hip_ctypes import Stream
        self.bufs, self.stream = [], Stream()

    def buf(self, nbytes=0, data=None, fill=None):
        from tests.hip_ctypes import DevBuf
        b = DevBuf(len(data) if data is not None else nbytes, data=data, fill=fill)
        self.bufs.append(b)
        return b

    def close(self):
        for b in self.bufs:
            b.free()
        self.stream.destroy()


@pytest.fixture()
def dev():
    d = Dev()
    yield d
    d.close()


# ---- A: aggregate keys ---------------------------------------------------------------------------------------------------------------------------

def expect_keys(pks, rows, bm_words, reg=B.REG_STATUS):
    want = [B.aggregate_key(pks, bits, bm_words, reg) for bits in rows]
    return b"".join(k for _, k in want), bytes(s for s, _ in want)


def test_aggregate_keys_oracle_and_g2_sum_identity_every_route(eng, registered):
    sks, pks = registered
    rows = [bits for _, bits in B.rows()]
    for bm_words in B.BM_WORDS:
        want_keys, want_st = expect_keys(pks, rows, bm_words)
        if bm_words == 3:
            assert set(want_st) == {0, 2, 4, 6}
        for name, opts in ROUTES:
            keys, st = with_options(eng, opts, lambda: eng.batch_aggregate_keys_bitmap(words(rows, bm_words), bm_words, len(rows)))
            assert st == want_st, (name, bm_words, list(st), list(want_st))
            assert keys == want_keys, (name, bm_words, [i for i in range(len(rows)) if keys[128 * i:128 * i + 128] != want_keys[128 * i:128 * i + 128]])
        # the defining identity: one segment per status-0 row, the registered encodings of its set keys in ascending order
        ok = [i for i in range(len(rows)) if want_st[i] == 0]
        segs, off = [], [0]
        for i in ok:
            held = B.held(rows[i], bm_words)
            segs += [pks[j] for j in held]
            off.append(off[-1] + len(held))
        sums, sum_st = eng.batch_g2_sum(b"".join(segs), off)
        assert sum_st == bytes(len(ok))
        keys, _ = eng.batch_aggregate_keys_bitmap(words(rows, bm_words), bm_words, len(rows))
        assert b"".join(keys[128 * i:128 * i + 128] for i in ok) == sums, bm_words
    assert eng.batch_aggregate_keys_bitmap([], 2, 0) == (b"", b"")
    # bm_words = 0 with a NULL bitmap
    keys = E.ctypes.create_string_buffer(256)
    st = E.ctypes.create_string_buffer(2)
    assert eng._lib.bn254_batch_aggregate_keys_bitmap(eng._h, None, 0, 2, 0, keys, st) == 0 and keys.raw == bytes(256) and st.raw == bytes(2)


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 129])
def test_aggregate_keys_both_sides_of_a_wave_host_and_device(eng, registered, dev, n):
    """n rows around the wave boundaries of both layouts (64 rows a wave with one lane per row, 32 on lane pairs), host and _device forms on
    the four routes; the _device form writes into buffers pre-filled with 0xA5, also in slices"""
    sks, pks = registered
    base = [bits for _, bits in B.rows()]
    rows = [base[(5 * i + i // len(base)) % len(base)] for i in range(n)]
    want_keys, want_st = expect_keys(pks, rows, 2)
    d_bits = dev.buf(data=u32(words(rows, 2)))
    for name, opts in ROUTES[:4] + ROUTES[-1:]:
        def call():
            d_keys, d_st = dev.buf(128 * n, fill=0xA5), dev.buf(n, fill=0xA5)
            eng.batch_aggregate_keys_bitmap_device(d_bits.ptr, 2, n, d_keys.ptr, d_st.ptr, stream=dev.stream.handle)
            dev.stream.synchronize()
            return eng.batch_aggregate_keys_bitmap(words(rows, 2), 2, n), (d_keys.download(), d_st.download())
        host, device = with_options(eng, opts, call)
        assert host == (want_keys, want_st) == device, (name, n)


def test_aggregate_keys_after_reregistration_and_without_keys(eng, registered, c):
    """a set registered between two calls takes effect (stale subset tables would give the old sums); with no keys any set bit gives 2"""
    sks, pks = registered
    rows = [bits for _, bits in B.rows()]
    first = eng.batch_aggregate_keys_bitmap(words(rows, 2), 2, len(rows))
    assert first == expect_keys(pks, rows, 2)
    rot = list(pks[1:B.N_GOOD] + pks[:1] + pks[B.N_GOOD:])
    rot[B.K_DUP0], rot[B.K_NEG1] = pks[7], pks[8]
    assert list(eng.register_keys(b"".join(rot))) == B.REG_STATUS
    for name, opts in ROUTES[:2]:
        got = with_options(eng, opts, lambda: eng.batch_aggregate_keys_bitmap(words(rows, 2), 2, len(rows)))
        assert got == expect_keys(rot, rows, 2) and got != first, name
    reg = list(eng.register_keys(b"".join(pks[:8])))                     # a smaller set: bits 8.. are out of range now
    assert eng.batch_aggregate_keys_bitmap(words(rows, 2), 2, len(rows)) == expect_keys(pks[:8], rows, 2, reg)
    eng.register_keys(b"")
    for bm_words in (2, 0):
        keys, st = eng.batch_aggregate_keys_bitmap(words(rows, bm_words), bm_words, len(rows))
        assert keys == bytes(128 * len(rows)) and list(st) == [2 if B.held(bits, bm_words) else 0 for bits in rows]


def test_aggregate_keys_refused_arguments(eng, registered, dev):
    n = 3
    d_bits, d_keys, d_st = dev.buf(data=u32([1, 0] * n) + bytes(4)), dev.buf(128 * n + 4), dev.buf(n)
    assert rc_of(lambda: eng.batch_aggregate_keys_bitmap([1, 0] * n, 2, n, flags=1)) == BAD_ARGUMENT
    assert rc_of(lambda: eng.batch_aggregate_keys_bitmap_device(d_bits.ptr, 2, n, d_keys.ptr, d_st.ptr, flags=2)) == BAD_ARGUMENT
    assert rc_of(lambda: eng.batch_aggregate_keys_bitmap_device(d_bits.ptr + 1, 2, n, d_keys.ptr, d_st.ptr)) == MISALIGNED
    assert rc_of(lambda: eng.batch_aggregate_keys_bitmap_device(d_bits.ptr, 2, n, d_keys.ptr + 2, d_st.ptr)) == MISALIGNED
    for args in ((None, 2, n, d_keys.ptr, d_st.ptr), (d_bits.ptr, 2, n, None, d_st.ptr), (d_bits.ptr, 2, n, d_keys.ptr, None)):
        assert rc_of(lambda: eng.batch_aggregate_keys_bitmap_device(*args)) == BAD_ARGUMENT
    eng.batch_aggregate_keys_bitmap_device(None, 0, n, d_keys.ptr, d_st.ptr)     # bm_words = 0: no bitmap to read
    eng.batch_aggregate_keys_bitmap_device(None, 2, 0, None, None)               # n = 0 returns 0
    eng.synchronize()
    assert d_keys.download(128 * n) == bytes(128 * n) and d_st.download() == bytes(n)


# ---- B: the verify that returns what it computed -------------------------------------------------------------------------------------------------

def export_call(eng, tuples, bm_words=2, flags=0, sigs=None, **kw):
    return eng.batch_verify_keyed_bitmap_export([t[0] for t in tuples], sigs if sigs is not None else b"".join(t[1] for t in tuples),
                                                words([t[2] for t in tuples], bm_words), bm_words, flags=flags, **kw)


def verify_call(eng, tuples, bm_words=2, flags=0, sigs=None):
    return eng.batch_verify_keyed_bitmap([t[0] for t in tuples], sigs if sigs is not None else b"".join(t[1] for t in tuples),
                                         words([t[2] for t in tuples], bm_words), bm_words, flags=flags)


def expect_export(tuples, pks, flags, hash_max_tries=B.HASH_MAX_TRIES):
    st = [B.export_status(t, pks, flags, hash_max_tries=hash_max_tries) for t in tuples]
    outs = [B.export_outputs(t, pks, s) for t, s in zip(tuples, st)]
    return bytes(st), b"".join(h for h, _ in outs), b"".join(k for _, k in outs)


def test_export_outputs_against_the_oracle(eng, registered, derived, dev):
    """every row with a valid, a wrong, an undecodable and the identity sigma, and a message that does not hash within 3 counters: statuses
    by construction, H(m) and the aggregate key from the oracle where the status is 0 or 9, zeros elsewhere — flags 0 and REJECT_IDENTITY,
    the routes of the sum, each output pointer NULL in turn, the _device form into 0xA5-filled buffers, and the plain verify afterwards"""
    sks, pks = registered
    tuples = list(B.export_tuples(derived["g2_not_in_subgroup"]))
    n = len(tuples)
    for flags in (0, B.FLAG_REJECT_IDENTITY):
        want = expect_export(tuples, pks, flags)
        assert {0, 1, 2, 4, 6, 9} <= set(want[0])
        for name, opts in ROUTES if flags == 0 else ROUTES[:1]:
            got = with_options(eng, {**opts, E.OPT_HASH_MAX_TRIES: B.HASH_MAX_TRIES}, lambda: export_call(eng, tuples, flags=flags))
            assert got[0] == want[0], (name, flags, [(i, g, w, tuples[i][3]) for i, (g, w) in enumerate(zip(got[0], want[0])) if g != w][:8])
            assert got[1] == want[1] and got[2] == want[2], (name, flags)
        got = with_options(eng, {E.OPT_HASH_MAX_TRIES: B.HASH_MAX_TRIES}, lambda: verify_call(eng, tuples, flags=flags))
        assert got == want[0], flags                                     # a following plain bitmap verify still returns its bytes
    want = expect_export(tuples, pks, 0, hash_max_tries=0)              # the reference's 255 counters: the message hashes
    assert want[0][-1] == 0 and want[1][-64:] != bytes(64)
    assert export_call(eng, tuples) == want
    assert export_call(eng, tuples, want_hashes=False) == (want[0], None, want[2])
    assert export_call(eng, tuples, want_keys=False) == (want[0], want[1], None)
    assert export_call(eng, tuples, want_hashes=False, want_keys=False) == (want[0], None, None) and verify_call(eng, tuples) == want[0]
    # the _device form on a caller's stream, whole and in slices
    blob, off = E.pack_messages([t[0] for t in tuples])
    d_msgs, d_off = dev.buf(data=bytes(blob)), dev.buf(data=struct.pack("<%dQ" % (n + 1), *off))
    d_sigs, d_bits = dev.buf(data=b"".join(t[1] for t in tuples) + bytes(4)), dev.buf(data=u32(words([t[2] for t in tuples], 2)))
    for opts in ({}, {E.OPT_MAX_CHUNK: 10}):
        d_st, d_h, d_k = dev.buf(n, fill=0xA5), dev.buf(64 * n + 4, fill=0xA5), dev.buf(128 * n + 4, fill=0xA5)
        with_options(eng, opts, lambda: eng.batch_verify_keyed_bitmap_export_device(d_msgs.ptr, d_off.ptr, d_sigs.ptr, d_bits.ptr, 2, n, d_st.ptr, d_h.ptr, d_k.ptr,
                                                                                    stream=dev.stream.handle))
        dev.stream.synchronize()
        assert (d_st.download(), d_h.download(64 * n), d_k.download(128 * n)) == want, opts
    assert rc_of(lambda: eng.batch_verify_keyed_bitmap_export_device(d_msgs.ptr, d_off.ptr, d_sigs.ptr, d_bits.ptr, 2, n, d_st.ptr, d_h.ptr + 2, d_k.ptr)) == MISALIGNED
    assert rc_of(lambda: eng.batch_verify_keyed_bitmap_export_device(d_msgs.ptr, d_off.ptr, d_sigs.ptr, d_bits.ptr, 2, n, d_st.ptr, d_h.ptr, d_k.ptr + 1)) == MISALIGNED
    assert rc_of(lambda: eng.batch_verify_keyed_bitmap_export_device(d_msgs.ptr, d_off.ptr, d_sigs.ptr, d_bits.ptr, 2, n, None, d_h.ptr, d_k.ptr)) == BAD_ARGUMENT


def test_export_compressed_sigmas(eng, registered, derived, c):
    """BN254_FLAG_G1_COMPRESSED: the decodable sigmas of the case set as 33-byte encodings, one of them with a bad prefix (3: outputs zero)"""
    sks, pks = registered
    tuples = [t for t in B.export_tuples(derived["g2_not_in_subgroup"]) if c.g1_validate(t[1], B.FLAG_REJECT_IDENTITY) == 0]
    enc = [c.g1_compress(t[1]) for t in tuples]
    bad = next(i for i, t in enumerate(tuples) if t[3] == "valid" and B.rule2(t[2], 2) == 0)
    enc[bad] = b"\x04" + enc[bad][1:]
    st = [B.export_status(t, pks, 0, hash_max_tries=0) for t in tuples]
    st[bad] = B.ST_ENCODING
    outs = [B.export_outputs(t, pks, s) for t, s in zip(tuples, st)]
    want = (bytes(st), b"".join(h for h, _ in outs), b"".join(k for _, k in outs))
    assert {0, 2, 3, 4, 6, 9} <= set(st)
    for opts in ({}, {E.OPT_MAX_CHUNK: 9}, {E.OPT_BITMAP_ROUTE: 2, E.OPT_PAIR_LANES: 0}):
        got = with_options(eng, opts, lambda: export_call(eng, tuples, flags=E.FLAG_G1_COMPRESSED, sigs=b"".join(enc)))
        assert got == want, opts
    assert verify_call(eng, tuples, flags=E.FLAG_G1_COMPRESSED, sigs=b"".join(enc)) == want[0]


@pytest.fixture(scope="module")
def many(eng, keyset, c):
    """enough tuples for the last row of the routing table: popcounts 1..3 over the good keys, every 5th sigma wrong, every 11th a refused
    key, every 13th sigma undecodable; signed on the device (the statuses are compared with the plain verify's, not derived).  Returns
    (tuples, their sigmas as 33-byte encodings: an undecodable sigma becomes an encoding with a bad prefix)"""
    sks, pks = keyset
    top = max(r[0] for r in eng.route_table()[:-1]) + 2
    rnd = random.Random(11)
    sets = [sorted(rnd.sample(range(B.N_GOOD), 1 + i % 3)) for i in range(top)]
    msgs = [D("bmo/many", i) for i in range(top)]
    sk_sums = [(sum(sks[j] for j in s) + (1 if i % 5 == 0 else 0)) % B.R or 1 for i, s in enumerate(sets)]
    sigs, st = eng.batch_sign(msgs, b"".join(s.to_bytes(32, "big") for s in sk_sums))
    assert st == bytes(top)
    enc = [c.g1_compress(sigs[64 * i:64 * i + 64]) for i in range(top)]
    sigma = [bytearray(sigs[64 * i:64 * i + 64]) for i in range(top)]
    for i in range(0, top, 13):
        sigma[i][40] ^= 4
        enc[i] = b"\x05" + enc[i][1:]
    for i in range(0, top, 11):
        sets[i] = sets[i] + [B.K_OFF_TWIST + (i // 11) % 3]
    return [(msgs[i], bytes(sigma[i]), sets[i]) for i in range(top)], enc


@pytest.mark.parametrize("which", range(4))
def test_export_statuses_equal_the_verify_at_every_routing_boundary(eng, registered, many, c, which):
    """n = a boundary of the routing table -1, +0, +1 (one boundary per case; the default table has four): the export call's status bytes
    are the plain bitmap verify's, with 64-byte and with compressed sigmas; its outputs are present exactly where the status is 0 or 9
    (spot-checked against the oracle)"""
    sks, pks = registered
    tuples, enc = many
    bounds = [r[0] for r in eng.route_table()[:-1]]
    assert 0 < len(bounds) <= 4, bounds                              # the cases of this test visit four boundaries: a longer table needs more cases
    b = bounds[which % len(bounds)]
    checked = 0
    for n in sorted({b - 1, b, b + 1} | ({1, 64, 65} if which == 0 else set())):
        t = tuples[:n]
        for flags, sigs in ((0, None), (E.FLAG_G1_COMPRESSED, b"".join(enc[:n]))):
            want = verify_call(eng, t, flags=flags, sigs=sigs)
            st, hashes, keys = export_call(eng, t, flags=flags, sigs=sigs)
            assert st == want, (n, flags, [(i, g, w) for i, (g, w) in enumerate(zip(st, want)) if g != w][:8])
            if n >= 65:
                assert {0, 4, 9} <= set(st) and (3 in st) == bool(flags)
            present = [s in (0, 9) for s in st]
            assert [hashes[64 * i:64 * i + 64] != bytes(64) for i in range(n)] == present, (n, flags)
            assert [keys[128 * i:128 * i + 128] != bytes(128) for i in range(n)] == present, (n, flags)
            for i in {1 % n, n // 2, n - 1}:                         # against the oracle at both ends and in the middle
                if present[i]:
                    assert hashes[64 * i:64 * i + 64] == c.hash_to_g1(t[i][0])[1] and keys[128 * i:128 * i + 128] == B.aggregate_key(pks, t[i][2], 2)[1], (n, i)
                    checked += 1
    assert checked


# ---- C: voting weights ---------------------------------------------------------------------------------------------------------------------------

def test_weights_against_python_integers(eng, registered, dev):
    sks, pks = registered
    rows = [bits for _, bits in B.rows()] + [list(range(B.N_KEYS)), list(range(B.N_GOOD)) + [B.K_IDENT, B.K_DUP0, B.K_NEG1]]
    assert rc_of(lambda: eng.batch_bitmap_weights(words(rows, 2), 2, len(rows))) == BAD_ARGUMENT          # no weights set yet
    for name, (weights, accepted) in sorted(B.weight_sets().items()):
        if not accepted:
            eng.set_key_weights(B.weight_sets()["small"][0])
            assert rc_of(lambda: eng.set_key_weights(weights)) == BAD_ARGUMENT                            # a total of 2^64
            assert rc_of(lambda: eng.batch_bitmap_weights(words(rows, 2), 2, len(rows))) == BAD_ARGUMENT  # ... leaves no weights set
            continue
        eng.set_key_weights(weights)
        for bm_words in B.BM_WORDS:
            want = [B.weight(weights, bits, bm_words) for bits in rows]
            got_w, got_st = eng.batch_bitmap_weights(words(rows, bm_words), bm_words, len(rows))
            assert (list(got_st), got_w) == ([s for s, _ in want], [w for _, w in want]), (name, bm_words)
    weights = B.weight_sets()["total_max"][0]
    eng.set_key_weights(weights)
    assert eng.batch_bitmap_weights(words([[B.K_IDENT]], 2), 2, 1) == ([weights[B.K_IDENT]], b"\0")       # an identity key counts its weight
    # the _device form, rows on both sides of a wave, into 0xA5-filled buffers
    for n in (1, 63, 64, 65, 129):
        many_rows = [rows[(3 * i) % len(rows)] for i in range(n)]
        d_bits, d_w, d_st = dev.buf(data=u32(words(many_rows, 2)) + bytes(4)), dev.buf(8 * n + 8, fill=0xA5), dev.buf(n, fill=0xA5)
        eng.batch_bitmap_weights_device(d_bits.ptr, 2, n, d_w.ptr, d_st.ptr, stream=dev.stream.handle)
        dev.stream.synchronize()
        want = [B.weight(weights, bits, 2) for bits in many_rows]
        assert list(struct.unpack("<%dQ" % n, d_w.download(8 * n))) == [w for _, w in want] and list(d_st.download()) == [s for s, _ in want], n
    assert rc_of(lambda: eng.batch_bitmap_weights_device(d_bits.ptr + 2, 2, 1, d_w.ptr, d_st.ptr)) == MISALIGNED
    assert rc_of(lambda: eng.batch_bitmap_weights_device(d_bits.ptr, 2, 1, d_w.ptr + 4, d_st.ptr)) == MISALIGNED
    assert rc_of(lambda: eng.batch_bitmap_weights_device(d_bits.ptr, 2, 1, None, d_st.ptr)) == BAD_ARGUMENT
    assert rc_of(lambda: eng.set_key_weights(weights[:-1])) == BAD_ARGUMENT                               # not the registered count
    assert rc_of(lambda: eng.batch_bitmap_weights(words(rows, 2), 2, len(rows))) == BAD_ARGUMENT          # a refused call leaves no weights set
    eng.set_key_weights(weights)
    assert eng.batch_bitmap_weights([], 2, 0) == ([], b"")
    eng.set_key_weights(None)                                                                             # forgotten on request
    assert rc_of(lambda: eng.batch_bitmap_weights(words(rows, 2), 2, len(rows))) == BAD_ARGUMENT


def test_every_registration_forgets_the_weights(eng, registered):
    sks, pks = registered
    weights = B.weight_sets()["small"][0]
    rows = [[0, 1, 2]]

    def armed():
        try:
            eng.batch_bitmap_weights(words(rows, 2), 2, 1)
            return True
        except E.NativeError as e:
            assert e.rc == BAD_ARGUMENT
            return False
    good = b"".join(sk_bytes(900 + j) for j in range(4))
    pk4, pop4, st = eng.batch_pop_prove(good)
    assert st == bytes(4)
    commitments, st = eng.batch_g2_mul(None, b"".join(sk_bytes(950 + j) for j in range(2)), 2, reduce_scalar=True)
    assert st == bytes(2)
    for register in (lambda: eng.register_keys(pk4), lambda: eng.register_keys_pop(pk4, pop4), lambda: eng.register_keys_commitments(commitments, 4)):
        eng.register_keys(b"".join(pks))
        eng.set_key_weights(weights)
        assert armed()
        register()
        assert not armed()
        eng.set_key_weights([5, 6, 7, 8])                            # the new set takes weights of its own count
        assert eng.batch_bitmap_weights(words(rows, 1), 1, 1) == ([18], b"\0")


def test_weights_over_a_large_key_set_one_row_per_wave_position(eng, registered):
    """4 096 + 3 keys (generator multiples from batch_g2_mul): 513 windows, the last one partial; 64 + 3 rows, one per position of a wave
    and into the next, each with its own pattern over the whole width; bits at and above n_keys give 2"""
    n_keys = 4096 + 3
    rnd = random.Random(47)
    pks, st = eng.batch_g2_mul(None, b"".join((j + 2).to_bytes(32, "big") for j in range(n_keys)), n_keys, reduce_scalar=True)
    assert st == bytes(n_keys)
    assert eng.register_keys(pks) == bytes(n_keys)
    weights = [rnd.randrange(0, 1 << 51) for _ in range(n_keys)]      # 4 099 x 2^51 < 2^64
    weights[n_keys - 1] = (1 << 51) - 1
    eng.set_key_weights(weights)
    bm_words = (n_keys + 31) // 32 + 1
    rows = [[j for j in range(n_keys) if (j % 67 == i or rnd.random() < 0.3)] for i in range(67)]
    rows[5] = [n_keys - 1]
    rows[6] = [n_keys]                                                # the first bit outside the set
    rows[7] = list(range(n_keys))
    rows[8] = [3, 32 * bm_words - 1]
    reg = [0] * n_keys
    want = [B.weight(weights, bits, bm_words, reg) for bits in rows]
    assert want[6] == (2, 0) and want[8] == (2, 0) and want[7] == (0, sum(weights)) and want[5] == (0, weights[-1])
    got_w, got_st = eng.batch_bitmap_weights(words(rows, bm_words), bm_words, len(rows))
    assert (list(got_st), got_w) == ([s for s, _ in want], [w for _, w in want])
    short = bm_words - 3                                              # a bitmap that cannot hold the last keys
    want = [B.weight(weights, bits, short, reg) for bits in rows]
    got_w, got_st = eng.batch_bitmap_weights(words(rows, short), short, len(rows))
    assert (list(got_st), got_w) == ([s for s, _ in want], [w for _, w in want])


def test_used_bits_of_a_collect_call_go_straight_in(eng, registered, c):
    """the signer_bits rows of bn254_batch_collect_keyed_bitmap are the weight call's and the key call's input as they are"""
    sks, pks = registered
    weights = B.weight_sets()["small"][0]
    eng.set_key_weights(weights)
    msgs = [D("bmo/collect", i) for i in range(3)]
    signers = [[0, 5, 9], [B.K_DUP0, 12], [3, 31, 32, 39]]
    shares = b"".join(c.sign(m, sks[j].to_bytes(32, "big")) for m, s in zip(msgs, signers) for j in s)
    share_st, tuple_st, agg, bits = eng.batch_collect_keyed_bitmap(msgs, shares, [j for s in signers for j in s], [len(s) for s in signers], 2)
    assert share_st == bytes(9) and tuple_st == bytes(3) and bits == words(signers, 2)
    assert eng.batch_bitmap_weights(bits, 2, 3) == ([sum(weights[j] for j in s) for s in signers], bytes(3))
    keys, st = eng.batch_aggregate_keys_bitmap(bits, 2, 3)
    assert (keys, st) == expect_keys(pks, signers, 2)
    got = eng.batch_verify_keyed_bitmap_export(msgs, agg, bits, 2)
    assert got == (bytes(3), b"".join(c.hash_to_g1(m)[1] for m in msgs), keys)


# ---- the mirrors -----------------------------------------------------------------------------------------------------------------------------------

def test_python_mirrors(eng, registered, c):
    from bn254_amd import api
    from bn254_amd.api import ECDSA, Error, ErrorKind, PublicKey, Signature
    sks, pks = registered
    msg = b"epoch 12"
    signers = [0, 7, 33]
    sigma = Signature(c.sign(msg, (sum(sks[j] for j in signers) % B.R).to_bytes(32, "big")))
    apk = B.aggregate_key(pks, signers, 2)[1]
    assert ECDSA.aggregate_public_key_signers(signers, engine=eng) == PublicKey(apk)
    res = ECDSA.batch_aggregate_public_keys_signers([signers, [1, B.K_NEG1], [2, B.K_BIG], [0, 1 << 40], []], engine=eng)
    assert res == [PublicKey(apk), PublicKey(bytes(128)), Error(ErrorKind.NotMemberError), Error(ErrorKind.IndexOutOfBounds), PublicKey(bytes(128))]
    with pytest.raises(Error):
        ECDSA.aggregate_public_key_signers([B.K_OFF_TWIST], engine=eng)
    h = c.hash_to_g1(msg)[1]
    assert ECDSA.verify_keyed_signers_export(msg, sigma, signers, engine=eng) == (None, h, PublicKey(apk))
    assert ECDSA.verify_keyed_signers_export(msg, c.g1_compress(sigma.raw), signers, engine=eng, compressed=True) == (None, h, PublicKey(apk))
    res = ECDSA.batch_verify_keyed_signers_export([(msg, sigma, signers), (msg, sigma, [0, 7]), (msg, sigma, [0, B.N_KEYS])], engine=eng)
    assert res == [(None, h, PublicKey(apk)), (Error(ErrorKind.VerificationFailed), h, PublicKey(B.aggregate_key(pks, [0, 7], 2)[1])),
                   (Error(ErrorKind.IndexOutOfBounds), bytes(64), PublicKey(bytes(128)))]
    # the formatter: the existing one on (m, sigma, the ORACLE's aggregate key)
    want = api.format_pairing_check_uncompressed_values(msg, sigma.raw, apk)
    assert api.format_pairing_check_keyed_signers(msg, sigma, signers, engine=eng) == want
    assert api.format_pairing_check_keyed_signers(msg, c.g1_compress(sigma.raw), signers, engine=eng, compressed=True) == want
    with pytest.raises(Error) as e:
        api.format_pairing_check_keyed_signers(msg, sigma, [0, 7], engine=eng)                 # 9: a failing aggregate is never formatted
    assert e.value.kind == ErrorKind.VerificationFailed
    with pytest.raises(Error) as e:
        api.format_pairing_check_keyed_signers(msg, Signature(bytes(64)), [1, B.K_NEG1], engine=eng)   # verifies (0), but the key is the identity
    assert e.value.kind == ErrorKind.PointInJacobian
    # weights
    weights = B.weight_sets()["edge"][0]
    ECDSA.register_key_weights(weights, engine=eng)
    assert ECDSA.signers_weight(signers, engine=eng) == sum(weights[j] for j in signers)
    assert ECDSA.batch_signers_weight([[2], [B.K_IDENT], [B.K_BIG], [B.N_KEYS + 5]], engine=eng) == [1 << 63, weights[B.K_IDENT], Error(ErrorKind.NotMemberError),
                                                                                                    Error(ErrorKind.IndexOutOfBounds)]
    with pytest.raises(E.NativeError):
        ECDSA.register_key_weights(B.weight_sets()["total_2_64"][0], engine=eng)
    ECDSA.register_key_weights(None, engine=eng)
    with pytest.raises(E.NativeError):
        ECDSA.signers_weight(signers, engine=eng)


def test_cpp_mirror_and_example(tmp_path):
    """host/bitmap_export_example.cpp — aggregate key, weight, export and the precompile formatters through bn254.hpp — builds with -Wall
    -Werror against the library and prints success"""
    from bn254_amd import _native
    host = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bn254_amd", "host")
    exe = str(tmp_path / "bitmap_export_example")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", os.path.join(host, "bitmap_export_example.cpp"), "-o", exe, _native.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "bitmap export: ok" in p.stdout, (p.stdout, p.stderr)
