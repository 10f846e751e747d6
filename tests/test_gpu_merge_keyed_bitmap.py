"""Merging partial signer-bitmap aggregates (include/bn254_hip.h: bn254_batch_merge_keyed_bitmap[_device]) on the GPU.
Identity 1: the partials' statuses are those of bn254_batch_verify_keyed_bitmap on the tuple's message repeated.  part_taken, the rows and the
counts are compared with tests/merge_model.py, the aggregate bytes with the oracle's g1_add, with both layouts of the select-and-sum forced and
by default.  Identity 2: the outputs fed to bn254_batch_verify_keyed_bitmap give 0 for every accepted tuple.  Identity 3: one-bit partials
give the exact collect's bytes.  Key sets and signatures are made on the CPU side of the library: a partial's signature is ONE scalar
multiplication of H(m) by the sum of its signers' secrets (batch_sign).  Run on the MI355X box: -m gpu."""
import os
import struct
import subprocess

import pytest

from bn254_amd import engine as E
from tests import collect_model, merge_model
from tests.datagen import D, sk_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
N_GOOD = 36
K_REFUSED, K_IDENT, K_DUP0, K_NEG1 = range(N_GOOD, N_GOOD + 4)
N_KEYS = N_GOOD + 4
BM = 2
SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130]
ALL_LANES = (1 << 31) - 1                     # the largest value the option takes: every tuple by a lane
LAYOUTS = [("all_waves", 1), ("all_lanes", ALL_LANES), ("default", E.MERGE_WAVE_MIN_PARTS_DEFAULT)]


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
def keyset(eng):
    """key set A, 40 entries: 36 good keys, then one off the twist (refused: 4), the identity (registered), key 0 AGAIN and the NEGATION of
    key 1.  Returns (secret keys as integers — 0 for the keys nobody signs for —, encodings)."""
    sks = [int.from_bytes(sk_bytes(900 + j), "big") % R for j in range(N_GOOD)]
    pks = derive(eng, sks)
    off_twist = bytearray(pks[3]); off_twist[100] ^= 2
    pks += [bytes(off_twist), bytes(128), pks[0], derive(eng, [R - sks[1]])[0]]
    sks += [0, 0, sks[0], R - sks[1]]
    reg = eng.register_keys(b"".join(pks))
    assert list(reg) == [0] * N_GOOD + [4, 0, 0, 0], reg[N_GOOD:]
    return sks, pks


def reg_set(eng, keyset):
    return eng.register_keys(b"".join(keyset[1]))


def sign_sums(eng, pairs):
    """pairs of (message, sum of secrets as an integer) -> signatures; a sum of 0 is the identity"""
    live = [(m, s % R) for m, s in pairs if s % R]
    sigs, st = eng.batch_sign([m for m, _ in live], b"".join(s.to_bytes(32, "big") for _, s in live)) if live else (b"", b"")
    assert st == bytes(len(live))
    it = iter(sigs[64 * i:64 * i + 64] for i in range(len(live)))
    return [next(it) if s % R else bytes(64) for _, s in pairs]


def row_of(bits, bm_words):
    row = [0] * bm_words
    for b in bits:
        row[b // 32] |= 1 << (b % 32)
    return row


def make(eng, c, secrets, tag, plan, bm_words):
    """plan: per tuple a list of (bits, kind); secrets[j] = the secret of bit j (0: none).  -> tuples (message, [(signature, row)]).  Kinds: ok;
    wrong (sigma + G1: 9); curve (a bit flipped: undecodable); big (a coordinate >= q: undecodable); also (the row holds one more bit, given
    as the LAST of bits, that no secret stands behind: beyond the key set, or a refused key); ident (the identity as the signature)"""
    g1 = c.g1_generator()
    msgs = [D("merge/%s" % tag, i) for i in range(len(plan))]
    flat = [(i, bits, kind) for i, t in enumerate(plan) for bits, kind in t]
    sigs = sign_sums(eng, [(msgs[i], sum(secrets[j] for j in (bits[:-1] if kind == "also" else bits))) for i, bits, kind in flat])
    tuples = [(m, []) for m in msgs]
    for (i, bits, kind), sg in zip(flat, sigs):
        if kind == "wrong":
            sg = c.g1_add(sg, g1)
        elif kind == "curve":
            sg = bytearray(sg); sg[40] ^= 4; sg = bytes(sg)
        elif kind == "big":
            sg = b"\xff" + sg[1:]
        elif kind == "ident":
            sg = bytes(64)
        tuples[i][1].append((sg, row_of(bits, bm_words)))
    return tuples


def plan_a():
    """twelve tuples over key set A: the ten sizes — partial t of tuple i signs for one to three good keys (so most of a long tuple overlaps
    what was taken), with wrong, undecodable, out-of-range and refused-key partials and empty rows mixed in — and two tuples of named cases"""
    plan = []
    for i, k in enumerate(SIZES):
        t_plan = []
        for t in range(k):
            a = (7 * i + 3 * t) % N_GOOD
            bits = [a] + ([(a + 11) % N_GOOD] if t % 3 == 1 else []) + ([(a + 23) % N_GOOD, K_IDENT] if t % 4 == 3 else [])
            kind = "ok"
            if k > 2 and t % 9 == 5:
                kind = "wrong"
            elif k > 2 and t % 9 == 6:
                kind = ["curve", "big", "also", "also", "ident", "ok", "ok"][(t // 9 + i) % 7]
                if kind == "also":
                    bits = bits + [[N_KEYS, K_REFUSED, 63][(t // 9) % 3]]
                elif (t // 9 + i) % 7 == 5:
                    bits = []                                        # an empty row with the identity: status 0, taken, adds nothing
                elif (t // 9 + i) % 7 == 6:
                    bits, kind = [], "wrong"                         # an empty row with a point: 9
            t_plan.append((bits, kind))
        plan.append(t_plan)
    plan.append([([0, 1], "ok"), ([1, 2], "ok"),                     # an overlap with a taken partial: not taken
                 ([2, 3], "ok"),                                     # a chain: overlaps only the partial that was not taken: taken
                 ([4, 5], "wrong"), ([5, 6], "ok"),                  # an overlap with a refused partial only: taken
                 ([7, 8], "ok"), ([7, 8], "ok"),                     # the same partial twice
                 ([9, K_NEG1], "ok"), ([10, K_NEG1], "ok"),          # an overlap in the set's highest key only
                 ([], "ok")])                                        # the empty row with the identity
    plan.append([([1, K_NEG1], "ok"),                                # a key and its negation: the identity, status 0
                 ([0], "ok"), ([K_DUP0], "ok"),                      # one key at two indices: both count
                 ([K_IDENT], "ok"),                                  # the identity key alone: the identity
                 ([K_REFUSED], "also"), ([11, K_REFUSED], "also"),   # a bit on the refused key: 4
                 ([12, N_KEYS], "also"),                             # a bit >= n_keys: 2
                 ([13], "curve"), ([14], "wrong")])
    return plan


NAMED_STATUS = [[0, 0, 0, 9, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 4, 4, 2, None, 9]]
NAMED_TAKEN = [[1, 0, 1, 0, 1, 1, 0, 1, 0, 1], [1, 1, 1, 1, 0, 0, 0, 0, 0]]


@pytest.fixture(scope="module")
def cases(eng, c, keyset):
    return make(eng, c, keyset[0] + [0] * 24, "cases", plan_a(), BM)


def flat(tuples):
    return ([t[0] for t in tuples], [s for t in tuples for s, _ in t[1]], [r for t in tuples for _, r in t[1]], [len(t[1]) for t in tuples])


def merge(eng, tuples, bm_words, flags=0):
    msgs, parts, rows, sizes = flat(tuples)
    return eng.merge_keyed_bitmap(msgs, b"".join(parts), [w for r in rows for w in r], sizes, bm_words, flags=flags, want_counts=True)


def bitmap_verify(eng, tuples, bm_words, flags=0):
    """identity 1's right-hand side: the bitmap verify on the tuple's message repeated once per partial"""
    msgs, parts, rows, sizes = flat(tuples)
    rep = [m for m, k in zip(msgs, sizes) for _ in range(k)]
    return eng.batch_verify_keyed_bitmap(rep, b"".join(parts), [w for r in rows for w in r], bm_words, flags=flags) if rep else b""


def expected(c, tuples, part_st, tuple_st, bm_words):
    """(taken, tuple statuses, aggregates, rows, counts) by the model and the oracle, for the given statuses"""
    _, parts, rows, sizes = flat(tuples)
    urows, counts, taken = merge_model.select(rows, part_st, sizes, tuple_st, bm_words)
    return bytes(taken), bytes(tuple_st), b"".join(merge_model.aggregates(c, parts, sizes, taken)), [w for r in urows for w in r], counts


def with_wave_min(eng, value, fn):
    try:
        eng.set_option(E.OPT_MERGE_WAVE_MIN_PARTS, value)
        return fn()
    finally:
        eng.set_option(E.OPT_MERGE_WAVE_MIN_PARTS, E.MERGE_WAVE_MIN_PARTS_DEFAULT)


def with_options(eng, opts, defaults, fn):
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            eng.set_option(k, defaults[k])


def check_all(eng, c, tuples, bm_words, flags=0, closed_loop=True):
    """identity 1, the model, the oracle and identity 2 on all three layouts; the six outputs byte-identical across them.  -> the outputs"""
    want_st = bitmap_verify(eng, tuples, bm_words, flags)
    n = len(tuples)
    want = expected(c, tuples, want_st, bytes(n), bm_words)
    seen = []
    for name, wave_min in LAYOUTS:
        got = with_wave_min(eng, wave_min, lambda: merge(eng, tuples, bm_words, flags))
        assert got[0] == want_st, (name, flags, [(p, a, b) for p, (a, b) in enumerate(zip(got[0], want_st)) if a != b][:8])
        assert got[1] == want[0], (name, flags, [p for p in range(len(want_st)) if got[1][p] != want[0][p]][:8])
        assert got[2] == want[1] and got[4] == want[3] and got[5] == want[4], (name, flags)
        assert got[3] == want[2], (name, flags, [i for i in range(n) if got[3][64 * i:64 * i + 64] != want[2][64 * i:64 * i + 64]])
        seen.append(got)
    assert seen[0] == seen[1] == seen[2]
    if closed_loop:                                                  # identity 2, flags 0 on the call's own outputs
        assert eng.batch_verify_keyed_bitmap([t[0] for t in tuples], seen[0][3], seen[0][4], bm_words) == bytes(n)
    return seen[0]


@pytest.mark.parametrize("flags", [0, E.FLAG_G2_SUBGROUP_CHECK, E.FLAG_REJECT_IDENTITY], ids=["flags0", "g2_subgroup", "reject_identity"])
def test_key_set_a_every_layout(eng, c, keyset, cases, flags):
    reg_set(eng, keyset)
    assert len(cases) == 12 and [len(t[1]) for t in cases][:10] == SIZES
    part_st, taken, tuple_st, agg, bits, counts = check_all(eng, c, cases, BM, flags)
    _, parts, _, sizes = flat(cases)
    if flags == 0:
        assert {0, 2, 4, 9} <= set(part_st) and part_st.count(0) > len(part_st) // 2, set(part_st)
        undecodable = [p for p in range(len(parts)) if c.g1_validate(parts[p], 0)]
        assert len(undecodable) >= 4 and all(part_st[p] == c.g1_validate(parts[p], 0) for p in undecodable)
        at = sum(SIZES)
        for j in range(2):
            st = list(part_st[at:at + sizes[10 + j]])
            assert [a if b is not None else None for a, b in zip(st, NAMED_STATUS[j])] == NAMED_STATUS[j], (j, st)
            assert list(taken[at:at + sizes[10 + j]]) == NAMED_TAKEN[j], j
            at += sizes[10 + j]
        assert counts[10] == 2 + 2 + 2 + 2 + 2 and counts[11] == 2 + 1 + 1 + 1
        assert agg[64 * 11:64 * 12] == sign_sums(eng, [(cases[11][0], 2 * keyset[0][0])])[0]      # (sk1 - sk1) + sk0 + sk0 + nothing
        assert 0 < counts[9] <= N_GOOD + 1 and sum(taken[sum(SIZES[:9]):sum(SIZES)]) < 60          # the longest tuple: most partials overlap
    if flags == E.FLAG_REJECT_IDENTITY:
        at = sum(SIZES) + sizes[10]
        assert part_st[at] != 0 and part_st[at + 3] != 0 and taken[at] == 0                        # the identity as a signature is refused at the decode


def test_identity_3_the_collect_inside(eng, c, keyset):
    """one-bit partials against bn254_batch_collect_keyed_bitmap on the same data: duplicates of a key, a valid and an invalid share of one
    key in both orders, the refused key, an index beyond the set, key 1 and its negation, key 0 at both its indices"""
    sks, _ = keyset
    reg_set(eng, keyset)
    plan = []
    for i, k in enumerate([0, 1, 5, 17, 64, 70]):
        t_plan = []
        for t in range(k):
            key = (5 * i + 3 * t) % N_KEYS if t % 7 else (t // 7) % 4
            kind = "ok"
            if key == K_REFUSED:
                kind = "also"
            elif t % 6 == 4:
                kind = "wrong"
            elif t % 13 == 12:
                key, kind = N_KEYS + 3, "also"
            t_plan.append(([key], kind))
        plan.append(t_plan)
    plan.append([([3], "wrong"), ([3], "ok"), ([4], "ok"), ([4], "wrong"), ([1], "ok"), ([K_NEG1], "ok"), ([0], "ok"), ([K_DUP0], "ok"), ([0], "ok")])
    tuples = make(eng, c, sks + [0] * 24, "identity3", plan, BM)
    msgs, parts, rows, sizes = flat(tuples)
    keys = [bits[0] for t in plan for bits, _ in t]
    share_st, ctuple_st, cagg, cbits, ccounts = eng.batch_collect_keyed_bitmap(msgs, b"".join(parts), keys, sizes, BM, want_counts=True)
    _, _, chosen = collect_model.select(keys, share_st, sizes, ctuple_st, BM)
    first = bytes(int(p in {s for pick in chosen for s in pick}) for p in range(len(keys)))
    assert {0, 2, 4, 9} <= set(share_st) and 0 < sum(first) < share_st.count(0)
    for name, wave_min in LAYOUTS:
        got = with_wave_min(eng, wave_min, lambda: merge(eng, tuples, BM))
        assert got == (share_st, first, ctuple_st, cagg, cbits, ccounts), name


def test_wide_rows_66_words(eng, c, keyset):
    """bm_words = 66 over 2 100 registered entries that repeat 8 distinct keys, overlaps only in words 64 and 65, tuples of 3 and of 70
    partials (distance 1 and distance 64 in the long one); and 64 entries at bm_words = 2 with an overlap in the last bit of the last word"""
    sks, pks = keyset
    try:
        reg = eng.register_keys(b"".join(pks[j % 8] for j in range(2100)))
        assert reg == bytes(2100)
        secrets = [sks[j % 8] for j in range(2100)] + [0] * 12
        long_t = [([100 + t], "ok") for t in range(70)]
        long_t[1] = ([101, 2060], "ok")
        long_t[65] = ([165, 2060], "ok")                              # word 64, 64 places behind the partial that holds the bit: the same lane
        long_t[2] = ([102, 2095], "ok")
        long_t[3] = ([103, 2095], "ok")                               # word 65, the next lane
        plan = [[([5, 2050], "ok"), ([6, 2050], "ok"), ([7, 2090], "ok")], long_t]
        tuples = make(eng, c, secrets, "wide66", plan, 66)
        part_st, taken, tuple_st, agg, bits, counts = check_all(eng, c, tuples, 66)
        assert part_st == bytes(73) and list(taken[:3]) == [1, 0, 1] and [p for p in range(70) if not taken[3 + p]] == [3, 65]
        assert counts == [4, 70] and bits[64] == 1 << 2 and bits[65] == 1 << 10 and bits[66 + 64] == 1 << 12 and bits[66 + 65] == 1 << 15
        reg = eng.register_keys(b"".join(pks[j % 8] for j in range(64)))
        assert reg == bytes(64)
        tuples = make(eng, c, secrets[:64], "last-bit", [[([3, 63], "ok"), ([4, 63], "ok"), ([5], "ok")]], 2)
        part_st, taken, tuple_st, agg, bits, counts = check_all(eng, c, tuples, 2)
        assert part_st == bytes(3) and list(taken) == [1, 0, 1] and bits == [(1 << 3) | (1 << 5), 1 << 31] and counts == [3]
    finally:
        reg_set(eng, keyset)


def test_wide_rows_130_words(eng, c, keyset):
    """bm_words = 130 over key set A: a partial that sets a bit in word 129 reads 2 and is not taken"""
    sks, _ = keyset
    reg_set(eng, keyset)
    plan = [[([0, 1], "ok"), ([2, 32 * 129 + 7], "also"), ([2, 3], "ok"), ([3, 4], "ok")],
            [([t % N_GOOD], "ok") if t != 40 else ([5, 32 * 129 + 31], "also") for t in range(66)]]
    tuples = make(eng, c, sks + [0] * (32 * 130 - N_KEYS), "wide130", plan, 130)
    part_st, taken, tuple_st, agg, bits, counts = check_all(eng, c, tuples, 130)
    assert list(part_st[:4]) == [0, 2, 0, 0] and list(taken[:4]) == [1, 0, 1, 0] and part_st[4 + 40] == 2 and taken[4 + 40] == 0
    assert counts == [4, N_GOOD] and not any(bits[2:130]) and not any(bits[132:260])


def sliced_cases(cases, total):
    """the tuples of `cases` with the longest one cut down so that the call has exactly `total` partials"""
    extra = sum(len(t[1]) for t in cases) - total
    assert 0 < extra < 130
    return [(m, p[:len(p) - extra] if len(p) == 130 else p) for m, p in cases]


def test_sliced_partials_same_bytes(eng, c, keyset, cases):
    """BN254_OPT_MAX_CHUNK = 64 over 300 partials: tuples straddle the slices; the same bytes as in one piece, on every layout"""
    reg_set(eng, keyset)
    tuples = sliced_cases(cases, 300)
    whole = merge(eng, tuples, BM)
    assert whole[0] == bitmap_verify(eng, tuples, BM) and whole[1:] == expected(c, tuples, whole[0], bytes(len(tuples)), BM)
    for name, wave_min in LAYOUTS:
        got = with_options(eng, {E.OPT_MAX_CHUNK: 64, E.OPT_MERGE_WAVE_MIN_PARTS: wave_min}, {E.OPT_MAX_CHUNK: 0, E.OPT_MERGE_WAVE_MIN_PARTS: E.MERGE_WAVE_MIN_PARTS_DEFAULT},
                           lambda: merge(eng, tuples, BM))
        assert got == whole, name


def test_no_keys_bm_words_0_and_n_0(eng, c, keyset, cases):
    """no keys registered: every partial with a set bit reads 2, an empty row is verified as the bitmap call verifies it; bm_words = 0 with
    NULL bit pointers; n = 0; NULL n_signers; then the set again (no stale state)"""
    import ctypes
    small = [t for t in cases if len(t[1]) <= 17]
    try:
        eng.register_keys(b"")
        part_st, taken, tuple_st, agg, bits, counts = check_all(eng, c, small, BM)
        _, parts, rows, _ = flat(small)
        assert all(st == (c.g1_validate(p, 0) or (2 if any(r) else 0 if p == bytes(64) else 9)) for st, p, r in zip(part_st, parts, rows))
        assert not any(bits) and not any(counts) and agg == bytes(64 * len(small)) and 0 < sum(taken) == part_st.count(0)
    finally:
        reg_set(eng, keyset)
    # bm_words = 0: every row is empty — the identity passes and is taken, a point reads 9
    g1 = c.g1_generator()
    empty = [(D("merge/bm0", 0), [(bytes(64), []), (g1, []), (bytes(64), [])]), (D("merge/bm0", 1), []), (D("merge/bm0", 2), [(g1, [])])]
    part_st, taken, tuple_st, agg, bits, counts = check_all(eng, c, empty, 0)
    assert list(part_st) == [0, 9, 0, 9] and list(taken) == [1, 0, 1, 0] and agg == bytes(192) and bits == [] and counts == [0, 0, 0]
    msgs, parts, _, sizes = flat(empty)
    blob, off = E.pack_messages(msgs)
    n, n_parts = len(empty), len(parts)
    pst, tkn, tst, out = (ctypes.create_string_buffer(k) for k in (n_parts, n_parts, n, 64 * n))
    poff = (ctypes.c_uint64 * (n + 1))(0, 3, 3, 4)
    rc = eng._lib.bn254_batch_merge_keyed_bitmap(eng._h, blob, off, b"".join(parts), None, poff, n_parts, n, 0, 0, pst, tkn, tst, out, None, None)
    assert rc == 0 and pst.raw == part_st and tkn.raw == taken and tst.raw == bytes(n) and out.raw == bytes(192)      # NULL bit pointers, NULL n_signers
    # n = 0 returns 0 whatever else is passed; the host form's offsets must start at 0, never decrease and end at n_parts
    assert eng._lib.bn254_batch_merge_keyed_bitmap(eng._h, None, None, None, None, None, 0, 0, BM, 0, None, None, None, None, None, None) == 0
    assert merge(eng, [], BM) == (b"", b"", b"", b"", [], [])
    for bad in ([1, 3, 3, 4], [0, 3, 2, 4], [0, 3, 3, 3], [0, 3, 3, 5]):
        rc = eng._lib.bn254_batch_merge_keyed_bitmap(eng._h, blob, off, b"".join(parts), None, (ctypes.c_uint64 * (n + 1))(*bad), n_parts, n, 0, 0, pst, tkn, tst,
                                                     out, None, None)
        assert rc == -10001, bad
    part_st, taken, tuple_st, agg, bits, counts = check_all(eng, c, small, BM)
    assert any(bits) and 0 in part_st


def test_device_form_range_rule_and_alignment(eng, c, keyset, cases):
    """the _device form on a caller's stream: the host form's bytes, a bitmap verify behind it on the same stream with no synchronisation in
    between; refused ranges — reversed, one past n_parts, one that starts before an earlier offset — give tuple status 2, an empty row, the
    identity and count 0, and partials of no accepted tuple read 2 and are not taken; misaligned parts / part_bits / offsets are refused;
    NULL n_signers"""
    from tests.hip_ctypes import DevBuf, Stream
    reg_set(eng, keyset)
    tuples = [t for t in cases if 0 < len(t[1]) <= 17][:7]
    msgs, parts, rows, sizes = flat(tuples)
    n, n_parts = len(tuples), len(parts)
    blob, off = E.pack_messages(msgs)
    off = list(off)
    poff = [sum(sizes[:i]) for i in range(n + 1)]
    u64 = lambda v: struct.pack("<%dQ" % len(v), *v)   # noqa: E731
    u32 = lambda v: struct.pack("<%dI" % len(v), *v)   # noqa: E731
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_msgs, d_moff, d_parts, d_rows = dev(bytes(blob)), dev(u64(off)), dev(b"".join(parts) + bytes(4)), dev(u32([w for r in rows for w in r]) + bytes(4))
        sizes_out = (n_parts, n_parts, n, 64 * n, 4 * BM * n, 4 * n)
        outs = [dev(nbytes=k) for k in sizes_out]
        d_vst = dev(nbytes=n)

        def run(part_off, parts_ptr=None, rows_ptr=None, poff_shift=0, counts=True):
            for b, k in zip(outs, sizes_out):
                b.upload(b"\xEE" * k)
            d_poff = dev(u64(part_off) + bytes(8))
            eng.merge_keyed_bitmap_device(d_msgs.ptr, d_moff.ptr, parts_ptr or d_parts.ptr, rows_ptr or d_rows.ptr, d_poff.ptr + poff_shift, n_parts, n, BM,
                                          *(b.ptr for b in outs[:5]), outs[5].ptr if counts else None, stream=stream.handle)
            eng.batch_verify_keyed_bitmap_device(d_msgs.ptr, d_moff.ptr, outs[3].ptr, outs[4].ptr, BM, n, d_vst.ptr, stream=stream.handle)
            stream.synchronize()
            raw = [b.download(k) for b, k in zip(outs, sizes_out)]
            return raw[0], raw[1], raw[2], raw[3], list(struct.unpack("<%dI" % (BM * n), raw[4])), list(struct.unpack("<%dI" % n, raw[5])), d_vst.download(n)

        host = merge(eng, tuples, BM)
        got = run(poff)
        assert got[:6] == host and got[6] == bytes(n)
        got = run(poff, counts=False)                                # NULL n_signers: the array is not touched
        assert got[:5] == host[:5] and got[5] == [0xEEEEEEEE] * n

        def refused(part_off, bad, orphans):
            g = run(part_off)
            for i in range(n):
                if i in bad:
                    assert g[2][i] == 2 and g[3][64 * i:64 * i + 64] == bytes(64) and g[4][BM * i:BM * i + BM] == [0] * BM and g[5][i] == 0, i
                else:
                    assert g[2][i] == 0 and g[3][64 * i:64 * i + 64] == host[3][64 * i:64 * i + 64] and g[5][i] == host[5][i], i
            for p in range(n_parts):
                assert (g[0][p], g[1][p]) == ((2, 0) if p in orphans else (host[0][p], host[1][p])), p
            assert all(g[6][i] == 0 for i in range(n))               # a refused tuple's empty row and identity verify too
        i = 2
        rev = poff[:]
        rev[i + 1] = poff[i] - 1                     # tuple i reversed; tuple i + 1 then starts before the earlier offset poff[i]: refused too
        refused(rev, {i, i + 1}, set(range(poff[i], poff[i + 2])))
        past = poff[:]
        past[n] = n_parts + 1                        # the last tuple runs one past n_parts
        refused(past, {n - 1}, set(range(poff[n - 1], n_parts)))
        lap = poff[:]
        lap[i + 2] = poff[i + 1] - 1                 # tuple i + 2 starts before the earlier offset poff[i + 1] (tuple i + 1 is left a reversed range)
        g = run(lap)
        assert g[2][i + 1] == 2 and g[2][i + 2] == 2 and g[2][i] == 0 and g[5][i + 1] == 0 and g[5][i + 2] == 0
        assert all(g[0][p] == 2 and g[1][p] == 0 for p in range(poff[i + 1], poff[i + 3]))
        assert run(poff)[:6] == host
        for kw in (dict(parts_ptr=d_parts.ptr + 1), dict(rows_ptr=d_rows.ptr + 2), dict(poff_shift=4)):
            with pytest.raises(E.NativeError) as e:
                run(poff, **kw)
            assert e.value.rc == -10002, kw          # BN254_E_MISALIGNED
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


WAVE_BLOCKS = 65536                                  # CL_WAVE_MAX_BLOCKS: the wave kernel's block cap
N_MANY = 70000


@pytest.mark.parametrize("wave_min", [E.MERGE_WAVE_MIN_PARTS_DEFAULT, 1], ids=["default", "all_waves"])
def test_beyond_the_grid(eng, c, keyset, wave_min):
    """70 000 tuples of one partial each, replicated from a few distinct valid partials (every eleventh sigma + G1), plus one tuple of 64 at
    the end, against the model: with every tuple sent to the wave kernel, the tuples from 65 536 on are reached by stride"""
    sks, _ = keyset
    reg_set(eng, keyset)
    pool = make(eng, c, sks, "many", [[([(3 * j) % N_GOOD, (3 * j + 1) % N_GOOD], "wrong" if j % 11 == 10 else "ok")] for j in range(33)], BM)
    last = make(eng, c, sks, "many-last", [[([t % 40 if t % 40 < N_GOOD else t % 7], "ok") for t in range(64)]], BM)[0]
    tuples = [pool[i % 33] for i in range(N_MANY)] + [last]
    assert len(tuples) > WAVE_BLOCKS + 64
    msgs, parts, rows, sizes = flat(tuples)
    part_st = bytes(9 if i % 33 % 11 == 10 else 0 for i in range(N_MANY)) + bytes(64)
    urows, counts, taken = merge_model.select(rows, part_st, sizes, bytes(len(tuples)), BM)
    agg = b"".join(parts[i] if taken[i] else bytes(64) for i in range(N_MANY)) + merge_model.aggregates(c, parts[N_MANY:], [64], taken[N_MANY:])[0]
    assert sum(taken[N_MANY:]) == N_GOOD and counts[-1] == N_GOOD and taken[:N_MANY].count(1) == part_st[:N_MANY].count(0)
    got = with_wave_min(eng, wave_min, lambda: eng.merge_keyed_bitmap(msgs, b"".join(parts), [w for r in rows for w in r], sizes, BM, want_counts=True))
    want = (part_st, bytes(taken), bytes(len(tuples)), agg, [w for r in urows for w in r], counts)
    for k, (name, width) in enumerate((("part_status", 1), ("part_taken", 1), ("tuple_status", 1), ("agg", 64), ("bits", BM), ("counts", 1))):
        diff = [] if got[k] == want[k] else [i for i in range(len(want[k]) // width) if got[k][width * i:width * i + width] != want[k][width * i:width * i + width]][:8]
        assert not diff, (name, diff)


def test_python_and_cpp_mirrors(eng, keyset, tmp_path):
    """ECDSA.merge_keyed_signers round-trips into ECDSA.verify_keyed_signers; so does the compiled C++ mirror"""
    from bn254_amd.api import ECDSA, Error, ErrorKind, PrivateKey, PublicKey, Signature
    sk = [PrivateKey(int.from_bytes(sk_bytes(j), "big")) for j in range(5)]
    pk = [PublicKey.from_private_key(s) for s in sk]
    ints = [int.from_bytes(sk_bytes(j), "big") for j in range(5)]
    try:
        assert ECDSA.register_keys(pk, engine=eng) == [None] * 5
        msg = b"round 11"
        part = lambda idx: Signature(sign_sums(eng, [(msg, sum(ints[j] for j in idx))])[0])      # noqa: E731
        wrong = Signature(sign_sums(eng, [(msg, ints[0] + 1)])[0])
        parts = [(part([0, 1]), [0, 1]), (part([1, 2]), [1, 2]), (wrong, [3]), (part([3, 4]), [4, 3]), (part([2]), [2, 9]), (part([2]), [2])]
        sigma, signers, statuses, taken = ECDSA.merge_keyed_signers(msg, parts, engine=eng)
        assert signers == [0, 1, 2, 3, 4] and taken == [True, False, False, True, False, True]
        assert statuses == [None, None, Error(ErrorKind.VerificationFailed), None, Error(ErrorKind.IndexOutOfBounds), None]
        for k, (sg, idx) in enumerate(parts):                         # statuses[k] is what verify_keyed_signers raises for partial k
            try:
                ECDSA.verify_keyed_signers(msg, sg, idx, engine=eng)
                assert statuses[k] is None
            except Error as e:
                assert statuses[k] == e
        assert ECDSA.verify_keyed_signers(msg, sigma, signers, engine=eng) is None
        res = ECDSA.batch_merge_keyed_signers([(msg, parts[:2]), (b"other", [])], engine=eng)
        assert res[0][1] == [0, 1] and res[0][3] == [True, False] and res[1][1] == [] and res[1][0].raw == bytes(64) and res[1][2] == [] == res[1][3]
        assert ECDSA.batch_verify_keyed_signers([(msg, res[0][0], res[0][1]), (b"other", res[1][0], [])], engine=eng) == [None, None]
    finally:
        reg_set(eng, keyset)
    src = tmp_path / "merge_mirror.cpp"
    src.write_text(CPP_MIRROR)
    exe = str(tmp_path / "merge_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "bn254_amd", "host"), str(src), "-L" + os.path.join(ROOT, "bn254_amd"),
                           "-lbn254hip", "-Wl,-rpath," + os.path.join(ROOT, "bn254_amd"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "merge mirror ok" in p.stdout, (p.stdout, p.stderr)


CPP_MIRROR = r"""
#include <cstdio>
#include "bn254.hpp"
int main() {
  try {
    bn254::PrivateKey k[3];
    for (int j = 0; j < 3; ++j) { k[j].bytes = {}; k[j].bytes[31] = (uint8_t)(7 + j); k[j].bytes[5] = 0x11; }
    std::vector<bn254::PublicKey> pk;
    for (int j = 0; j < 3; ++j) pk.push_back(bn254::PublicKey::from_private_key(k[j]));
    if (bn254::ECDSA::register_keys(pk) != std::vector<uint8_t>{0, 0, 0}) return 2;
    std::vector<uint8_t> msg = {'m', 'e', 'r', 'g', 'e'};
    auto s0 = bn254::ECDSA::sign(msg, k[0]), s1 = bn254::ECDSA::sign(msg, k[1]), s2 = bn254::ECDSA::sign(msg, k[2]);
    // a child's partial for keys 0 and 1, built by the collect; then the merge of it with shares of keys 1 and 2 and an index outside the set
    auto child = bn254::ECDSA::aggregate_keyed_signers(msg, {s0, s1}, {0, 1}, 3);
    if (child.signer_indices != std::vector<uint32_t>{0, 1}) return 3;
    auto r = bn254::ECDSA::merge_keyed_signers(msg, {{child.signature, {0, 1}}, {s1, {1}}, {s2, {2}}, {s2, {1}}, {s2, {2, 7}}}, 3);
    if (r.signer_indices != std::vector<uint32_t>{0, 1, 2} || r.statuses != std::vector<uint8_t>{0, 0, 0, 9, 2} ||
        r.taken != std::vector<uint8_t>{1, 0, 1, 0, 0}) return 4;
    bn254::ECDSA::verify_keyed_signers(msg, r.signature, r.signer_indices, 3);
    try { bn254::ECDSA::verify_keyed_signers(msg, r.signature, {0, 1}, 3); return 5; }
    catch (const bn254::Error& e) { if (e.kind != bn254::ErrorKind::VerificationFailed) return 6; }
    printf("merge mirror ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
"""
