"""ONE case set for what the signer-bitmap calls return besides a status byte (include/bn254_hip.h: bn254_batch_aggregate_keys_bitmap,
bn254_batch_verify_keyed_bitmap_export, bn254_batch_bitmap_weights), shared by the host compilation of the kernels' bodies
(tests/test_bitmap_out_cases.py) and the GPU suite (tests/test_gpu_bitmap_out.py).  Every expectation comes from the oracle's g2_add,
hash_to_g1 and sign and from Python integers — never from the library under test.

The key set is the one of tests/test_gpu_verify_keyed_bitmap.py, restated: 40 good keys, one off the twist (4), one outside the subgroup
(4), one with a coordinate >= q (6), the identity, key 0 again and the negation of key 1 — 46 keys, a multiple of neither 8 nor 32 (a
partial last window and a partial last word)."""
import functools
import random

from tests.datagen import D, sk_bytes

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
N_GOOD = 40
K_OFF_TWIST, K_OFF_SUB, K_BIG, K_IDENT, K_DUP0, K_NEG1 = range(N_GOOD, N_GOOD + 6)
N_KEYS = N_GOOD + 6
REG_STATUS = [0] * N_GOOD + [4, 4, 6, 0, 0, 0]
BM_WORDS = (0, 1, 2, 3)
ST_HASH, ST_OOB, ST_ENCODING, ST_GROUP_POINT, ST_MEMBER, ST_FAILED = 1, 2, 3, 4, 6, 9
FLAG_REJECT_IDENTITY = 2
HASH_MAX_TRIES = 3                                           # the BN254_OPT_HASH_MAX_TRIES the hash-failure cases are built for


def oracle():
    from oracle import c_oracle
    return c_oracle


@functools.lru_cache(maxsize=None)
def keyset(g2_not_in_subgroup_hex):
    """(secret keys as integers — 0 for a key that contributes nothing —, the 46 encodings)"""
    c = oracle()
    sks = [int.from_bytes(sk_bytes(500 + j), "big") % R for j in range(N_GOOD)]
    pks = [c.public_key_g2(s.to_bytes(32, "big")) for s in sks]
    off_twist = bytearray(pks[3]); off_twist[100] ^= 2
    big = bytearray(pks[5]); big[0] = 0xFF
    neg1 = c.public_key_g2((R - sks[1]).to_bytes(32, "big"))
    pks += [bytes(off_twist), bytes.fromhex(g2_not_in_subgroup_hex), bytes(big), bytes(128), pks[0], neg1]
    sks += [0, 0, 0, 0, sks[0], R - sks[1]]
    assert len(pks) == N_KEYS and [c.g2_validate(p) if p != bytes(128) else 0 for p in pks] == REG_STATUS
    return tuple(sks), tuple(pks)


def rows():
    """(name, set bits): every shape of a row the issue names"""
    rnd = random.Random(41)
    out = [("pop%d" % p, sorted(rnd.sample(range(N_GOOD), p))) for p in (0, 1, 2, 8, 9)]
    out += [("all_good", list(range(N_GOOD))), ("all_members", list(range(N_GOOD)) + [K_IDENT, K_DUP0, K_NEG1]),
            ("identity_only", [K_IDENT]), ("identity_among", [4, K_IDENT, 30]), ("doubling", [0, K_DUP0]), ("doubling_among", [0, 9, K_DUP0, 17]),
            ("cancel", [1, K_NEG1]), ("cancel_among", [1, 2, K_NEG1]), ("negation_only", [K_NEG1]), ("last_key_of_word0", [31]), ("first_key_of_word1", [32]),
            ("refused_lowest", [2, K_OFF_TWIST]), ("refused_then_refused", [K_OFF_SUB, 3, K_BIG]), ("refused_6", [K_BIG]),
            ("refused_before_oob", [6, K_BIG, N_KEYS + 1]), ("oob_at_n_keys", [5, N_KEYS]), ("oob_only", [N_KEYS + 20]), ("oob_end_of_word1", [7, 63]),
            ("oob_word2", [64]), ("oob_end_of_word2", [8, 95])]
    return out


def held(bits, bm_words):
    """the set bits a bitmap of bm_words words can hold"""
    return sorted(j for j in set(bits) if j // 32 < bm_words)


def to_words(bits, bm_words):
    w = [0] * bm_words
    for j in held(bits, bm_words):
        w[j // 32] |= 1 << (j % 32)
    return w


def rule2(bits, bm_words, reg=REG_STATUS):
    """the status of the lowest bad set bit: 2 at or above the set, else the key's registration status; restated, not imported"""
    for j in held(bits, bm_words):
        if j >= len(reg):
            return ST_OOB
        if reg[j]:
            return reg[j]
    return 0


def aggregate_key(pks, bits, bm_words, reg=REG_STATUS):
    """(status, 128 bytes) call A owes the row: the oracle's g2_add over the set keys in ascending order, zeros under a non-zero status"""
    return _aggregate_key(tuple(pks), tuple(held(bits, bm_words)), tuple(reg))


@functools.lru_cache(maxsize=None)
def _aggregate_key(pks, held_bits, reg):
    st = next((ST_OOB if j >= len(reg) else reg[j] for j in held_bits if j >= len(reg) or reg[j]), 0)
    apk = bytes(128)
    if st == 0:
        c = oracle()
        for j in held_bits:
            apk = c.g2_add(apk, pks[j])
    return st, apk


def weight_sets():
    """name -> (46 weights, accepted?)"""
    rnd = random.Random(43)
    small = [rnd.randrange(1, 1 << 40) for _ in range(N_KEYS)]
    edge = [0, 1, 1 << 63] + [rnd.randrange(0, 1 << 32) for _ in range(N_KEYS - 3)]
    edge[K_IDENT] = 12345                                   # the identity key counts its weight
    full = list(edge)
    full[3] += (1 << 64) - 1 - sum(full)                    # the total is exactly 2^64 - 1
    over = list(full)
    over[4] += 1                                            # ... and exactly 2^64: refused
    assert sum(full) == (1 << 64) - 1 and sum(over) == 1 << 64 and all(0 <= w < 1 << 64 for w in full + over)
    return {"small": (small, True), "edge": (edge, True), "total_max": (full, True), "total_2_64": (over, False), "all_zero": ([0] * N_KEYS, True),
            "one_key_max": ([0] * 7 + [(1 << 64) - 1] + [0] * (N_KEYS - 8), True)}


def weight(weights, bits, bm_words, reg=REG_STATUS):
    """(status, weight) the weight call owes the row, in Python integers"""
    st = rule2(bits, bm_words, reg)
    return st, (sum(weights[j] for j in held(bits, bm_words)) if st == 0 else 0)


@functools.lru_cache(maxsize=None)
def unhashable_message():
    """a message whose hash needs more than HASH_MAX_TRIES counters (by the oracle's count, with room for either way of counting)"""
    c = oracle()
    for i in range(10000):
        m = D("bmo/unhashable", i)
        st, _, tries = c.hash_to_g1(m)
        if st == 0 and tries >= min_tries() + HASH_MAX_TRIES + 2:
            return m
    raise AssertionError("no such message")


def hashable_message(i):
    """the i-th message of the export cases: one that hashes at its FIRST counter, so that HASH_MAX_TRIES leaves it alone"""
    c = oracle()
    return next(m for m in (D("bmo/export/%d" % i, k) for k in range(1000)) if c.hash_to_g1(m)[2] == min_tries())


@functools.lru_cache(maxsize=None)
def min_tries():
    """what the oracle reports for a message that needs one counter (the smallest count over a few hundred messages)"""
    c = oracle()
    return min(c.hash_to_g1(D("bmo/probe", k))[2] for k in range(200))


@functools.lru_cache(maxsize=None)
def export_tuples(g2_not_in_subgroup_hex):
    """Call B's tuples at bm_words = 2: per row a valid sigma, a wrong one (9: outputs present), an undecodable one and the identity sigma;
    then a message that does not hash under HASH_MAX_TRIES.  Each: (message, sigma 64 B, set bits, kind)."""
    c = oracle()
    sks, _ = keyset(g2_not_in_subgroup_hex)
    g1 = c.g1_generator()
    out = []
    for i, (name, bits) in enumerate(rows()):
        m = hashable_message(i)
        total = sum(sks[j] for j in held(bits, 2) if j < N_KEYS) % R
        sigma = c.sign(m, total.to_bytes(32, "big")) if total else bytes(64)
        bad = bytearray(sigma if total else g1); bad[40] ^= 4
        out += [(m, sigma, tuple(bits), "valid"), (m, c.g1_add(sigma, g1), tuple(bits), "wrong"), (m, bytes(bad), tuple(bits), "undecodable"),
                (m, bytes(64), tuple(bits), "identity")]
    m = unhashable_message()
    out.append((m, c.sign(m, sks[0].to_bytes(32, "big")), (0,), "unhashable"))
    return tuple(out)


def export_status(t, pks, flags=0, bm_words=2, hash_max_tries=HASH_MAX_TRIES):
    """the status the bitmap verify owes tuple t, by construction: sigma's decode, rule 2, the hash, the pairing"""
    m, sigma, bits, kind = t
    st = oracle().g1_validate(sigma, flags & FLAG_REJECT_IDENTITY)
    if st:
        return st
    st = rule2(bits, bm_words)
    if st:
        return st
    if kind == "unhashable" and hash_max_tries:
        return ST_HASH
    if kind in ("valid", "unhashable"):                     # with the reference's 255 counters the message hashes, and its sigma is valid
        return 0
    if kind == "identity":                                  # e(identity, -G2) == 1: the check passes iff the aggregate key is the identity too
        return 0 if aggregate_key(pks, bits, bm_words)[1] == bytes(128) else ST_FAILED
    return ST_FAILED


def export_outputs(t, pks, status, bm_words=2):
    """(H(m) 64 B, aggregate key 128 B) call B owes tuple t under its final status: present iff the status is 0 or 9"""
    if status not in (0, ST_FAILED):
        return bytes(64), bytes(128)
    st, h, _ = oracle().hash_to_g1(t[0])
    assert st == 0
    return h, aggregate_key(pks, t[2], bm_words)[1]
