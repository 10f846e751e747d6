"""One case set for check_public_keys (the reference's src/ecdsa.rs:78-93; bn254_batch_check_public_keys), shared by the CPU test (the
one-lane kernel body compiled for the host, plain and bound-tracking: tests/test_cpk_cases.py) and the GPU test (every layout and
route of the call, tests/test_gpu_check_public_keys.py): the same bytes and the same expected status on both sides.

A case is Case(pk_g2, pk_g1, name): 128 and 64 uncompressed bytes, all-zero = the identity of the batch ABI.  Keys are derived from
secrets by oracle/c_oracle.py (public_key_g2 / public_key_g1, which reduce the secret mod r as Fr::from_slice does); every fault is
made here on the bytes.  The EXPECTED status of a case under a flags value (bit 0 = G2 subgroup check, bit 1 = reject identities) is
oracle.c_oracle.check_public_keys and nothing else: pk_g2 is decoded first (ecdsa.rs:82), then pk_g1, the first fault is the status,
else 0 / 9 from e(G1::one(), pk_g2) * e(pk_g1, -G2::one()) == 1.  Nothing here imports the library under test or its host build.

No reference vector holds an identity key or a fault under check_public_keys: those statuses are UNPINNED beyond the oracle's
restatement (all-zero bytes = the identity is this project's batch ABI, include/bn254_hip.h), as the x.im >= q code of the
compressed decoder is (tests/codec_cases.py).  ANCHORS below are the statuses the oracle gave when the set was written; the CPU
test asserts them, so a change of the oracle is noticed too.

The set is padded with further matching pairs to a PRIME length L: tiled over a batch, every case then walks through every lane, lane
pair, octet, wave and workgroup slot of the kernels.
"""
import collections
import functools
import hashlib
import json
import os

from oracle import bn254_model as m
from oracle import c_oracle as c
from tests import group_cases as gc

Q, R = m.Q, m.R
ST_OK, ST_GROUP, ST_MEMBER, ST_FAILED = m.OK, m.ERR_INVALID_GROUP_POINT, m.ERR_NOT_MEMBER, m.ERR_VERIFICATION_FAILED
FLAGS = (0, 1, 2, 3)                                          # bit 0: BN254_FLAG_G2_SUBGROUP_CHECK, bit 1: BN254_FLAG_REJECT_IDENTITY
Case = collections.namedtuple("Case", "pk_g2 pk_g1 name")
O1, O2 = bytes(64), bytes(128)

# status under flags 0 / 1 / 2 / 3, as the oracle gave them when the set was written
ANCHORS = {
    "matching pair": (0, 0, 0, 0),
    "different secrets": (9, 9, 9, 9),
    "pk_g1 negated": (9, 9, 9, 9),
    "both identity": (0, 0, 4, 4),
    "identity, valid pk_g1": (9, 9, 4, 4),
    "valid pk_g2, identity": (9, 9, 4, 4),
    "off-subgroup pk_g2, valid pk_g1": (9, 4, 9, 4),
    "valid pk_g2, off-curve pk_g1": (4, 4, 4, 4),
    "valid pk_g2, pk_g1 x >= q": (6, 6, 6, 6),
    "off-twist pk_g2, pk_g1 x >= q": (4, 4, 4, 4),
}
# both operands bad: name -> the flags value under which the two single-operand codes are meant to differ
ORDER_PAIRS = {
    "order: pk_g2 x >= q, off-curve pk_g1": 0,
    "off-twist pk_g2, pk_g1 x >= q": 0,
    "order: off-subgroup pk_g2, pk_g1 x >= q": 1,
    "order: pk_g2 y.im >= q, off-curve pk_g1": 0,
    "order: identity pk_g2, pk_g1 x >= q": 2,
    "order: pk_g2 x >= q, identity pk_g1": 2,
}


def be(v):
    return int(v).to_bytes(32, "big")


def _secret(tag):
    return int.from_bytes(hashlib.sha256(b"cpk-" + tag).digest(), "big") % (R - 1) + 1


def keys(sk):
    """(sk G2, sk G1) of a secret < 2^256, reduced mod r by the derivation"""
    return c.public_key_g2(be(sk)), c.public_key_g1(be(sk))


def _words(b):
    return [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]


def _join(w):
    return b"".join(be(v) for v in w)


def neg(b):
    """the negative of an uncompressed point of either group: every y coordinate negated"""
    w = _words(b)
    half = len(w) // 2
    return _join(w[:half] + [(-v) % Q for v in w[half:]])


def coord(b, idx, value):
    w = _words(b)
    w[idx] = value
    return _join(w)


def off_curve(b):
    """the last coordinate + 1: the same x, no point of the curve / the twist"""
    w = _words(b)
    out = coord(b, len(w) - 1, (w[-1] + 1) % Q)
    G = gc.G2 if len(b) == 128 else gc.G1
    assert G.decode(out)[0] == ST_GROUP
    return out


def _golden_not_in_subgroup():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derived_vectors.json")) as f:
        return bytes.fromhex(json.load(f)["g2_not_in_subgroup"])


def _is_prime(n):
    return n > 1 and all(n % d for d in range(2, int(n ** 0.5) + 1))


@functools.lru_cache(maxsize=None)
def cases():
    out = []

    def add(name, pk_g2, pk_g1):
        assert len(pk_g2) == 128 and len(pk_g1) == 64
        out.append(Case(bytes(pk_g2), bytes(pk_g1), name))

    sk = [_secret(b"%d" % i) for i in range(12)]
    k2, k1 = zip(*(keys(s) for s in sk))
    # ---- matching pairs
    add("matching pair", *keys(1))
    assert keys(1) == (c.g2_generator(), c.g1_generator())
    add("matching pair, sk = r - 1", *keys(R - 1))
    assert keys(R - 1) == (neg(c.g2_generator()), neg(c.g1_generator()))
    for i in range(4):
        add("matching pair, random %d" % i, k2[i], k1[i])
    for name, s in (("r + 5", R + 5), ("2^256 - 1", (1 << 256) - 1), ("random above r", R + sk[4] % ((1 << 256) - R))):
        assert R <= s < 1 << 256
        assert keys(s) == keys(s % R)                         # the reducing derivation, Fr::from_slice
        add("matching pair, sk >= r: " + name, *keys(s))
    # ---- mismatches
    add("different secrets", k2[5], k1[6])
    add("different secrets, sk and sk + 1", keys(sk[5])[0], keys(sk[5] + 1)[1])
    add("pk_g1 negated", k2[7], neg(k1[7]))
    add("pk_g2 negated", neg(k2[7]), k1[7])
    add("both negated", neg(k2[7]), neg(k1[7]))              # (-sk) G2 with (-sk) G1: matches again
    add("pk_g1 = 2 sk G1", k2[8], c.g1_add(k1[8], k1[8]))
    assert c.g1_add(k1[8], k1[8]) == c.public_key_g1(be(2 * sk[8] % R))
    # ---- identities
    add("both identity", O2, O1)
    add("identity, valid pk_g1", O2, k1[9])
    add("valid pk_g2, identity", k2[9], O1)
    add("identity, G1::one()", O2, c.g1_generator())
    # ---- decode faults in pk_g1, beside the matching pk_g2
    x1, y1 = _words(k1[10])
    add("valid pk_g2, off-curve pk_g1", k2[10], off_curve(k1[10]))
    add("valid pk_g2, pk_g1 x >= q", k2[10], coord(k1[10], 0, x1 + Q))       # reduced mod q it would be the matching key
    add("valid pk_g2, pk_g1 y >= q", k2[10], coord(k1[10], 1, y1 + Q))
    add("valid pk_g2, pk_g1 x == q", k2[10], coord(k1[10], 0, Q))
    add("valid pk_g2, pk_g1 x = 2^256 - 1", k2[10], coord(k1[10], 0, (1 << 256) - 1))
    # ---- decode faults in pk_g2, beside the matching pk_g1
    w2 = _words(k2[11])
    add("off-twist pk_g2, valid pk_g1", off_curve(k2[11]), k1[11])
    for idx, nm in enumerate(("x.re", "x.im", "y.re", "y.im")):
        add("pk_g2 %s >= q, valid pk_g1" % nm, coord(k2[11], idx, w2[idx] + Q), k1[11])
    outside = [_golden_not_in_subgroup()] + [gc.G2.enc(p) for p in gc.twist_points_outside_subgroup()]
    for b in outside:
        assert gc.G2.decode(b)[0] == ST_OK and c.g2_validate(b, 1) == ST_GROUP and c.g2_validate(b, 0) == ST_OK
    add("off-subgroup pk_g2, valid pk_g1", outside[0], k1[0])
    add("off-subgroup pk_g2 (1), valid pk_g1", outside[1], k1[1])
    add("off-subgroup pk_g2 (2), G1::one()", outside[2], c.g1_generator())
    add("off-subgroup pk_g2 (3), identity", outside[3], O1)
    add("off-subgroup pk_g2 (4), off-curve pk_g1", outside[4], off_curve(k1[2]))
    # ---- both operands bad, with different codes: pk_g2's is the one reported
    bad1_x = coord(k1[3], 0, _words(k1[3])[0] + Q)
    add("order: pk_g2 x >= q, off-curve pk_g1", coord(k2[3], 0, _words(k2[3])[0] + Q), off_curve(k1[3]))
    add("off-twist pk_g2, pk_g1 x >= q", off_curve(k2[3]), bad1_x)
    add("order: off-subgroup pk_g2, pk_g1 x >= q", outside[1], bad1_x)
    add("order: pk_g2 y.im >= q, off-curve pk_g1", coord(k2[4], 3, (1 << 256) - 1), off_curve(k1[4]))
    add("order: identity pk_g2, pk_g1 x >= q", O2, bad1_x)
    add("order: pk_g2 x >= q, identity pk_g1", coord(k2[4], 1, _words(k2[4])[1] + Q), O1)
    # ---- padding to a prime length: further matching pairs
    i = 0
    while not _is_prime(len(out)):
        add("matching pair, padding %d" % i, *keys(_secret(b"pad-%d" % i)))
        i += 1
    assert len({(cs.pk_g2, cs.pk_g1) for cs in out}) == len(out) == len({cs.name for cs in out})
    assert set(ANCHORS) | set(ORDER_PAIRS) <= {cs.name for cs in out}
    return tuple(out)


def length():
    """L: a prime"""
    return len(cases())


def names():
    return [cs.name for cs in cases()]


@functools.lru_cache(maxsize=None)
def expected(flags):
    """the oracle's status of every case under `flags`, as bytes"""
    return bytes(c.check_public_keys(cs.pk_g2, cs.pk_g1, flags) for cs in cases())


@functools.lru_cache(maxsize=None)
def order_pair_codes():
    """{name: (flags, code with only pk_g2's fault, code with only pk_g1's fault, code of the pair)}: each fault beside a VALID
    matching other operand, from the oracle"""
    good2, good1 = keys(_secret(b"order-good"))
    by = {cs.name: cs for cs in cases()}
    out = {}
    for name, flags in ORDER_PAIRS.items():
        cs = by[name]
        out[name] = (flags, c.check_public_keys(cs.pk_g2, good1, flags), c.check_public_keys(good2, cs.pk_g1, flags),
                     c.check_public_keys(cs.pk_g2, cs.pk_g1, flags))
    return out


@functools.lru_cache(maxsize=None)
def _columns():
    cs = cases()
    return [x.pk_g2 for x in cs], [x.pk_g1 for x in cs]


def tiled(n, flags, shift=0):
    """(pk_g2 bytes, pk_g1 bytes, expected bytes) of a batch of n items: case (i + shift) % L at item i"""
    g2, g1 = _columns()
    want, ln = expected(flags), len(g2)
    idx = [(i + shift) % ln for i in range(n)]
    return b"".join(g2[j] for j in idx), b"".join(g1[j] for j in idx), bytes(want[j] for j in idx)


def case_at(i, shift=0):
    return cases()[(i + shift) % length()]


def first_difference(got, want, shift=0):
    """None, or a short description of the first item whose status differs (with its case name), and how many differ"""
    if got == want:
        return None
    assert len(got) == len(want), (len(got), len(want))
    bad = [i for i in range(len(want)) if got[i] != want[i]]
    i = bad[0]
    return "item %d of %d (%s): got %d, want %d; %d items differ" % (i, len(want), case_at(i, shift).name, got[i], want[i], len(bad))


def histogram(flags):
    return dict(sorted(collections.Counter(expected(flags)).items()))
