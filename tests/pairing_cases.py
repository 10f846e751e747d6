"""One case set for the pairing products (bn254_batch_pairing, _check, _device; bn::pairing_batch as the reference calls it at
src/ecdsa.rs:57 and :86), shared by the CPU test (the kernel bodies compiled for the host: tests/test_pairing_cases.py) and the GPU
test (every route of the call: tests/test_gpu_pairing.py): the same bytes and the same expected status and Gt on both sides.

A case is Case(g1, g2, k, name): k * 64 and k * 128 uncompressed bytes, k pairs of one item, all-zero = the identity of the batch ABI.
Points are multiples of the generators made by oracle/c_oracle.py; every fault is made here on the bytes.  The EXPECTED status and Gt
of a case under a flags value (bit 0 = G2 subgroup check, bit 1 = reject identities) are oracle.c_oracle.batch_pairing and nothing
else: inside a pair G1 is decoded before G2, across the pairs of an item the lowest index comes first, the first fault is the status,
else 0 / 9 from prod_j e(g1[j], g2[j]) == 1, a pair with an identity operand contributing one.  Nothing here imports the library under
test or its host build.

For an item whose status is a decode error the oracle has no Gt.  include/bn254_hip.h defines one: the product with the GENERATOR in
place of every operand that did not decode.  gt_of_failed() restates that with the oracle's validators and the oracle's pairing.

No reference vector holds a product of more than two pairs, an identity operand or a fault under these calls: those statuses are
UNPINNED beyond the oracle's restatement.  ANCHORS below are the statuses the oracle gave when the set was written; the CPU test
asserts them, so a change of the oracle is noticed too.

The cases of each k are padded with generic products to a PRIME count: tiled over a batch, every case then walks through every lane,
lane pair, wave and workgroup slot of the kernels.
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
KS = (1, 2, 3, 4)
Case = collections.namedtuple("Case", "g1 g2 k name")
O1, O2 = bytes(64), bytes(128)
NTHREADS = 8

# status under flags 0 / 1 / 2 / 3, as the oracle gave them when the set was written
ANCHORS = {
    "k=1: generic 0": (9, 9, 9, 9),
    "k=1: every pair both identities": (0, 0, 4, 4),
    "k=1: identity G1 in pair 0": (0, 0, 4, 4),
    "k=1: G2 off the subgroup in pair 0": (9, 4, 9, 4),
    "k=1: G1 x >= q in pair 0": (6, 6, 6, 6),
    "k=2: e(aP,Q) e(-aP,Q)": (0, 0, 0, 0),
    "k=2: e(aP,Q) e(P,-aQ)": (0, 0, 0, 0),
    "k=2: identity G2 in pair 1": (9, 9, 4, 4),
    "k=2: G2 off the twist in pair 1": (4, 4, 4, 4),
    "k=2: order: G2 off the twist in pair 0, G1 x >= q in pair 1": (4, 4, 4, 4),
    "k=2: order: G2 x.re >= q in pair 0, G1 off the curve in pair 1": (6, 6, 6, 6),
    "k=2: order: G2 off the subgroup in pair 0, G1 x >= q in pair 1": (6, 4, 6, 4),
    "k=3: e(aP,Q) e(bP,Q) e(-(a+b)P,Q)": (0, 0, 0, 0),
    "k=3: cancelling pairs around an identity pair": (0, 0, 4, 4),
    "k=3: G2 y.im >= q in pair 2": (6, 6, 6, 6),
    "k=3: order: identity G1 in pair 0, G1 x >= q in pair 2": (6, 6, 4, 4),
    "k=3: order: G1 x >= q in pair 0, identity G1 in pair 2": (6, 6, 6, 6),
    "k=4: e(aP,Q) e(bP,Q) e(cP,Q) e(-(a+b+c)P,Q)": (0, 0, 0, 0),
    "k=4: e(aP,Q) e(-aP,Q) e(bP',Q') e(P',-bQ')": (0, 0, 0, 0),
    "k=4: every pair both identities": (0, 0, 4, 4),
    "k=4: G1 off the curve in pair 2": (4, 4, 4, 4),
    "k=4: G2 off the subgroup in pair 3": (9, 4, 9, 4),
    "k=4: P and -P with the same Q, first and last pair": (9, 9, 9, 9),
}


def be(v):
    return int(v).to_bytes(32, "big")


def _scalar(tag):
    return int.from_bytes(hashlib.sha256(b"pairing-" + tag).digest(), "big") % (R - 1) + 1


@functools.lru_cache(maxsize=None)
def g1_of(a):
    """a * G1::one(), a taken mod r"""
    return c.g1_mul(c.g1_generator(), be(a % R))


@functools.lru_cache(maxsize=None)
def g2_of(b):
    return c.g2_mul(c.g2_generator(), be(b % R))


def _words(b):
    return [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]


def _join(w):
    return b"".join(be(v) for v in w)


def neg(b):
    """the negative of an uncompressed point of either group: every y coordinate negated"""
    if b in (O1, O2):
        return b
    w = _words(b)
    half = len(w) // 2
    return _join(w[:half] + [(-v) % Q for v in w[half:]])


def coord(b, idx, value):
    w = _words(b)
    w[idx] = value
    return _join(w)


def above_q(b, idx):
    """coordinate idx + q: reduced mod q it would be the same point"""
    out = coord(b, idx, _words(b)[idx] + Q)
    G = gc.G2 if len(b) == 128 else gc.G1
    assert G.decode(out)[0] == ST_MEMBER
    return out


def off_curve(b):
    """the last coordinate + 1: the same x, no point of the curve / the twist"""
    w = _words(b)
    out = coord(b, len(w) - 1, (w[-1] + 1) % Q)
    G = gc.G2 if len(b) == 128 else gc.G1
    assert G.decode(out)[0] == ST_GROUP
    return out


@functools.lru_cache(maxsize=None)
def outside_subgroup():
    """points of the twist outside the order-r subgroup: the golden one, then tests/group_cases.py's"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "derived_vectors.json")) as f:
        out = [bytes.fromhex(json.load(f)["g2_not_in_subgroup"])]
    out += [gc.G2.enc(p) for p in gc.twist_points_outside_subgroup()]
    for b in out:
        assert gc.G2.decode(b)[0] == ST_OK and c.g2_validate(b, 1) == ST_GROUP and c.g2_validate(b, 0) == ST_OK
    return tuple(out)


G2_COORDS = ("x.re", "x.im", "y.re", "y.im")
# single faults: name -> (group, what it does to the operand's bytes; `j` numbers the placements for the off-subgroup points)
FAULTS = collections.OrderedDict([
    ("G1 off the curve", (1, lambda b, j: off_curve(b))),
    ("G1 x >= q", (1, lambda b, j: above_q(b, 0))),
    ("G1 y >= q", (1, lambda b, j: above_q(b, 1))),
    ("G2 off the twist", (2, lambda b, j: off_curve(b))),
    ("G2 x.re >= q", (2, lambda b, j: above_q(b, 0))),
    ("G2 x.im >= q", (2, lambda b, j: above_q(b, 1))),
    ("G2 y.re >= q", (2, lambda b, j: above_q(b, 2))),
    ("G2 y.im >= q", (2, lambda b, j: above_q(b, 3))),
    ("G2 off the subgroup", (2, lambda b, j: outside_subgroup()[j % len(outside_subgroup())])),
    ("identity G1", (1, lambda b, j: O1)),
    ("identity G2", (2, lambda b, j: O2)),
])


def placements(k):
    """the first, a middle and the last pair of an item of k pairs"""
    return sorted({0, k // 2, k - 1})


def _is_prime(n):
    return n > 1 and all(n % d for d in range(2, int(n ** 0.5) + 1))


class _Builder:
    def __init__(self, k):
        self.k, self.out, self.order, self.n_fresh = k, [], {}, 0

    def fresh(self, count=None):
        """`count` (default k) pairs of points no other case of this k uses"""
        ps, qs = [], []
        for _ in range(self.k if count is None else count):
            ps.append(g1_of(_scalar(b"p-%d-%d" % (self.k, self.n_fresh))))
            qs.append(g2_of(_scalar(b"q-%d-%d" % (self.k, self.n_fresh))))
            self.n_fresh += 1
        return ps, qs

    def add(self, name, ps, qs):
        assert len(ps) == len(qs) == self.k and all(len(p) == 64 for p in ps) and all(len(q) == 128 for q in qs), name
        self.out.append(Case(b"".join(ps), b"".join(qs), self.k, "k=%d: %s" % (self.k, name)))

    def fault(self, ps, qs, kind, j, serial=0):
        """a copy of the item with fault `kind` in pair j"""
        group, make = FAULTS[kind]
        ps, qs = list(ps), list(qs)
        if group == 1:
            ps[j] = make(ps[j], serial)
        else:
            qs[j] = make(qs[j], serial)
        return ps, qs

    def add_order(self, flags, first, second):
        """both faults in one item; `first` = (kind, pair) comes earlier in the oracle's order than `second`.  Recorded with the two
        items that carry one of the faults each, for order_pair_codes()"""
        ps, qs = self.fresh()
        (k1, j1), (k2, j2) = first, second
        assert (j1, FAULTS[k1][0]) < (j2, FAULTS[k2][0])
        a, b = self.fault(ps, qs, k1, j1, 1), self.fault(ps, qs, k2, j2, 1)
        both = self.fault(*a, k2, j2, 1)
        name = "order: %s in pair %d, %s in pair %d" % (k1, j1, k2, j2)
        self.add(name, *both)
        self.order["k=%d: %s" % (self.k, name)] = (flags, (b"".join(a[0]), b"".join(a[1])), (b"".join(b[0]), b"".join(b[1])))


def _build(k):
    b = _Builder(k)
    pos = placements(k)
    last = k - 1
    # ---- generic products
    for i in range(3):
        b.add("generic %d" % i, *b.fresh())
    # ---- products that are one by bilinearity
    s = [_scalar(b"s-%d-%d" % (k, i)) for i in range(8)]
    if k == 2:
        (P,), (Qq,) = b.fresh(1)
        b.add("e(aP,Q) e(-aP,Q)", [g1_of(s[0]), neg(g1_of(s[0]))], [Qq, Qq])
        b.add("e(aP,Q) e(P,-aQ)", [g1_of(s[1] * s[2]), g1_of(s[2])], [g2_of(s[3]), neg(g2_of(s[1] * s[3]))])
        b.add("e(-aP,Q) e(aP,Q), the negative first", [neg(P), P], [Qq, Qq])
    if k == 3:
        (_,), (Qq,) = b.fresh(1)
        b.add("e(aP,Q) e(bP,Q) e(-(a+b)P,Q)", [g1_of(s[0]), g1_of(s[1]), neg(g1_of(s[0] + s[1]))], [Qq, Qq, Qq])
        b.add("e(aP,Q) e(P,bQ) e(-P,(a+b)Q)", [g1_of(s[2] * s[4]), g1_of(s[4]), neg(g1_of(s[4]))],
              [g2_of(s[5]), g2_of(s[3] * s[5]), g2_of((s[2] + s[3]) * s[5])])
        (P,), (Qq,) = b.fresh(1)
        (P2,), (Q2,) = b.fresh(1)
        b.add("cancelling pairs around an identity pair", [P, O1, neg(P)], [Qq, Q2, Qq])
        b.add("cancelling pairs around an identity G2", [P2, P, neg(P2)], [Q2, O2, Q2])
    if k == 4:
        (_,), (Qq,) = b.fresh(1)
        b.add("e(aP,Q) e(bP,Q) e(cP,Q) e(-(a+b+c)P,Q)", [g1_of(s[0]), g1_of(s[1]), g1_of(s[2]), neg(g1_of(s[0] + s[1] + s[2]))], [Qq] * 4)
        b.add("e(aP,Q) e(-aP,Q) e(bP',Q') e(P',-bQ')", [g1_of(s[3]), neg(g1_of(s[3])), g1_of(s[4] * s[5]), g1_of(s[5])],
              [Qq, Qq, g2_of(s[6]), neg(g2_of(s[4] * s[6]))])
        (P, P2), (Qq, Q2) = b.fresh(2)
        b.add("two cancelling couples, interleaved", [P, P2, neg(P), neg(P2)], [Qq, Q2, Qq, Q2])
        b.add("cancelling pairs around two identity pairs", [P, O1, P2, neg(P)], [Qq, Q2, O2, Qq])
    # ---- P and -P paired with the same Q inside one item, beside pairs that do not cancel
    if k >= 2:
        ps, qs = b.fresh()
        ps[last], qs[last] = neg(ps[0]), qs[0]
        b.add("P and -P with the same Q, first and last pair", ps, qs)
        ps, qs = b.fresh()
        ps[1], qs[1] = neg(ps[0]), qs[0]
        b.add("P and -P with the same Q, pairs 0 and 1", ps, qs)
        ps, qs = b.fresh()
        ps[last], qs[last] = ps[0], neg(qs[0])
        b.add("P with Q and with -Q, first and last pair", ps, qs)
    # ---- identity operands
    for j in pos:
        ps, qs = b.fresh()
        b.add("identity G1 in pair %d" % j, *b.fault(ps, qs, "identity G1", j))
        b.add("identity G2 in pair %d" % j, *b.fault(ps, qs, "identity G2", j))
        if k > 1:                                             # k = 1: "every pair both identities" below
            b.add("both identities in pair %d" % j, *b.fault(*b.fault(ps, qs, "identity G1", j), "identity G2", j))
    ps, qs = b.fresh()
    b.add("every pair both identities", [O1] * k, [O2] * k)
    b.add("every pair an identity G1", [O1] * k, qs)
    b.add("every pair an identity G2", ps, [O2] * k)
    if k >= 2:
        b.add("every pair an identity, G1 and G2 in turn", [O1 if j % 2 == 0 else ps[j] for j in range(k)], [qs[j] if j % 2 == 0 else O2 for j in range(k)])
    # ---- single faults, in the first, a middle and the last pair
    serial = 0
    for kind in list(FAULTS)[:9]:
        for j in pos:
            ps, qs = b.fresh()
            b.add("%s in pair %d" % (kind, j), *b.fault(ps, qs, kind, j, serial))
            serial += 1
    (P,), (_,) = b.fresh(1)
    b.add("G1 x == q in pair %d" % last, *(lambda ps, qs: (ps[:last] + [coord(P, 0, Q)], qs))(*b.fresh()))
    b.add("G1 x = 2^256 - 1 in pair 0", *(lambda ps, qs: ([coord(P, 0, (1 << 256) - 1)] + ps[1:], qs))(*b.fresh()))
    if k >= 2:                                                # a product over a point outside the subgroup that the oracle may call one
        ps, qs = b.fresh()
        T = outside_subgroup()[1]
        ps[1], qs[0], qs[1] = neg(ps[0]), T, T
        b.add("P and -P with the same G2 off the subgroup", ps, qs)
    # ---- two faults whose codes differ under the named flags value: the earlier one is reported
    for j in pos:                                             # G1 and G2 of the same pair
        b.add_order(0, ("G1 x >= q", j), ("G2 off the twist", j))
        b.add_order(0, ("G1 off the curve", j), ("G2 x.im >= q", j))
    b.add_order(1, ("G1 y >= q", last), ("G2 off the subgroup", last))
    b.add_order(2, ("identity G1", 0), ("G2 x.re >= q", 0))
    b.add_order(2, ("G1 x >= q", last), ("identity G2", last))
    if k >= 2:
        for j in pos[:-1]:                                    # G2 of one pair, G1 of the next
            b.add_order(0, ("G2 off the twist", j), ("G1 x >= q", j + 1))
            b.add_order(0, ("G2 x.re >= q", j), ("G1 off the curve", j + 1))
        b.add_order(0, ("G2 y.im >= q", 0), ("G1 off the curve", last))
        b.add_order(2, ("identity G1", 0), ("G1 x >= q", last))
        b.add_order(2, ("G1 x >= q", 0), ("identity G1", last))
        b.add_order(2, ("identity G2", 0), ("G2 x.im >= q", last))
        b.add_order(1, ("G2 off the subgroup", 0), ("G1 x >= q", 1))
        b.add_order(1, ("G2 off the subgroup", 0), ("G2 y.re >= q", last))
    # ---- padding to a prime count: further generic products
    i = 0
    while not _is_prime(len(b.out)):
        b.add("generic, padding %d" % i, *b.fresh())
        i += 1
    assert len({(cs.g1, cs.g2) for cs in b.out}) == len(b.out) == len({cs.name for cs in b.out})
    return tuple(b.out), b.order


@functools.lru_cache(maxsize=None)
def _built(k):
    return _build(k)


def cases_of(k):
    """the cases of k pairs per item; their count is a prime"""
    return _built(k)[0]


def cases():
    return tuple(cs for k in KS for cs in cases_of(k))


def names(k=None):
    return [cs.name for cs in (cases() if k is None else cases_of(k))]


def order_pairs():
    """{name: flags value under which the two single-fault codes are meant to differ}"""
    return {name: v[0] for k in KS for name, v in _built(k)[1].items()}


def _oracle(cs, k, flags):
    gt, st = c.batch_pairing(b"".join(x.g1 for x in cs), b"".join(x.g2 for x in cs), len(cs), k, flags, nthreads=NTHREADS)
    return st, tuple(gt[384 * i:384 * i + 384] for i in range(len(cs)))


@functools.lru_cache(maxsize=None)
def expected(k, flags):
    """(statuses as bytes, Gt of every case) of the cases of k under `flags`, from the oracle; its Gt of a failed item is all-zero"""
    return _oracle(cases_of(k), k, flags)


def substituted(cs, flags):
    """the case with the generator in place of every operand that the oracle's decoder refuses under `flags`"""
    g1 = b"".join(p if c.g1_validate(p, flags) == ST_OK else c.g1_generator() for p in (cs.g1[64 * j:64 * j + 64] for j in range(cs.k)))
    g2 = b"".join(q if c.g2_validate(q, flags) == ST_OK else c.g2_generator() for q in (cs.g2[128 * j:128 * j + 128] for j in range(cs.k)))
    return Case(g1, g2, cs.k, cs.name)


@functools.lru_cache(maxsize=None)
def gt_of_failed(k, flags):
    """{index into cases_of(k): Gt} for the cases whose status under `flags` is a decode error: the oracle's product of the substituted
    item (include/bn254_hip.h, at bn254_batch_pairing)"""
    st = expected(k, flags)[0]
    idx = [i for i in range(len(st)) if st[i] not in (ST_OK, ST_FAILED)]
    sub = [substituted(cases_of(k)[i], flags) for i in idx]
    st2, gt = _oracle(sub, k, 0) if sub else (b"", ())
    assert all(s in (ST_OK, ST_FAILED) for s in st2)
    return dict(zip(idx, gt))


@functools.lru_cache(maxsize=None)
def full_gt(k, flags):
    """the Gt bytes the header promises for every case of k: the oracle's where the status is 0 or 9, gt_of_failed elsewhere"""
    gt, failed = list(expected(k, flags)[1]), gt_of_failed(k, flags)
    for i, g in failed.items():
        gt[i] = g
    return tuple(gt)


@functools.lru_cache(maxsize=None)
def order_pair_codes():
    """{name: (flags, status with only the earlier fault, status with only the later fault, status of the case)}, from the oracle"""
    out = {}
    for k in KS:
        nm = names(k)
        for name, (flags, a, b) in _built(k)[1].items():
            st = expected(k, flags)[0]
            out[name] = (flags, c.batch_pairing(a[0], a[1], 1, k, flags)[1][0], c.batch_pairing(b[0], b[1], 1, k, flags)[1][0], st[nm.index(name)])
    return out


def tile(cases_of_k, n, shift=0):
    """(g1 bytes, g2 bytes, indices) of a batch of n items: case (i + shift) % L at item i"""
    ln = len(cases_of_k)
    idx = [(i + shift) % ln for i in range(n)]
    return b"".join(cases_of_k[j].g1 for j in idx), b"".join(cases_of_k[j].g2 for j in idx), idx


@functools.lru_cache(maxsize=None)
def tiled(k, n, flags, shift=0):
    """(g1 bytes, g2 bytes, expected statuses, expected Gt bytes — full_gt —, indices) of the cases of k tiled over n items"""
    g1, g2, idx = tile(cases_of(k), n, shift)
    st, gt = expected(k, flags)[0], full_gt(k, flags)
    return g1, g2, bytes(st[j] for j in idx), b"".join(gt[j] for j in idx), tuple(idx)


def first_difference(k, idx, got, want, width=1):
    """None, or a short description of the first item whose status (width 1) or Gt (width 384) differs, with its case name"""
    if got == want:
        return None
    assert len(got) == len(want) == width * len(idx), (len(got), len(want), len(idx))
    bad = [i for i in range(len(idx)) if got[width * i:width * (i + 1)] != want[width * i:width * (i + 1)]]
    i = bad[0]
    what = "got %d, want %d" % (got[i], want[i]) if width == 1 else "Gt differs"
    return "item %d of %d (%s): %s; %d items differ" % (i, len(idx), cases_of(k)[idx[i]].name, what, len(bad))


def histogram(k, flags):
    return dict(sorted(collections.Counter(expected(k, flags)[0]).items()))


# ---- items longer than the oracle's MAX_PAIRS ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_pair(seed, j):
    a, b = _scalar(b"long-a-%d-%d" % (seed, j)), _scalar(b"long-b-%d-%d" % (seed, j))
    return a, b, g1_of(a), g2_of(b)


@functools.lru_cache(maxsize=None)
def long_item(k, seed, one=False):
    """(g1 bytes, g2 bytes, expected status, expected Gt) of ONE item of k pairs (a_j G1::one(), b_j G2::one()).  By bilinearity its
    product is e((sum a_j b_j mod r) G1::one(), G2::one()): ONE oracle pairing, whatever k.  one=True: the last pair is
    (-(sum of the others) G1::one(), G2::one()) and cancels the rest — Gt one, status 0.  Items of one seed share their first pairs."""
    assert k >= 2
    pairs = [_long_pair(seed, j) for j in range(k - 1 if one else k)]
    total = sum(a * b for a, b, _, _ in pairs) % R
    ps, qs = [p for _, _, p, _ in pairs], [q for _, _, _, q in pairs]
    if one:
        ps.append(neg(g1_of(total)))
        qs.append(c.g2_generator())
        total = 0
    assert one or total != 0
    gt, st = c.batch_pairing(g1_of(total) if total else O1, c.g2_generator(), 1, 1, 0)
    assert st[0] == (ST_OK if one else ST_FAILED)
    return b"".join(ps), b"".join(qs), st[0], gt
