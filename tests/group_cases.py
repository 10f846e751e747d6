"""One case builder for the group operations and the Fq12 hook, shared by the CPU tests (the device source compiled for the host,
tests/test_hostsim_group.py) and the GPU tests (tests/test_gpu_group_ops.py): the same inputs and the same expected outputs on both
sides, so that a CPU-only failure, a GPU-only failure (the wave vote, the compiler) and a failure on both mean different things.

Every expected value comes from oracle/bn254_model.py (affine big-integer arithmetic) — the edges — or from oracle/c_oracle.py — the
bulk of the random multiplications —, and each records which (`src`).  Nothing here imports the library under test or its host build;
tests/test_group_cases.py checks that, the presence of every named kind of case, and the agreement of the two oracles.

Statuses: 6 = NotMemberError (a coordinate >= q), 4 = InvalidGroupPoint (not on the curve).  Of two faulty operands the first
one's code is reported (`a` before `b`; in a sum the earliest point), the order in which the reference decodes its arguments.
"""
import functools
import hashlib
import random

from oracle import bn254_model as m
from oracle import c_oracle as c

Q, R = m.Q, m.R
WAVE = 64
ST_OK, ST_GROUP, ST_MEMBER = m.OK, m.ERR_INVALID_GROUP_POINT, m.ERR_NOT_MEMBER


def be(v):
    return int(v).to_bytes(32, "big")


class Group:
    """the model's view of one group: encoding, arithmetic, decoder"""

    def __init__(self, name):
        self.name = name
        g2 = name == "g2"
        self.size = 128 if g2 else 64
        self.zero = bytes(self.size)
        self.gen = m.G2_GEN if g2 else m.G1_GEN
        self.add, self.mul, self.neg = (m.g2_add, m.g2_mul, m.g2_neg) if g2 else (m.g1_add, m.g1_mul, m.g1_neg)
        self.c_add, self.c_mul = (c.g2_add, c.g2_mul) if g2 else (c.g1_add, c.g1_mul)
        self._g2 = g2

    def enc(self, p):
        if p is None:
            return self.zero
        return m.g2_to_uncompressed(p) if self._g2 else m.g1_to_uncompressed(p)

    def decode(self, b):
        """(status, point): all-zero bytes are the identity of the batch ABI; otherwise the model's from_uncompressed without
        the subgroup check (the group entry points take any point of the curve / the twist)"""
        if b == self.zero:
            return ST_OK, None
        try:
            return ST_OK, (m.g2_from_uncompressed(b, subgroup_check=False) if self._g2 else m.g1_from_uncompressed(b))
        except m.Bn254Error as e:
            return e.code, None

    def words(self, b):
        return [int.from_bytes(b[i:i + 32], "big") for i in range(0, self.size, 32)]

    def from_words(self, w):
        return b"".join(be(v) for v in w)


G1, G2 = Group("g1"), Group("g2")


def _scalar(tag):
    return int.from_bytes(hashlib.sha256(tag).digest(), "big") % R


def chain(G, tag, n):
    """n points P0 + i D of the order-r subgroup (P0, D = hashed multiples of the generator): one affine addition each"""
    p, d = G.mul(G.gen, _scalar(b"p0-" + tag)), G.mul(G.gen, _scalar(b"d-" + tag))
    out = []
    for _ in range(n):
        out.append(p)
        p = G.add(p, d)
    return out


@functools.lru_cache(maxsize=None)
def twist_points_outside_subgroup(n=4):
    """points of the twist y^2 = x^3 + 3/xi that are not in the order-r subgroup (the cofactor is 2q - r: a random one never is)"""
    rnd, out = random.Random(2024), []
    while len(out) < n:
        x = (rnd.randrange(Q), rnd.randrange(Q))
        y = m.f2_sqrt(m.f2_add(m.f2_mul(m.f2_mul(x, x), x), m.B2))
        if y is None:
            continue
        p = (x, y)
        assert m.g2_on_curve(p) and not m.g2_in_subgroup(p)
        out.append(p)
    return tuple(out)


# ---- additions -------------------------------------------------------------------------------------------------------------------
ADD_KINDS = ("P+P", "P+(-P)", "O+P", "P+O", "O+O", "a>=q", "b off curve", "a>=q, b off curve", "a off curve, b>=q", "coordinate == q",
             "x == 0, y != 0")
ADD_STATUS_KINDS = ADD_KINDS[5:10]
ADD_SIZES = (1, 63, 64, 65, 200)


def _off_curve(G, p):
    w = G.words(G.enc(p))
    w[-1] = (w[-1] + 1) % Q
    b = G.from_words(w)
    assert G.decode(b)[0] == ST_GROUP
    return b


def _coord(G, p, idx, value):
    w = G.words(G.enc(p))
    w[idx] = value
    return G.from_words(w)


def _x_zero_point(G):
    """x = 0 with y != 0: a point of the curve when b has a square root (then it is an ordinary operand), off the curve otherwise"""
    if G is G1:
        y = m.fq_sqrt(m.B1)
        return G.from_words([0, y if y is not None else 1])
    y = m.f2_sqrt(m.B2)
    y = y if y is not None else (1, 0)
    return G.from_words([0, 0, y[0], y[1]])


def _add_case(G, kind, pool, i):
    """(a bytes, b bytes) of one case of `kind`; i varies the operands and, for the status cases, the faulty coordinate"""
    nw = G.size // 32
    p, q = pool[(2 * i) % len(pool)], pool[(2 * i + 1) % len(pool)]
    P, Qb = G.enc(p), G.enc(q)
    if kind == "ordinary":
        return P, Qb
    if kind == "P+P":
        return P, P
    if kind == "P+(-P)":
        return P, G.enc(G.neg(p))
    if kind == "O+P":
        return G.zero, P
    if kind == "P+O":
        return P, G.zero
    if kind == "O+O":
        return G.zero, G.zero
    if kind == "a>=q":
        return _coord(G, p, i % nw, Q + 1 + i), Qb
    if kind == "b off curve":
        return P, _off_curve(G, q)
    if kind == "a>=q, b off curve":
        return _coord(G, p, (i + 1) % nw, (1 << 256) - 1 - i), _off_curve(G, q)
    if kind == "a off curve, b>=q":
        return _off_curve(G, p), _coord(G, q, i % nw, Q + 7)
    if kind == "coordinate == q":
        return (P, _coord(G, q, i % nw, Q)) if i & 1 else (_coord(G, p, i % nw, Q), Qb)
    if kind == "x == 0, y != 0":
        return (_x_zero_point(G), Qb) if i & 1 else (P, _x_zero_point(G))
    raise KeyError(kind)


def _add_expect(G, a, b):
    sa, pa = G.decode(a)
    sb, pb = G.decode(b)
    st = sa if sa != ST_OK else sb
    return (G.zero if st != ST_OK else G.enc(G.add(pa, pb))), st


def _add_batches(G, pool, extra_ordinary):
    """list of batches, each a list of items {kind, a, b, want, status}.  Layouts (waves of 64 lanes; a FAILED lane is exceptional
    too: the kernel replaces its operands by generator + generator, the doubling case):
      n = 1    one batch per kind (the one-item launch of the typed API);
      n = 63   ordinary lanes and ONE exceptional lane, one batch per kind;
      n = 64   a wave with no exceptional lane (the vote says no), and a wave of exceptional lanes only;
      n = 65   a full ordinary wave, and a second wave that is one exceptional lane, one batch per kind;
      n = 200  wave 0 none, wave 1 only exceptional lanes, wave 2 exactly one (P+P), the ragged wave 3 exactly one (P+(-P))."""
    counter = [0]

    def item(kind):
        i = counter[0]
        counter[0] += 1
        if kind == "ordinary" and extra_ordinary and i % 9 == 4:
            a, b = G.enc(extra_ordinary[0]), G.enc(extra_ordinary[1])
            kind = "ordinary, outside the subgroup"
        else:
            a, b = _add_case(G, kind, pool, i)
        want, st = _add_expect(G, a, b)
        return {"kind": kind, "a": a, "b": b, "want": want, "status": st}

    batches = [[item(k)] for k in ("ordinary",) + ADD_KINDS]
    for j, k in enumerate(ADD_KINDS):
        lane = (5 * j + 3) % 63
        batches.append([item(k if t == lane else "ordinary") for t in range(63)])
    batches.append([item("ordinary") for _ in range(64)])
    batches.append([item(ADD_KINDS[t % len(ADD_KINDS)]) for t in range(64)])
    for k in ADD_KINDS:
        batches.append([item("ordinary") for _ in range(64)] + [item(k)])
    big = [item("ordinary") for _ in range(64)] + [item(ADD_KINDS[(t * 7) % len(ADD_KINDS)]) for t in range(64)]
    big += [item("P+P" if t == 17 else "ordinary") for t in range(64)] + [item("P+(-P)" if t == 5 else "ordinary") for t in range(8)]
    batches.append(big)
    assert sorted({len(b) for b in batches}) == list(ADD_SIZES)
    return batches


@functools.lru_cache(maxsize=None)
def add_batches(group):
    G = G2 if group == "g2" else G1
    pool = chain(G, b"add-" + group.encode(), 48)
    return _add_batches(G, pool, twist_points_outside_subgroup()[:2] if G is G2 else None)


def wave_profile(batch, exceptional):
    """per wave of a batch: how many lanes are exceptional"""
    return [sum(1 for it in batch[w:w + WAVE] if exceptional(it)) for w in range(0, len(batch), WAVE)]


def _jac(G, p, lam, ident=None):
    """Jacobian triple bytes of p scaled by lam: (lam^2 x, lam^3 y, lam); p None: the identity as (X, Y, 0) with X, Y = ident"""
    fq2 = G is G2
    one = (1, 0) if fq2 else 1
    mul = m.f2_mul if fq2 else (lambda a, b: a * b % Q)
    enc = (lambda v: be(v[0]) + be(v[1])) if fq2 else be
    if p is None:
        zero = (0, 0) if fq2 else 0
        return enc(ident[0]) + enc(ident[1]) + enc(zero)
    l2 = mul(lam, lam)
    return enc(mul(p[0], l2)) + enc(mul(p[1], mul(l2, lam))) + enc(mul(one, lam))


@functools.lru_cache(maxsize=None)
def jacobian_add_cases(group):
    """[{kind, p, q, want}] for jac_add itself, on operands no byte decoder produces: the identity as ANY triple with Z = 0 (the documented
    meaning of Z = 0, bn254_curve.h) — among them X = 0, and the other operand's own X and Y, where the P = -Q test fires as well and the
    priority of the overrides decides — and points with Z != 1 on either side.  Host build only: no entry point takes Jacobian input."""
    G = G2 if group == "g2" else G1
    fq2 = G is G2
    rnd = random.Random(31 if fq2 else 30)
    fe = (lambda: (rnd.randrange(1, Q), rnd.randrange(Q))) if fq2 else (lambda: rnd.randrange(1, Q))
    lift = (lambda v: (v, 0)) if fq2 else (lambda v: v)
    p, q = chain(G, b"jac-" + group.encode(), 2)
    idents = [(lift(1), lift(1)), (lift(0), lift(1)), (lift(0), lift(0)), (lift(1), lift(0)), (fe(), fe()), (p[0], p[1]), (p[0], G.neg(p)[1]), (q[0], q[1])]
    cases = []
    for i, ident in enumerate(idents):
        for lam in (lift(1), fe()):
            cases.append({"kind": "O + P", "p": _jac(G, None, None, ident), "q": _jac(G, p, lam), "want": G.enc(p)})
            cases.append({"kind": "P + O", "p": _jac(G, p, lam), "q": _jac(G, None, None, ident), "want": G.enc(p)})
        cases.append({"kind": "O + O", "p": _jac(G, None, None, ident), "q": _jac(G, None, None, idents[(i + 3) % len(idents)]), "want": G.zero})
    for _ in range(6):
        l1, l2 = fe(), fe()
        cases.append({"kind": "P + Q", "p": _jac(G, p, l1), "q": _jac(G, q, l2), "want": G.enc(G.add(p, q))})
        cases.append({"kind": "P + P", "p": _jac(G, p, l1), "q": _jac(G, p, l2), "want": G.enc(G.add(p, p))})
        cases.append({"kind": "P + (-P)", "p": _jac(G, p, l1), "q": _jac(G, G.neg(p), l2), "want": G.zero})
        cases.append({"kind": "P + Q", "p": _jac(G, q, lift(1)), "q": _jac(G, p, l2), "want": G.enc(G.add(p, q))})
    return cases


# ---- G2 multiplication -----------------------------------------------------------------------------------------------------------
def window_digits(k):
    """the signed 4-bit recoding of jac_mul_window<8, true> (bn254_curve.h): digits in [-8, 8], index 64 = the final carry"""
    digits, carry = [], 0
    for j in range(64):
        v = ((k >> (4 * j)) & 15) + carry
        carry = 1 if v > 8 else 0
        digits.append(v - 16 * carry)
    digits.append(carry)
    assert sum(d * 16 ** j for j, d in enumerate(digits)) == k
    return digits


def ladder_hits(k):
    """windows at which the ladder, on a point of order r, adds a table entry to an accumulator that holds the same point
    ("doubling") or its negative ("cancellation"): [(window, kind)] — the accumulator is 16 x prefix, compared mod r"""
    digits, acc, hits = window_digits(k), 0, []
    for j in range(64, -1, -1):
        if j != 64:
            acc *= 16
        d = digits[j]
        if d and acc % R:
            if (acc - d) % R == 0:
                hits.append((j, "doubling"))
            if (acc + d) % R == 0:
                hits.append((j, "cancellation"))
        acc += d
    assert acc == k
    return hits


@functools.lru_cache(maxsize=None)
def ladder_hit_scalars():
    """k < 2^256 with a hit: the accumulator before window j is m r +- d (d the digit), a multiple of 16 below 2^256 / 16^j — with
    r > 2^253 that leaves the last window only.  Candidates are built from that equation and kept if the restated recoding agrees."""
    out = {}
    for mult in range(1, 6):
        for d in range(-8, 9):
            for acc in (mult * R + d, mult * R - d):
                k = acc + d
                if d and acc % 16 == 0 and 0 <= k < 1 << 256:
                    hits = ladder_hits(k)
                    if hits:
                        out[k] = tuple(hits)
    kinds = {h[1] for hits in out.values() for h in hits}
    assert kinds == {"doubling", "cancellation"}, kinds
    return out


EDGE_SCALARS = (0, 1, 2, 7, 8, 9, 15, 16, 17, int("8" * 64, 16), int("9" * 64, 16), int("7" * 64, 16), 1 << 128, 1 << 253, (1 << 256) - 1,
                (1 << 256) - 16, R - 2, R - 1, R, R + 1) + tuple(mm * R for mm in range(2, 6)) + tuple(mm * R - 2 * mm for mm in range(2, 6))
MUL_BASE_KINDS = ("generator", "subgroup", "subgroup", "outside the subgroup", "outside the subgroup", "identity", "invalid")


@functools.lru_cache(maxsize=None)
def g2_mul_cases():
    """{items, scalars, points, want[reduce], status}: items interleave the seven bases under every edge scalar (a wave mixes bases),
    then the random scalars over the bases in turn.  want / status are per reduce_scalar value (False: the 256-bit integer as it is,
    True: mod r, Fr::from_slice)."""
    G = G2
    sub = chain(G, b"mul-bases", 2)
    out_sub = twist_points_outside_subgroup()[2:4]
    bases = [G.enc(G.gen), G.enc(sub[0]), G.enc(sub[1]), G.enc(out_sub[0]), G.enc(out_sub[1]), G.zero, _off_curve(G, sub[0])]
    decoded = [G.decode(b) for b in bases]
    edge = list(EDGE_SCALARS) + sorted(set(ladder_hit_scalars()) - set(EDGE_SCALARS))
    rnd = random.Random(4242)
    rand256 = [rnd.randrange(1 << 256) for _ in range(150)]
    rand_r = [rnd.randrange(R) for _ in range(50)]
    items = [{"base": bi, "k": k, "set": "edge"} for k in edge for bi in range(len(bases))]
    items += [{"base": i % len(bases), "k": k, "set": "random 256-bit"} for i, k in enumerate(rand256)]
    items += [{"base": (i + 3) % len(bases), "k": k, "set": "random < r"} for i, k in enumerate(rand_r)]
    if len(items) % WAVE == 0:
        items.append({"base": 1, "k": 3, "set": "edge"})
    cache = {}

    def model_mul(bi, k):
        if (bi, k) not in cache:
            cache[(bi, k)] = G.enc(G.mul(decoded[bi][1], k))
        return cache[(bi, k)]

    observable = 0
    for n_it, it in enumerate(items):
        st, _ = decoded[it["base"]]
        it["kind"] = MUL_BASE_KINDS[it["base"]]
        it["status"] = st
        for reduce in (False, True):
            k = it["k"] % R if reduce else it["k"]
            if st != ST_OK:
                want, src = G.zero, "model"
            elif it["set"] == "edge" or n_it % 10 == 0 or it["kind"] == "identity":
                want, src = model_mul(it["base"], k), "model"
            else:
                want, src = G.c_mul(bases[it["base"]], be(k)), "c_oracle"
            it["want", reduce], it["src", reduce] = want, src
        if it["kind"] == "outside the subgroup" and it["k"] >= R and it["want", False] != it["want", True]:
            observable += 1
    # what makes reduce_scalar observable at all: off the subgroup k P and (k mod r) P differ
    assert observable >= 1
    return {"items": items, "bases": bases, "observable": observable,
            "points": b"".join(bases[it["base"]] for it in items), "scalars": b"".join(be(it["k"]) for it in items)}


# ---- segmented sums ---------------------------------------------------------------------------------------------------------------
SUM_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 1000)


def _sum_expect(G, pts):
    """(want bytes, status, exceptional steps) of one segment as the sum kernels define it: invalid points are skipped, the first
    error is the status and zeroes the output; a step is exceptional when the running sum is +-the next point (neither the identity)"""
    acc, st, ex, ident = None, ST_OK, [], 0
    for j, b in enumerate(pts):
        s, p = G.decode(b)
        if s != ST_OK:
            st = st if st != ST_OK else s
            continue
        if p is None:
            ident += 1
        elif acc is not None and acc[0] == p[0]:
            ex.append((j, "doubling" if acc == p else "cancellation"))
        acc = G.add(acc, p)
    return (G.zero if st != ST_OK else G.enc(acc)), st, ex, ident


class _SumCall:
    def __init__(self, G, name, segments, notes, planted):
        self.name, self.segments, self.notes, self.planted = name, segments, notes, planted
        self.seg_off = [0]
        for s in segments:
            self.seg_off.append(self.seg_off[-1] + len(s))
        self.points = b"".join(b"".join(s) for s in segments)
        exp = [_sum_expect(G, s) for s in segments]
        self.want, self.status = [e[0] for e in exp], [e[1] for e in exp]
        self.exceptional, self.identity_terms = [e[2] for e in exp], [e[3] for e in exp]


def _plant(G, seg, step, kind):
    """make step `step` of the segment exceptional: the point there becomes the running sum of the ones before it (doubling) or its
    negative (cancellation: the sum goes to O and the segment continues from there, O + P)"""
    acc = None
    for b in seg[:step]:
        acc = G.add(acc, G.decode(b)[1])
    assert acc is not None
    seg[step] = G.enc(acc if kind == "doubling" else G.neg(acc))


@functools.lru_cache(maxsize=None)
def sum_calls(group):
    G = G2 if group == "g2" else G1
    pool = [G.enc(p) for p in chain(G, b"sum-" + group.encode(), 5000)]
    rnd = random.Random(77 if G is G1 else 78)
    cursor = [0]

    def take(n):
        out = [pool[(cursor[0] + i) % len(pool)] for i in range(n)]
        cursor[0] += n + 1
        return out

    bad6 = lambda i: _coord(G, G.decode(pool[i])[1], i % (G.size // 32), Q + i)       # noqa: E731
    bad4 = lambda i: _off_curve(G, G.decode(pool[i])[1])                              # noqa: E731
    # --- call 1: 136 segments = two full waves and a ragged third; lengths from SUM_LENGTHS, shuffled, then the segments that
    # carry a plant are swapped to fixed lanes
    lengths = [1000] * 2 + [65] * 5 + [64] * 5 + [63] * 5 + [0, 1, 2, 3] * 29 + [0, 1, 3]
    assert len(lengths) == 136 and set(lengths) == set(SUM_LENGTHS)
    rnd.shuffle(lengths)

    def place(pos, length):
        j = next(j for j in range(len(lengths)) if lengths[j] == length and j not in fixed)
        lengths[pos], lengths[j] = lengths[j], lengths[pos]
        fixed.add(pos)

    fixed = set()
    # wave 0: lanes 9, 10, 11 long enough to be mid-loop at step 30 of lane 10; lane 40: the first 1000-point segment
    # wave 1: lane 64 + 20 is the second 1000-point segment — from step 65 on it is the only lane of its wave still looping
    layout = {9: 65, 10: 64, 11: 63, 12: 65, 20: 63, 21: 3, 22: 63, 23: 2, 28: 64, 29: 1, 30: 3, 31: 2, 32: 3, 33: 3, 35: 3, 36: 2, 37: 3, 38: 3,
              40: 1000, 84: 1000, 90: 65, 91: 1, 100: 64, 101: 63, 130: 65, 131: 3, 132: 2, 133: 64, 134: 3, 135: 1}
    for pos, length in layout.items():
        place(pos, length)
    assert all(n <= 65 for i, n in enumerate(lengths[64:128]) if i != 20)
    segs = [take(n) for n in lengths]
    notes, planted = {}, set()

    def plant(i, step, kind, note):
        _plant(G, segs[i], step, kind)
        notes[i] = note
        planted.add(i)

    plant(10, 30, "doubling", "doubling, neighbours mid-loop")
    plant(12, 31, "cancellation", "cancellation then O + P, neighbours mid-loop")
    plant(84, 500, "cancellation", "")
    plant(84, 700, "doubling", "cancellation then O + P, then a doubling, in the only lane still looping")
    plant(40, 999, "doubling", "doubling at the last step of a 1000-point segment")
    plant(35, 1, "cancellation", "P, -P, Q")
    plant(36, 1, "doubling", "P, P")
    segs[37] = [G.zero, segs[37][1], G.zero]; notes[37] = "identity terms around a point"
    segs[38] = [G.zero] * 3; notes[38] = "identity terms only"
    segs[90][10] = G.zero; segs[90][11] = G.zero; notes[90] = "identity terms mid-segment"
    segs[20][31] = bad4(31); notes[20] = "one invalid point in the middle"
    segs[22][5] = bad6(5); segs[22][40] = bad4(40); notes[22] = "two invalid points, codes 6 then 4"
    segs[28][60] = bad4(60); segs[28][61] = bad6(61); notes[28] = "two invalid points, codes 4 then 6"
    segs[30] = [bad4(1), bad6(2), bad4(3)]; notes[30] = "invalid points only"
    segs[32] = [bad6(7), segs[32][1], segs[32][2]]; notes[32] = "invalid point first"
    plant(130, 64, "doubling", "doubling at the last step, in the ragged wave")
    segs[132] = [bad6(9), segs[132][1]]; notes[132] = "invalid point in the ragged wave"
    plant(134, 2, "cancellation", "sum cancels at the last step, in the ragged wave")
    for faulty in (20, 22, 28, 30, 32, 132):
        assert len(segs[faulty + 1]) >= 1 and faulty + 1 not in notes          # the segment after each faulty one is an ordinary one
    calls = [_SumCall(G, "ragged", segs, notes, planted)]
    # --- call 2: one segment of 5 000 points (one lane, one launch of one wave)
    cursor[0] = 0
    one = take(5000)
    _plant(G, one, 2500, "doubling")
    calls.append(_SumCall(G, "single long", [one], {0: "doubling mid-way"}, {0}))
    # --- call 3: many empty segments at both ends
    mid = [take(3), take(64), take(1), take(2), take(65)]
    _plant(G, mid[4], 33, "doubling")
    calls.append(_SumCall(G, "empty ends", [[] for _ in range(70)] + mid + [[] for _ in range(70)], {74: "doubling"}, {74}))
    # the plants are the ONLY exceptional steps: nothing happened by accident elsewhere
    for call in calls:
        for i, ex in enumerate(call.exceptional):
            assert bool(ex) == (i in call.planted), (call.name, i, ex)
    return calls


# ---- Fq12 -------------------------------------------------------------------------------------------------------------------------
FP12_OPS = {"mul": 0, "sqr": 1, "inv": 2, "conj": 3, "frob1": 4, "frob2": 5, "frob3": 6, "cyclotomic_sqr": 7}


def f12_from_bytes(b):
    """inverse of bn254_model.f12_to_bytes: 384 bytes in tower order -> the model's six Fq2 coefficients (index = power of w)"""
    assert len(b) == 384
    w = [int.from_bytes(b[i:i + 32], "big") for i in range(0, 384, 32)]
    f2 = [(w[2 * i], w[2 * i + 1]) for i in range(6)]            # a0 a1 a2 b0 b1 b2
    return [f2[0], f2[3], f2[1], f2[4], f2[2], f2[5]]


def _f12_conj(a):
    return [m.f2_neg(x) if i & 1 else x for i, x in enumerate(a)]


@functools.lru_cache(maxsize=None)
def fp12_elements():
    """[(kind, element)]"""
    rnd = random.Random(1212)
    r2 = lambda: (rnd.randrange(Q), rnd.randrange(Q))    # noqa: E731
    els = [("zero", [m.F2_ZERO] * 6), ("one", list(m.F12_ONE))]
    for val, kind in ((1, "basis 1"), (Q - 1, "basis q-1")):
        for i in range(12):
            e = [m.F2_ZERO] * 6
            e[i // 2] = (val, 0) if i % 2 == 0 else (0, val)
            els.append((kind, e))
    els.append(("subfield Fq", [(rnd.randrange(Q), 0)] + [m.F2_ZERO] * 5))
    els.append(("subfield Fq2", [r2()] + [m.F2_ZERO] * 5))
    els.append(("subfield Fq6", [r2(), m.F2_ZERO, r2(), m.F2_ZERO, r2(), m.F2_ZERO]))           # even powers of w: Fq2[v], v = w^2
    for _ in range(3):
        els.append(("sparse line", [r2(), r2(), m.F2_ZERO, r2(), m.F2_ZERO, m.F2_ZERO]))        # the shape of bn254_model._line
    g1, g2 = c.g1_generator(), c.g2_generator()
    for i in range(4):
        p, q = c.g1_mul(g1, be(_scalar(b"f12-a%d" % i))), c.g2_mul(g2, be(_scalar(b"f12-b%d" % i)))
        els.append(("miller", f12_from_bytes(c.miller_loop(p, q))))
        els.append(("gt", f12_from_bytes(c.pairing(p, q))))
    for _ in range(40):
        els.append(("random", [r2() for _ in range(6)]))
    for kind, e in els:
        assert f12_from_bytes(m.f12_to_bytes(e)) == e, kind
    return tuple((k, tuple(e)) for k, e in els)


@functools.lru_cache(maxsize=None)
def fp12_cases():
    """[{op, kind, a, b, want}] (bytes; b None for the unary ops), expectations from the model's polynomial arithmetic"""
    els = [(k, list(e)) for k, e in fp12_elements()]
    by = lambda kind: [e for k, e in els if k == kind]     # noqa: E731
    rand, dense = by("random"), by("random")[0]
    tb = m.f12_to_bytes
    cases = []

    def case(op, kind, a, b, want):
        cases.append({"op": op, "kind": kind, "a": tb(a), "b": None if b is None else tb(b), "want": tb(want)})

    zero, one = els[0][1], els[1][1]
    pairs = [("0 * x", zero, dense), ("x * 0", dense, zero), ("1 * x", one, dense), ("x * 1", dense, one)]
    pairs += [("sparse * dense", s, rand[i + 1]) for i, s in enumerate(by("sparse line"))]
    pairs += [("dense * sparse", rand[i + 5], s) for i, s in enumerate(by("sparse line"))]
    pairs += [("sparse * sparse", by("sparse line")[0], by("sparse line")[1])]
    pairs += [("basis * dense", e, rand[i % 40]) for i, e in enumerate(by("basis 1") + by("basis q-1"))]
    pairs += [("basis * basis", by("basis 1")[i], by("basis 1")[(5 * i + 7) % 12]) for i in range(12)]
    pairs += [("subfield * dense", by(k)[0], rand[9]) for k in ("subfield Fq", "subfield Fq2", "subfield Fq6")]
    pairs += [("miller * gt", a, b) for a, b in zip(by("miller"), by("gt"))]
    pairs += [("distinct random", rand[i], rand[(i + 1) % 40]) for i in range(40)]
    for kind, a, b in pairs:
        assert a != b
        case("mul", kind, a, b, m.f12_mul(a, b))
    for kind, e in els:
        case("sqr", kind, e, None, m.f12_mul(e, e))
        case("conj", kind, e, None, _f12_conj(e))
    # Frobenius: every basis element (each coefficient constant on its own), and a few of every other kind
    frob_in = [(k, e) for k, e in els if k.startswith("basis")] + [(k, by(k)[0]) for k in ("subfield Fq2", "subfield Fq6", "sparse line", "miller", "gt")]
    frob_in += [("random", e) for e in rand[:6]]
    for kind, e in frob_in:
        for power in (1, 2, 3):
            case("frob%d" % power, kind, e, None, m.f12_pow(e, Q ** power))
    # inversion (a^(q^12 - 2), 0.3 s each): non-zero inputs only — what fp12_inv returns for 0 is not documented
    inv_in = [("one", one)] + [("basis 1", by("basis 1")[i]) for i in (1, 2, 7, 11)] + [("basis q-1", by("basis q-1")[i]) for i in (0, 5)]
    inv_in += [(k, by(k)[0]) for k in ("subfield Fq", "subfield Fq2", "subfield Fq6", "sparse line", "miller", "gt")] + [("random", e) for e in rand[:7]]
    for kind, e in inv_in:
        want = m.f12_pow(e, Q ** 12 - 2)
        assert m.f12_mul(want, e) == list(m.F12_ONE)
        case("inv", kind, e, None, want)
    for e in by("gt"):
        case("cyclotomic_sqr", "gt", e, None, m.f12_mul(e, e))
    return cases


def is_exceptional(G, it):
    """an addition lane that takes one of jac_add's overrides: an identity operand, equal x (P = +-Q), or a failed decode (the
    kernel then adds the generator to itself)"""
    return it["status"] != ST_OK or it["a"] == G.zero or it["b"] == G.zero or it["a"][:G.size // 2] == it["b"][:G.size // 2]
