"""The Jacobi symbol of the hash filter (bn254_amd/csrc/bn254_hash.h: u256_is_square_mod_q, jacobi_passes<8/6/4/2>, u256_jacobi_symbol) —
references, a mirror of the pass structure and the case set, shared by tests/test_jacobi_cases.py (the host build, CPU) and
tests/test_gpu_jacobi.py (the device, through bn254_debug_jacobi).  Python integers only; nothing here imports the library.

REFERENCES, independent of the device algorithm: Euler's criterion (mode 0), (x^3 + 3) mod q and Euler's criterion on it (mode 1), a textbook
Jacobi symbol by remainders (mode 2).

MIRROR (`mirror`): the passes of ONE lane as the header runs them without its wave votes (the host build's control flow; on the device a lane
may stay in a wider phase because a neighbour needs it, which changes no value).  Its verdict is checked against the references like any other
implementation; its counters exist to PROVE COVERAGE: which phases ran, where a whole word was shifted out, which strip counts, swaps and sign
rules a case exercised.  tests/test_jacobi_cases.py asserts the coverage conditions from them.

CASE SET: `mode0_cases`, `mode1_cases`, `mode2_cases` -> lists of Case(cls, a, b).  What uniformly random values never do is put there on
purpose: a low word of zero (probability 2^-32 per pass), strips of up to 31 bits, operands that enter a narrow phase directly (moduli of 64,
128 and 192 bits), symbol 0, and inputs slow for the passes.  Under q the slowest input the seeded hill-climb finds takes 207 passes (20 000
random values: 154 to 203); the slowest case of the whole set is mode 2's a = 2^253 under b = 2^254 - 1 with 261.  The budget is 600, and the
passes cannot need more than 508: each removes at least one bit of |a| + |n|."""
import functools
import random
from collections import namedtuple

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
BUDGET = 600
PHASES = (8, 6, 4, 2)
WIDTHS = (64, 128, 192, 254)                      # mode-2 moduli: the first three enter phases 2, 4 and 6 directly
N_RANDOM = 4096

Case = namedtuple("Case", "cls a b")


# ---- references ------------------------------------------------------------------------------------------------------------------------
def is_square(a):
    """Euler's criterion; 0 counts as a square (the filter's convention and fp_sqrt's)"""
    assert 0 <= a < Q
    return pow(a, (Q - 1) // 2, Q) in (0, 1)


def curve_rhs(x):
    return (x ** 3 + 3) % Q


def jacobi(a, n):
    """the textbook Jacobi symbol (a / n) of an odd n >= 1 by remainders: -1, 0 or 1"""
    assert n > 0 and n & 1
    a %= n
    r = 1
    while a:
        while a % 2 == 0:
            a //= 2
            if n % 8 in (3, 5):
                r = -r
        a, n = n, a
        if a % 4 == 3 and n % 4 == 3:
            r = -r
        a %= n
    return r if n == 1 else 0


def want0(a):
    """the flag byte of mode 0"""
    return 1 if is_square(a) else 0


def want1(x):
    """(out_value, flag byte) of mode 1: filter (bit 0) and square root (bit 1) both say whether x^3 + 3 is a square"""
    v = curve_rhs(x)
    return v, (3 if is_square(v) else 0)


def want2(a, b):
    """the flag byte of mode 2: 0 symbol +1, 1 symbol -1, 2 symbol 0"""
    return {1: 0, -1: 1, 0: 2}[jacobi(a, b)]


# ---- the mirror ------------------------------------------------------------------------------------------------------------------------
class Trace:
    """what one lane's passes did.  symbol: 0 / 1 / 2 as mode 2 reports it.  passes: all of them; per_phase / shifts: by phase width, passes
    and whole-word shifts (a[0] == 0); strips: the set of strip counts s; swaps / stays: passes with o < n and without; rule2: the set of
    (s & 1, n & 7) the (2/n) rule met (it flips t iff s is odd and n = 3, 5 mod 8); recip: the set of (o & 3, n & 3) at a swap (reciprocity
    flips t iff both are 3)."""
    __slots__ = ("symbol", "passes", "per_phase", "shifts", "strips", "swaps", "stays", "rule2", "recip", "left")

    def entered_directly(self, w):
        """the lane's first pass ran in phase w (none in a wider one)"""
        return self.per_phase[w] > 0 and all(self.per_phase[v] == 0 for v in PHASES if v > w)


def mirror(a, n, budget=BUDGET):
    assert n & 1 and n >= 3 and 0 <= a < n < 1 << 256
    tr = Trace()
    tr.per_phase = dict.fromkeys(PHASES, 0)
    tr.shifts = dict.fromkeys(PHASES, 0)
    tr.strips, tr.rule2, tr.recip = set(), set(), set()
    tr.passes = tr.swaps = tr.stays = 0
    t = 0
    for w in PHASES:
        fits = 1 << (32 * (w - 2))
        while budget > 0:
            if a == 0:
                break
            if w > 2 and a < fits and n < fits:
                break
            budget -= 1
            tr.passes += 1
            tr.per_phase[w] += 1
            if a & 0xFFFFFFFF == 0:
                a >>= 32
                tr.shifts[w] += 1
                continue
            s = (a & -a).bit_length() - 1
            tr.strips.add(s)
            tr.rule2.add((s & 1, n & 7))
            t ^= s & ((n >> 1) ^ (n >> 2)) & 1
            o = a >> s
            if o < n:
                tr.swaps += 1
                tr.recip.add((o & 3, n & 3))
                t ^= ((o & n) >> 1) & 1
                a, n = n - o, o
            else:
                tr.stays += 1
                a = o - n
    tr.left = a
    tr.symbol = 2 if n != 1 else t
    return tr


def mirror_is_square(a):
    """mode 0's verdict by the mirror: the symbol over q is not -1 (0 only for a = 0, which counts as a square)"""
    return mirror(a, Q).symbol != 1


# ---- the case set ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def slow_values(starts=4, steps=1000, seed=0x1ac0b1):
    """the slowest values below q a bit-flip hill-climb on the mirror finds: from the slowest of 32 seeded values, flip one bit (three times
    in ten, two) of the upper half — the low words steer the first passes, so such a step keeps the head of the run — and keep every flip
    that does not cost the passes less; deterministic.  -> [(passes, value)], slowest first"""
    rng = random.Random(seed)
    found = []
    for _ in range(starts):
        v = max((rng.randrange(1, Q) for _ in range(32)), key=lambda x: mirror(x, Q).passes)
        best = mirror(v, Q).passes
        for _ in range(steps):
            c = v ^ (1 << rng.randrange(128, 254))
            if rng.random() < 0.3:
                c ^= 1 << rng.randrange(128, 254)
            if not 0 < c < Q:
                continue
            p = mirror(c, Q).passes
            if p >= best:
                v, best = c, p
        found.append((best, v))
    return sorted(found, reverse=True)


def _odd(rng, bits):
    return rng.getrandbits(bits) | 1 | (1 << (bits - 1))


@functools.lru_cache(maxsize=None)
def mode0_cases():
    rng = random.Random(0x0a0b)
    cs = [Case("small", v, None) for v in (0, 1, 2, 3, 4, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2)]
    for k in range(257):
        cs += [Case("powers of two", v, None) for v in (1 << k, Q - (1 << k), (1 << k) - 1) if 0 < v < Q]
    for s in range(1, 32):                          # every strip count, under odd parts of several sizes
        cs += [Case("odd << s", _odd(rng, bits) << s, None) for bits in (222, 200, 97, 33)]
    for j in range(1, 7):                           # whole words of zeros below k: the a[0] == 0 branch, j times in a row
        room = 253 - 32 * j
        for k in (1, 3, _odd(rng, room), _odd(rng, min(40, room)), _odd(rng, room - 5) << 5, rng.getrandbits(room) | 1):
            assert 0 < k << (32 * j) < Q
            cs.append(Case("k << 32j", k << (32 * j), None))
    cs += [Case("slow", v, None) for _, v in slow_values()]
    cs += [Case("random", rng.randrange(Q), None) for _ in range(N_RANDOM)]
    return tuple(cs)


@functools.lru_cache(maxsize=None)
def mode1_cases():
    rng = random.Random(0x0a0c)
    cs = [Case("small", x, None) for x in (0, 1, 2, Q - 1, Q - 2)]
    for k in range(1, 9):                           # 2^(29k) < q up to k = 8: a one in limb k alone, and limbs 0 .. k-1 full
        cs += [Case("limb boundary", 1 << (29 * k), None), Case("limb boundary", (1 << (29 * k)) - 1, None)]
    cs += [Case("random", rng.randrange(Q), None) for _ in range(N_RANDOM)]
    return tuple(cs)


def moduli(width, rng):
    """four odd moduli of exactly `width` bits: a random one, all ones, a multiple of 105 (so that symbols of 0 exist), and 2^(width-1) + 1"""
    lo, hi = -(-(1 << (width - 1)) // 105), ((1 << width) - 1) // 105
    g = rng.randrange(lo, hi) | 1
    ms = [_odd(rng, width), (1 << width) - 1, 105 * g, (1 << (width - 1)) + 1]
    assert all(m & 1 and m.bit_length() == width for m in ms), width
    return ms


@functools.lru_cache(maxsize=None)
def mode2_cases():
    rng = random.Random(0x0a0d)
    cs = []
    for width in WIDTHS:
        tag = "%d bits: " % width
        for b in moduli(width, rng):
            for j in range(1, (width - 1) // 32 + 1):       # a = k << 32j below b: the word shift in the phase b starts in, and in every narrower one
                room = (b >> (32 * j)).bit_length() - 1
                ks = {1} | ({_odd(rng, room), rng.getrandbits(room) | 1} if room > 1 else set())
                cs += [Case(tag + "k << 32j", k << (32 * j), b) for k in sorted(ks) if k << (32 * j) < b]
            cs += [Case(tag + "edges", a, b) for a in (0, 1, 2, b - 1, b - 2, (b - 1) // 2, (b + 1) // 2)]
            for f in (3, 5, 7, 15, 21, 35, 105):            # a shares a factor with b whenever f divides b: symbol 0, reached in a narrow phase
                cs += [Case(tag + "shared factor", f * rng.randrange(1, b // f), b), Case(tag + "shared factor", b - f, b)]
            for s in (1, 2, 31):
                cs.append(Case(tag + "random", (_odd(rng, width - 33) << s) % b, b))
            cs += [Case(tag + "random", rng.randrange(b), b) for _ in range(48)]
        for _ in range(256):                                # random moduli of this width
            b = _odd(rng, width)
            cs.append(Case(tag + "random", rng.randrange(b), b))
    for b in (3, 5, 7, 9, 15, 105):                         # the smallest moduli: b = 3 is the least the hook accepts
        cs += [Case("tiny modulus", a, b) for a in range(b)]
    cs += [Case("mode-0 set over q", c.a, Q) for c in mode0_cases()]
    return tuple(cs)


def be(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def ints(blob):
    return [int.from_bytes(blob[i:i + 32], "big") for i in range(0, len(blob), 32)]
