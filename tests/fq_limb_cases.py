"""The Fq / Fq2 primitives of the field layer (bn254_amd/csrc/bn254_field.h, bn254_fp2_pair.h) on RAW LIMB VECTORS — a model in plain Python
integers, the primitives' contracts restated as predicates, and the case set, shared by tests/test_fq_limb_cases.py (the four host twins, CPU)
and tests/test_gpu_fq_limbs.py (the device, through bn254_debug_fq2_limbs in both layouts).  Nothing here imports the library.

An element is 9 signed limbs, value(l) = sum l_i 2^(29 i), Montgomery form with R = 2^261.  tight(V) is the unique vector of that value whose
limbs 0..7 are balanced digits in [-2^28, 2^28), the top limb absorbing the rest.

MODEL (`expected`): limb-wise identities for the lazy ring operations; tight(V) for a carry; tight(sum c_j V_j - k q) for the weak reductions
with k = floor((top + BN_WEAK_HALF) * BN_WEAK_KMUL / 2^32) as the header states it; the balanced 2^26 split for the multiplication by 8 and by
xi = 9 + i; for every Montgomery product the closed form  T = sum x_t y_t,  m = the representative of -T / q mod 2^261 with nine balanced 29-bit
digits,  V = (T + m q) / 2^261 exactly,  limbs = tight(V); V mod q as floor digits for canon and V / R mod q as eight 32-bit words for to_u256;
the predicates on the residues.  The inverse has no closed form for its LIMBS (they depend on the division steps): the model checks
a * inv(a) = R^2 (mod q), inv(0) = 0 and tightness, and the exact words come from the host twin.  `mont_columns` is a transliteration of
BN_MONT_PRODUCT_BODY / BN_MONT_DUAL_BODY over exact integers: it returns the limbs (the closed form is asserted against it on every product
case) and the largest and smallest value the 64-bit accumulator takes — the real contract of a product, asserted to fit int64.

CONTRACT (`check_contract`): what the interval tracker of the host builds (-DBN_TRACK_BOUNDS) demands of each primitive, restated from the
source comments on the numbers of the case itself (min / max of limbs 0..7, |top limb|, value / q) — in the pair layout's form, where the host
code selects operands by role with fp_select and the tracker therefore takes the UNION of the two candidates' intervals; that form implies the
classic layout's.  Every case of the set is asserted to satisfy it; tests/test_fq_limb_cases.py ties the predicates to the tracker's own by
running the tracking builds on every case.

CASES (`cases(op)`), seeded: canonical edges; tight vectors with extreme digits (all -2^28, all 2^28 - 1, alternating, one extreme digit at each
position) at values / q of +-0.5, 1, 5, 80 and, where the op allows, up to its bound; lazy vectors with every limb at +-k 2^28 up to the k the
column bound admits; non-canonical representatives of exact multiples of q and their neighbours; carries that ripple through all limbs;
limbs at the 2^26 split boundaries; a few hundred random in-contract vectors per op.

WHAT KEEPS THE SET FROM BEING TAME (`check_tameness`): every product op — mul, sqr, mul_fp and the squarings inside inv — has a case whose
largest exact accumulator value lies above 2^62 and one below -2^62, and every op with a value bound has a case within 1 % of it."""
import functools
import os
import random
import re
import struct
from collections import namedtuple
from fractions import Fraction

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
W, L = 29, 9
MASK, HALF = (1 << W) - 1, 1 << (W - 1)
RBITS = W * L
R = 1 << RBITS
RINV = pow(R, -1, Q)
QINV_NEG = (-pow(Q, -1, R)) % R
I32 = 1 << 31
I64 = 1 << 63
SPREAD = 26

_HDR = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bn254_amd", "csrc", "bn254_constants.h")).read()


def _const(name):
    return re.search(r"#define %s ([-0-9.a-fx]+)" % name, _HDR).group(1)


WEAK_KMUL, WEAK_HALF = int(_const("BN_WEAK_KMUL")), int(_const("BN_WEAK_HALF"))
TOP_PER_Q, R_OVER_Q = Fraction(_const("BN_TOP_PER_Q")), Fraction(_const("BN_R_OVER_Q"))
assert int(_const("BN_LIMBS")) == L and int(_const("BN_W")) == W
COL_EXTRA = L * HALF * HALF + (1 << 37)
VALUE_CAP, WEAK_CAP, CANON_CAP = 500, 600, 80

OPS = dict(add=0, sub=1, neg=2, dbl=3, conj=4, mul_i=5, select=6, norm=7, reduce_weak=8, lin2_reduce=9, lin4_reduce=10, mul8=11, mul_xi=12,
           mul_xi_n=13, mul=14, sqr=15, mul_fp=16, inv=17, canon=18, to_u256=19, is_zero=20, eq=21, u512_greater=22, norm_floor=23)
PRODUCT_OPS = ("mul", "sqr", "mul_fp", "inv")
FLAG_OPS = ("is_zero", "eq", "u512_greater")
N_RANDOM = 256

ZERO = (0,) * L
ZERO2 = (ZERO, ZERO)
# a: the four Fq2 operands ((re limbs, im limbs), ...), k: the four int32 factors
Case = namedtuple("Case", "op tag a k")


# ---- integers and limbs ------------------------------------------------------------------------------------------------------------------
def value(l):
    return sum(int(x) << (W * i) for i, x in enumerate(l))


def bal(x, bits=W):
    """the sign-extended low `bits` bits of x"""
    x &= (1 << bits) - 1
    return x - (1 << bits) if x >> (bits - 1) else x


def tight(v):
    out = []
    for _ in range(L - 1):
        d = bal(v)
        out.append(d)
        v = (v - d) >> W
    return tuple(out + [v])


def floor_digits(v):
    out = []
    for _ in range(L - 1):
        out.append(v & MASK)
        v >>= W
    return tuple(out + [v])


QL = tight(Q)


def fits_i32(l):
    return all(-I32 < x < I32 for x in l)


def voq(l):
    return Fraction(value(l), Q)


# ---- the Montgomery product ----------------------------------------------------------------------------------------------------------------
def mont_closed(t):
    """V of the closed form, with the tracker's claim |V| <= |T| / R + 0.501 q asserted"""
    x, m = (t * QINV_NEG) % R, 0
    for i in range(L):
        d = bal(x)
        m += d << (W * i)
        x = (x - d) >> W
    assert (t + m * Q) % R == 0
    v = (t + m * Q) >> RBITS
    assert abs(v) * R * 1000 <= abs(t) * 1000 + 501 * Q * R
    return v


def mont_columns(pairs):
    """BN_MONT_PRODUCT_BODY (one pair) / BN_MONT_DUAL_BODY (two) over exact integers, multiply-adds in source order:
    (limbs, largest accumulator value, smallest accumulator value)"""
    acc, hi, lo = 0, 0, 0
    m, r = [0] * L, [0] * L
    n0 = QINV_NEG & MASK
    for k in range(2 * L - 1):
        for i in range(L):
            j = k - i
            if 0 <= j < L:
                for x, y in pairs:
                    acc += x[i] * y[j]
                    hi, lo = max(hi, acc), min(lo, acc)
        for i in range(L):
            j = k - i
            if 0 <= j < L and not (k < L and i >= k):
                acc += m[i] * QL[j]
                hi, lo = max(hi, acc), min(lo, acc)
        if k < L:
            m[k] = bal((acc & 0xFFFFFFFF) * n0)
            acc += m[k] * QL[0]
            hi, lo = max(hi, acc), min(lo, acc)
            assert acc & MASK == 0
            acc >>= W
        else:
            r[k - L] = bal(acc)
            acc = (acc + HALF) >> W
    r[L - 1] = acc
    return tuple(r), hi, lo


def mont(pairs, stats=None):
    """the limbs of Montgomery-reduce(sum x y): closed form, asserted word for word against the transliterated body, every accumulator
    value asserted inside int64; stats (a dict) collects the extreme accumulator values"""
    v = mont_closed(sum(value(x) * value(y) for x, y in pairs))
    limbs, hi, lo = mont_columns(pairs)
    assert -I64 <= lo and hi < I64, (hi, lo)
    assert limbs == tight(v) and fits_i32(limbs), (limbs, tight(v))
    if stats is not None:
        stats["col_hi"] = max(stats.get("col_hi", 0), hi)
        stats["col_lo"] = min(stats.get("col_lo", 0), lo)
    return limbs


# ---- limb-wise pieces --------------------------------------------------------------------------------------------------------------------
def ladd(a, b):
    return tuple(x + y for x, y in zip(a, b))


def lsub(a, b):
    return tuple(x - y for x, y in zip(a, b))


def lneg(a):
    return tuple(-x for x in a)


def spread_lo(x):
    return bal(x, SPREAD)


def spread_hi(x):
    return (x + (1 << (SPREAD - 1))) >> SPREAD


def mul8(a):
    """fp_mul8_spread: a_i = h_i 2^26 + l_i with l_i in [-2^25, 2^25); limb i = 8 l_i + h_(i-1), the top limb 8 a_top + h_(top-1)"""
    out, h = [], 0
    for i in range(L - 1):
        out.append(spread_lo(a[i]) * 8 + h)
        h = spread_hi(a[i])
    out.append(a[L - 1] * 8 + h)
    assert value(out) == 8 * value(a)
    am = max(abs(x) for x in a[:L - 1])
    assert all(abs(x) <= HALF + am // (1 << SPREAD) + 1 for x in out[:L - 1])          # the tracker's stated bound
    return tuple(out)


def weak_k(top):
    return ((top + WEAK_HALF) * WEAK_KMUL) >> 32


def lin_reduce(terms):
    """fp_reduce_weak / fp_lin2_reduce / fp_lin4_reduce on [(limbs, factor), ...]: tight(sum c V - k q), the stated bound asserted"""
    top = sum(l[L - 1] * c for l, c in terms)
    assert -I32 < top + WEAK_HALF < I32
    v = sum(value(l) * c for l, c in terms) - weak_k(top) * Q
    vv = sum(abs(c) * abs(voq(l)) for l, c in terms)
    assert abs(Fraction(v, Q)) <= Fraction(51, 100) + Fraction(3, 10000) * vv, (float(Fraction(v, Q)), float(vv))
    return tight(v)


def mul_xi(a):
    a0, a1 = a
    r0, r1 = lsub(ladd(mul8(a0), a0), a1), ladd(ladd(mul8(a1), a1), a0)
    assert value(r0) == 9 * value(a0) - value(a1) and value(r1) == 9 * value(a1) + value(a0)
    for r, own, p in ((r0, a0, a1), (r1, a1, a0)):           # the stated limb bound: 2^28 + |own_i| + |partner_i| (+ what mul8 adds: am / 2^26 + 1)
        am = max(abs(x) for x in own[:L - 1])
        assert all(abs(r[i]) <= HALF + am // (1 << SPREAD) + 1 + abs(own[i]) + abs(p[i]) for i in range(L - 1))
    return r0, r1


def canon_value(l):
    return value(l) % Q


def plain_value(l):
    return value(l) * RINV % Q


def u256_words(x):
    return tuple(bal((x >> (32 * i)) & 0xFFFFFFFF, 32) for i in range(8)) + (0,)


# ---- the model ---------------------------------------------------------------------------------------------------------------------------
def expected(c, stats=None):
    """(18 limbs, flag) of the case; limbs = None for inv (the exact words come from the host twin, check_inv verifies them)"""
    a, b, cc, d = c.a
    k, op = c.k, c.op
    flag, r = 0, ZERO2
    if op == "add": r = (ladd(a[0], b[0]), ladd(a[1], b[1]))
    elif op == "sub": r = (lsub(a[0], b[0]), lsub(a[1], b[1]))
    elif op == "neg": r = (lneg(a[0]), lneg(a[1]))
    elif op == "dbl": r = (ladd(a[0], a[0]), ladd(a[1], a[1]))
    elif op == "conj": r = (a[0], lneg(a[1]))
    elif op == "mul_i": r = (lneg(a[1]), a[0])
    elif op == "select": r = a if k[0] != 0 else b
    elif op == "norm": r = (tight(value(a[0])), tight(value(a[1])))
    elif op == "norm_floor": r = (floor_digits(value(a[0])), floor_digits(value(a[1])))
    elif op == "reduce_weak": r = tuple(lin_reduce([(a[j], 1)]) for j in (0, 1))
    elif op == "lin2_reduce": r = tuple(lin_reduce([(a[j], k[0]), (b[j], k[1])]) for j in (0, 1))
    elif op == "lin4_reduce": r = tuple(lin_reduce([(a[j], k[0]), (b[j], k[1]), (cc[j], k[2]), (d[j], k[3])]) for j in (0, 1))
    elif op == "mul8": r = (mul8(a[0]), mul8(a[1]))
    elif op == "mul_xi": r = mul_xi(a)
    elif op == "mul_xi_n": r = mul_xi((tight(value(a[0])), tight(value(a[1]))))
    elif op == "mul": r = (mont([(a[0], b[0]), (lneg(a[1]), b[1])], stats), mont([(a[0], b[1]), (a[1], b[0])], stats))
    elif op == "sqr": r = (mont([(ladd(a[0], a[1]), lsub(a[0], a[1]))], stats), mont([(ladd(a[0], a[0]), a[1])], stats))
    elif op == "mul_fp": r = (mont([(a[0], b[0])], stats), mont([(a[1], b[0])], stats))
    elif op == "inv":
        mont([(a[0], a[0])], stats); mont([(a[1], a[1])], stats)              # its two squarings see the raw operand
        r = None
    elif op == "canon": r = (floor_digits(canon_value(a[0])), floor_digits(canon_value(a[1])))
    elif op == "to_u256": r = (u256_words(plain_value(a[0])), u256_words(plain_value(a[1])))
    elif op == "is_zero": flag = int(value(a[0]) % Q == 0 and value(a[1]) % Q == 0)
    elif op == "eq": flag = int((value(a[0]) - value(b[0])) % Q == 0 and (value(a[1]) - value(b[1])) % Q == 0)
    elif op == "u512_greater": flag = int((plain_value(a[1]), plain_value(a[0])) > (plain_value(b[1]), plain_value(b[0])))
    else: raise ValueError(op)
    if r is not None:
        assert fits_i32(r[0]) and fits_i32(r[1]), (op, c.tag)
        r = tuple(r[0]) + tuple(r[1])
    return r, flag


def check_inv(c, got):
    """what the model knows of an inverse: a * inv(a) = R^2 (mod q) in Fq2, inv(0) = 0, tight limbs"""
    g0, g1 = tuple(got[:L]), tuple(got[L:])
    a0, a1, x0, x1 = value(c.a[0][0]), value(c.a[0][1]), value(g0), value(g1)
    assert g0 == tight(x0) and g1 == tight(x1), c.tag
    if a0 % Q == 0 and a1 % Q == 0:
        assert g0 == ZERO and g1 == ZERO, c.tag
    else:
        assert (a0 * x0 - a1 * x1 - R * R) % Q == 0 and (a0 * x1 + a1 * x0) % Q == 0, c.tag


# ---- the contract: the tracker's intervals on the case's own numbers ------------------------------------------------------------------------
Bd = namedtuple("Bd", "lo hi top vlo vhi")


def bd_of(l):
    v = voq(l)
    return Bd(min(l[:L - 1]), max(l[:L - 1]), abs(l[L - 1]), v, v)


def b_absmax(x): return max(abs(x.lo), abs(x.hi), x.top)
def b_limb(x): return max(abs(x.lo), abs(x.hi))
def b_vabs(x): return max(abs(x.vlo), abs(x.vhi))
def b_i32(x): assert b_absmax(x) < I32, "limb exceeds int32"; return x
def b_add(a, b): return b_i32(Bd(a.lo + b.lo, a.hi + b.hi, a.top + b.top, a.vlo + b.vlo, a.vhi + b.vhi))
def b_sub(a, b): return b_i32(Bd(a.lo - b.hi, a.hi - b.lo, a.top + b.top, a.vlo - b.vhi, a.vhi - b.vlo))
def b_neg(a): return Bd(-a.hi, -a.lo, a.top, -a.vhi, -a.vlo)
def b_union(a, b): return Bd(min(a.lo, b.lo), max(a.hi, b.hi), max(a.top, b.top), min(a.vlo, b.vlo), max(a.vhi, b.vhi))
def b_tight(vlo, vhi): return Bd(-HALF, HALF, max(abs(vlo), abs(vhi)) * TOP_PER_Q + 2, vlo, vhi)


def b_norm(a):
    assert b_absmax(a) + HALF + 64 < I32, "norm input"
    return b_tight(a.vlo, a.vhi)


def b_weak(terms):
    """terms: [(Bd, factor)]: fp_reduce_weak (one term, factor 1) / fp_lin2_reduce / fp_lin4_reduce"""
    vv = sum(abs(c) * b_vabs(x) for x, c in terms)
    if len(terms) == 1:
        assert b_absmax(terms[0][0]) + (1 << 22) < I32, "reduce_weak input limbs"
    else:
        assert sum(abs(c) * x.top for x, c in terms) + (1 << 22) < I32, "lin_reduce input"
        assert sum(abs(c) for _, c in terms) <= 64, "lin4_reduce factors"
    assert vv <= WEAK_CAP, "weak reduction input value"
    return b_tight(-Fraction(3, 10000) * vv - Fraction(51, 100), Fraction(3, 10000) * vv + Fraction(51, 100))


def b_mul8(a):
    am = b_limb(a)
    assert am + (1 << 25) + 64 < I32 and 8 * a.top + 64 < I32, "mul8_spread input"
    g = Fraction(am, 1 << SPREAD) + 1
    return Bd(-HALF - g, HALF + g, 8 * a.top + g, 8 * a.vlo, 8 * a.vhi)


def b_col(a, b):
    A, B, At, Bt = b_limb(a), b_limb(b), a.top, b.top
    return max(8 * A * B, 7 * A * B + A * Bt + At * B, At * Bt)


def b_prod(x, y):
    c = [x.vlo * y.vlo, x.vlo * y.vhi, x.vhi * y.vlo, x.vhi * y.vhi]
    return min(c) / R_OVER_Q, max(c) / R_OVER_Q


def b_mul(a, b):
    assert b_col(a, b) + COL_EXTRA < I64, "mul column overflow"
    assert b_vabs(a) * b_vabs(b) / R_OVER_Q <= VALUE_CAP, "mul value bound"
    lo, hi = b_prod(a, b)
    return b_tight(lo - Fraction(501, 1000), hi + Fraction(501, 1000))


def b_dual(x0, y0, x1, y1):
    assert b_col(x0, y0) + b_col(x1, y1) + COL_EXTRA < I64, "pair product column overflow"
    (l0, h0), (l1, h1) = b_prod(x0, y0), b_prod(x1, y1)
    assert max(abs(l0 + l1), abs(h0 + h1)) <= VALUE_CAP, "pair product value bound"
    return b_tight(l0 + l1 - Fraction(501, 1000), h0 + h1 + Fraction(501, 1000))


def b_canon(a):
    one = b_tight(0, 1)
    b_mul(a, one)
    assert b_vabs(a) <= CANON_CAP, "canon input value"


def b_mul_xi(a):
    """the pair layout's host form: 8 own + own + select(role, partner, -partner)"""
    for own, p in ((a[0], a[1]), (a[1], a[0])):
        b_add(b_add(b_mul8(own), own), b_union(p, b_neg(p)))


def check_contract(c):
    """assert that the case lies inside its primitive's contract (AssertionError names the clause)"""
    op, k = c.op, c.k
    for o in c.a:
        assert fits_i32(o[0]) and fits_i32(o[1]) and len(o[0]) == L and len(o[1]) == L
    assert all(-I32 <= x < I32 for x in k)
    A, B, C, D = [(bd_of(o[0]), bd_of(o[1])) for o in c.a]
    both = (0, 1)
    if op == "add": [b_add(A[j], B[j]) for j in both]
    elif op == "sub": [b_sub(A[j], B[j]) for j in both]
    elif op == "dbl": [b_add(A[j], A[j]) for j in both]
    elif op in ("neg", "conj", "mul_i", "select"): pass
    elif op == "norm": [b_norm(A[j]) for j in both]
    elif op == "norm_floor": assert all(b_absmax(A[j]) + 64 < I32 for j in both), "norm_floor input"
    elif op == "reduce_weak": [b_weak([(A[j], 1)]) for j in both]
    elif op == "lin2_reduce": [b_weak([(A[j], k[0]), (B[j], k[1])]) for j in both]
    elif op == "lin4_reduce": [b_weak([(A[j], k[0]), (B[j], k[1]), (C[j], k[2]), (D[j], k[3])]) for j in both]
    elif op == "mul8": [b_mul8(A[j]) for j in both]
    elif op == "mul_xi": b_mul_xi(A)
    elif op == "mul_xi_n": b_mul_xi((b_norm(A[0]), b_norm(A[1])))
    elif op == "mul":
        u = b_union(B[0], B[1])
        b_dual(A[0], u, A[1], b_union(B[0], b_neg(B[1])))                 # real role: a0 b0 + a1 (-b1)
        b_dual(A[1], u, A[0], b_union(B[1], b_neg(B[0])))                 # imaginary role: a1 b0 + a0 b1
    elif op == "sqr":
        for own, p in ((A[0], A[1]), (A[1], A[0])):
            b_mul(b_union(b_add(own, own), b_add(own, p)), b_union(p, b_sub(own, p)))
    elif op == "mul_fp": [b_mul(A[j], B[0]) for j in both]
    elif op == "inv":
        t = [b_mul(A[j], A[j]) for j in both]
        n = b_add(t[0], t[1])
        b_canon(n)
        inv = b_mul(Bd(-2 * HALF, 2 * HALF, 2 * TOP_PER_Q + 4, -2, 2), b_tight(0, 1))
        [b_mul(A[j], inv) for j in both]
    elif op in ("canon", "to_u256"): [b_canon(A[j]) for j in both]
    elif op == "is_zero": [b_weak([(A[j], 1)]) for j in both]
    elif op == "eq": [b_weak([(b_sub(A[j], B[j]), 1)]) for j in both]
    elif op == "u512_greater": [b_canon(X[j]) for X in (A, B) for j in both]
    else: raise ValueError(op)


# ---- building blocks of the cases -----------------------------------------------------------------------------------------------------------
def to_mont(x):
    return x * R % Q


def with_top(low8, target):
    """limbs 0..7 as given, the top limb chosen so that value / q is as close to `target` as a top limb gets (within 1.6e-7)"""
    low = value(tuple(low8) + (0,))
    want = Fraction(target) * Q - low
    top = int(round(want / (1 << (W * (L - 1)))))
    return tuple(low8) + (top,)


def rep(n, lazy, rng):
    """a non-canonical representative of the integer n: limbs 0..7 random within +-lazy 2^28, made exact by adding tight(remainder) —
    limbs 0..7 end within +-(lazy + 1) 2^28"""
    noise = tuple(rng.randint(-lazy * HALF, lazy * HALF) for _ in range(L - 1)) + (0,)
    out = ladd(noise, tight(n - value(noise)))
    assert value(out) == n
    return out


EXTREME_PATTERNS = [(-HALF,) * 8, (HALF - 1,) * 8, (-HALF, HALF - 1) * 4, (HALF - 1, -HALF) * 4]
for _p in range(8):
    for _s in (-HALF, HALF - 1):
        EXTREME_PATTERNS.append(tuple(_s if i == _p else (37 * (i + 1) * (1 if i & 1 else -1)) for i in range(8)))


def canonical_edges(floor_forms=True):
    """the Montgomery forms of 0, 1, 2, q - 1, q - 2 and 2^256 mod q as tight limbs, two of them also as digits in [0, 2^29)"""
    return [tight(to_mont(x)) for x in (0, 1, 2, Q - 1, Q - 2, (1 << 256) % Q)] + ([floor_digits(to_mont(x)) for x in (1, Q - 1)] if floor_forms else [])


def both_signs(ts):
    return [s * t for t in ts for s in (1, -1)]


def tight_extremes(targets):
    return [with_top(p, t) for p in EXTREME_PATTERNS for t in targets]


def lazy_limbs(kmax, target, signs):
    """limbs 0..7 at +-kmax 2^28 (kmax may be fractional), sign pattern `signs` (a function of the limb index), value / q near target"""
    m = int(kmax * HALF)
    return with_top(tuple(m * signs(i) for i in range(8)), target)


SIGN_PATTERNS = [lambda i: 1, lambda i: -1, lambda i: 1 if i & 1 else -1, lambda i: -1 if i % 3 else 1]


def elems(vmax, kmax, rng, n_random=N_RANDOM // 2, top_room=1):
    """a pool of Fq limb vectors with |value / q| <= vmax and limbs 0..7 within +-kmax 2^28: the families of the module docstring"""
    targets = [t for t in (Fraction(1, 2), 1, 5, 80, 500, 600) if t < vmax]      # a top limb hits a target to 1.6e-7: the bound itself comes as exact multiples
    targets = sorted(set([-t for t in targets] + targets + [0]))
    out = canonical_edges(kmax >= 2) + tight_extremes(targets)
    ks = [k for k in (2, 3, 4) if k <= kmax] + ([kmax] if kmax > 1 else [])
    for k in ks:
        for s in SIGN_PATTERNS:
            for t in (0, Fraction(1, 2), -min(5, vmax)):
                out.append(lazy_limbs(k, t, s))
    edge = Fraction(vmax) * Fraction(999, 1000)
    out += [with_top(EXTREME_PATTERNS[0], edge), with_top(EXTREME_PATTERNS[1], -edge)]
    for _ in range(n_random):
        out.append(rep(rng.randint(-int(edge * Q), int(edge * Q)), max(int(kmax) - 1, 0), rng))
        out.append(tight(rng.randint(-int(edge * Q), int(edge * Q))))
    assert all(abs(voq(l)) <= vmax and max(abs(x) for x in l[:8]) <= kmax * HALF and fits_i32(l) for l in out)
    return out


def pairs_of(es, stride=7):
    """Fq2 operands from a pool: every element once as the real coefficient, another one of the pool as the imaginary"""
    n = len(es)
    return [(es[i], es[(i * stride + 3) % n]) for i in range(n)]


def _mk(op, tag, a=ZERO2, b=ZERO2, c=ZERO2, d=ZERO2, k=(0, 0, 0, 0)):
    return Case(op, tag, (a, b, c, d), tuple(k))


def _rng(op):
    return random.Random("fq-limb-cases/" + op)


def multiples(ks, rng, lazy=5):
    return [(k, rep(k * Q, lazy, rng)) for k in ks]


ZERO_KS = [0, 1, -1, 2, -2, 3, -3, 79, -79, 80, -80, 599, -599, 600, -600]


def _bump(l, dlt):
    return (l[0] + dlt,) + tuple(l[1:])


# ---- the case set ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cases(op):
    rng = _rng(op)
    out = []
    add = lambda tag, **kw: out.append(_mk(op, tag, **kw))
    if op in ("add", "sub"):
        es = pairs_of(elems(300, 3, rng))
        for i, a in enumerate(es):
            add("pool%d" % i, a=a, b=es[(i * 5 + 1) % len(es)])
        big = ((I32 // 2 - 1,) * 8 + (I32 // 2 - 1,), (-(I32 // 2) + 1,) * 8 + (I32 // 2 - 1,))
        add("limit", a=big, b=big if op == "add" else (lneg(big[0]), lneg(big[1])))
    elif op == "dbl":
        for i, a in enumerate(pairs_of(elems(300, Fraction(39, 10), rng))):
            add("pool%d" % i, a=a)
        add("limit", a=((I32 // 2 - 1,) * 9, (-(I32 // 2) + 1,) * 8 + (I32 // 2 - 1,)))
    elif op in ("neg", "conj", "mul_i", "select"):
        es = pairs_of(elems(600, 7, rng))
        for i, a in enumerate(es):
            add("pool%d" % i, a=a, b=es[(i * 5 + 1) % len(es)], k=(0 if i % 3 == 0 else rng.choice([1, -1, I32 - 1, -I32, 256]), 0, 0, 0))
        add("limit", a=((I32 - 1,) * 9, (-I32 + 1,) * 9), b=((-I32 + 1,) * 9, (I32 - 1,) * 9), k=(1, 0, 0, 0))
    elif op in ("norm", "norm_floor", "mul_xi_n"):
        vmax = 590 if op != "mul_xi_n" else 55
        lim = I32 - HALF - 65 if op != "norm_floor" else I32 - 65
        es = elems(vmax, 6, rng)
        es += [(HALF,) + (HALF - 1,) * 7 + (0,), (-HALF - 1,) + (-HALF,) * 7 + (0,), (HALF,) + (HALF - 1,) * 7 + (-1,),
               (2 * HALF - 1,) + (2 * HALF - 1,) * 7 + (5,), (-2 * HALF,) * 8 + (-5,)]           # carries that ripple through all eight limbs
        top = int(vmax * TOP_PER_Q) if op == "mul_xi_n" else lim
        es += [(lim,) * 8 + (top,), (-lim,) * 8 + (-top,), tuple(lim if i & 1 else -lim for i in range(8)) + (top,),
               (lim,) * 8 + (-top + (1 << 24),)]
        for i, a in enumerate(pairs_of(es)):
            add("pool%d" % i, a=a)
    elif op == "reduce_weak":
        es = elems(600, 6, rng)
        es += [r for _, r in multiples(ZERO_KS, rng)] + [rep(600 * Q - 1, 6, rng), rep(-600 * Q + 1, 6, rng)]
        lim = I32 - (1 << 22) - 1
        es += [with_top((lim,) * 8, 3), with_top((-lim,) * 8, -3), (0,) * 8 + (int(Fraction(5999, 10) * TOP_PER_Q),)]
        es += [with_top(tuple(rng.randint(-HALF, HALF - 1) for _ in range(8)), Fraction(h, 2) + e) for h in range(-9, 10)
               for e in (Fraction(-1, 1000), 0, Fraction(1, 1000))]                                 # around the rounding points of k
        for i, a in enumerate(pairs_of(es)):
            add("pool%d" % i, a=a)
    elif op in ("lin2_reduce", "lin4_reduce"):
        if op == "lin2_reduce":
            ks = [(3, -2), (3, 2), (-3, 2), (1, 1), (1, -1), (2, 0), (0, 1), (-1, -1), (5, 7), (32, -32)]
        else:
            ks = [(1, 1, 1, 1), (1, -1, 1, -1), (3, -2, 5, 7), (64, 0, 0, 0), (16, 16, 16, 16), (-16, 16, -16, 16), (0, 0, 0, 1), (2, 3, -4, -5)]
        for ki, kk in enumerate(ks):
            s = sum(abs(x) for x in kk)
            es = pairs_of(elems(Fraction(600, s), 7, rng, n_random=16))
            n = len(es)
            for i, a in enumerate(es):
                ops_ = [a, es[(i * 5 + 1) % n], es[(i * 11 + 2) % n], es[(i * 13 + 5) % n]]
                kfull = tuple(kk) + (0,) * (4 - len(kk))
                add("k%d/pool%d" % (ki, i), a=ops_[0], b=ops_[1], c=ops_[2], d=ops_[3], k=kfull)
    elif op == "mul8":
        lim = I32 - (1 << 25) - 65
        es = elems(84, 7, rng)
        b25 = 1 << 25
        for base in (0, 1 << 26, -(1 << 26), 5 << 26, -(7 << 26)):
            for e in (b25, b25 - 1, -b25, -b25 + 1, -b25 - 1, b25 + 1):
                es.append(with_top((base + e,) * 8, 1))
                es.append(with_top(tuple((base + e) * (1 if i & 1 else -1) for i in range(8)), -1))
        es += [(lim,) * 8 + (HALF - 9,), (-lim,) * 8 + (-HALF + 9,), tuple(lim if i & 1 else -lim for i in range(8)) + (HALF - 9,)]
        for i, a in enumerate(pairs_of(es)):
            add("pool%d" % i, a=a)
    elif op == "mul_xi":
        es = elems(55, 3, rng)
        b25 = 1 << 25
        for base in (0, 1 << 26, -(3 << 26)):
            for e in (b25, b25 - 1, -b25, -b25 + 1):
                es.append(with_top((base + e,) * 8, 1))
        ps = pairs_of(es)
        ps += [(x, lneg(x)) for x in es[::9]] + [(lneg(x), x) for x in es[4::9]]                  # opposite signs in the two coefficients
        m = (I32 - HALF - 64) // 2 - 16                                                         # own + partner + 2^28 + own / 2^26 + 1 < 2^31
        top = int(55 * TOP_PER_Q)
        ps += [((m,) * 8 + (top,), (m,) * 8 + (top,)), ((m,) * 8 + (top,), (-m,) * 8 + (-top,)), ((-m,) * 8 + (-top,), (m,) * 8 + (top,)),
               ((-m,) * 8 + (top,), (-m,) * 8 + (-top,))]
        for i, a in enumerate(ps):
            add("pool%d" % i, a=a)
    elif op == "mul":
        tgt = Fraction(2055, 10)                               # 2 v^2 / (R / q) = 498.9: within 1 % of the value cap
        es = canonical_edges() + tight_extremes(both_signs([Fraction(1, 2), 1, 5, 80, tgt]))
        ps = pairs_of(es)
        for i, a in enumerate(ps):
            add("tight%d" % i, a=a, b=ps[(i * 5 + 1) % len(ps)])
        lz = lambda kk, s, t=0: lazy_limbs(kk, t, s)
        P, N, ALT = SIGN_PATTERNS[0], SIGN_PATTERNS[1], SIGN_PATTERNS[2]
        for ka, kb in ((3, 2), (2, 3), (7, 1), (1, 7), (Fraction(27, 10), Fraction(27, 10)), (2, 1), (1, 2), (4, Fraction(18, 10))):
            for sa0, sa1, sb0, sb1 in ((P, P, P, N), (N, N, P, N), (P, P, P, P), (P, N, N, P), (ALT, ALT, ALT, P), (P, ALT, N, ALT), (N, P, P, P)):
                add("lazy%s/%s" % (ka, kb), a=(lz(ka, sa0), lz(ka, sa1, 1)), b=(lz(kb, sb0, -1), lz(kb, sb1, Fraction(1, 2))))
        es = elems(40, 2, rng)
        ps = pairs_of(es)
        for i, a in enumerate(ps):
            add("pool%d" % i, a=a, b=ps[(i * 5 + 1) % len(ps)])
    elif op == "sqr":
        tgt = Fraction(2050, 10)
        es = canonical_edges() + tight_extremes(both_signs([Fraction(1, 2), 1, 5, 80]))
        for i, a in enumerate(pairs_of(es)):
            add("tight%d" % i, a=a)
        for p in EXTREME_PATTERNS[:4]:
            add("edge", a=(with_top(p, tgt), with_top(p, tgt)))
            add("edge", a=(with_top(p, -tgt), with_top(p, -tgt)))
            add("edge", a=(with_top(p, 144), with_top(p, -144)))
        P, N, ALT = SIGN_PATTERNS[0], SIGN_PATTERNS[1], SIGN_PATTERNS[2]
        for k0, k1 in ((Fraction(19, 10), Fraction(19, 10)), (Fraction(27, 10), Fraction(1, 100)), (Fraction(1, 100), Fraction(27, 10)),
                       (Fraction(5, 2), Fraction(1, 5)), (1, 2), (2, 1)):
            for s0, s1 in ((P, P), (P, N), (N, P), (N, N), (ALT, P), (P, ALT), (ALT, ALT), (ALT, lambda i: -1 if i & 1 else 1)):
                add("lazy%s/%s" % (k0, k1), a=(lazy_limbs(k0, 0, s0), lazy_limbs(k1, Fraction(1, 2), s1)))
        # all limbs of both coefficients of ONE SIGN, where the unions of the tracker's rule stay small.  Equal magnitudes: the imaginary product
        # (2 a0) a1 fills the column bound, 8 x 5.4 x 2.7 units.  Unequal ones: (a0 + a1)(a0 - a1) is the most negative (or positive) column
        # the contract admits, 8 x 4.2 x -2.0 units at 1.1 / 3.1.
        for k0, k1 in ((Fraction(27, 10), Fraction(27, 10)), (Fraction(11, 10), Fraction(31, 10)), (Fraction(31, 10), Fraction(11, 10)),
                       (2, Fraction(29, 10)), (Fraction(29, 10), 2)):
            for sg in (P, N):                              # one sign throughout: the tracker's intervals of a0 + a1 and a0 - a1 are then the limbs' own
                for t0, t1 in ((0, Fraction(1, 2)), (1, -1), (-5, 5)):
                    add("lazy-same-sign%s/%s" % (k0, k1), a=(lazy_limbs(k0, t0, sg), lazy_limbs(k1, t1, sg)))
        for i, a in enumerate(pairs_of(elems(60, Fraction(3, 2), rng))):
            add("pool%d" % i, a=a)
    elif op == "mul_fp":
        tgt = 290
        es = canonical_edges() + tight_extremes(both_signs([Fraction(1, 2), 1, 5, 80, tgt]))
        ps = pairs_of(es)
        for i, a in enumerate(ps):
            add("tight%d" % i, a=a, b=ps[(i * 5 + 1) % len(ps)])
        for ka, kb in ((7, 2), (2, 7), (Fraction(38, 10), Fraction(38, 10)), (3, 4), (1, 7)):
            for sa in SIGN_PATTERNS:
                for sb in SIGN_PATTERNS[:3]:
                    add("lazy%s/%s" % (ka, kb), a=(lazy_limbs(ka, 0, sa), lazy_limbs(ka, -1, SIGN_PATTERNS[2])), b=(lazy_limbs(kb, Fraction(1, 2), sb), ZERO))
        es = elems(100, 3, rng)
        ps = pairs_of(es)
        for i, a in enumerate(ps):
            add("pool%d" % i, a=a, b=ps[(i * 5 + 1) % len(ps)])
    elif op == "inv":
        es = canonical_edges() + tight_extremes(both_signs([Fraction(1, 2), 1, 5, 80, Fraction(815, 10)]))
        for i, a in enumerate(pairs_of(es)):
            add("tight%d" % i, a=a)
        z = canonical_edges()[0]
        one = canonical_edges()[1]
        add("zero", a=(z, z)); add("zero-lazy", a=(rep(3 * Q, 2, rng), rep(-5 * Q, 2, rng)))
        add("one", a=(one, z)); add("i", a=(z, one))
        add("edge", a=(with_top(EXTREME_PATTERNS[0], Fraction(815, 10)), with_top(EXTREME_PATTERNS[1], -Fraction(815, 10))))
        for k0 in (2, 3, Fraction(38, 10)):
            for s0 in SIGN_PATTERNS:
                for s1 in SIGN_PATTERNS[:3]:
                    add("lazy%s" % k0, a=(lazy_limbs(k0, 0, s0), lazy_limbs(k0, 1, s1)))
        for i, a in enumerate(pairs_of(elems(40, 2, rng))):
            add("pool%d" % i, a=a)
    elif op in ("canon", "to_u256"):
        es = elems(80, 7, rng)
        for kq in range(-80, 81):
            for off in (0, Q - 1, -1, 1):
                n = kq * Q + off
                if abs(n) <= 80 * Q:
                    es.append(rep(n, rng.choice([0, 1, 3, 6]), rng))
        for i, a in enumerate(pairs_of(es)):
            add("pool%d" % i, a=a)
    elif op == "is_zero":
        zs = multiples(ZERO_KS, rng) + multiples(ZERO_KS, rng, lazy=1) + [(0, ZERO), (1, QL), (-1, lneg(QL))]
        for i, (kq, z) in enumerate(zs):
            other = zs[(i * 7 + 3) % len(zs)][1]
            add("zero%d/%d" % (kq, i), a=(z, other))
            for dlt in (1, -1):
                if abs(value(z) + dlt) <= 600 * Q:
                    add("off%d/%d" % (kq, i), a=(_bump(z, dlt), other))
                    add("off%d/%d im" % (kq, i), a=(other, _bump(z, dlt)))
        for i, a in enumerate(pairs_of(elems(600, 6, rng))):
            add("pool%d" % i, a=a)
    elif op == "eq":
        for i, kq in enumerate(ZERO_KS + ZERO_KS):
            n0, n1 = rng.randint(-Q, Q) - kq * Q // 2, rng.randint(-Q, Q) + kq * Q // 2
            b = (rep(n0, 2, rng), rep(n1, 2, rng))
            a = (rep(n0 + kq * Q, 2, rng), rep(n1 - kq * Q, 2, rng))
            add("same%d" % kq, a=a, b=b)
            for dlt in (1, -1):
                if abs(voq(_bump(a[0], dlt)) - voq(b[0])) <= 600:
                    add("off%d" % kq, a=(_bump(a[0], dlt), a[1]), b=b)
                if abs(voq(_bump(a[1], dlt)) - voq(b[1])) <= 600:
                    add("off%d im" % kq, a=(a[0], _bump(a[1], dlt)), b=b)
        es = pairs_of(elems(290, 3, rng))
        for i, a in enumerate(es):
            add("pool%d" % i, a=a, b=es[(i * 5 + 1) % len(es)] if i % 4 else a)
    elif op == "u512_greater":
        xs = [0, 1, 2, Q - 1, Q - 2, Q // 2, (1 << 224), (1 << 224) - 1, (1 << 253) + 12345] + [rng.randrange(Q) for _ in range(12)]
        enc = lambda x: rep(to_mont(x) + rng.randint(-80, 79) * Q, rng.choice([0, 2, 6]), rng)
        for im_a in xs[:9]:
            for im_b in (im_a, (im_a + 1) % Q, (im_a - 1) % Q, xs[rng.randrange(len(xs))]):
                for re_a in (xs[rng.randrange(len(xs))], 0, Q - 1):
                    for re_b in (re_a, (re_a + 1) % Q, (re_a - 1) % Q):
                        add("order", a=(enc(re_a), enc(im_a)), b=(enc(re_b), enc(im_b)))
        for _ in range(N_RANDOM):
            add("random", a=(enc(rng.choice(xs)), enc(rng.choice(xs))), b=(enc(rng.choice(xs)), enc(rng.choice(xs))))
    else:
        raise ValueError(op)
    return tuple(out)


def all_cases():
    return {op: cases(op) for op in OPS}


# ---- what keeps the set from being tame (asserted by tests/test_fq_limb_cases.py; not measurements) ------------------------------------------
# an op's value bound, and the largest |value / q| its contract's clause sees in a case
VALUE_BOUNDS = dict(reduce_weak=600, lin2_reduce=600, lin4_reduce=600, is_zero=600, eq=600, canon=80, to_u256=80, u512_greater=80,
                    mul=500, sqr=500, mul_fp=500, inv=80)


def bound_reach(c):
    """the quantity the op's value clause bounds, on this case (0 where the op has none)"""
    op, k = c.op, c.k
    v = [[abs(voq(o[j])) for j in (0, 1)] for o in c.a]
    if op in ("reduce_weak", "is_zero", "canon", "to_u256"): return max(v[0])
    if op == "u512_greater": return max(v[0] + v[1])
    if op == "eq": return max(abs(voq(c.a[0][j]) - voq(c.a[1][j])) for j in (0, 1))
    if op == "lin2_reduce": return max(abs(k[0]) * v[0][j] + abs(k[1]) * v[1][j] for j in (0, 1))
    if op == "lin4_reduce": return max(sum(abs(k[t]) * v[t][j] for t in range(4)) for j in (0, 1))
    if op == "mul": return max(v[0][0] * max(v[1]) + v[0][1] * max(v[1]), 0) / R_OVER_Q
    if op == "sqr":
        a0, a1 = voq(c.a[0][0]), voq(c.a[0][1])
        return max(max(2 * abs(o), abs(a0 + a1)) * max(abs(p), abs(o - p)) for o, p in ((a0, a1), (a1, a0))) / R_OVER_Q
    if op == "mul_fp": return max(v[0]) * v[1][0] / R_OVER_Q
    if op == "inv": return 2 * (max(v[0]) ** 2 / R_OVER_Q + Fraction(501, 1000))
    return 0


COLUMN_FLOOR = dict(mul=1 << 62, mul_fp=1 << 62, inv=1 << 62, sqr=1 << 62)


def op_stats(op):
    """{cases, col_hi, col_lo, reach} of an op's case set: the extreme accumulator values of its products and the largest bounded quantity"""
    st = {}
    for c in cases(op):
        expected(c, st)
    st["cases"] = len(cases(op))
    st["reach"] = max(bound_reach(c) for c in cases(op))
    st["max_voq"] = max(abs(voq(o[j])) for c in cases(op) for o in c.a for j in (0, 1))
    return st


def check_tameness(op, st):
    if op in COLUMN_FLOOR:
        assert st["col_hi"] > COLUMN_FLOOR[op], (op, st["col_hi"].bit_length())
        assert st["col_lo"] < -COLUMN_FLOOR[op], (op, st["col_lo"].bit_length())
    if op in VALUE_BOUNDS:
        assert Fraction(99, 100) * VALUE_BOUNDS[op] <= st["reach"] <= VALUE_BOUNDS[op], (op, float(st["reach"]))


# ---- buffers of the hook -------------------------------------------------------------------------------------------------------------------
def pack(cs):
    """(operand bytes, factor bytes) of a list of cases in the hook's format: n x 4 x 18 and n x 4 native int32"""
    words, ks = [], []
    for c in cs:
        for o in c.a:
            words.extend(o[0]); words.extend(o[1])
        ks.extend(bal(x, 32) for x in c.k)
    return struct.pack("=%di" % len(words), *words), struct.pack("=%di" % len(ks), *ks)


def unpack(out, flags, n):
    """[(18 limbs, flag)] from the hook's output buffers"""
    w = struct.unpack("=%di" % (18 * n), out)
    return [(tuple(w[18 * i:18 * i + 18]), flags[i]) for i in range(n)]
