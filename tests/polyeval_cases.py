"""The case set of bn254_batch_g2_poly_eval (include/bn254_hip.h), shared by tests/test_polyeval_cases.py (host compilation) and
tests/test_gpu_poly_eval.py: the smallest shapes at which each piece can go wrong.  A case is ONE polynomial — its coefficients as known
multiples a_k of the generator (or, for the coefficients outside the order-r subgroup, as bytes), the decode faults planted in it — and the
points xs it is evaluated at.  tests/polyeval_model.py says what each evaluation must give."""
import random

from oracle import bn254_model as M
from tests import polyeval_model as PM

R = M.R
WAVE = 64
# empty; one lane's; both sides of the shipped split (16); one coefficient per lane of the wave layout with and without empty lanes; chunks of
# 2, 3 and 4 coefficients with a ragged last chunk (65, 127, 129, 171, 200) and without (128)
LENGTHS = [0, 1, 2, 3, 15, 16, 17, 63, 64, 65, 127, 128, 129, 171, 200]
# no bit, one bit, both sides of 8 and of 16 bits, the top bit alone, every bit
POINTS = [0, 1, 2, 3, 255, 256, 257, 65535, 65536, 1 << 31, (1 << 32) - 1]
# what the instrumented builds of the host compilation run: these lengths, every pattern, the first point of each case
LIGHT_LENGTHS = [0, 1, 2, 3, 17, 65]


def chunk_len(n):
    return -(-n // WAVE)


def case(name, a, xs, faults=None, points=None):
    return {"name": name, "a": None if a is None else [v % R for v in a], "xs": list(xs), "faults": dict(faults or {}), "points": points}


def times_linear(g, x):
    """the coefficients of (X - x) g(X), lowest degree first"""
    out = [0] * (len(g) + 1)
    for k, gk in enumerate(g):
        out[k] = (out[k] - x * gk) % R
        out[k + 1] = (out[k + 1] + gk) % R
    return out


def tree_partner(n):
    """the lane whose product is the first the tree adds to lane 0's: the largest power of two below the number of non-empty chunks"""
    chunks = -(-n // chunk_len(n))
    c = 1
    while 2 * c < chunks:
        c *= 2
    return c


def cases_for(n, cursor):
    """every case of one length; cursor: where in POINTS this length starts drawing its points"""
    rnd = random.Random(7000 + n)
    at = [cursor]

    def some(count=2, nonzero=False):
        out = []
        while len(out) < count:
            x = POINTS[at[0] % len(POINTS)]
            at[0] += 1
            if x or not nonzero:
                out.append(x)
        return out

    def rand(k):
        return [rnd.randrange(1, R) for _ in range(k)]

    out = [case("random", rand(n), POINTS if n in (3, 17, 65) else some(3))]
    if n == 0:
        return out
    out.append(case("all_identity", [0] * n, some()))
    if n >= 2:
        out.append(case("identity_top", rand(n - 1) + [0], some()))
        out.append(case("identity_bottom", [0] + rand(n - 1), some()))
        a = rand(n)
        out.append(case("equal_neighbours", [a[0]] * n, [1]))                       # the mixed addition meets P = Q at every step
        x = some(1, nonzero=True)[0]
        v = rnd.randrange(1, R)
        out.append(case("through_identity", [pow(-x, n - 1 - k, R) * v for k in range(n)], [x]))   # x acc + C_k = O at every step below the top
        x = some(1)[0]
        out.append(case("root_at_x", times_linear(rand(n - 1), x), [x]))
        # lane 0's product and its first partner's in the tree: equal, then opposite (a_j = +- x^(c L) a_(c L + j) over chunk 0)
        x = some(1, nonzero=True)[0]
        L, c = chunk_len(n), tree_partner(n)
        for name, sign in (("tree_equal", 1), ("tree_opposite", -1)):
            a = rand(n)
            for j in range(L):
                a[j] = sign * pow(x, c * L, R) * a[c * L + j] if c * L + j < n else 0
            out.append(case(name, a, [x]))
    if n >= 3:
        a = rand(n)
        a[n // 2] = 0
        out.append(case("identity_middle", a, some()))
    if chunk_len(n) >= 2:
        x = some(1)[0]
        L = chunk_len(n)
        a = rand(n)
        a[L:2 * L] = times_linear(rand(L - 1), x)                                 # chunk 1's partial is the identity
        out.append(case("chunk_root", a, [x]))
    # decode faults: off the curve or a coordinate >= q, at the first, a middle and the last coefficient; two different ones: the first wins
    out.append(case("fault_first", rand(n), some(1), faults={0: "curve"}))
    out.append(case("fault_last", rand(n), some(1), faults={n - 1: "big"}))
    if n >= 3:
        out.append(case("fault_middle", rand(n), some(1), faults={n // 2: "big"}))
        out.append(case("two_faults", rand(n), some(1), faults={n // 2: "curve", n - 1: "big"}))
        out.append(case("two_faults_swapped", rand(n), some(1), faults={1: "big", n - 1: "curve"}))
    if n <= PM.GROUP_MAX_COEFFS:
        # coefficients outside the order-r subgroup: group arithmetic in Python integers is the only model
        pts = [M.g2_to_uncompressed(M.g2_mul(M.G2_GEN, 3 + k)) for k in range(n)]
        pts[n - 1] = PM.off_subgroup_point(100 * n)
        if n == 3:
            pts[0] = PM.off_subgroup_point(7)
        out.append(case("off_subgroup", None, some(3), points=pts))
    return out


def all_cases():
    """(length, case) over LENGTHS"""
    out = []
    for i, n in enumerate(LENGTHS):
        out += [(n, cs) for cs in cases_for(n, 3 * i)]
    return out


def is_light(n, cs):
    return n in LIGHT_LENGTHS
