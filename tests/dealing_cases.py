"""The case set of bn254_ctx_check_dealing and bn254_batch_g2_msm (include/bn254_hip.h), shared by tests/test_dealing_cases.py (host
compilation) and tests/test_gpu_dealing.py.  A case is a key set given by its secrets (pk_j = s_j * G2::one(), key j standing for
x_j = j + 1), the faults planted in it, the threshold it is checked under and what the call must say.  Every failing case must read 9 under
each of SEEDS, every passing one the same bytes under each."""
import random

from oracle import bn254_model as M
from tests import threshold_model as TM

R = M.R
SHAPES = [(1, 1), (2, 1), (2, 2), (3, 2), (5, 3), (33, 17), (64, 43), (65, 33), (97, 65)]
DEVICE_ONLY_SHAPES = [(256, 171)]
SEEDS = [bytes(32), bytes(range(32)), bytes(255 - i for i in range(32))]
# lengths of a segment of the weighted sum: empty, one lane, both sides of the default lane / wave split, of one wave and of two
SEGMENT_LENGTHS = [0, 1, 2, 15, 16, 17, 63, 64, 65, 129]
# the scalars every segment carries: 0, 1, r - 1, r, 2^256 - 1
EDGE_SCALARS = [0, 1, R - 1, R, (1 << 256) - 1]
# planted decode faults -> the status registration gives the key
FAULT_STATUS = {"curve": 4, "big": 6}


def poly(rnd, degree):
    """coefficients (f(0) first) of a random polynomial of exactly this degree; degree < 0: the zero polynomial"""
    if degree < 0:
        return [0]
    return [rnd.randrange(R) for _ in range(degree)] + [rnd.randrange(1, R)]


def case(name, t, secrets, expect, faults=None, pop_fail=None):
    return {"name": name, "t": t, "secrets": list(secrets), "expect": expect, "faults": dict(faults or {}), "pop_fail": pop_fail}


def cases_for(n, t):
    """every case of one shape.  expect: "pass", "fail" (status 9, no key named) or ("bad", key index, status or None = the registration's)"""
    rnd = random.Random(1000 * n + t)
    honest = TM.deal(poly(rnd, t - 1), n)
    out = [case("honest", t, honest, "pass")]
    if t >= 2:
        out.append(case("degree_t_minus_2", t, TM.deal(poly(rnd, t - 2), n), "pass"))
    if n > t:
        out.append(case("degree_t", t, TM.deal(poly(rnd, t), n), "fail"))
        high, low = rnd.randrange(t, n), rnd.randrange(t)
        for name, at in (("replaced_high", high), ("replaced_low", low)):
            s = list(honest)
            s[at] = (s[at] + rnd.randrange(1, R)) % R
            out.append(case(name, t, s, "fail"))
        # P + D and P' - D: the plain sum of the keys does not change, the weighted one does
        s, d = list(honest), rnd.randrange(1, R)
        s[low], s[high] = (s[low] + d) % R, (s[high] - d) % R
        out.append(case("cancelling_pair", t, s, "fail"))
    if n >= 3 and t >= 2:
        g = poly(rnd, t - 2)                                          # f(x) = (x - 3) g(x): key 2 is the identity
        f = [(-3 * g[0]) % R] + [(g[e - 1] - 3 * g[e]) % R for e in range(1, len(g))] + [g[-1]]
        s = TM.deal(f, n)
        assert s[2] == 0
        out.append(case("root_at_3", t, s, "pass"))
    out.append(case("zero_polynomial", t, [0] * n, "pass"))
    out.append(case("threshold_1_equal_keys", 1, [honest[0]] * n, "pass"))
    if n >= 2:
        out.append(case("threshold_1_one_differs", 1, [honest[0]] * (n - 1) + [(honest[0] + 1) % R], "fail"))
    # decode faults: at the lowest index with a second, different one behind it (the lowest wins), and at a higher index alone
    faults = {0: "curve"}
    if n >= 2:
        faults[n - 1] = "big"
    out.append(case("fault_lowest", t, honest, ("bad", 0, FAULT_STATUS["curve"]), faults=faults))
    if n >= 2:
        at = n - 1 if n < 4 else n // 2
        out.append(case("fault_higher", t, honest, ("bad", at, FAULT_STATUS["big"]), faults={at: "big"}))
    out.append(case("pop_failed", t, honest, ("bad", n // 2, None), pop_fail=n // 2))
    out.append(case("threshold_n_plus_1", n + 1, honest, "fail"))
    return out


def plant(key128, kind):
    """a decode fault in a key's bytes: off the curve, or a coordinate at or above q"""
    if kind == "curve":
        b = bytearray(key128 if key128 != bytes(128) else M.g2_to_uncompressed(M.G2_GEN))
        b[100] ^= 4
        return bytes(b)
    return b"\xff" + bytes(key128[1:])


def random_shapes(count, limit, seed):
    rnd = random.Random(seed)
    out = []
    for _ in range(count):
        n = rnd.randrange(1, limit + 1)
        out.append((n, rnd.randrange(1, n + 1)))
    return out
