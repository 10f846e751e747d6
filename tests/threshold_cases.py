"""The case set of the threshold call (include/bn254_hip.h: bn254_batch_threshold_combine_keyed), shared by its host compilation
(tests/test_threshold_cases.py) and the GPU tests: Fr operands, Lagrange point sets, key sets and tuple shapes.  Inputs only — the
expectations are tests/threshold_model.py's."""
import random

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
INV2 = (R + 1) // 2

# ---- Fr ----------------------------------------------------------------------------------------------------------------------------------------
FR_OPERANDS = [0, 1, R - 1, R, R + 1, (1 << 256) - 1, (1 << 256) % R]
# pairs whose product is 0, 1 and r - 1 mod r
FR_PRODUCT_PAIRS = [(0, 5), (R, R - 1), (2, INV2), (R - 1, R - 1), (0xDEADBEEF, pow(0xDEADBEEF, -1, R)), (R - 1, 1), (2, (R - 1) * INV2 % R), (R + 1, R - 1)]
FR_INVERSES = [1, 2, R - 1, 0xDEADBEEF]
# the uint32_t load: the operand's low word is what is loaded, whatever stands above it
FR_U32_LOADS = [0xFFFFFFFF, 1 << 32, (1 << 32) + 5, (R << 1) + 0x80000000, ((1 << 256) - 1) ^ 0x7FFFFFFF]


def fr_pairs():
    """every operand against every operand, then the product pairs"""
    return [(a, b) for a in FR_OPERANDS for b in FR_OPERANDS] + FR_PRODUCT_PAIRS


def fr_random(n, seed):
    rnd = random.Random(seed)
    return [(rnd.randrange(1 << 256), rnd.randrange(1 << 256)) for _ in range(n)]


# ---- Lagrange point sets -------------------------------------------------------------------------------------------------------------------------
def lagrange_sets():
    rnd = random.Random(20261020)
    shuffled = list(range(1, 10))
    rnd.shuffle(shuffled)
    wide = sorted(rnd.sample(range(1, 1 << 32), 65))
    return [[7], [1], [1, 2], [3, 9], list(range(1, 10)), list(range(9, 0, -1)), shuffled, [1000, 1001], [(1 << 32) - 2, (1 << 32) - 1],
            [1, (1 << 32) - 1], [(1 << 32) - 1, 1], list(range(1, 66)), wide, [31, 32, 33, 63, 64, 65, 96, 97]]


# ---- key sets: (name, number of keys, the dealing's threshold or None for independent keys, f(0) or None for a random one) -----------------------
KEY_SETS = [("dealt9_t1", 9, 1, None), ("dealt9_t2", 9, 2, None), ("dealt9_t5", 9, 5, None), ("dealt9_t9", 9, 9, None),
            ("dealt70_t63", 70, 63, None), ("dealt70_t64", 70, 64, None), ("dealt70_t65", 70, 65, None),
            ("random9", 9, None, None), ("zero9_t5", 9, 5, 0), ("ident9", 9, None, None)]
IDENT_KEY = 2     # of "ident9": the identity as a registered key (secret 0) — its all-zero share verifies, and its term is the identity


def coefficients(name, t, secret):
    """the polynomial of a dealt set: f(0) first"""
    rnd = random.Random("threshold/" + name)
    c = [rnd.randrange(1, R) for _ in range(t)]
    if secret is not None:
        c[0] = secret
    return c


def independent_secrets(name, n):
    rnd = random.Random("threshold/" + name)
    sks = [rnd.randrange(1, R) for _ in range(n)]
    if name == "ident9":
        sks[IDENT_KEY] = 0
    return sks


def secrets_of(name, n, dealt_t, secret):
    """-> (the n share secrets, f(0) or None for independent keys); key j's secret is f(j + 1)"""
    if dealt_t is None:
        return independent_secrets(name, n), None
    c = coefficients(name, dealt_t, secret)
    return [sum(a * pow(x, e, R) for e, a in enumerate(c)) % R for x in range(1, n + 1)], c[0]


# ---- tuples: lists of (key index, kind) ------------------------------------------------------------------------------------------------------------
# kind -> the share and the status it earns: "ok" the key's signature (0), "wrong" another point of the curve (9), "curve" a byte flipped off the
# curve (4), "big" a coordinate >= q (6, NotMemberError: the decoder's code for it), "oob" a valid signature naming key n_keys + 3 (2),
# "again" the previous share of the tuple repeated.  (A key registered with a failed proof of possession: test_gpu_threshold.py, its own set.)
KIND_STATUS = {"ok": 0, "wrong": 9, "curve": 4, "big": 6, "oob": 2}


def full_shapes(t, n_keys):
    """every tuple shape of the case set for a threshold t over n_keys keys (t >= 2, n_keys >= t + 3)"""
    low = list(range(t))
    shapes = [
        ("exactly_t", [(j, "ok") for j in low]),
        ("t_minus_1", [(j, "ok") for j in low[:-1]]),
        ("more_than_t", [(j, "ok") for j in range(n_keys)]),
        ("upper_keys", [(j, "ok") for j in range(n_keys - t, n_keys)]),
        ("descending", [(j, "ok") for j in range(n_keys - 1, n_keys - t - 2, -1)]),
        ("twice", [(0, "ok"), (0, "again")] + [(j, "ok") for j in low[1:]] + [(low[-1], "again")]),
        ("valid_then_invalid", [(0, "ok"), (0, "wrong")] + [(j, "ok") for j in low[1:]]),
        ("invalid_then_valid", [(1, "wrong"), (1, "ok"), (0, "ok")] + [(j, "ok") for j in low[2:]]),
        ("empty", []),
        ("all_bad", [(0, "wrong"), (1, "curve"), (2, "big"), (3, "oob")]),
    ]
    for kind in ("wrong", "curve", "big", "oob"):      # the fault among the lowest keys: key 1 drops out, the next key moves up
        shapes.append(("low_" + kind, [(0, "ok"), (1, kind)] + [(j, "ok") for j in range(2, t + 1)]))
        shapes.append(("low_" + kind + "_short", [(0, "ok"), (1, kind)] + [(j, "ok") for j in range(2, t)]))
    return shapes


def short_shapes(t, n_keys):
    """exactly t (the upper keys, shuffled), t - 1, and everybody (the lowest t used)"""
    rnd = random.Random(t * 1000 + n_keys)
    upper = list(range(n_keys - t, n_keys))
    rnd.shuffle(upper)
    shapes = [("exactly_t", [(j, "ok") for j in upper]), ("everybody", [(j, "ok") for j in range(n_keys)])]
    if t > 1:
        shapes.append(("t_minus_1", [(j, "ok") for j in upper[:-1]]))
    return shapes


def shapes_for(name, n_keys, t):
    if name == "dealt9_t5":
        return full_shapes(t, n_keys)
    if name in ("random9", "zero9_t5", "ident9"):      # the shapes whose bytes depend on the key set
        return [s for s in full_shapes(t, n_keys) if s[0] in ("exactly_t", "t_minus_1", "more_than_t", "descending", "twice", "low_wrong")]
    return short_shapes(t, n_keys)


def threshold_of(name, dealt_t):
    return dealt_t if dealt_t is not None else 5
