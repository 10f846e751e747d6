"""bn254_batch_threshold_combine_keyed restated (include/bn254_hip.h): Fr and the Lagrange coefficients in Python integers, rank and select
over the collect's rows, the group signature as sum lambda_j sigma_j through oracle.bn254_model's g1_mul / g1_add (valid for ANY key set),
and — for keys dealt from one polynomial — the signature under f(0).  Shared by tests/test_threshold_cases.py (host compilation) and the
GPU tests.  Nothing here comes from the code under test."""
from oracle import bn254_model as M
from tests import collect_model

R = M.R


def fr_op(op, a, b=0):
    """the Fr hook's operations on operands reduced mod r: 0 mul, 1 add, 2 sub, 3 neg, 4 inv (0 -> 0), 5 the value itself
    (op 6, the uint32 load, reads the raw operand: fr_load_u32)"""
    a, b = a % R, b % R
    if op == 0:
        return a * b % R
    if op == 1:
        return (a + b) % R
    if op == 2:
        return (a - b) % R
    if op == 3:
        return -a % R
    if op == 4:
        return pow(a, -1, R) if a else 0
    return a


def fr_load_u32(a):
    """op 6 of the hook: the operand's low 32 bits (of the bytes as given, before any reduction) loaded as a uint32_t"""
    return a & 0xFFFFFFFF


def lagrange_at_zero(xs):
    """the coefficients of the distinct points xs, in their order: prod x_k / prod (x_k - x_j) over k != j, mod r"""
    out = []
    for j, xj in enumerate(xs):
        num = den = 1
        for k, xk in enumerate(xs):
            if k != j:
                num = num * xk % R
                den = den * (xk - xj) % R
        out.append(num * pow(den, -1, R) % R)
    return out


def deal(coeffs, n):
    """the n share secrets f(1) .. f(n) of the polynomial with the given coefficients (f(0) first)"""
    return [sum(c * pow(x, e, R) for e, c in enumerate(coeffs)) % R for x in range(1, n + 1)]


def select(share_keys, share_status, sizes, tuple_status, bm_words, threshold):
    """-> per tuple (status, |V|, row, chosen): row = S (the `threshold` lowest keys of V) when |V| >= threshold, else V with status 9;
    chosen = [(key, index of its first status-0 share)] for the keys of S, in key order; a tuple whose status is non-zero already keeps it"""
    rows, counts, picked = collect_model.select(share_keys, share_status, sizes, tuple_status, bm_words)
    out = []
    for i, row in enumerate(rows):
        if tuple_status[i]:
            out.append((tuple_status[i], 0, [0] * bm_words, []))
            continue
        first = {}
        for s in picked[i]:
            first[share_keys[s]] = s
        members = sorted(first)
        if len(members) < threshold:
            out.append((9, len(members), row, []))
            continue
        kept = members[:threshold]
        used = [0] * bm_words
        for j in kept:
            used[j // 32] |= 1 << (j % 32)
        out.append((0, len(members), used, [(j, first[j]) for j in kept]))
    return out


def to_point(b64):
    return None if b64 == bytes(64) else M.g1_from_uncompressed(b64)


def to_bytes(p):
    return bytes(64) if p is None else M.g1_to_uncompressed(p)


def weighted_sum(points, scalars):
    """sum k_s P_s over 64-byte encodings, scalars as integers (used as they are)"""
    acc = None
    for p, k in zip(points, scalars):
        acc = M.g1_add(acc, M.g1_mul(to_point(p), k))
    return to_bytes(acc)


def group_signature(shares, chosen):
    """expectation 1: sum lambda_j(S) sigma_j over the chosen (key, share index) pairs, x_j = j + 1"""
    lam = lagrange_at_zero([j + 1 for j, _ in chosen])
    return weighted_sum([shares[s] for _, s in chosen], lam)


def signature_under(message, secret):
    """expectation 2, for dealt keys: the signature of the message under f(0)"""
    return to_bytes(M.sign(message, secret % R)) if secret % R else bytes(64)
