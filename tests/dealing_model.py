"""bn254_ctx_check_dealing and bn254_batch_g2_msm restated (include/bn254_hip.h) in Python integers: the weights rho_j, the coefficients c_j of
the degree check from their definition, the weighted sum in G2 through oracle.bn254_model's g2_mul / g2_add, and the call's four outcomes.
Shared by tests/test_dealing_cases.py (host compilation) and tests/test_gpu_dealing.py.  Nothing here comes from the code under test."""
import hashlib

from oracle import bn254_model as M
from tests import threshold_model as TM

R = M.R
NO_KEY = 0xFFFFFFFF


def rho(seed, j):
    """the 128-bit weight of index j: the first 16 bytes of SHA-256(seed || le64(j)), little-endian, 0 mapped to 1"""
    v = int.from_bytes(hashlib.sha256(bytes(seed) + int(j).to_bytes(8, "little")).digest()[:16], "little")
    return v or 1


def basis_at(t, k, x):
    """L_k(x) over the points x_i = i + 1, i < t, straight from the definition"""
    num = den = 1
    for i in range(t):
        if i != k:
            num = num * (x - (i + 1)) % R
            den = den * ((k + 1) - (i + 1)) % R
    return num * pow(den, -1, R) % R


def coefficients_by_definition(n, t, seed):
    """c_j = rho_j for j >= t, c_k = -sum_j rho_j L_k(x_j) for k < t — O(t^2 (n - t)): the small shapes"""
    rhos = {j: rho(seed, j) for j in range(t, n)}
    return [-sum(rhos[j] * basis_at(t, k, j + 1) for j in rhos) % R for k in range(t)] + [rhos[j] for j in range(t, n)]


def coefficients(n, t, seed):
    """the same in barycentric form: L_k(x_j) = N_j / ((x_j - x_k) D_k), N_j = prod_i (x_j - x_i), D_k = prod_{i != k} (x_k - x_i), each
    product written out (no factorials: those are the code under test's)"""
    rhos = {j: rho(seed, j) for j in range(t, n)}
    d_inv = []
    for k in range(t):
        d = 1
        for i in range(t):
            if i != k:
                d = d * (k - i) % R
        d_inv.append(pow(d, -1, R))
    big_n = {}
    for j in rhos:
        v = 1
        for i in range(t):
            v = v * (j - i) % R
        big_n[j] = v
    out = []
    for k in range(t):
        s = sum(rhos[j] * big_n[j] * pow(j - k, -1, R) for j in rhos) % R
        out.append(-s * d_inv[k] % R)
    return out + [rhos[j] for j in range(t, n)]


def evaluate(coeffs, x):
    return sum(c * pow(x, e, R) for e, c in enumerate(coeffs)) % R


def g2_point(b128):
    return None if b128 == bytes(128) else M.g2_from_uncompressed(b128, subgroup_check=False)


def g2_bytes(p):
    return bytes(128) if p is None else M.g2_to_uncompressed(p)


def g2_weighted_sum(points, scalars):
    """sum k_s P_s over 128-byte encodings, scalars as integers (used as they are)"""
    acc = None
    for p, k in zip(points, scalars):
        acc = M.g2_add(acc, M.g2_mul(g2_point(p), k))
    return g2_bytes(acc)


def group_key(keys, t):
    """K = sum_{k<t} lambda_k pk_k over the points 1 .. t"""
    return g2_weighted_sum(keys[:t], TM.lagrange_at_zero(list(range(1, t + 1))))


def check(keys, key_status, t, seed):
    """the call on 128-byte keys and their registration statuses -> (status, bad_key, group_pk), by group arithmetic in Python integers"""
    n = len(keys)
    for j, st in enumerate(key_status):
        if st:
            return st, j, bytes(128)
    if t > n:
        return 9, NO_KEY, bytes(128)
    if t < n and g2_weighted_sum(keys, coefficients(n, t, seed)) != bytes(128):
        return 9, NO_KEY, bytes(128)
    return 0, NO_KEY, group_key(keys, t)


def check_scalars(secrets, key_status, t, seed):
    """the same for keys pk_j = s_j * G2::one() given by their scalars: the sums are taken in Fr -> (status, bad_key, scalar of K or None)"""
    n = len(secrets)
    for j, st in enumerate(key_status):
        if st:
            return st, j, None
    if t > n:
        return 9, NO_KEY, None
    if t < n and sum(c * s for c, s in zip(coefficients(n, t, seed), secrets)) % R:
        return 9, NO_KEY, None
    lam = TM.lagrange_at_zero(list(range(1, t + 1)))
    return 0, NO_KEY, sum(a * s for a, s in zip(lam, secrets)) % R
