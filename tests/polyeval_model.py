"""bn254_batch_g2_poly_eval and bn254_ctx_register_keys_commitments restated (include/bn254_hip.h) in Python integers: the value of a
polynomial with G2 coefficients at an integer point, once in Fr for coefficients that are known multiples a_k of the generator — the expected
point is (sum a_k x^k mod r) * G2::one(), one key derivation of the C oracle — and once by group arithmetic over oracle.bn254_model's g2_mul /
g2_add (tests/dealing_model.py: g2_weighted_sum), which also serves coefficients OUTSIDE the order-r subgroup; and the call's statuses.
Shared by tests/test_polyeval_cases.py (host compilation) and the GPU tests.  Nothing here comes from the code under test."""
from oracle import bn254_model as M
from tests import dealing_cases as DC
from tests import dealing_model as DM

R = M.R
# polynomials up to this many coefficients are also evaluated by group arithmetic (an off-subgroup coefficient only there): x^k < 2^64 < r,
# so the scalar of the defining identity, x^k mod r, is the integer power Horner's rule multiplies by
GROUP_MAX_COEFFS = 3
IDENTITY = bytes(128)
ST_OK, ST_INDEX_OOB = 0, 2


def powers(x, n):
    """x^k mod r for k < n, with 0^0 = 1: the scalars of the defining identity"""
    return [pow(x, k, R) for k in range(n)]


def eval_scalar(a, x):
    """sum a_k x^k mod r"""
    return sum(ak * xk for ak, xk in zip(a, powers(x, len(a)))) % R


def key_of(c, scalar):
    """scalar * G2::one() as 128 bytes by the C oracle; the identity as zero bytes"""
    scalar %= R
    return c.public_key_g2(scalar.to_bytes(32, "big")) if scalar else IDENTITY


def eval_by_group(points, x):
    """sum (x^k mod r) C_k over 128-byte encodings by group arithmetic in Python integers"""
    return DM.g2_weighted_sum(points, powers(x, len(points)))


def off_subgroup_point(seed):
    """a point of the twist curve that is NOT in the order-r subgroup (legal for a call that decodes with flags 0), as 128 bytes"""
    k = seed
    while True:
        k += 1
        x = (k % M.Q, 1)
        y = M.f2_sqrt(M.f2_add(M.f2_mul(M.f2_mul(x, x), x), M.B2))
        if y is None:
            continue
        p = (x, y)
        assert M.g2_on_curve(p)
        if not M.g2_in_subgroup(p):
            return M.g2_to_uncompressed(p)


def coefficients(c, case):
    """the 128-byte coefficients of a case, its faults planted"""
    pts = list(case["points"]) if case.get("points") is not None else [key_of(c, v) for v in case["a"]]
    for at, kind in case["faults"].items():
        pts[at] = DC.plant(pts[at], kind)
    return pts


def expected(c, case, x):
    """(status, 128 bytes) of one evaluation of a case's polynomial: the lowest faulty coefficient's status with the identity, else the value"""
    if case["faults"]:
        at = min(case["faults"])
        return DC.FAULT_STATUS[case["faults"][at]], IDENTITY
    if case.get("points") is not None:
        assert len(case["points"]) <= GROUP_MAX_COEFFS
        return ST_OK, eval_by_group(case["points"], x)
    return ST_OK, key_of(c, eval_scalar(case["a"], x))


def cross_check(c, case, x):
    """the model against itself: the oracle's product against group arithmetic, on the polynomials short enough for Python"""
    assert not case["faults"] and case.get("points") is None and len(case["a"]) <= GROUP_MAX_COEFFS
    return key_of(c, eval_scalar(case["a"], x)) == eval_by_group([key_of(c, v) for v in case["a"]], x)


def share_keys(c, a, n):
    """pk_j = f(j + 1) * G2 for j < n: what bn254_ctx_register_keys_commitments registers"""
    return [key_of(c, eval_scalar(a, j + 1)) for j in range(n)]
