"""bn254_batch_g2_vector_combine and bn254_ctx_reshare_commitments restated (include/bn254_hip.h) in Python integers.  Points are known
multiples a * G2::one(), so an expected output is the scalar sum lambda_i a_i,k mod r turned into bytes by ONE key derivation of the C oracle
(tests/polyeval_model.py: key_of); group arithmetic in Python integers (tests/dealing_model.py: g2_weighted_sum) serves only the points that
are not known multiples — outside the order-r subgroup —, with at most 3 terms.  The Lagrange coefficients are the textbook formula, written
here.  Shared by tests/test_reshare_cases.py (host compilation) and the GPU tests.  Nothing here comes from the code under test."""
from oracle import bn254_model as M
from tests import dealing_cases as DC
from tests import dealing_model as DM
from tests import polyeval_model as PM

R = M.R
IDENTITY = bytes(128)
GROUP_MAX_TERMS = 3
ST_OK, ST_INDEX_OOB, ST_FAILED = 0, 2, 9
key_of = PM.key_of


def lagrange_at_zero(keys):
    """lambda_j = prod_{k != j} x_k / (x_k - x_j) mod r over the points x = key + 1 — the weights with sum lambda_j f(x_j) = f(0)"""
    xs = [k + 1 for k in keys]
    out = []
    for j, xj in enumerate(xs):
        num = den = 1
        for k, xk in enumerate(xs):
            if k != j:
                num = num * xk % R
                den = den * (xk - xj) % R
        out.append(num * pow(den, -1, R) % R)
    return out


def evaluate(coeffs, x):
    return sum(c * pow(x, e, R) for e, c in enumerate(coeffs)) % R


def combine_scalars(a, scalars):
    """[sum_i scalars[i] a[i][k] mod r for k]: the combined vector of known multiples"""
    if not a:
        return []
    return [sum(s * row[k] for s, row in zip(scalars, a)) % R for k in range(len(a[0]))]


# ---- vector combine --------------------------------------------------------------------------------------------------------------------------------
def vc_points(c, case):
    """the d x len points of a case as 128-byte encodings, its faults planted"""
    pts = [list(row) for row in case["points"]] if case.get("points") is not None else [[key_of(c, v) for v in row] for row in case["a"]]
    for (i, k), kind in case["faults"].items():
        pts[i][k] = DC.plant(pts[i][k], kind)
    return pts


def vc_expected(c, case):
    """[(status, 128 bytes) per column]: the first faulty point in VECTOR order gives the column its status and the identity"""
    out = []
    for k in range(case["len"]):
        bad = sorted(i for (i, kk) in case["faults"] if kk == k)
        if bad:
            out.append((DC.FAULT_STATUS[case["faults"][(bad[0], k)]], IDENTITY))
        elif case.get("points") is not None:
            assert case["d"] <= GROUP_MAX_TERMS
            out.append((ST_OK, DM.g2_weighted_sum([row[k] for row in case["points"]], case["scalars"])))
        else:
            out.append((ST_OK, key_of(c, sum((s % R) * row[k] for s, row in zip(case["scalars"], case["a"])))))
    return out


def cross_check(c, a, scalars):
    """the model against itself: the oracle's product against group arithmetic, at most 3 terms"""
    assert len(a) <= GROUP_MAX_TERMS
    return [key_of(c, v) for v in combine_scalars(a, scalars)] == [
        DM.g2_weighted_sum([key_of(c, row[k]) for row in a], scalars) for k in range(len(a[0]))]


# ---- reshare ---------------------------------------------------------------------------------------------------------------------------------------
def registered_keys(c, case):
    """(the n old keys as bytes with their faults planted, the registration status each must get: 0, a decode status, or 9 for a failed proof)"""
    keys, st = [], []
    for j, s in enumerate(case["secrets"]):
        kind = case["key_faults"].get(j)
        keys.append(DC.plant(key_of(c, s), kind) if kind else key_of(c, s))
        st.append(DC.FAULT_STATUS[kind] if kind else ST_FAILED if j in case["pop_fail"] else ST_OK)
    return keys, st


def dealer_vectors(c, case):
    """dealer-major 128-byte commitments, faults planted"""
    out = []
    for i, (_, vec) in enumerate(case["dealers"]):
        row = [key_of(c, v) for v in vec]
        for (ii, k), kind in case["faults"].items():
            if ii == i:
                row[k] = DC.plant(row[k], kind)
        out.append(row)
    return out


def dealer_statuses(case):
    """rules 1 to 5, the first that applies"""
    n = len(case["secrets"])
    out = []
    for i, (key, vec) in enumerate(case["dealers"]):
        bad = sorted(k for (ii, k) in case["faults"] if ii == i)
        if key >= n:
            out.append(ST_INDEX_OOB)
        elif case["key_faults"].get(key):
            out.append(DC.FAULT_STATUS[case["key_faults"][key]])
        elif key in case["pop_fail"]:
            out.append(ST_FAILED)
        elif bad:
            out.append(DC.FAULT_STATUS[case["faults"][(i, bad[0])]])
        elif vec[0] % R != case["secrets"][key] % R:
            out.append(ST_FAILED)
        else:
            out.append(ST_OK)
    return out


def bits_of(keys, bm_words):
    row = [0] * bm_words
    for k in keys:
        row[k >> 5] |= 1 << (k & 31)
    return row


def reshare_expected(case):
    """(status, dealer statuses, the keys of used_bits, the positions taken, their lambdas, the scalars of the commitments or None)"""
    st = dealer_statuses(case)
    q = [i for i, s in enumerate(st) if s == ST_OK]
    t = case["threshold"]
    if len(q) < t:
        return ST_FAILED, st, [case["dealers"][i][0] for i in q], [], [], None
    taken = q[:t]                                               # dealer keys increase strictly: the t lowest key indices of Q
    keys = [case["dealers"][i][0] for i in taken]
    lam = lagrange_at_zero(keys)
    return ST_OK, st, keys, taken, lam, combine_scalars([case["dealers"][i][1] for i in taken], lam)
