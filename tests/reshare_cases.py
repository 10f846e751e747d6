"""The case sets of bn254_batch_g2_vector_combine and bn254_ctx_reshare_commitments (include/bn254_hip.h), shared by
tests/test_reshare_cases.py (host compilation) and the GPU tests: the smallest shapes at which each piece can go wrong.  A vector-combine case
is d vectors of len known multiples of the generator, d scalars, the decode faults planted; a reshare case is an old committee by its secrets
(pk_j = s_j * G2::one()), the faults of its registration, and the dealers — (key index, the coefficients of the sub-dealing's polynomial) —
with the faults planted in their vectors.  tests/reshare_model.py says what each must give."""
import random

from oracle import bn254_model as M
from tests import polyeval_model as PM
from tests import reshare_model as RM

R = M.R
# (d, len): one term; one vector; one column; a term wave spans columns; both sides of the sums' default split (16); both sides of one wave;
# three chunks of the wave layout with a ragged last one
VC_SHAPES = [(1, 1), (1, 5), (2, 1), (3, 50), (15, 3), (16, 3), (17, 3), (63, 2), (64, 2), (65, 2), (130, 3)]
# what the instrumented builds of the host compilation run
VC_LIGHT = [(1, 1), (1, 5), (2, 1), (17, 3), (65, 2)]
EDGE_SCALARS = [0, 1, R - 1, R, (1 << 256) - 1, R + 5]
# old (n, t) -> new (n', t')
COMMITTEES = [((1, 1), (1, 1)), ((3, 2), (4, 3)), ((5, 3), (3, 2)), ((7, 5), (7, 5)), ((70, 47), (70, 47))]
RS_LIGHT = COMMITTEES[:3]
DEVICE_ONLY_COMMITTEE = ((256, 171), (256, 171))


def vc_case(name, a, scalars, reduce=0, faults=None, points=None):
    src = a if a is not None else points
    return {"name": name, "d": len(src), "len": len(src[0]) if src else 0, "a": a, "scalars": list(scalars), "reduce": reduce, "faults": dict(faults or {}),
            "points": points}


def vc_cases_for(d, ln):
    rnd = random.Random(9000 + 131 * d + ln)

    def mat():
        return [[rnd.randrange(1, R) for _ in range(ln)] for _ in range(d)]

    def scal():
        return [rnd.randrange(1, R) for _ in range(d)]

    out = [vc_case("random", mat(), scal())]
    edge = [EDGE_SCALARS[(i + d) % len(EDGE_SCALARS)] for i in range(d)]
    out.append(vc_case("edge_scalars_taken", mat(), edge, reduce=0))
    out.append(vc_case("edge_scalars_reduced", mat(), edge, reduce=1))
    a = mat()
    a[0][0] = 0
    a[d - 1][ln - 1] = 0
    a[d // 2] = [0] * ln
    out.append(vc_case("identity_points", a, scal()))
    # column 0: the products are +v, -v, +v, .. — the lane's running sum is the identity after every second term, the tree meets P = -Q
    a, s, v = mat(), scal(), rnd.randrange(1, R)
    for i in range(d):
        a[i][0] = (v if i % 2 == 0 else -v) * pow(s[i], -1, R) % R
    out.append(vc_case("through_identity", a, s))
    # ... all equal: the lane adds P to P, the tree equal partial sums at every level where both sides hold as many terms
    a, s = mat(), scal()
    for i in range(d):
        a[i][0] = v * pow(s[i], -1, R) % R
    out.append(vc_case("equal_products", a, s))
    out.append(vc_case("fault_first", mat(), scal(), faults={(0, 0): "curve"}))
    out.append(vc_case("fault_last", mat(), scal(), faults={(d - 1, ln - 1): "big"}))
    if d >= 3:
        out.append(vc_case("fault_middle", mat(), scal(), faults={(d // 2, ln // 2): "big"}))
    if d >= 2:
        out.append(vc_case("two_faults_one_column", mat(), scal(), faults={(d // 2, 0): "curve", (d - 1, 0): "big"} if d >= 3 else {(0, 0): "big", (1, 0): "curve"}))
    if d <= RM.GROUP_MAX_TERMS:
        # points outside the order-r subgroup: group arithmetic in Python integers is the only model; small scalars keep it quick
        pts = [[M.g2_to_uncompressed(M.g2_mul(M.G2_GEN, 3 + i + 5 * k)) for k in range(ln)] for i in range(d)]
        pts[d - 1][0] = PM.off_subgroup_point(100 * d + ln)
        pts[0][ln - 1] = PM.off_subgroup_point(7 * d + ln)
        out.append(vc_case("off_subgroup", None, [rnd.randrange(1, 1 << 16) for _ in range(d)], points=pts))
    return out


def all_vc_cases():
    return [((d, ln), cs) for d, ln in VC_SHAPES for cs in vc_cases_for(d, ln)]


# ---- reshare ---------------------------------------------------------------------------------------------------------------------------------------
def rs_case(name, secrets, dealers, threshold, t_new, key_faults=None, pop_fail=(), faults=None):
    return {"name": name, "secrets": list(secrets), "dealers": [(k, list(v)) for k, v in dealers], "threshold": threshold, "t_new": t_new,
            "key_faults": dict(key_faults or {}), "pop_fail": set(pop_fail), "faults": dict(faults or {})}


def old_committee(n, t):
    """the old polynomial (f(0) first) and its n shares"""
    rnd = random.Random(500 * n + t)
    f = [rnd.randrange(1, R) for _ in range(t)]
    return f, [RM.evaluate(f, j + 1) for j in range(n)]


def sub_dealing(share, t_new, seed):
    """the coefficients of g with g(0) = share, degree t_new - 1"""
    rnd = random.Random(seed)
    return [share % R] + [rnd.randrange(1, R) for _ in range(t_new - 1)]


def honest_dealers(secrets, t_new, keys):
    return [(k, sub_dealing(secrets[k], t_new, 77 * k + t_new)) for k in keys]


def rs_cases_for(old, new):
    (n, t), (_, t_new) = old, new
    _, secrets = old_committee(n, t)
    everyone = list(range(n))
    out = [rs_case("honest_all", secrets, honest_dealers(secrets, t_new, everyone), t, t_new),
           rs_case("honest_exactly_t_high", secrets, honest_dealers(secrets, t_new, everyone[n - t:]), t, t_new)]
    if n > t:
        spread = sorted(everyone[::2] + everyone[1::2][:max(0, t - len(everyone[::2]))])
        out.append(rs_case("honest_spread", secrets, honest_dealers(secrets, t_new, spread), t, t_new))
    # too few dealers, and a threshold above the key set
    out.append(rs_case("threshold_above_d", secrets, honest_dealers(secrets, t_new, everyone[:t - 1] or everyone[:1]), t if t > 1 else 2, t_new))
    out.append(rs_case("threshold_above_n", secrets, honest_dealers(secrets, t_new, everyone), n + 1, t_new))
    # an index past the key set behind the honest ones: status 2, S unchanged
    d = honest_dealers(secrets, t_new, everyone) + [(n, sub_dealing(5, t_new, 1)), (n + 9, sub_dealing(6, t_new, 2))]
    out.append(rs_case("index_out_of_range", secrets, d, t, t_new))
    if n - 1 < t:
        return out
    low, mid = 0, t_new // 2

    singles = []
    singles.append(("refused_key", None, dict(key_faults={low: "curve"})))
    singles.append(("pop_failed", None, dict(pop_fail={low})))
    singles.append(("fault_commitment_0", None, dict(faults={(low, 0): "big"})))
    singles.append(("fault_commitment_last", None, dict(faults={(low, t_new - 1): "curve"})))
    if t_new >= 3:
        singles.append(("fault_commitment_middle", None, dict(faults={(low, mid): "big"})))
    if t_new >= 2:
        singles.append(("two_decode_faults", None, dict(faults={(low, t_new - 1): "big", (low, t_new - 2): "curve"})))
    singles.append(("d0_other_key", lambda v: [secrets[(low + 1) % n]] + v[1:], {}))
    singles.append(("d0_negated_key", lambda v: [-v[0] % R] + v[1:], {}))
    singles.append(("d0_identity", lambda v: [0] + v[1:], {}))
    # the rule order: a refused key in front of a decode fault in front of a wrong D_0
    singles.append(("key_status_before_decode", lambda v: [v[0] + 1] + v[1:], dict(key_faults={low: "big"}, faults={(low, 0): "curve"})))
    singles.append(("decode_before_d0", lambda v: [v[0] + 1] + v[1:], dict(faults={(low, t_new - 1): "curve"})))
    for name, change, kw in singles:
        d = honest_dealers(secrets, t_new, everyone)
        if change:
            d[low] = (d[low][0], [x % R for x in change(d[low][1])])
        out.append(rs_case(name, secrets, d, t, t_new, **kw))
    # a registered identity key: zero bytes as D_0 qualify
    s = list(secrets)
    s[low] = 0
    out.append(rs_case("identity_key_qualifies", s, honest_dealers(s, t_new, everyone), t, t_new))
    # too few qualified: n - t + 1 dealers fall out for different reasons — status 9, the row is Q
    d = honest_dealers(secrets, t_new, everyone)
    faults, key_faults = {}, {}
    for i in range(n - t + 1):
        if i % 3 == 0:
            faults[(i, 0)] = "curve"
        elif i % 3 == 1:
            d[i] = (d[i][0], [(d[i][1][0] + 1) % R] + d[i][1][1:])
        else:
            key_faults[i] = "big"
    out.append(rs_case("too_few_qualified", secrets, d, t, t_new, key_faults=key_faults, faults=faults))
    return out


def all_rs_cases():
    return [((old, new), cs) for old, new in COMMITTEES for cs in rs_cases_for(old, new)]
