"""What the randomised verification of keyed aggregates over distinct messages must do, written from the header's rule alone
(include/bn254_hip.h: bn254_batch_aggregate_verify_distinct_keyed_randomized, bn254_debug_agg_rand_last / _sums) — no GPU, no library:
- r_model / model: the weights r_i and, from the oracle, the (group, key) bucket sums, S_g and the group verdicts;
- grouping: the counters of bn254_debug_agg_rand_last for a batch whose exact statuses are known;
- the batch PLANS of tests/test_gpu_aggregate_distinct_keyed_randomized_groups.py (sizes, key indices, what is wrong with which aggregate)
  and the conditions they must meet, so that a CPU-only run pins both before a device relies on them.
A helper module, not a test file."""
import hashlib
import random

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
LAMBDA = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd        # BN254_FLAG_RAND_GLV's eigenvalue (include/bn254_hip.h)


def r_model(seed, i, mode):
    """the header's r_i: SHA-256(seed32 || le64(i)) read little-endian, 16 bytes (RAND64: 8), 0 -> 1; GLV: k1 + k2 lambda mod r with k1, k2
    the two 64-bit halves"""
    d = hashlib.sha256(seed + i.to_bytes(8, "little")).digest()
    if mode == 2:
        k1, k2 = int.from_bytes(d[:8], "little"), int.from_bytes(d[8:16], "little")
        return (k1 or (0 if k2 else 1)) + k2 * LAMBDA
    r = int.from_bytes(d[:8 if mode == 1 else 16], "little")
    return r or 1


ORACLE_MAX_PAIRS = 16                                              # pairs one pairing_check of the oracle takes


def model(c, pks, hs, kidx, sigs, off, seed, mode, group_pairs, at_check=None, lo=None, sks=None):
    """the header's group rule from the oracle: per group the bucket sums of r_i H(m_j) by key, S_g = sum r_i sigma_i, and
    pairing_check over (non-empty key buckets, S_g) against (their keys, -G2).  at_check (default: everyone) leaves the other aggregates
    out; lo (default off[i]) gives the first message of each aggregate where the caller's offsets are not monotone.  A group with more
    pairs than one pairing_check of the oracle takes needs sks (32-byte secret keys, pks[k] = sks[k] G2): by bilinearity its product is
    e(sum_k sks[k] B_k - S_g, G2), which is one iff sum_k sks[k] B_k == S_g — the same condition, decided in G1."""
    K, m, n = len(pks), len(hs), len(sigs)
    G = max(group_pairs, K)
    ng = m // G + 1
    neg_g2 = c.g2_mul(c.g2_generator(), (R - 1).to_bytes(32, "big"))
    live = [True] * n if at_check is None else at_check
    lo = off if lo is None else lo
    nagg = [0] * ng
    for i in range(n):
        if live[i]:
            nagg[lo[i] // G] += 1
    sums, cnt = [bytes(64)] * (ng * (K + 1)), [0] * (ng * (K + 1))
    for i in range(n):
        if not live[i]:
            continue
        g = lo[i] // G
        r = 1 if nagg[g] == 1 else r_model(seed, i, mode) % R
        for j in range(off[i], off[i + 1]):
            if pks[kidx[j]] != bytes(128):
                b = g * (K + 1) + kidx[j]
                sums[b] = c.g1_add(sums[b], c.g1_mul(hs[j], r.to_bytes(32, "big")))
                cnt[b] += 1
        b = g * (K + 1) + K
        sums[b] = c.g1_add(sums[b], c.g1_mul(sigs[i], r.to_bytes(32, "big")))
    verdict, pairs = [], 0
    for g in range(ng):
        if not nagg[g]:
            verdict.append(255)
            continue
        keys = [k for k in range(K) if cnt[g * (K + 1) + k]]
        pairs += len(keys) + 1
        g1s = b"".join(sums[g * (K + 1) + k] for k in keys) + sums[g * (K + 1) + K]
        g2s = b"".join(pks[k] for k in keys) + neg_g2
        if len(keys) + 1 <= ORACLE_MAX_PAIRS:
            verdict.append(c.pairing_check(g1s, g2s, len(keys) + 1))
            continue
        acc = bytes(64)
        for k in keys:
            assert c.g2_mul(c.g2_generator(), sks[k]) == pks[k], k
            acc = c.g1_add(acc, c.g1_mul(sums[g * (K + 1) + k], sks[k]))
        verdict.append(0 if acc == sums[g * (K + 1) + K] else 9)
    return sums, verdict, pairs


def groups_of(sizes, at_check, K, group_pairs, lo=None):
    """{group: [its aggregates at the check]} — G = max(group_pairs, K), group of aggregate i = lo_i // G"""
    G = max(group_pairs, K)
    if lo is None:
        lo, pos = [], 0
        for k in sizes:
            lo.append(pos)
            pos += k
    out = {}
    for i in range(len(sizes)):
        if at_check[i]:
            out.setdefault(lo[i] // G, []).append(i)
    return out


def grouping(sizes, at_check, bad, key_idx, key_inf, K, group_pairs, lo=None):
    """the counters bn254_debug_agg_rand_last must report, from the header's rule: at_check[i] = the exact call gives aggregate i 0 or 9,
    bad[i] = it gives 9; key_idx = the flat key indices, key_inf[k] = registered key k is the identity.  Groups counted = those with an
    aggregate at the check; table pairs of such a group = the distinct non-identity keys of its aggregates at the check, + 1 for (S_g, -G2);
    failed = two or more at the check and a 9 among them; re-checked = the aggregates at the check of the failed groups."""
    if lo is None:
        lo, pos = [], 0
        for k in sizes:
            lo.append(pos)
            pos += k
    members = groups_of(sizes, at_check, K, group_pairs, lo)
    out = dict(groups=len(members), table_pairs=0, failed_groups=0, rechecked=0, single_groups=0)
    for g, agg in members.items():
        keys = {key_idx[j] for i in agg for j in range(lo[i], lo[i] + sizes[i])}
        out["table_pairs"] += len([k for k in keys if not key_inf[k]]) + 1
        if len(agg) == 1:
            out["single_groups"] += 1
        elif any(bad[i] for i in agg):
            out["failed_groups"] += 1
            out["rechecked"] += len(agg)
    return out


HOOK_FIELDS = ("groups", "table_pairs", "failed_groups", "rechecked", "single_groups")


def grouping_from_statuses(aggs, want, key_inf, group_pairs):
    """grouping() for a batch of (messages, sigma, key indices) whose exact statuses are `want`"""
    return grouping([len(a[0]) for a in aggs], [s in (0, 9) for s in want], [s == 9 for s in want], [x for a in aggs for x in a[2]], key_inf,
                    len(key_inf), group_pairs)


# ---- the batch plans of the GPU tests -------------------------------------------------------------------------------------------------------
# The key set of tests/test_gpu_aggregate_distinct_keyed.py: 64 good keys, then off the twist (4), outside the subgroup (4), a coordinate
# >= q (6), the identity.
N_GOOD, N_KEYS = 64, 68
KIDX_OFF_TWIST, KIDX_OFF_SUB, KIDX_BIG, KIDX_IDENT = 64, 65, 66, 67
KEY_INF = [False] * 67 + [True]
SIZES = [0, 1, 2, 3, 5, 8, 13, 21, 34, 55, 70, 130]
GROUP_PAIRS = (1, 200, 4096)


def _msg(tag, a, j):
    return hashlib.sha256(b"aggdr/groups/%s/%d/%d" % (tag.encode(), a, j)).digest() + b"/%d" % j


class Agg:
    """one planned aggregate: msgs and kidx as the call gets them; signed = [(message, key, multiplicity)] whose signatures sum to sigma;
    sig = what is then done to sigma (None, "plus_g", "plus_d", "minus_d", "off_curve", "big_x"); label = "ok" (exact status 0), "bad" (9)
    or "out" (not at the check: any other byte)"""

    def __init__(self, msgs, kidx, signed=None, sig=None, label="ok"):
        self.msgs, self.kidx, self.sig, self.label = list(msgs), list(kidx), sig, label
        self.signed = [(m, k, 1) for m, k in zip(msgs, kidx) if k < N_GOOD] if signed is None else signed


def plain(tag, a, k, t, n_ident=0):
    """k messages under keys (t + 7 j) % 64 (distinct for k <= 64) and n_ident more under the identity key, spread through the aggregate"""
    kidx = [(t + 7 * j) % N_GOOD for j in range(k)]
    for x in range(n_ident):
        kidx.insert((x * 3) % (len(kidx) + 1), KIDX_IDENT)
    return Agg([_msg(tag, a, j) for j in range(len(kidx))], kidx)


def ragged_plan(tag="ragged", reps=3, seed=7):
    """reps copies of SIZES and as many more of its six smallest (so that groups of 68 messages also hold several aggregates) in seeded
    shuffled order, all valid: every third non-empty aggregate carries identity-key pairs, the empty ones
    have sigma = O; two aggregates consist of identity-key pairs only (sigma = O)"""
    rnd = random.Random(seed)
    sizes = SIZES * reps + SIZES[:6] * reps
    rnd.shuffle(sizes)
    plan = []
    for a, k in enumerate(sizes):
        plan.append(plain(tag, a, k, rnd.randrange(N_GOOD), n_ident=(1 + a % 2) if k and a % 3 == 0 else 0))
    for x in range(2):
        plan.insert(rnd.randrange(len(plan)), plain(tag, 1000 + x, 0, 0, n_ident=2))
    return plan


def spoil(agg, how, rnd):
    """one aggregate of a valid plan made wrong: how = a key of OUT (leaves the check) or of BAD (fails it)"""
    a = Agg(agg.msgs, agg.kidx, agg.signed, agg.sig, agg.label)
    k = len(a.msgs)
    if how in ("off_curve", "big_x", "plus_g"):
        a.sig = how
    elif how == "swap":                                                  # two messages under different good keys change places
        x = [j for j in range(k) if a.kidx[j] < N_GOOD]
        assert len(x) >= 2 and a.kidx[x[0]] != a.kidx[x[1]]
        a.msgs[x[0]], a.msgs[x[1]] = a.msgs[x[1]], a.msgs[x[0]]
    elif how == "key":
        x = rnd.choice([j for j in range(k) if a.kidx[j] < N_GOOD])
        a.kidx[x] = (a.kidx[x] + 1) % N_GOOD
    else:
        a.kidx[rnd.randrange(k)] = {"off_twist": KIDX_OFF_TWIST, "off_sub": KIDX_OFF_SUB, "big_key": KIDX_BIG, "n_keys": N_KEYS,
                                    "all_ones": 0xFFFFFFFF}[how]
    a.label = "out" if how in OUT else "bad"
    return a


OUT = ("off_curve", "big_x", "off_twist", "off_sub", "big_key", "n_keys", "all_ones")
BAD = ("plus_g", "swap", "key")


def interleaved_plan(seed=11):
    """the ragged plan with a spoiled copy of an aggregate (every way of OUT in turn) put in front of two in three of its aggregates: these
    keep the exact call's byte and leave the check; everyone else still passes"""
    rnd = random.Random(seed)
    plan, x = [], 0
    for a, agg in enumerate(ragged_plan("inter", seed=seed)):
        if a % 3 != 2:
            how = OUT[x % len(OUT)]
            x += 1
            plan.append(spoil(plain("inter/out", a, 1 + a % 8, rnd.randrange(N_GOOD)), how, rnd))
        plan.append(agg)
    return plan


def failing_plan(group_pairs, seed=13):
    """the ragged plan with ONE aggregate spoiled (every way of BAD in turn) in every third group that has two or more aggregates"""
    rnd = random.Random(seed)
    plan = ragged_plan("fail", seed=seed)
    members = groups_of([len(a.msgs) for a in plan], [True] * len(plan), N_KEYS, group_pairs)
    x = 0
    for g in sorted(members)[::3]:
        cand = [i for i in members[g] if len([k for k in plan[i].kidx if k < N_GOOD]) >= 2]
        if len(members[g]) >= 2 and cand:
            plan[cand[0]] = spoil(plan[cand[0]], BAD[x % 3], rnd)
            x += 1
    assert x >= min(2, len([g for g in members if len(members[g]) >= 2]))
    return plan


def cancelling_plan(group_pairs, seed=17):
    """sigma_a + D and sigma_b - D in two DIFFERENT groups of two or more: both groups fail"""
    plan = ragged_plan("cancel", seed=seed)
    members = groups_of([len(a.msgs) for a in plan], [True] * len(plan), N_KEYS, group_pairs)
    multi = [g for g in sorted(members) if len(members[g]) >= 2]
    assert len(multi) >= 2
    for g, how in ((multi[0], "plus_d"), (multi[-1], "minus_d")):
        i = members[g][-1]
        plan[i].sig, plan[i].label = how, "bad"
    return plan


def edges_plan(G):
    """for groups of G messages: aggregates whose lo is an exact multiple of G; one longer than 2 G, so that the groups it covers hold nobody;
    a group of identity-key aggregates with sigma = O only (S_g = O, no key bucket); m an exact multiple of G with trailing empty aggregates
    at lo == m, which form the last group by themselves (table pairs = 1)"""
    plan, t = [], 0

    def add(k, n_ident=0):
        nonlocal t
        plan.append(plain("edges%d" % G, len(plan), k, t, n_ident))
        t += 5

    add(G - 3), add(3)                                                   # group 0, full to its end
    add(2), add(0), add(2 * G + 5)                                       # group 1: lo = G exactly, an empty one, the long one to 3 G + 7
    add(G - 9), add(1), add(1)                                           # group 3 (group 2 holds nobody), ends at 4 G
    add(0, n_ident=G // 2), add(0, n_ident=G - G // 2)                   # group 4: identity keys only
    add(G - 1), add(1)                                                   # group 5 ... m = 6 G
    add(0), add(0), add(0)                                               # group 6: lo == m
    return plan


def repeated_plan(cs, neighbour, G=N_KEYS, seed=19):
    """per c in cs one aggregate that names the same (message, key) c times (sigma = c signatures), alone at the check in its group of G
    messages when neighbour is false (r = 1), else behind a small valid aggregate (both weighted); an aggregate that is not at the check
    (a key index outside the set) fills each group up to the next multiple of G"""
    rnd = random.Random(seed)
    plan, pos = [], 0
    for a, cc in enumerate(cs):
        if neighbour:
            plan.append(plain("rep/nb", a, 2, rnd.randrange(N_GOOD)))
        m, k = _msg("rep", a, 0), rnd.randrange(N_GOOD)
        plan.append(Agg([m] * cc, [k] * cc, signed=[(m, k, cc)]))
        pos += cc + (2 if neighbour else 0)
        if pos % G:
            plan.append(spoil(plain("rep/fill", a, G - pos % G, rnd.randrange(N_GOOD)), "n_keys", rnd))
            pos += G - pos % G
    return plan


RUN_LENGTHS = [256, 1, 255, 512, 257, 255, 511, 1, 513, 255, 255, 257, 512]     # per key 0, 1, ... of ONE group, in key order


def run_starts(lengths, wg):
    """(offset in its workgroup, length) of every sorted run of k_aggr_sum's level 0: buckets lie in key order"""
    out, pos = [], 0
    for n in lengths:
        out.append((pos % wg, n))
        pos += n
    return out


def runs_plan(seed=23, n_agg=160):
    """one group whose key k is named RUN_LENGTHS[k] times, the entries dealt to n_agg aggregates in shuffled order"""
    rnd = random.Random(seed)
    keys = [k for k, n in enumerate(RUN_LENGTHS) for _ in range(n)]
    rnd.shuffle(keys)
    cut = sorted(rnd.sample(range(1, len(keys)), n_agg - 1))
    plan = []
    for a, (lo, hi) in enumerate(zip([0] + cut, cut + [len(keys)])):
        plan.append(Agg([_msg("runs", a, j) for j in range(hi - lo)], keys[lo:hi]))
    return plan


def check_runs(wg):
    """the run-boundary plan meets k_aggr_sum's edges for workgroups of wg elements (AGGR_SUM_WG)"""
    runs = run_starts(RUN_LENGTHS, wg)
    assert {n for _, n in runs} >= {1, wg - 1, wg, wg + 1, 2 * wg - 1, 2 * wg, 2 * wg + 1}
    assert {o for o, _ in runs} >= {0, 1, wg - 1}
    assert (0, wg) in runs and (0, 2 * wg) in runs                        # a run that is a workgroup, a run that is two
    assert any(o != 0 and o + n == wg for o, n in runs)                   # a run that starts inside a workgroup and ends with it
    assert any(o == 0 and n >= wg for o, n in runs)                       # a workgroup whose first run also reaches its end
    assert sum(RUN_LENGTHS) < 4096                                        # one group at GROUP_PAIRS = 4096


def labels(plan, hash_failed=None):
    """(at_check, bad) of a plan; hash_failed(message) -> bool takes the aggregates with such a message off the check"""
    at = [a.label != "out" and not (hash_failed and any(hash_failed(m) for m in a.msgs)) for a in plan]
    return at, [a.label == "bad" and at[i] for i, a in enumerate(plan)]


def plan_grouping(plan, group_pairs, key_inf=KEY_INF, hash_failed=None, reject_identity=False):
    at, bad = labels(plan, hash_failed)
    if reject_identity:
        at = [x and KIDX_IDENT not in a.kidx for x, a in zip(at, plan)]
        bad = [b and x for b, x in zip(bad, at)]
    return grouping([len(a.msgs) for a in plan], at, bad, [k for a in plan for k in a.kidx], key_inf, N_KEYS, group_pairs)


def check_passing(plan, group_pairs, interleaved=False, **kw):
    """the conditions a 'passing' batch must meet before the device sees it: at least half of the counted groups have two or more
    aggregates at the check; interleaved: at least a quarter of all aggregates are not at the check and at least a quarter of the passing
    groups contain one"""
    at, bad = labels(plan, kw.get("hash_failed"))
    if kw.get("reject_identity"):
        at = [x and KIDX_IDENT not in a.kidx for x, a in zip(at, plan)]
    assert not any(b and x for b, x in zip(bad, at))
    sizes = [len(a.msgs) for a in plan]
    members = groups_of(sizes, at, N_KEYS, group_pairs)
    multi = [g for g, agg in members.items() if len(agg) >= 2]
    assert 2 * len(multi) >= len(members) and multi, (group_pairs, len(multi), len(members))
    if interleaved:
        assert 4 * at.count(False) >= len(plan), (at.count(False), len(plan))
        everyone = groups_of(sizes, [True] * len(plan), N_KEYS, group_pairs)
        with_out = [g for g in members if any(not at[i] for i in everyone[g])]
        assert 4 * len(with_out) >= len(members), (group_pairs, len(with_out), len(members))
    return members
