"""The groups of bn254_batch_aggregate_verify_distinct_keyed_randomized that PASS, on the GPU.  A group of two or more aggregates whose
combined check passes is the one place where the library answers 0 without an exact pairing check, and a wrong G1 side (scaling, counting
sort, segmented sums, table pairs, S_g) only makes a group fail and fall back to the exact re-check: the status bytes stay right.  So every
case here compares, besides the status bytes with the exact keyed call's, the counters of bn254_debug_agg_rand_last field by field with
tests/aggr_model.py's grouping() — a batch that should pass has failed_groups == 0 and rechecked == 0 — and the bucket sums, S_g and
verdicts of bn254_debug_agg_rand_sums byte for byte with model() (oracle g1_mul / g1_add / pairing_check, hashlib for r_i).  The batches
are the plans of tests/aggr_model.py; the conditions they must meet are asserted before the device is called (and, without a GPU, by
tests/test_aggregate_distinct_keyed_randomized.py).  Run on the MI355X box: -m gpu."""
import pytest

from bn254_amd import engine as E
from tests import aggr_model as AM
from tests.conftest import ws_default
from tests.test_gpu_aggregate_distinct_keyed import c, eng, keyed, keyset, reg_set  # noqa: F401
from tests.test_gpu_aggregate_distinct_keyed_randomized import MODES, SEEDS, diff, rand

pytestmark = pytest.mark.gpu

R = AM.R
BIG = 1 << 20


@pytest.fixture(autouse=True)
def randomised(eng, keyset):  # noqa: F811
    reg_set(eng, keyset)
    eng.set_option(E.OPT_AGG_RAND_MIN_PAIRS, 0)
    yield
    eng.set_option(E.OPT_AGG_RAND_MIN_PAIRS, ws_default("AGG_RAND_MIN_PAIRS_DEFAULT"))
    eng.set_option(E.OPT_AGG_RAND_GROUP_PAIRS, ws_default("AGG_RAND_GROUP_PAIRS_DEFAULT"))
    eng.set_option(E.OPT_HASH_MAX_TRIES, 0)
    reg_set(eng, keyset)


def materialise(eng, c, keyset, plan):  # noqa: F811
    """(messages, sigma, key indices) per planned aggregate: every distinct (message, key) signed once on the device, sigma = the sum of
    multiplicity x signature, then what the plan does to sigma"""
    sks = keyset[0]
    pairs = sorted({(m, k) for a in plan for m, k, _ in a.signed})
    sig = {}
    if pairs:
        out, st = eng.batch_sign([m for m, _ in pairs], b"".join(sks[k] for _, k in pairs))
        assert st == bytes(len(pairs))
        sig = {p: out[64 * i:64 * i + 64] for i, p in enumerate(pairs)}
    g1 = c.g1_generator()
    d, minus_d = c.g1_mul(g1, (12345).to_bytes(32, "big")), c.g1_mul(g1, (R - 12345).to_bytes(32, "big"))
    parts, off = [], [0]
    for a in plan:
        parts += [sig[(m, k)] if n == 1 else c.g1_mul(sig[(m, k)], n.to_bytes(32, "big")) for m, k, n in a.signed]
        off.append(len(parts))
    import ctypes
    nonempty = [i for i in range(len(plan)) if off[i + 1] > off[i]]
    sums = {}
    if nonempty:
        out, st = eng.batch_g1_sum(b"".join(parts), (ctypes.c_uint64 * (len(nonempty) + 1))(*([off[i] for i in nonempty] + [off[nonempty[-1] + 1]])))
        assert st == bytes(len(nonempty))
        sums = {i: out[64 * x:64 * x + 64] for x, i in enumerate(nonempty)}
    aggs = []
    for i, a in enumerate(plan):
        s = sums.get(i, bytes(64))
        if a.sig == "plus_g":
            s = c.g1_add(s, g1)
        elif a.sig == "plus_d":
            s = c.g1_add(s, d)
        elif a.sig == "minus_d":
            s = c.g1_add(s, minus_d)
        elif a.sig == "off_curve":
            s = bytearray(s); s[40] ^= 4; s = bytes(s)
        elif a.sig == "big_x":
            s = b"\xff" + s[1:]
        else:
            assert a.sig is None
        aggs.append((a.msgs, s, a.kidx))
    return aggs


def the_hook(eng):  # noqa: F811
    h = eng.debug_agg_rand_last()
    assert h["ran"] == 1, h
    return {k: h[k] for k in AM.HOOK_FIELDS}


_hash = {}


class MemoOracle:
    """the oracle with g1_mul remembered: the same r_i H(m_j) is asked for again for every group size (the model is run as it stands)"""

    def __init__(self, c):  # noqa: F811
        self._c, self._mul = c, {}

    def __getattr__(self, name):
        return getattr(self._c, name)

    def g1_mul(self, p, k):
        if (p, k) not in self._mul:
            self._mul[(p, k)] = self._c.g1_mul(p, k)
        return self._mul[(p, k)]


_memo = []


def hashes(c, msgs):  # noqa: F811
    out = []
    for m in msgs:
        if m not in _hash:
            st, h, _ = c.hash_to_g1(m)
            assert st == 0
            _hash[m] = h
        out.append(_hash[m])
    return out


def check_sums(eng, c, keyset, aggs, want, seed, mode, gp):  # noqa: F811
    """bn254_debug_agg_rand_sums after a randomised call against model(): per group the aggregates at the check, S_g, the table pairs in
    ascending key order with their bucket sums, and the verdict of the group's check"""
    pks = keyset[1]
    K = len(pks)
    off = [0]
    for a in aggs:
        off.append(off[-1] + len(a[0]))
    at = [s in (0, 9) for s in want]
    kidx = [x for a in aggs for x in a[2]]
    hs = hashes(c, [m for a, live in zip(aggs, at) for m in (a[0] if live else [b""] * len(a[0]))])    # only live aggregates' points are read
    if not _memo or _memo[0][0] is not aggs:                            # one memory per batch
        _memo[:] = [(aggs, MemoOracle(c))]
    sums, verdict, pairs = AM.model(_memo[0][1], pks, hs, kidx, [a[1] for a in aggs], off, seed, mode, gp, at_check=at, sks=keyset[0])
    got = eng.debug_agg_rand_sums()
    assert len(got) == len(verdict) and sum(len(g["pairs"]) + 1 for g in got if g["nagg"]) == pairs
    members = AM.groups_of([len(a[0]) for a in aggs], at, K, gp)
    for g, dev in enumerate(got):
        assert dev["nagg"] == len(members.get(g, [])), g
        keys = [k for k, _ in dev["pairs"]]
        assert keys == sorted(set(keys)), (g, keys)                     # ascending key order, as the scan of the bucket counts lays them
        want_keys = [k for k in range(K) if sums[g * (K + 1) + k] != bytes(64)]
        assert keys == want_keys, (g, keys, want_keys)
        for k, p in dev["pairs"]:
            assert p == sums[g * (K + 1) + k], (g, k)
        assert dev["s"] == sums[g * (K + 1) + K], g
        if dev["nagg"]:
            assert dev["verdict"] == verdict[g], (g, dev["verdict"], verdict[g])


def run(eng, c, keyset, plan, gps, flags=0, seeds=SEEDS, sums_for=(), passing=True, hash_tries=0, **plan_kw):  # noqa: F811
    """statuses == the exact keyed call's == the plan's labels; the hook == grouping() from those statuses == the plan's own prediction;
    for the group sizes in sums_for also the bucket sums (first seed).  Returns the exact statuses."""
    aggs = materialise(eng, c, keyset, plan)
    eng.set_option(E.OPT_HASH_MAX_TRIES, hash_tries)                    # after the signing, which hashes too
    want = keyed(eng, aggs, flags)
    at, bad = AM.labels(plan, plan_kw.get("hash_failed"))
    if plan_kw.get("reject_identity"):
        at = [x and AM.KIDX_IDENT not in a.kidx for x, a in zip(at, plan)]
    for i, s in enumerate(want):
        assert (s in (0, 9)) == at[i] and (s == 9) == (bad[i] and at[i]), (i, s, plan[i].label, plan[i].sig)
    key_inf = AM.KEY_INF
    for gp in gps:
        w = AM.grouping_from_statuses(aggs, want, key_inf, gp)
        assert w == AM.plan_grouping(plan, gp, **plan_kw)
        if passing:
            assert w["failed_groups"] == 0 and w["rechecked"] == 0 and w["groups"] > w["single_groups"], w
        eng.set_option(E.OPT_AGG_RAND_GROUP_PAIRS, gp)
        for seed in seeds:
            for mode, (name, mf) in enumerate(MODES):
                got = rand(eng, aggs, seed, flags | mf)
                assert got == want, (gp, name, diff(got, want))
                h = the_hook(eng)
                assert h == w, (gp, name, h, w)
                if gp in sums_for and seed == seeds[0]:
                    check_sums(eng, c, keyset, aggs, want, seed, mode, gp)
    return want


def test_ragged_groups_pass_without_a_recheck(eng, c, keyset):  # noqa: F811
    """sizes 0 .. 130 shuffled, identity-key pairs, empty aggregates with sigma = O, aggregates of identity keys only: every group passes
    its combined check — no failed group, nothing re-checked — with groups of 68, 200 and 4 096 messages"""
    plan = AM.ragged_plan()
    for gp in AM.GROUP_PAIRS:
        AM.check_passing(plan, gp)
    want = run(eng, c, keyset, plan, AM.GROUP_PAIRS)
    assert want == bytes(len(plan))


def test_members_off_the_check_leave_their_groups_passing(eng, c, keyset):  # noqa: F811
    """the same with aggregates that are not at the check in between (sigma off the curve / a coordinate >= q; refused keys; key indices
    n_keys and 0xFFFFFFFF): they keep the exact call's byte, add nothing to any sum, and the groups around them still pass.  The bucket
    sums, S_g and verdicts against the oracle.  With REJECT_IDENTITY at registration the identity-key aggregates leave the check too"""
    plan = AM.interleaved_plan()
    for gp in AM.GROUP_PAIRS:
        AM.check_passing(plan, gp, interleaved=True)
        AM.check_passing(plan, gp, interleaved=True, reject_identity=True)
    want = run(eng, c, keyset, plan, AM.GROUP_PAIRS, sums_for=AM.GROUP_PAIRS)
    assert {2, 4, 6} <= set(want) and 9 not in want
    assert reg_set(eng, keyset, flags=2)[AM.KIDX_IDENT] == 4
    want = run(eng, c, keyset, plan, AM.GROUP_PAIRS, reject_identity=True)
    assert want.count(4) >= len([a for a in plan if a.label == "ok" and AM.KIDX_IDENT in a.kidx]) > 0


def test_hash_failures_leave_their_groups_passing(eng, c, keyset):  # noqa: F811
    """OPT_HASH_MAX_TRIES = 3: an aggregate with a message that finds no point in three tries gets the exact call's byte and leaves the
    check; what stays at the check still passes in groups"""
    plan = AM.interleaved_plan()
    tries = {}

    def hash_failed(m):
        if m not in tries:
            tries[m] = c.hash_to_g1(m)[2]
        return tries[m] > 3
    at, _ = AM.labels(plan, hash_failed)
    assert at.count(True) >= 8 and at.count(False) > [a.label for a in plan].count("out")
    w = AM.plan_grouping(plan, 4096, hash_failed=hash_failed)
    assert w["groups"] == 1 and w["single_groups"] == 0
    run(eng, c, keyset, plan, (1, 4096), passing=False, hash_tries=3, hash_failed=hash_failed)
    assert the_hook(eng)["failed_groups"] == 0 and the_hook(eng)["rechecked"] == 0


def assert_failed_groups(eng, plan, gp):  # noqa: F811
    """the verdict bytes of the last call: 9 for exactly the groups that hold a planned wrong aggregate"""
    members = AM.groups_of([len(a.msgs) for a in plan], [a.label != "out" for a in plan], AM.N_KEYS, gp)
    planned = sorted(g for g, agg in members.items() if any(plan[i].label == "bad" for i in agg))
    got = eng.debug_agg_rand_sums()
    assert sorted(g for g, dev in enumerate(got) if dev["nagg"] and dev["verdict"] == 9) == planned, (gp, planned)
    assert all(dev["verdict"] == 0 for g, dev in enumerate(got) if dev["nagg"] and g not in planned)


def test_localised_failures(eng, c, keyset):  # noqa: F811
    """one wrong aggregate (sigma + G1, two messages swapped, a key index changed) in every third group: exactly those groups fail and
    only their members are re-checked; sigma_a + D and sigma_b - D in two different groups fail both"""
    for gp in AM.GROUP_PAIRS:
        plan = AM.failing_plan(gp)
        w = AM.plan_grouping(plan, gp)
        assert w["failed_groups"] >= 1 and w["rechecked"] < len(plan) or gp == 4096
        want = run(eng, c, keyset, plan, (gp,), passing=False, sums_for=(200,))     # at 200: the sums survive the re-check of the failed groups
        assert want.count(9) == w["failed_groups"] == [a.label for a in plan].count("bad")
        assert_failed_groups(eng, plan, gp)
    for gp in (1, 200):
        plan = AM.cancelling_plan(gp)
        assert AM.plan_grouping(plan, gp)["failed_groups"] == 2
        assert run(eng, c, keyset, plan, (gp,), passing=False).count(9) == 2
        assert_failed_groups(eng, plan, gp)


def test_group_edges(eng, c, keyset):  # noqa: F811
    """lo an exact multiple of G; an aggregate longer than 2 G (the groups it covers hold nobody); m an exact multiple of G; trailing empty
    aggregates at lo == m as a group of their own; a group of identity-key aggregates with sigma = O (S_g = O, no key bucket)"""
    for G in (AM.N_KEYS, 200):
        plan = AM.edges_plan(G)
        AM.check_passing(plan, G)
        want = run(eng, c, keyset, plan, (G,), sums_for=(G,))
        assert want == bytes(len(plan))
        sums = eng.debug_agg_rand_sums()
        assert [g["nagg"] for g in sums] == [2, 3, 0, 3, 2, 2, 3]
        assert sums[4]["pairs"] == [] and sums[4]["s"] == bytes(64) and sums[6]["pairs"] == [] and sums[6]["s"] == bytes(64)
        assert sums[2]["pairs"] == [] and sums[2]["s"] == bytes(64)


REPEATS = [2, 3, 4, 255, 256, 257, 513]


def test_repeated_message_and_key_inside_an_aggregate(eng, c, keyset):  # noqa: F811
    """an aggregate that names one (message, key) c times: its entries are EQUAL points of one bucket, so the sum tree adds P + P at every
    round (and equal partials across workgroups); alone in its group (r = 1) and beside a neighbour (weighted).  0, no failed group, the
    bucket sums against the oracle; one copy's key index changed -> 9"""
    for nb in (False, True):
        plan = AM.repeated_plan(REPEATS, nb)
        w = AM.plan_grouping(plan, 1)
        assert w["groups"] == len(REPEATS) and w["single_groups"] == (0 if nb else len(REPEATS)) and w["failed_groups"] == 0
        want = run(eng, c, keyset, plan, (1,), sums_for=(1,), passing=nb)
        assert want.count(0) == len(REPEATS) * (2 if nb else 1) and 9 not in want
        if nb:                                                          # groups of 200 / 4 096: the repeated aggregates share groups, all weighted
            for gp in (200, 4096):
                AM.check_passing(plan, gp)
            run(eng, c, keyset, plan, (200, 4096), sums_for=(200, 4096))
        assert the_hook(eng)["failed_groups"] == 0 and the_hook(eng)["rechecked"] == 0
        for a in plan:
            if len(a.msgs) in (256, 513) and a.label == "ok":
                a.kidx[len(a.msgs) // 2] = (a.kidx[0] + 1) % AM.N_GOOD
                a.label = "bad"
        want = run(eng, c, keyset, plan, (1,), passing=False)
        assert want.count(9) == 2


def test_equal_partials_on_every_level(eng, c, keyset):  # noqa: F811
    """one aggregate of 2^17 + 1 copies of one (message, key) beside a small neighbour: three levels of the segmented sums, equal partial
    sums meet on each.  0 and no failed group; one copy's key index changed -> 9"""
    wg = ws_default("AGGR_SUM_WG")
    cc = (1 << 17) + 1
    assert cc + 2 + 2 > 2 * wg * wg                                      # entries = messages + aggregates: three levels
    m, k = AM._msg("rep/big", 0, 0), 9
    plan = [AM.plain("rep/big/nb", 0, 2, 5), AM.Agg([m] * cc, [k] * cc, signed=[(m, k, cc)])]
    assert AM.plan_grouping(plan, BIG) == dict(groups=1, table_pairs=len({k for a in plan for k in a.kidx}) + 1, failed_groups=0, rechecked=0,
                                               single_groups=0)
    assert run(eng, c, keyset, plan, (BIG,)) == bytes(2)
    plan[1].kidx[cc - 3] = (plan[1].kidx[0] + 1) % AM.N_GOOD
    plan[1].label = "bad"
    assert run(eng, c, keyset, plan, (BIG,), passing=False) == bytes([0, 9])


def test_bucket_run_boundaries(eng, c, keyset):  # noqa: F811
    """one group whose sorted bucket runs have lengths 1, 255, 256, 257, 511, 512, 513 and start at offsets 0, 1, 255 of a workgroup of the
    segmented sums: a run that is a workgroup, one that is two, one that ends with its workgroup.  The group passes; the sums against the
    oracle (also split into groups of 68 and 200)"""
    AM.check_runs(ws_default("AGGR_SUM_WG"))
    plan = AM.runs_plan()
    assert AM.plan_grouping(plan, 4096) == dict(groups=1, table_pairs=len(AM.RUN_LENGTHS) + 1, failed_groups=0, rechecked=0, single_groups=0)
    for gp in AM.GROUP_PAIRS:
        AM.check_passing(plan, gp)
    want = run(eng, c, keyset, plan, (4096, 200, 1), sums_for=(4096, 200, 1))
    assert want == bytes(len(plan))


def test_device_form_with_reversed_and_overlapping_members(eng, c, keyset):  # noqa: F811
    """the _device form: after every fourth aggregate agg_off steps back by one, so that one member is reversed and the next overlaps its
    predecessor (both 2, as the exact _device call says; the messages of the overlapping one belong to nobody).  The valid members around
    them still pass in groups: statuses, the counters with lo_i = agg_off[i], and the sums, S_g and verdicts against the oracle"""
    from tests.hip_ctypes import DevBuf, Stream
    from bn254_amd.engine import pack_messages
    plan = AM.ragged_plan("dev")
    aggs = materialise(eng, c, keyset, plan)
    off = [0]
    for a in aggs:
        off.append(off[-1] + len(a[0]))
    m = off[-1]
    A, sigmas, out = [0], [], []                                        # agg_off, one sigma per member, the members that must get 2
    for i, a in enumerate(aggs):
        if i % 4 == 3 and len(a[0]) and off[i] >= 1:
            sigmas.append(bytes(64))                                    # [off_i, off_i - 1): reversed
            A.append(off[i] - 1)
            out += [len(sigmas) - 1, len(sigmas)]                       # ... and [off_i - 1, off_i+1) starts before its predecessor's end
        sigmas.append(a[1])
        A.append(off[i + 1])
    n = len(sigmas)
    assert A[-1] == m and len(A) == n + 1 and len(out) >= 8
    lo = A[:-1]
    sizes = [max(0, A[i + 1] - A[i]) for i in range(n)]
    msgs, kidx = [x for a in aggs for x in a[0]], [x for a in aggs for x in a[2]]
    blob, moff = pack_messages(msgs)
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    st_dev, bufs = Stream(), []
    try:
        def dev(data):
            b = DevBuf(len(data), data=data)
            bufs.append(b)
            return b
        d_msgs, d_off, d_sigs, d_idx, d_agg = dev(blob), dev(u64(moff)), dev(b"".join(sigmas)), dev(u32(kidx)), dev(u64(A))
        d_st = DevBuf(n, fill=0xEE)
        bufs.append(d_st)
        eng.batch_aggregate_verify_distinct_keyed_device(d_msgs.ptr, d_off.ptr, d_idx.ptr, m, d_sigs.ptr, d_agg.ptr, n, d_st.ptr, stream=st_dev.handle)
        st_dev.synchronize()
        want = bytes(d_st.download(n))
        assert [i for i in range(n) if want[i] == 2] == out and set(want) == {0, 2}, want
        at = [s == 0 for s in want]
        hs = hashes(c, msgs)
        for gp in (1, 200):
            w = AM.grouping(sizes, at, [False] * n, kidx, AM.KEY_INF, AM.N_KEYS, gp, lo=lo)
            members = AM.groups_of(sizes, at, AM.N_KEYS, gp, lo=lo)
            everyone = AM.groups_of(sizes, [True] * n, AM.N_KEYS, gp, lo=lo)
            multi = [g for g in members if len(members[g]) >= 2]
            assert 2 * len(multi) >= len(members) and any(not at[i] for g in multi for i in everyone[g])
            assert w["failed_groups"] == 0 and w["rechecked"] == 0
            eng.set_option(E.OPT_AGG_RAND_GROUP_PAIRS, gp)
            for seed in SEEDS:
                for mode, (name, mf) in enumerate(MODES):
                    eng.batch_aggregate_verify_distinct_keyed_randomized_device(d_msgs.ptr, d_off.ptr, d_idx.ptr, m, d_sigs.ptr, d_agg.ptr, n, seed, d_st.ptr,
                                                                                 flags=mf, stream=st_dev.handle)
                    st_dev.synchronize()
                    got = bytes(d_st.download(n))
                    assert got == want, (gp, name, diff(got, want))
                    assert the_hook(eng) == w, (gp, name, the_hook(eng), w)
                    if seed == SEEDS[0]:
                        sums, verdict, pairs = AM.model(c, keyset[1], hs, kidx, sigmas, A, seed, mode, gp, at_check=at, lo=lo, sks=keyset[0])
                        dev_sums = eng.debug_agg_rand_sums()
                        K = AM.N_KEYS
                        assert len(dev_sums) == len(verdict) and pairs == w["table_pairs"]
                        for g, d in enumerate(dev_sums):
                            assert d["nagg"] == len(members.get(g, [])), g
                            assert d["pairs"] == [(k, sums[g * (K + 1) + k]) for k in range(K) if sums[g * (K + 1) + k] != bytes(64)], g
                            assert d["s"] == sums[g * (K + 1) + K] and (not d["nagg"] or d["verdict"] == verdict[g] == 0), g
    finally:
        st_dev.synchronize()
        for b in bufs:
            b.free()
        st_dev.destroy()
