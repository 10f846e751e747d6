"""bn254_batch_collect_keyed_bitmap_optimistic[_device] on the GPU (include/bn254_hip.h): every comparison against
bn254_batch_collect_keyed_bitmap on the same context and against tests/collect_opt_model.py over the oracle; what the route did, as
bn254_debug_collect_opt_last counts it.  The routes are forced with options 40 = 0 and 41 = 0 unless said otherwise, and restored.
The key set has 40 keys (five whole windows of the subset tables, a word and a quarter of a bitmap row; test_set_of_43_keys adds three, so
that the last window and the last word are both partial): 36 good ones, one off the twist (registration status 4), the identity, key 0
AGAIN and the NEGATION of key 1.  Ten tuples of 0 .. 130 shares: a tuple's candidates name distinct keys (39 keys can sign), so the longer tuples are filled up with shares that
name indices outside the set (status 2 by rule 2, not candidates) between the candidates — both strides of the wave layout hold candidates.
Run on the MI355X box: -m gpu."""
import os
import re
import subprocess

import pytest

from bn254_amd import engine as E
from tests import collect_model
from tests import collect_opt_model as M
from tests.datagen import D, sk_bytes
from tests.test_gpu_collect_keyed_bitmap import collect, derive, flat, sign

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R
N_GOOD = 36
K_BAD, K_IDENT, K_DUP0, K_NEG1 = range(N_GOOD, N_GOOD + 4)
N_KEYS = N_GOOD + 4
SIGNABLE = list(range(N_GOOD)) + [K_IDENT, K_DUP0, K_NEG1]
BM = 2
SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130]
FORCE = {E.OPT_COLLECT_OPT_MIN_SHARES: 0, E.OPT_COLLECT_OPT_MIN_TUPLE_SHARES: 0}


def ws_default(name):
    text = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


DEFAULTS = {E.OPT_COLLECT_OPT_MIN_SHARES: E.COLLECT_OPT_MIN_SHARES_DEFAULT, E.OPT_COLLECT_OPT_MIN_TUPLE_SHARES: E.COLLECT_OPT_MIN_TUPLE_SHARES_DEFAULT,
            E.OPT_MAX_CHUNK: 0, E.OPT_COLLECT_WAVE_MIN_SHARES: ws_default("COLLECT_WAVE_MIN_SHARES_DEFAULT"),
            E.OPT_TRIO_MAX_BATCH: ws_default("TRIO_MAX_BATCH_DEFAULT"), E.OPT_NONET_MAX_BATCH: ws_default("NONET_MAX_BATCH_DEFAULT"),
            E.OPT_LM_MAX_BATCH: ws_default("LM_MAX_BATCH_DEFAULT")}
SMALL_OFF = {E.OPT_TRIO_MAX_BATCH: 0, E.OPT_NONET_MAX_BATCH: 0, E.OPT_LM_MAX_BATCH: 0}


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


@pytest.fixture(scope="module")
def keyset(eng):
    """-> (secret keys as integers, 0 where nobody can sign; encodings; registration statuses)"""
    assert (E.OPT_TRIO_MAX_BATCH, E.OPT_NONET_MAX_BATCH, E.OPT_LM_MAX_BATCH) == (6, 13, 15)
    sks = [int.from_bytes(sk_bytes(900 + j), "big") % R for j in range(N_GOOD)]
    pks = derive(eng, sks)
    off_twist = bytearray(pks[3]); off_twist[100] ^= 2
    pks += [bytes(off_twist), bytes(128), pks[0], derive(eng, [R - sks[1]])[0]]
    sks += [0, 0, sks[0], R - sks[1]]
    reg = list(eng.register_keys(b"".join(pks)))
    assert reg == [0] * N_GOOD + [4, 0, 0, 0] and N_KEYS % 32
    return sks, pks, reg


def reg_set(eng, keyset):
    assert list(eng.register_keys(b"".join(keyset[1]))) == keyset[2]


def with_options(eng, opts, fn):
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            eng.set_option(k, DEFAULTS[k])


def plan_valid(sizes=SIZES):
    """per tuple [(key, kind)]: candidates ("ok") of distinct signable keys at every step-th position, fillers (a valid signature naming an
    index outside the set) between them"""
    out = []
    for i, k in enumerate(sizes):
        step = (k + len(SIGNABLE) - 1) // len(SIGNABLE) or 1
        out.append([(SIGNABLE[(j // step + 3 * i) % len(SIGNABLE)], "ok") if j % step == 0 else (N_KEYS + j, "filler") for j in range(k)])
    return out


def materialise(eng, c, keyset, tag, plan):
    """kinds: ok; filler; wrong (a valid signature of ANOTHER message by the key); big (a coordinate >= q); curve (off the curve); nkeys (a
    valid share naming index n_keys); badkey (naming the status-4 key); plus (sigma + G1); minus (sigma - G1)"""
    sks = keyset[0]
    msgs = [D("collect-opt/%s" % tag, i) for i in range(len(plan))]
    other = D("collect-opt/%s/other" % tag, 0)
    want = [(other if kind == "wrong" else msgs[i], sks[key] if key < N_KEYS and sks[key] else sks[0]) for i, t in enumerate(plan) for key, kind in t]
    sigs = iter(sign(eng, want)) if want else iter(())
    g1 = c.g1_generator()
    neg_g1 = c.g1_mul(g1, (R - 1).to_bytes(32, "big"))
    tuples = []
    for i, t in enumerate(plan):
        rows = []
        for key, kind in t:
            sg = next(sigs)
            if key == K_IDENT and kind in ("ok", "wrong"):
                sg = bytes(64) if kind == "ok" else g1
            if kind == "big":
                sg = b"\xFF" + sg[1:]
            elif kind == "curve":
                sg = bytearray(sg); sg[40] ^= 4; sg = bytes(sg)
            elif kind == "nkeys":
                key = N_KEYS
            elif kind == "badkey":
                key = K_BAD
            elif kind == "plus":
                sg = c.g1_add(sg, g1)
            elif kind == "minus":
                sg = c.g1_add(sg, neg_g1)
            rows.append((sg, key))
        tuples.append((msgs[i], rows))
    return tuples


def opt(eng, tuples, flags=0, bm_words=BM, opts=None):
    """-> (the five outputs, the hook's counters) with the route forced, plus opts"""
    o = dict(FORCE)
    o.update(opts or {})
    msgs, shares, keys, sizes = flat(tuples)

    def call():
        out = eng.batch_collect_keyed_bitmap_optimistic(msgs, b"".join(shares), keys, sizes, bm_words, flags=flags, want_counts=True)
        return out, eng.debug_collect_opt_last()
    return with_options(eng, o, call)


def model(c, keyset, tuples, bm_words=BM, min_tuple=0, flags=0):
    """-> ((share_status, tuple_status, agg, bits, counts) as the engine returns them, hook) by tests/collect_opt_model.py over the oracle"""
    msgs, shares, keys, sizes = flat(tuples)
    pre = M.precheck([c.g1_validate(s, flags) for s in shares], keys, keyset[2], sizes, [0] * len(sizes))
    tuple_check, share_check = M.oracle_checks(c, msgs, shares, keys, sizes, keyset[1])
    out = M.collect(keys, pre, sizes, [0] * len(sizes), bm_words, min_tuple, tuple_check, share_check)
    agg = b"".join(collect_model.aggregates(c, shares, out["chosen"]))
    return (bytes(out["share_status"]), bytes(len(sizes)), agg, [w for r in out["rows"] for w in r], out["counts"]), out["hook"]


def candidates(tuples, reg, i):
    return sum(1 for _, key in tuples[i][1] if key < N_KEYS and reg[key] == 0)


@pytest.fixture(scope="module")
def valid(eng, c, keyset):
    return materialise(eng, c, keyset, "valid", plan_valid())


def test_every_share_valid(eng, c, keyset, valid):
    """case 1: all five outputs are the exact call's and the model's; no share is verified exactly, every tuple with a candidate passes; the
    outputs verify as bitmap aggregates.  Default routing, the small-batch layouts off (the lane-pair family serves the tuple check), every
    tuple summed by a wave, every tuple by a lane, and a bitmap one word wider than the set needs"""
    reg_set(eng, keyset)
    assert [len(t[1]) for t in valid] == SIZES
    exact = collect(eng, valid)
    assert eng.debug_collect_opt_last() == dict(checked=0, passed=0, exact_tuples=0, exact_shares=0)
    want, want_hook = model(c, keyset, valid)
    assert exact == want and set(exact[0]) == {0, 2} and exact[4][-1] == 33 and exact[4][6] == 32
    assert want_hook == dict(checked=9, passed=9, exact_tuples=0, exact_shares=0)
    msgs = [t[0] for t in valid]
    for name, opts in (("default", {}), ("small_off", SMALL_OFF), ("all_waves", {E.OPT_COLLECT_WAVE_MIN_SHARES: 1}),
                       ("all_lanes", {E.OPT_COLLECT_WAVE_MIN_SHARES: 1 << 30})):
        got, hook = opt(eng, valid, opts=opts)
        assert got[0] == exact[0], (name, [(s, a, b) for s, (a, b) in enumerate(zip(got[0], exact[0])) if a != b][:8])
        assert got == exact, (name, [i for i in range(len(valid)) if got[2][64 * i:64 * i + 64] != exact[2][64 * i:64 * i + 64]])
        assert hook == want_hook, (name, hook)
        assert with_options(eng, opts, lambda: eng.batch_verify_keyed_bitmap(msgs, got[2], got[3], BM)) == bytes(len(valid)), name
    got, hook = opt(eng, valid, bm_words=3)
    assert got == collect(eng, valid, bm_words=3) == model(c, keyset, valid, bm_words=3)[0] and hook == want_hook
    assert all(got[3][3 * i + 2] == 0 for i in range(len(valid)))
    # the defaults: a call of a few hundred shares is the exact call
    msgs_, shares, keys, sizes = flat(valid)
    assert len(keys) < E.COLLECT_OPT_MIN_SHARES_DEFAULT
    assert eng.batch_collect_keyed_bitmap_optimistic(msgs_, b"".join(shares), keys, sizes, BM, want_counts=True) == exact
    assert eng.debug_collect_opt_last()["checked"] == 0


def test_set_of_43_keys(eng, c, keyset):
    """three more keys behind the set (43: no multiple of 8 or of 32): tuples whose candidates sit in the partial last window of the subset
    tables, all valid and with one wrong share"""
    sks, pks, reg = keyset
    more = [int.from_bytes(sk_bytes(990 + j), "big") % R for j in range(3)]
    wide = (sks + more, pks + derive(eng, more), reg + [0, 0, 0])
    try:
        assert list(eng.register_keys(b"".join(wide[1]))) == wide[2]
        plan = [[(40, "ok"), (41, "ok"), (42, "ok"), (K_NEG1, "ok"), (2, "ok")], [(42, "ok"), (41, "wrong"), (33, "ok")], [(43, "ok"), (42, "ok")]]
        msgs = [D("collect-opt/wide", i) for i in range(3)]
        other = D("collect-opt/wide/other", 0)
        sigs = iter(sign(eng, [(other if kind == "wrong" else msgs[i], wide[0][key] if key < 43 else wide[0][0]) for i, t in enumerate(plan) for key, kind in t]))
        tuples = [(msgs[i], [(next(sigs), key) for key, _ in t]) for i, t in enumerate(plan)]
        exact = collect(eng, tuples)
        assert list(exact[0]) == [0] * 6 + [9, 0, 2, 0] and exact[4] == [5, 2, 1] and exact[3][1] == 0x780 | 0x80
        got, hook = opt(eng, tuples)
        assert got == exact and hook == dict(checked=3, passed=2, exact_tuples=1, exact_shares=3)
        assert (got, hook) == model(c, wide, tuples)
    finally:
        reg_set(eng, keyset)


def test_one_wrong_share(eng, c, keyset):
    """case 2: a valid signature of another message in the 15-share tuple and in the 65-share one (there in the second stride of the wave
    layout): the exact call's outputs; exactly the candidates of those two tuples are verified one by one"""
    reg_set(eng, keyset)
    plan = plan_valid()
    i15, i65 = SIZES.index(15), SIZES.index(65)
    plan[i15][4] = (plan[i15][4][0], "wrong")
    assert plan[i65][64][1] == "ok"
    plan[i65][64] = (plan[i65][64][0], "wrong")
    tuples = materialise(eng, c, keyset, "wrong", plan)
    exact = collect(eng, tuples)
    assert exact[0].count(9) == 2
    want, want_hook = model(c, keyset, tuples)
    n_cand = candidates(tuples, keyset[2], i15) + candidates(tuples, keyset[2], i65)
    assert want == exact and want_hook == dict(checked=9, passed=7, exact_tuples=2, exact_shares=n_cand) and n_cand == 15 + 33
    for opts in ({}, SMALL_OFF, {E.OPT_COLLECT_WAVE_MIN_SHARES: 1 << 30}):
        got, hook = opt(eng, tuples, opts=opts)
        assert got == exact, opts
        assert hook == want_hook, (opts, hook)


def test_shares_refused_by_rules_1_to_3(eng, c, keyset):
    """case 3: a coordinate >= q, a point off the curve, a key index >= n_keys and the status-4 key inside otherwise valid tuples — and the
    identity under REJECT_IDENTITY: the exact call's outputs, and the tuples still pass optimistically"""
    reg_set(eng, keyset)
    plan = plan_valid()
    for i, kinds in ((SIZES.index(15), ["big", "curve", "nkeys", "badkey"]), (SIZES.index(17), ["curve", "badkey"]), (SIZES.index(63), ["big", "nkeys"])):
        at = [j for j, (_, kind) in enumerate(plan[i]) if kind == "ok"][1:]
        for j, kind in zip(at[::3], kinds):
            plan[i][j] = (plan[i][j][0], kind)
    tuples = materialise(eng, c, keyset, "refused", plan)
    for flags in (0, 2):
        exact = collect(eng, tuples, flags)
        want, want_hook = model(c, keyset, tuples, flags=flags)
        assert {0, 2, 4, 6} <= set(exact[0]) and 9 not in exact[0]
        assert want == exact and want_hook == dict(checked=9, passed=9, exact_tuples=0, exact_shares=0)
        got, hook = opt(eng, tuples, flags)
        assert got == exact and hook == want_hook, (flags, hook)
    assert collect(eng, tuples, 2)[0] != collect(eng, tuples, 0)[0]         # the identity key's share is refused under REJECT_IDENTITY


def test_duplicates_go_the_exact_way(eng, c, keyset):
    """case 4: two valid shares of one key; a valid and an invalid share of one key in both orders; a duplicate 64 positions apart in a
    70-share tuple (one lane's stride in the wave layout): sent to the exact route, the exact call's outputs"""
    reg_set(eng, keyset)
    long = [(SIGNABLE[j % 39], "ok") if j < 39 else (N_KEYS + j, "filler") for j in range(70)]
    long[66] = (long[2][0], "ok")
    plan = [[(5, "ok"), (5, "ok"), (6, "ok")], [(7, "ok"), (7, "wrong"), (8, "ok")], [(7, "wrong"), (7, "ok"), (8, "ok")], long,
            [(9, "ok"), (10, "ok"), (11, "ok")]]
    tuples = materialise(eng, c, keyset, "dup", plan)
    exact = collect(eng, tuples)
    assert exact[4] == [2, 2, 2, 39, 3] and exact[0].count(9) == 2
    want, want_hook = model(c, keyset, tuples)
    assert want == exact and want_hook == dict(checked=1, passed=1, exact_tuples=4, exact_shares=3 + 3 + 3 + 40)
    for opts in ({}, {E.OPT_COLLECT_WAVE_MIN_SHARES: 1}, {E.OPT_COLLECT_WAVE_MIN_SHARES: 1 << 30}):
        got, hook = opt(eng, tuples, opts=opts)
        assert got == exact and hook == want_hook, (opts, hook)


def test_the_deviation_pinned(eng, c, keyset):
    """case 5: sigma_a + D and sigma_b - D (D = G1) among six valid shares.  The optimistic call gives both 0 and sets bits a and b; the
    aggregate is the exact call's aggregate for the honest shares; the bitmap verify accepts it.  The exact call gives 9, 9 — and so does
    the optimistic one with the per-tuple minimum above the tuple's length"""
    reg_set(eng, keyset)
    a, b = 12, 20
    honest_plan = [[(2, "ok"), (a, "ok"), (5, "ok"), (K_NEG1, "ok"), (b, "ok"), (K_IDENT, "ok"), (30, "ok"), (1, "ok")], [(3, "ok"), (4, "ok")]]
    forged_plan = [[(k, {a: "plus", b: "minus"}.get(k, kind)) for k, kind in honest_plan[0]], honest_plan[1]]
    honest, forged = materialise(eng, c, keyset, "deviation", honest_plan), materialise(eng, c, keyset, "deviation", forged_plan)
    ia, ib = 1, 4
    exact_honest, exact_forged = collect(eng, honest), collect(eng, forged)
    assert exact_honest[0] == bytes(10) and list(exact_forged[0]) == [9 if s in (ia, ib) else 0 for s in range(10)]
    got, hook = opt(eng, forged)
    assert got[0] == bytes(10) and hook == dict(checked=2, passed=2, exact_tuples=0, exact_shares=0)
    assert (got[3][a // 32] >> (a % 32)) & 1 and (got[3][b // 32] >> (b % 32)) & 1
    assert got[1:] == exact_honest[1:]                                     # tuple statuses, aggregates, rows and counts of the honest input
    assert got[2] != exact_forged[2] and got[4] == [8, 2] and exact_forged[4] == [6, 2]
    assert eng.batch_verify_keyed_bitmap([t[0] for t in forged], got[2], got[3], BM) == bytes(2)
    assert (got, hook) == model(c, keyset, forged)
    got, hook = opt(eng, forged, opts={E.OPT_COLLECT_OPT_MIN_TUPLE_SHARES: 9})
    assert got == exact_forged and hook == dict(checked=0, passed=0, exact_tuples=2, exact_shares=10)


def test_edge_cases(eng, c, keyset):
    """case 6: a key and its negation both signing (two bits, identity aggregate, passes); the identity key with an identity share; an empty
    tuple; a tuple whose shares are all refused; key 0 under both of its indices"""
    reg_set(eng, keyset)
    plan = [[(1, "ok"), (K_NEG1, "ok")], [(K_IDENT, "ok")], [], [(3, "big"), (4, "curve"), (5, "nkeys"), (6, "badkey"), (N_KEYS + 3, "filler")],
            [(0, "ok"), (K_DUP0, "ok")], [(8, "ok")]]
    tuples = materialise(eng, c, keyset, "edge", plan)
    exact = collect(eng, tuples)
    assert exact[4] == [2, 1, 0, 0, 2, 1] and exact[2][:128] == bytes(128) and list(exact[0][3:8]) == [6, 4, 2, 4, 2]
    want, want_hook = model(c, keyset, tuples)
    assert want == exact and want_hook == dict(checked=4, passed=4, exact_tuples=0, exact_shares=0)
    got, hook = opt(eng, tuples)
    assert got == exact and hook == want_hook, hook
    assert eng.batch_verify_keyed_bitmap([t[0] for t in tuples], got[2], got[3], BM) == bytes(len(tuples))
    # a per-tuple minimum of 2 sends the two one-share tuples the exact way: the same bytes
    got, hook = opt(eng, tuples, opts={E.OPT_COLLECT_OPT_MIN_TUPLE_SHARES: 2})
    assert got == exact and hook == dict(checked=2, passed=2, exact_tuples=2, exact_shares=2)
    assert (got, hook) == model(c, keyset, tuples, min_tuple=2)


def test_slicing(eng, c, keyset, valid):
    """case 7: BN254_OPT_MAX_CHUNK = 64 — the 130-share tuple straddles three slices of the shares, the ten tuples' check runs in one piece
    (with 7: in two).  All valid, then a wrong share of that tuple inside its second slice: the unsliced call's outputs and counters"""
    reg_set(eng, keyset)
    whole, hook_whole = opt(eng, valid)
    for chunk in (64, 7):
        got, hook = opt(eng, valid, opts={E.OPT_MAX_CHUNK: chunk})
        assert got == whole and hook == hook_whole, chunk
    plan = plan_valid()
    lo = sum(SIZES[:9])
    j = 16
    assert 256 <= lo + j < 320 and plan[9][j][1] == "ok"
    plan[9][j] = (plan[9][j][0], "wrong")
    tuples = materialise(eng, c, keyset, "sliced", plan)
    exact = collect(eng, tuples)
    assert exact[0][lo + j] == 9 and exact[0].count(9) == 1
    whole, hook_whole = opt(eng, tuples)
    assert whole == exact and hook_whole == dict(checked=9, passed=8, exact_tuples=1, exact_shares=33)
    for chunk in (64, 7):
        got, hook = opt(eng, tuples, opts={E.OPT_MAX_CHUNK: chunk})
        assert got == whole and hook == hook_whole, (chunk, hook)


def test_whole_call_routing(eng, c, keyset, valid):
    """case 8: no keys registered, and option 40 above n_shares: the exact call's bytes, nothing checked optimistically.  One below the
    bound the route is taken"""
    n_sh = sum(SIZES)
    try:
        eng.register_keys(b"")
        exact = collect(eng, valid, bm_words=0)
        got, hook = opt(eng, valid, bm_words=0)
        assert got == exact and 0 not in got[0] and hook == dict(checked=0, passed=0, exact_tuples=0, exact_shares=0)
    finally:
        reg_set(eng, keyset)
    exact = collect(eng, valid)
    got, hook = opt(eng, valid, opts={E.OPT_COLLECT_OPT_MIN_SHARES: n_sh + 1})
    assert got == exact and hook == dict(checked=0, passed=0, exact_tuples=0, exact_shares=0)
    got, hook = opt(eng, valid, opts={E.OPT_COLLECT_OPT_MIN_SHARES: n_sh})
    assert got == exact and hook["checked"] == 9


def test_device_form(eng, c, keyset, valid):
    """cases 6 and 9: the _device form on a caller's stream against the exact _device call and the host form — the plain case, a reversed
    share range, an overlapping one (tuple_status 2, the shares read 2), a reversed message offset (5); misaligned keys and a bitmap one
    word short are refused"""
    from tests.hip_ctypes import DevBuf, Stream
    from bn254_amd.engine import pack_messages
    reg_set(eng, keyset)
    tuples = [t for t in valid if 0 < len(t[1]) <= 17]
    tuples = tuples + materialise(eng, c, keyset, "device", [[(4, "ok"), (5, "wrong"), (6, "ok")], [(7, "ok"), (7, "ok")], [(1, "ok"), (K_NEG1, "ok")], [(9, "ok")]])
    msgs, shares, keys, sizes = flat(tuples)
    n, n_shares = len(tuples), len(keys)
    blob, off = pack_messages(msgs)
    off = list(off)
    soff = [sum(sizes[:i]) for i in range(n + 1)]
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    stream = Stream()
    bufs = []
    lens = (n_shares, n, 64 * n, 4 * BM * n, 4 * n)

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_msgs, d_shares, d_keys = dev(bytes(blob)), dev(b"".join(shares)), dev(u32(keys) + bytes(4))
        outs = [dev(nbytes=k) for k in lens]

        def run(moff, share_off, optimistic):
            for b, k in zip(outs, lens):
                b.upload(b"\xEE" * k)
            head = (d_msgs.ptr, dev(u64(moff)).ptr, d_shares.ptr, d_keys.ptr, dev(u64(share_off)).ptr, n_shares, n, BM)
            fn = eng.batch_collect_keyed_bitmap_optimistic_device if optimistic else eng.batch_collect_keyed_bitmap_device
            fn(*head, *(b.ptr for b in outs), stream=stream.handle)
            stream.synchronize()
            return tuple(b.download(k) for b, k in zip(outs, lens)), eng.debug_collect_opt_last()

        def both(moff, share_off):
            exact, hook0 = run(moff, share_off, False)
            got, hook = with_options(eng, FORCE, lambda: run(moff, share_off, True))
            assert hook0["checked"] == 0 and hook["checked"] > 0 and hook["exact_tuples"] >= 2
            assert got == exact
            return got
        host, hook_host = opt(eng, tuples)
        g = both(off, soff)
        assert g[0] == host[0] and g[1] == host[1] and g[2] == host[2]
        assert g[3] == u32(host[3]) and g[4] == u32(host[4])
        assert with_options(eng, FORCE, lambda: run(off, soff, True))[1] == hook_host
        i = 2
        rev = soff[:]
        rev[i + 1] = soff[i] - 1                     # tuple i reversed; tuple i + 1 then starts before the earlier offset soff[i]
        g = both(off, rev)
        assert g[1][i] == 2 and g[1][i + 1] == 2 and all(g[0][s] == 2 for s in range(soff[i], soff[i + 2]))
        assert g[2][64 * i:64 * (i + 2)] == bytes(128) and g[3][4 * BM * i:4 * BM * (i + 2)] == bytes(8 * BM) and g[4][4 * i:4 * (i + 2)] == bytes(8)
        lap = soff[:]
        lap[i + 1] = soff[i + 2]                     # tuple i swallows tuple i + 1; tuple i + 2 then starts before an earlier offset
        lap[i + 2] = soff[i + 1]
        g = both(off, lap)
        assert g[1][i] == 0 and g[1][i + 1] == 2 and g[1][i + 2] == 2 and all(g[0][s] == 2 for s in range(soff[i + 2], soff[i + 3]))
        k = next(j for j in range(1, n - 1) if off[j + 1] > off[j])
        mrev = off[:]
        mrev[k + 1] = off[k] - 1
        g = both(mrev, soff)
        assert g[1][k] == 5 and g[4][4 * k:4 * k + 4] == bytes(4) and all(g[0][s] == 5 for s in range(soff[k], soff[k + 1]) if host[0][s] in (0, 9))
        args = (d_msgs.ptr, dev(u64(off)).ptr, d_shares.ptr)
        with pytest.raises(E.NativeError) as e:
            eng.batch_collect_keyed_bitmap_optimistic_device(*args, d_keys.ptr + 1, dev(u64(soff)).ptr, n_shares, n, BM, *(b.ptr for b in outs), stream=stream.handle)
        assert e.value.rc == -10002                    # BN254_E_MISALIGNED
        with pytest.raises(E.NativeError) as e:
            eng.batch_collect_keyed_bitmap_optimistic_device(*args, d_keys.ptr, dev(u64(soff)).ptr, n_shares, n, BM - 1, *(b.ptr for b in outs), stream=stream.handle)
        assert e.value.rc == -10001                    # BN254_E_BAD_ARGUMENT: the bitmap cannot hold key 39
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


def test_stage_intervals(eng, c, keyset, valid):
    """bn254_ctx_last_kernel_ms after a profiled call: four non-negative intervals, and the tuples' Miller loop and final exponentiation among them"""
    reg_set(eng, keyset)
    try:
        eng.set_profiling(True)
        got, hook = opt(eng, valid)
        ms = eng.last_kernel_ms()
    finally:
        eng.set_profiling(False)
    print("optimistic collect ms", ms)
    assert hook["passed"] == 9 and all(v >= 0 for v in ms.values()) and ms["miller_loop"] > 0


def test_python_and_cpp_mirrors(eng, keyset, tmp_path):
    """case 9: ECDSA.aggregate_keyed_signers_optimistic returns what the exact mirror returns and round-trips into
    ECDSA.verify_keyed_signers; so does the compiled C++ mirror"""
    from bn254_amd.api import ECDSA, Error, ErrorKind, PrivateKey, PublicKey
    sk = [PrivateKey(int.from_bytes(sk_bytes(j), "big")) for j in range(4)]
    pk = [PublicKey.from_private_key(s) for s in sk]
    try:
        assert ECDSA.register_keys(pk, engine=eng) == [None] * 4
        msg = b"round 12"
        sigs = [ECDSA.sign(msg, s) for s in sk]
        bad = ECDSA.sign(b"round 11", sk[3])
        for args in ((msg, [sigs[2], sigs[0], sigs[1]], [2, 0, 1]), (msg, [sigs[2], sigs[0], bad, sigs[1]], [2, 0, 3, 9]),
                     (msg, [sigs[2], sigs[0], sigs[1], sigs[2], sigs[3]], [2, 0, 3, 2, 9])):
            want = ECDSA.aggregate_keyed_signers(*args, engine=eng)

            def call():
                return ECDSA.aggregate_keyed_signers_optimistic(*args, engine=eng), eng.debug_collect_opt_last()
            got, hook = with_options(eng, FORCE, call)
            assert (hook["passed"] == 1) != (hook["exact_tuples"] == 1) and hook["checked"] + hook["exact_tuples"] >= 1, hook
            assert got[0].raw == want[0].raw and got[1] == want[1] and got[2] == want[2]
            assert ECDSA.verify_keyed_signers(msg, got[0], got[1], engine=eng) is None
        assert got[2] == [None, None, Error(ErrorKind.VerificationFailed), None, Error(ErrorKind.IndexOutOfBounds)]
        res = with_options(eng, FORCE, lambda: ECDSA.batch_aggregate_keyed_signers_optimistic([(msg, sigs, [0, 1, 2, 3]), (b"other", [], [])], engine=eng))
        assert res[0][1] == [0, 1, 2, 3] and res[1][1] == [] and res[1][0].raw == bytes(64)
    finally:
        reg_set(eng, keyset)
    src = tmp_path / "collect_opt_mirror.cpp"
    src.write_text(CPP_MIRROR)
    exe = str(tmp_path / "collect_opt_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "bn254_amd", "host"), str(src), "-L" + os.path.join(ROOT, "bn254_amd"),
                           "-lbn254hip", "-Wl,-rpath," + os.path.join(ROOT, "bn254_amd"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "collect opt mirror ok" in p.stdout, (p.stdout, p.stderr)


CPP_MIRROR = r"""
#include <cstdio>
#include "bn254.hpp"
int main() {
  try {
    bn254::PrivateKey k[3];
    for (int j = 0; j < 3; ++j) { k[j].bytes = {}; k[j].bytes[31] = (uint8_t)(7 + j); k[j].bytes[5] = 0x12; }
    std::vector<bn254::PublicKey> pk;
    for (int j = 0; j < 3; ++j) pk.push_back(bn254::PublicKey::from_private_key(k[j]));
    if (bn254::ECDSA::register_keys(pk) != std::vector<uint8_t>{0, 0, 0}) return 2;
    bn254::Engine& e = bn254::Engine::default_engine();
    if (bn254_ctx_set_option(e.raw(), BN254_OPT_COLLECT_OPT_MIN_SHARES, 0) || bn254_ctx_set_option(e.raw(), BN254_OPT_COLLECT_OPT_MIN_TUPLE_SHARES, 0)) return 9;
    std::vector<uint8_t> msg = {'c', 'o', 'l', 'l', 'e', 'c', 't'}, other = {'x'};
    auto s0 = bn254::ECDSA::sign(msg, k[0]), s1 = bn254::ECDSA::sign(msg, k[1]), s2 = bn254::ECDSA::sign(msg, k[2]), w1 = bn254::ECDSA::sign(other, k[1]);
    uint64_t hook[4];
    auto good = bn254::ECDSA::aggregate_keyed_signers_optimistic(msg, {s2, s0, s1}, {2, 0, 1}, 3);
    auto want = bn254::ECDSA::aggregate_keyed_signers(msg, {s2, s0, s1}, {2, 0, 1}, 3);
    if (good.signer_indices != want.signer_indices || good.statuses != want.statuses || good.signature.raw != want.signature.raw) return 3;
    auto r = bn254::ECDSA::aggregate_keyed_signers_optimistic(msg, {s2, s0, w1, s2}, {2, 0, 1, 5}, 3);
    if (bn254_debug_collect_opt_last(e.raw(), hook) || hook[0] != 1 || hook[1] != 0 || hook[2] != 1 || hook[3] != 3) return 6;
    auto x = bn254::ECDSA::aggregate_keyed_signers(msg, {s2, s0, w1, s2}, {2, 0, 1, 5}, 3);
    if (r.signer_indices != std::vector<uint32_t>{0, 2} || r.statuses != std::vector<uint8_t>{0, 0, 9, 2}) return 4;
    if (r.signer_indices != x.signer_indices || r.statuses != x.statuses || r.signature.raw != x.signature.raw) return 5;
    bn254::ECDSA::verify_keyed_signers(msg, r.signature, r.signer_indices, 3);
    auto b = bn254::ECDSA::batch_aggregate_keyed_signers_optimistic({{msg, {s0, s1}, {0, 1}}, {other, {}, {}}}, 3);
    if (b.size() != 2 || b[0].signer_indices != std::vector<uint32_t>{0, 1} || !b[1].signer_indices.empty()) return 7;
    printf("collect opt mirror ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
"""
