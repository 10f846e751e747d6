"""bn254_batch_merge_keyed_bitmap_optimistic[_device] (include/bn254_hip.h) on the GPU.  Every case is compared with the
exact merge on the same context, with tests/merge_opt_model.py, and with the counters of bn254_debug_merge_opt_last.  The model's two
callbacks are independent of the route under test: part_check is the exact merge's status (identity 1: the bitmap verify), tuple_check the
bitmap verify of the model's own provisional sum (the oracle's g1_add) against the model's own union row.  The route is forced with
BN254_OPT_MERGE_OPT_MIN_PARTS = 0 and the option restored afterwards, so no test depends on the measured default.  Identity 2 on every call:
the outputs fed to bn254_batch_verify_keyed_bitmap with flags 0 give 0 for every accepted tuple.  Key set A, the plan and the helpers are
those of tests/test_gpu_merge_keyed_bitmap.py.  Run on the MI355X box: -m gpu."""
import ctypes
import os
import struct
import subprocess

import pytest

from bn254_amd import engine as E
from tests import merge_model
from tests import merge_opt_model as M
from tests import test_gpu_merge_keyed_bitmap as G
from tests.datagen import D, sk_bytes
from tests.test_gpu_merge_keyed_bitmap import BM, K_DUP0, K_IDENT, K_NEG1, K_REFUSED, LAYOUTS, N_GOOD, N_KEYS, SIZES, c, eng, keyset  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = G.ROOT
SMALL_BATCH = {E.OPT_TRIO_MAX_BATCH: 16384, E.OPT_NONET_MAX_BATCH: 3072, E.OPT_LM_MAX_BATCH: 1536}      # the options' defaults (bn254_ws.h)
ZERO_HOOK = dict(checked=0, passed=0, exact_tuples=0, exact_parts=0)
SIGNING = list(range(N_GOOD)) + [K_IDENT, K_DUP0, K_NEG1]            # the 39 bits somebody can sign for (K_IDENT: with the secret 0)


def with_options(eng, opts, fn):
    defaults = {E.OPT_MERGE_OPT_MIN_PARTS: E.MERGE_OPT_MIN_PARTS_DEFAULT, E.OPT_MERGE_WAVE_MIN_PARTS: E.MERGE_WAVE_MIN_PARTS_DEFAULT, E.OPT_MAX_CHUNK: 0}
    defaults.update(SMALL_BATCH)
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            eng.set_option(k, defaults[k])


def opt(eng, tuples, bm_words=BM, flags=0, opts=None, min_parts=0):
    """-> (the six outputs, the hook's counters) with the route forced (option 45 = min_parts), plus opts"""
    msgs, parts, rows, sizes = G.flat(tuples)
    o = {E.OPT_MERGE_OPT_MIN_PARTS: min_parts}
    o.update(opts or {})

    def call():
        out = eng.merge_keyed_bitmap_optimistic(msgs, b"".join(parts), [w for r in rows for w in r], sizes, bm_words, flags=flags, want_counts=True)
        return out, eng.debug_merge_opt_last()
    return with_options(eng, o, call)


def model(eng, c, tuples, exact, bm_words=BM):
    """-> ((part_status, taken, tuple_status, agg, bits, counts) as the engine returns them, hook) by tests/merge_opt_model.py.  `exact`: the
    exact merge's outputs on the same input — a partial with 0 or 9 there passed rules 1-3 (a candidate), and that byte is its part_check"""
    msgs, parts, rows, sizes = G.flat(tuples)
    n = len(tuples)
    tuple_st = list(exact[2])
    pre = [0 if st in (0, 9) else st for st in exact[0]]
    # the tuple check of every tuple at once: the provisional first fit over the candidates, summed by the oracle, through the bitmap verify
    urows, _, taken = merge_model.select(rows, pre, sizes, tuple_st, bm_words)
    agg = b"".join(merge_model.aggregates(c, parts, sizes, taken))
    verdicts = eng.batch_verify_keyed_bitmap(msgs, agg, [w for r in urows for w in r], bm_words) if n else b""
    out = M.merge(rows, pre, sizes, tuple_st, bm_words, lambda i, row, tk: verdicts[i], lambda p: exact[0][p])
    final_agg = b"".join(merge_model.aggregates(c, parts, sizes, out["taken"]))
    return (bytes(out["part_status"]), bytes(out["taken"]), bytes(tuple_st), final_agg, [w for r in out["rows"] for w in r], out["counts"]), out["hook"]


def check(eng, c, tuples, bm_words=BM, flags=0, layouts=LAYOUTS, opts=None, same_as_exact=True):
    """the optimistic call on every layout against the model and (unless a cancelling pair is planted) the exact merge's bytes; the hook
    against the model's; identity 2.  -> (outputs, hook)"""
    exact = G.merge(eng, tuples, bm_words, flags)
    want, want_hook = model(eng, c, tuples, exact, bm_words)
    if same_as_exact:
        assert want == exact
    msgs = [t[0] for t in tuples]
    n = len(tuples)
    for name, wave_min in layouts:
        o = {E.OPT_MERGE_WAVE_MIN_PARTS: wave_min}
        o.update(opts or {})
        got, hook = opt(eng, tuples, bm_words, flags, opts=o)
        for k, label in enumerate(("part_status", "part_taken", "tuple_status", "agg", "bits", "counts")):
            assert got[k] == want[k], (name, flags, label, [i for i in range(len(want[k])) if got[k][i] != want[k][i]][:8] if k != 3 else
                                       [i for i in range(n) if got[3][64 * i:64 * i + 64] != want[3][64 * i:64 * i + 64]])
        assert hook == want_hook, (name, flags, hook, want_hook)
        if n:                                                            # identity 2, flags 0 on the call's own outputs
            closed = eng.batch_verify_keyed_bitmap(msgs, got[3], got[4], bm_words)
            assert all(closed[i] == 0 for i in range(n) if got[2][i] == 0), name
    return want, want_hook


@pytest.fixture(scope="module")
def cases(eng, c, keyset):
    return G.make(eng, c, keyset[0] + [0] * 24, "cases", G.plan_a(), BM)


def valid_plan():
    """the ten sizes, every partial valid and pairwise disjoint: partial t < 39 signs for SIGNING[t] alone; the long tuples are filled two
    ways — identity partials with empty rows (candidates: taken, they add nothing) and partials with a bit >= n_keys (2: no candidates)"""
    plan = []
    for k in SIZES:
        t_plan = []
        for t in range(k):
            if t < len(SIGNING):
                t_plan.append(([SIGNING[t]], "ok"))
            elif t % 2:
                t_plan.append(([], "ok"))
            else:
                t_plan.append(([N_KEYS + t % 24], "also"))
        plan.append(t_plan)
    return plan


@pytest.fixture(scope="module")
def valid(eng, c, keyset):
    return G.make(eng, c, keyset[0] + [0] * 24, "opt-valid", valid_plan(), BM)


def test_every_partial_valid(eng, c, keyset, valid):
    G.reg_set(eng, keyset)
    want, hook = check(eng, c, valid)
    assert hook == dict(checked=9, passed=9, exact_tuples=0, exact_parts=0)          # every tuple that has a candidate
    sizes = [len(t[1]) for t in valid]
    assert set(want[0]) == {0, 2} and want[5] == [min(k, 39) for k in sizes]
    assert list(want[1]) == [int(st == 0) for st in want[0]]                         # every candidate taken, the empty-row identities too
    # the tuple check on the lane-pair kernels: the small-batch options off
    check(eng, c, valid, opts={k: 0 for k in SMALL_BATCH})


def test_stage_intervals(eng, c, keyset, valid):
    """bn254_ctx_last_kernel_ms after a profiled optimistic merge (its tuple check and queue stages are the collect's, with their events): four
    non-negative intervals, and the tuples' Miller loop and final exponentiation among them"""
    G.reg_set(eng, keyset)
    try:
        eng.set_profiling(True)
        got, hook = opt(eng, valid)
        ms = eng.last_kernel_ms()
    finally:
        eng.set_profiling(False)
    print("optimistic merge ms", ms)
    assert hook["passed"] == 9 and len(ms) == 4 and all(v >= 0 for v in ms.values()) and ms["miller_loop"] > 0


@pytest.mark.parametrize("flags", [0, E.FLAG_G2_SUBGROUP_CHECK, E.FLAG_REJECT_IDENTITY], ids=["flags0", "g2_subgroup", "reject_identity"])
def test_plan_a_is_the_exact_merge(eng, c, keyset, cases, flags):
    """wrong, undecodable, out-of-range, refused-key and overlapping partials: a sum off by k * G1 never cancels, so all six outputs are the
    exact merge's bytes"""
    G.reg_set(eng, keyset)
    want, hook = check(eng, c, cases, flags=flags)
    assert hook["checked"] + hook["exact_tuples"] >= 11 and hook["exact_tuples"] >= 8 and hook["exact_parts"] > 100, hook
    if flags == 0:
        assert {0, 2, 4, 9} <= set(want[0])


def test_one_wrong_partial(eng, c, keyset, valid):
    """one partial of the 17-partial tuple replaced by sigma + G1: that tuple alone goes the exact way"""
    G.reg_set(eng, keyset)
    tuples = [(m, list(p)) for m, p in valid]
    i = SIZES.index(17)
    tuples[i][1][4] = (c.g1_add(tuples[i][1][4][0], c.g1_generator()), tuples[i][1][4][1])
    want, hook = check(eng, c, tuples)
    assert hook == dict(checked=9, passed=8, exact_tuples=1, exact_parts=17)
    at = sum(SIZES[:i])
    assert list(want[0][at:at + 17]) == [0] * 4 + [9] + [0] * 12 and want[5][i] == 16


def test_identity_sums_and_the_deviation(eng, c, keyset):
    sks, _ = keyset
    G.reg_set(eng, keyset)
    plan = [[([0, 1], "ok"), ([2, 3], "ok"), ([4], "ok")],
            [([1], "ok"), ([K_NEG1], "ok")],                             # a key and its negation in two partials: the identity sum passes
            [([5], "ok"), ([], "ok"), ([6], "ok")]]
    all_honest = honest = G.make(eng, c, sks + [0] * 24, "opt-cancel", plan, BM)
    g1 = c.g1_generator()
    neg_g1 = c.g1_mul(g1, (M.R - 1).to_bytes(32, "big"))
    forged = [(m, list(p)) for m, p in honest]
    forged[0][1][0] = (c.g1_add(honest[0][1][0][0], g1), honest[0][1][0][1])
    forged[0][1][1] = (c.g1_add(honest[0][1][1][0], neg_g1), honest[0][1][1][1])
    forged[2][1][0] = (c.g1_add(honest[2][1][0][0], g1), honest[2][1][0][1])          # ... and with an empty row: sigma + G1, -G1 on no key
    forged[2][1][1] = (neg_g1, honest[2][1][1][1])
    all_forged = forged
    for flags, n in ((0, 3), (E.FLAG_REJECT_IDENTITY, 2)):              # (the third tuple holds the identity as a partial: refused at the decode there)
        honest, forged = all_honest[:n], all_forged[:n]
        n_p = sum(len(t[1]) for t in honest)
        exact_honest = G.merge(eng, honest, BM, flags)
        assert exact_honest[0] == bytes(n_p) and exact_honest[1] == b"\x01" * n_p and exact_honest[3][64:128] == bytes(64)
        want, hook = check(eng, c, honest, flags=flags)
        assert want == exact_honest and hook == dict(checked=n, passed=n, exact_tuples=0, exact_parts=0)
        exact_forged = G.merge(eng, forged, BM, flags)
        assert list(exact_forged[0]) == [9, 9, 0, 0, 0, 9, 9, 0][:n_p]
        want, hook = check(eng, c, forged, flags=flags, same_as_exact=False)
        assert hook == dict(checked=n, passed=n, exact_tuples=0, exact_parts=0)
        assert want[0] == bytes(n_p) and want[1] == b"\x01" * n_p                        # both read 0 and are taken
        assert want[3] == exact_honest[3] and want[4] == exact_honest[4] and want[5] == exact_honest[5]      # the valid aggregate of the union row


def test_one_bit_rows_are_the_optimistic_collect(eng, c, keyset):
    sks, _ = keyset
    G.reg_set(eng, keyset)
    plan = []
    for i, k in enumerate([0, 1, 5, 17, 39]):
        t_plan = []
        for t in range(k):
            key = SIGNING[(5 * i + t) % 39]                              # distinct keys within a tuple
            t_plan.append(([key], "wrong" if (i, t) == (3, 6) else "ok"))
        plan.append(t_plan)
    plan.append([([3], "ok"), ([K_REFUSED], "also"), ([N_KEYS + 3], "also"), ([7], "curve")])
    tuples = G.make(eng, c, sks + [0] * 24, "opt-onebit", plan, BM)
    msgs, parts, rows, sizes = G.flat(tuples)
    keys = [bits[0] for t in plan for bits, _ in t]
    got, hook = opt(eng, tuples)
    assert hook == dict(checked=5, passed=4, exact_tuples=1, exact_parts=17)
    for min_shares in (E.COLLECT_OPT_MIN_SHARES_DEFAULT, 0):
        try:
            eng.set_option(E.OPT_COLLECT_OPT_MIN_SHARES, min_shares)
            share_st, ctuple_st, cagg, cbits, ccounts = eng.batch_collect_keyed_bitmap_optimistic(msgs, b"".join(parts), keys, sizes, BM, want_counts=True)
        finally:
            eng.set_option(E.OPT_COLLECT_OPT_MIN_SHARES, E.COLLECT_OPT_MIN_SHARES_DEFAULT)
        assert (got[0], got[2], got[3], got[4], got[5]) == (share_st, ctuple_st, cagg, cbits, ccounts), min_shares
    assert list(got[1]) == [int(st == 0) for st in got[0]] and {0, 2, 4, 9} <= set(got[0])
    check(eng, c, tuples)


def test_slicing(eng, c, keyset, valid, cases):
    """BN254_OPT_MAX_CHUNK = 5: the ten (and twelve) tuples are hashed and checked in pieces, the partials queued in slices, the failing
    tuples lie across slice boundaries; the same bytes and the same counters as in one piece"""
    G.reg_set(eng, keyset)
    tuples = [(m, list(p)) for m, p in valid]
    i = SIZES.index(17)
    tuples[i][1][4] = (c.g1_add(tuples[i][1][4][0], c.g1_generator()), tuples[i][1][4][1])
    assert sum(SIZES[:i]) % 5 and (sum(SIZES[:i]) + 17) // 5 > sum(SIZES[:i]) // 5 + 2
    whole, hook_whole = opt(eng, tuples)
    assert hook_whole == dict(checked=9, passed=8, exact_tuples=1, exact_parts=17) and whole == G.merge(eng, tuples, BM)
    for chunk in (5, 64):
        got, hook = opt(eng, tuples, opts={E.OPT_MAX_CHUNK: chunk})
        assert got == whole and hook == hook_whole, (chunk, hook)
    mixed = G.sliced_cases(cases, 300)
    check(eng, c, mixed, opts={E.OPT_MAX_CHUNK: 7}, layouts=LAYOUTS[2:])


def test_wide_rows_66_words(eng, c, keyset):
    """bm_words = 66 over 2 100 registered entries that repeat 8 distinct keys, in the wave layout: a disjoint tuple of 70 partials with bits in
    words 64 and 65 (CHECK, passes), the same with one wrong partial, and overlaps only in words 64 and 65 (distance 1 and 64: EXACT)"""
    sks, pks = keyset
    try:
        reg = eng.register_keys(b"".join(pks[j % 8] for j in range(2100)))
        assert reg == bytes(2100)
        secrets = [sks[j % 8] for j in range(2100)] + [0] * 12
        disjoint = [([100 + t, 2030 + t], "ok") for t in range(70)]
        wrong = list(disjoint)
        wrong[67] = (wrong[67][0], "wrong")
        long_t = [([100 + t], "ok") for t in range(70)]
        long_t[1] = ([101, 2060], "ok")
        long_t[65] = ([165, 2060], "ok")                              # word 64, 64 places behind the partial that holds the bit: the same lane
        long_t[2] = ([102, 2095], "ok")
        long_t[3] = ([103, 2095], "ok")                               # word 65, the next lane
        plan = [disjoint, wrong, [([5, 2050], "ok"), ([6, 2050], "ok"), ([7, 2090], "ok")], long_t]
        tuples = G.make(eng, c, secrets, "opt-wide66", plan, 66)
        want, hook = check(eng, c, tuples, 66, layouts=LAYOUTS[:1] + LAYOUTS[2:])
        assert hook == dict(checked=2, passed=1, exact_tuples=3, exact_parts=70 + 3 + 70)
        assert want[5] == [140, 138, 4, 70] and want[0].count(9) == 1
    finally:
        G.reg_set(eng, keyset)


def test_beyond_the_wave_grid(eng, c, keyset):
    """70 000 tuples of one partial each with the wave layout forced (the tuples from 65 536 on are reached by stride), every eleventh of the
    33 distinct ones sigma + G1, plus one disjoint tuple of 36 at the end: the exact merge's bytes, and the counters by hand"""
    sks, _ = keyset
    G.reg_set(eng, keyset)
    pool = G.make(eng, c, sks, "opt-many", [[([(3 * j) % N_GOOD, (3 * j + 1) % N_GOOD], "wrong" if j % 11 == 10 else "ok")] for j in range(33)], BM)
    last = G.make(eng, c, sks, "opt-many-last", [[([t], "ok") for t in range(N_GOOD)]], BM)[0]
    tuples = [pool[i % 33] for i in range(G.N_MANY)] + [last]
    msgs, parts, rows, sizes = G.flat(tuples)
    args = (msgs, b"".join(parts), [w for r in rows for w in r], sizes, BM)
    bad = sum(1 for i in range(G.N_MANY) if i % 33 % 11 == 10)

    def both():
        exact = eng.merge_keyed_bitmap(*args, want_counts=True)
        got = eng.merge_keyed_bitmap_optimistic(*args, want_counts=True)
        return exact, got, eng.debug_merge_opt_last()
    exact, got, hook = with_options(eng, {E.OPT_MERGE_OPT_MIN_PARTS: 0, E.OPT_MERGE_WAVE_MIN_PARTS: 1}, both)
    assert exact[0].count(9) == bad and exact[0].count(0) == G.N_MANY + N_GOOD - bad and exact[5][-1] == N_GOOD
    for k, (name, width) in enumerate((("part_status", 1), ("part_taken", 1), ("tuple_status", 1), ("agg", 64), ("bits", BM), ("counts", 1))):
        diff = [] if got[k] == exact[k] else [i for i in range(len(exact[k]) // width) if got[k][width * i:width * i + width] != exact[k][width * i:width * i + width]][:8]
        assert not diff, (name, diff)
    assert hook == dict(checked=G.N_MANY + 1, passed=G.N_MANY + 1 - bad, exact_tuples=bad, exact_parts=bad)
    assert eng.batch_verify_keyed_bitmap(msgs, got[3], got[4], BM) == bytes(len(tuples))


def test_routing_and_arguments(eng, c, keyset, valid, cases):
    small = [t for t in cases if len(t[1]) <= 17]
    # no keys registered: the exact merge's bytes, and the hook says "did not run"
    try:
        eng.register_keys(b"")
        got, hook = opt(eng, small)
        assert got == G.merge(eng, small, BM) and hook == ZERO_HOOK and not any(got[4])
    finally:
        G.reg_set(eng, keyset)
    # option 45 above n_parts: the same; at n_parts: the route
    n_parts = sum(len(t[1]) for t in valid)
    exact = G.merge(eng, valid, BM)
    got, hook = opt(eng, valid, min_parts=n_parts + 1)
    assert got == exact and hook == ZERO_HOOK
    got, hook = opt(eng, valid, min_parts=n_parts)
    assert got == exact and hook["checked"] == 9
    assert G.merge(eng, valid, BM) == exact and eng.debug_merge_opt_last() == ZERO_HOOK          # the exact merge clears the hook
    # bm_words = 0: every row is empty — the identity is a candidate that passes, a point fails its tuple's check
    g1 = c.g1_generator()
    empty = [(D("merge-opt/bm0", 0), [(bytes(64), []), (g1, []), (bytes(64), [])]), (D("merge-opt/bm0", 1), []), (D("merge-opt/bm0", 2), [(g1, [])]),
             (D("merge-opt/bm0", 3), [(bytes(64), [])])]
    want, hook = check(eng, c, empty, 0)
    assert list(want[0]) == [0, 9, 0, 9, 0] and list(want[1]) == [1, 0, 1, 0, 1] and hook == dict(checked=3, passed=1, exact_tuples=2, exact_parts=4)
    # ... with NULL bit pointers and NULL n_signers
    msgs, parts, _, sizes = G.flat(empty)
    blob, off = E.pack_messages(msgs)
    n, n_p = len(empty), len(parts)
    pst, tkn, tst, out = (ctypes.create_string_buffer(k) for k in (n_p, n_p, n, 64 * n))
    poff = (ctypes.c_uint64 * (n + 1))(0, 3, 3, 4, 5)
    lib = eng._lib.bn254_batch_merge_keyed_bitmap_optimistic

    def raw():
        return lib(eng._h, blob, off, b"".join(parts), None, poff, n_p, n, 0, 0, pst, tkn, tst, out, None, None)
    assert with_options(eng, {E.OPT_MERGE_OPT_MIN_PARTS: 0}, raw) == 0
    assert pst.raw == want[0] and tkn.raw == want[1] and tst.raw == bytes(n) and out.raw == bytes(64 * n)
    # n = 0 returns 0 whatever else is passed; the host form's offsets must start at 0, never decrease and end at n_parts
    assert lib(eng._h, None, None, None, None, None, 0, 0, BM, 0, None, None, None, None, None, None) == 0
    assert opt(eng, [])[0] == (b"", b"", b"", b"", [], [])
    for bad in ([1, 3, 3, 4, 5], [0, 3, 2, 4, 5], [0, 3, 3, 4, 4], [0, 3, 3, 4, 6]):
        rc = lib(eng._h, blob, off, b"".join(parts), None, (ctypes.c_uint64 * (n + 1))(*bad), n_p, n, 0, 0, pst, tkn, tst, out, None, None)
        assert rc == -10001, bad


def test_device_form(eng, c, keyset, valid):
    """the _device form on a caller's stream, a bitmap verify behind it with no synchronisation in between: the host form's bytes; a
    reversed range gives tuple status 2, an empty row, the identity and count 0, its partials 2 and not taken; NULL n_signers; a misaligned
    pointer is refused"""
    from tests.hip_ctypes import DevBuf, Stream
    G.reg_set(eng, keyset)
    tuples = [(m, list(p)) for m, p in valid if 0 < len(p) <= 17]
    tuples[3][1][2] = (c.g1_add(tuples[3][1][2][0], c.g1_generator()), tuples[3][1][2][1])      # the 16-partial tuple fails its check
    msgs, parts, rows, sizes = G.flat(tuples)
    n, n_parts = len(tuples), len(parts)
    blob, off = E.pack_messages(msgs)
    poff = [sum(sizes[:i]) for i in range(n + 1)]
    u64 = lambda v: struct.pack("<%dQ" % len(v), *v)   # noqa: E731
    u32 = lambda v: struct.pack("<%dI" % len(v), *v)   # noqa: E731
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_msgs, d_moff, d_parts, d_rows = dev(bytes(blob)), dev(u64(list(off))), dev(b"".join(parts) + bytes(4)), dev(u32([w for r in rows for w in r]) + bytes(4))
        sizes_out = (n_parts, n_parts, n, 64 * n, 4 * BM * n, 4 * n)
        outs = [dev(nbytes=k) for k in sizes_out]
        d_vst = dev(nbytes=n)

        def run(part_off, parts_ptr=None, poff_shift=0, counts=True):
            for b, k in zip(outs, sizes_out):
                b.upload(b"\xEE" * k)
            d_poff = dev(u64(part_off) + bytes(8))

            def call():
                eng.merge_keyed_bitmap_optimistic_device(d_msgs.ptr, d_moff.ptr, parts_ptr or d_parts.ptr, d_rows.ptr, d_poff.ptr + poff_shift, n_parts, n, BM,
                                                         *(b.ptr for b in outs[:5]), outs[5].ptr if counts else None, stream=stream.handle)
                eng.batch_verify_keyed_bitmap_device(d_msgs.ptr, d_moff.ptr, outs[3].ptr, outs[4].ptr, BM, n, d_vst.ptr, stream=stream.handle)
                stream.synchronize()
                return eng.debug_merge_opt_last()
            hook = with_options(eng, {E.OPT_MERGE_OPT_MIN_PARTS: 0}, call)
            raw = [b.download(k) for b, k in zip(outs, sizes_out)]
            return (raw[0], raw[1], raw[2], raw[3], list(struct.unpack("<%dI" % (BM * n), raw[4])), list(struct.unpack("<%dI" % n, raw[5])), d_vst.download(n)), hook

        host, host_hook = opt(eng, tuples)
        assert host == G.merge(eng, tuples, BM) and host_hook == dict(checked=n, passed=n - 1, exact_tuples=1, exact_parts=16)
        got, hook = run(poff)
        assert got[:6] == host and got[6] == bytes(n) and hook == host_hook
        got, hook = run(poff, counts=False)                          # NULL n_signers: the array is not touched
        assert got[:5] == host[:5] and got[5] == [0xEEEEEEEE] * n
        i = 1
        rev = poff[:]
        rev[i + 1] = poff[i] - 1                     # tuple i reversed; tuple i + 1 then starts before the earlier offset poff[i]: refused too
        g, hook = run(rev)
        orphans = set(range(poff[i], poff[i + 2]))
        for t in range(n):
            if t in (i, i + 1):
                assert g[2][t] == 2 and g[3][64 * t:64 * t + 64] == bytes(64) and g[4][BM * t:BM * t + BM] == [0] * BM and g[5][t] == 0, t
            else:
                assert g[2][t] == 0 and g[3][64 * t:64 * t + 64] == host[3][64 * t:64 * t + 64] and g[5][t] == host[5][t], t
        for p in range(n_parts):
            assert (g[0][p], g[1][p]) == ((2, 0) if p in orphans else (host[0][p], host[1][p])), p
        assert g[6] == bytes(n) and hook == dict(checked=n - 2, passed=n - 3, exact_tuples=1, exact_parts=16)
        for kw in (dict(parts_ptr=d_parts.ptr + 1), dict(poff_shift=4)):
            with pytest.raises(E.NativeError) as e:
                run(poff, **kw)
            assert e.value.rc == -10002, kw          # BN254_E_MISALIGNED
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


def test_python_and_cpp_mirrors(eng, keyset, tmp_path):
    """ECDSA.merge_keyed_signers_optimistic gives what ECDSA.merge_keyed_signers gives and round-trips into ECDSA.verify_keyed_signers; so does
    the compiled C++ mirror"""
    from bn254_amd.api import ECDSA, Error, ErrorKind, PrivateKey, PublicKey, Signature
    sk = [PrivateKey(int.from_bytes(sk_bytes(j), "big")) for j in range(5)]
    pk = [PublicKey.from_private_key(s) for s in sk]
    ints = [int.from_bytes(sk_bytes(j), "big") for j in range(5)]
    try:
        assert ECDSA.register_keys(pk, engine=eng) == [None] * 5
        msg = b"round 12"
        part = lambda idx: Signature(G.sign_sums(eng, [(msg, sum(ints[j] for j in idx))])[0])      # noqa: E731
        wrong = Signature(G.sign_sums(eng, [(msg, ints[0] + 1)])[0])
        parts = [(part([0, 1]), [0, 1]), (part([1, 2]), [1, 2]), (wrong, [3]), (part([3, 4]), [4, 3]), (part([2]), [2, 9]), (part([2]), [2])]
        eng.set_option(E.OPT_MERGE_OPT_MIN_PARTS, 0)
        for items in (parts, parts[:1] + parts[3:4]):                 # an overlap and a wrong partial (the exact way); then neither (one check)
            r = ECDSA.merge_keyed_signers_optimistic(msg, items, engine=eng)
            x = ECDSA.merge_keyed_signers(msg, items, engine=eng)
            assert r[0].raw == x[0].raw and r[1:] == x[1:]
            assert ECDSA.verify_keyed_signers(msg, r[0], r[1], engine=eng) is None
        sigma, signers, statuses, taken = ECDSA.merge_keyed_signers_optimistic(msg, parts, engine=eng)
        assert signers == [0, 1, 2, 3, 4] and taken == [True, False, False, True, False, True]
        assert statuses == [None, None, Error(ErrorKind.VerificationFailed), None, Error(ErrorKind.IndexOutOfBounds), None]
        res = ECDSA.batch_merge_keyed_signers_optimistic([(msg, parts[:2]), (b"other", [])], engine=eng)
        assert res[0][1] == [0, 1] and res[0][3] == [True, False] and res[1][1] == [] and res[1][0].raw == bytes(64) and res[1][2] == [] == res[1][3]
    finally:
        eng.set_option(E.OPT_MERGE_OPT_MIN_PARTS, E.MERGE_OPT_MIN_PARTS_DEFAULT)
        G.reg_set(eng, keyset)
    src = tmp_path / "merge_opt_mirror.cpp"
    src.write_text(CPP_MIRROR)
    exe = str(tmp_path / "merge_opt_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "bn254_amd", "host"), str(src), "-L" + os.path.join(ROOT, "bn254_amd"),
                           "-lbn254hip", "-Wl,-rpath," + os.path.join(ROOT, "bn254_amd"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "merge opt mirror ok" in p.stdout, (p.stdout, p.stderr)


CPP_MIRROR = r"""
#include <cstdio>
#include "bn254.hpp"
int main() {
  try {
    bn254::PrivateKey k[3];
    for (int j = 0; j < 3; ++j) { k[j].bytes = {}; k[j].bytes[31] = (uint8_t)(7 + j); k[j].bytes[5] = 0x11; }
    std::vector<bn254::PublicKey> pk;
    for (int j = 0; j < 3; ++j) pk.push_back(bn254::PublicKey::from_private_key(k[j]));
    if (bn254::ECDSA::register_keys(pk) != std::vector<uint8_t>{0, 0, 0}) return 2;
    bn254::Engine::default_engine().set_option(bn254::Engine::OPT_MERGE_OPT_MIN_PARTS, 0);
    std::vector<uint8_t> msg = {'m', 'e', 'r', 'g', 'e'};
    auto s0 = bn254::ECDSA::sign(msg, k[0]), s1 = bn254::ECDSA::sign(msg, k[1]), s2 = bn254::ECDSA::sign(msg, k[2]);
    auto child = bn254::ECDSA::aggregate_keyed_signers(msg, {s0, s1}, {0, 1}, 3);
    if (child.signer_indices != std::vector<uint32_t>{0, 1}) return 3;
    // disjoint and valid: one check; then an overlap, a wrong partial and an index outside the set: the exact way, the exact mirror's result
    auto a = bn254::ECDSA::merge_keyed_signers_optimistic(msg, {{child.signature, {0, 1}}, {s2, {2}}}, 3);
    if (a.signer_indices != std::vector<uint32_t>{0, 1, 2} || a.statuses != std::vector<uint8_t>{0, 0} || a.taken != std::vector<uint8_t>{1, 1}) return 7;
    bn254::ECDSA::verify_keyed_signers(msg, a.signature, a.signer_indices, 3);
    std::vector<bn254::ECDSA::PartialAggregate> parts = {{child.signature, {0, 1}}, {s1, {1}}, {s2, {2}}, {s2, {1}}, {s2, {2, 7}}};
    auto r = bn254::ECDSA::merge_keyed_signers_optimistic(msg, parts, 3);
    auto x = bn254::ECDSA::merge_keyed_signers(msg, parts, 3);
    if (r.signer_indices != std::vector<uint32_t>{0, 1, 2} || r.statuses != std::vector<uint8_t>{0, 0, 0, 9, 2} ||
        r.taken != std::vector<uint8_t>{1, 0, 1, 0, 0}) return 4;
    if (r.signature.raw != x.signature.raw || r.signer_indices != x.signer_indices || r.statuses != x.statuses || r.taken != x.taken) return 8;
    bn254::ECDSA::verify_keyed_signers(msg, r.signature, r.signer_indices, 3);
    try { bn254::ECDSA::verify_keyed_signers(msg, r.signature, {0, 1}, 3); return 5; }
    catch (const bn254::Error& e) { if (e.kind != bn254::ErrorKind::VerificationFailed) return 6; }
    printf("merge opt mirror ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
"""
