"""bn254_batch_threshold_combine_keyed_optimistic[_device] on the GPU (include/bn254_hip.h): the case set of the exact call
(tests/threshold_cases.py) under the group key f(0) * G2.  Expectations come from tests/threshold_opt_model.py — the pre-check from the
oracle's decoder, the tuple check from the oracle's verify of the model's interpolated signature under the group key, the share checks from
bn254_batch_verify_keyed — and from the exact call on the same inputs (identities A and B).  The optimistic route is forced with option
46 = 0 unless said otherwise, and EVERY test that claims the route ran holds bn254_debug_threshold_opt_last to the model's four counts: a
call that quietly fell back to the exact route would pass every byte comparison.  Run on the MI355X box: -m gpu."""
import os
import re
import subprocess

import pytest

from bn254_amd import engine as E
from tests import test_gpu_threshold as TG
from tests import threshold_cases as TC
from tests import threshold_model as TM
from tests import threshold_opt_model as OM

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = TC.R
FORCE = {E.OPT_THRESHOLD_OPT_MIN_SHARES: 0}
PASSING = ["exactly_t", "more_than_t", "upper_keys", "descending", "low_curve", "low_big", "low_oob"]
GOING_EXACT = ["t_minus_1", "twice", "valid_then_invalid", "invalid_then_valid", "empty", "all_bad", "low_wrong", "low_wrong_short", "low_curve_short",
               "low_big_short", "low_oob_short"]


def ws_default(name):
    text = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    return int(re.search(r"#define %s (\d+)" % name, text).group(1))


DEFAULTS = {E.OPT_THRESHOLD_OPT_MIN_SHARES: E.THRESHOLD_OPT_MIN_SHARES_DEFAULT, E.OPT_PAIR_LANES: 1, E.OPT_MAX_CHUNK: 0,
            E.OPT_COLLECT_WAVE_MIN_SHARES: ws_default("COLLECT_WAVE_MIN_SHARES_DEFAULT"), E.OPT_TRIO_MAX_BATCH: ws_default("TRIO_MAX_BATCH_DEFAULT"),
            E.OPT_NONET_MAX_BATCH: ws_default("NONET_MAX_BATCH_DEFAULT"), E.OPT_LM_MAX_BATCH: ws_default("LM_MAX_BATCH_DEFAULT")}
SMALL_OFF = {E.OPT_TRIO_MAX_BATCH: 0, E.OPT_NONET_MAX_BATCH: 0, E.OPT_LM_MAX_BATCH: 0}
ZERO_HOOK = dict(checked=0, passed=0, exact_tuples=0, exact_shares=0)


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def with_options(eng, opts, fn):
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            eng.set_option(k, DEFAULTS[k])


class Sets:
    """the key sets of the case set, each built at its first use: tuples, the keyed verify's statuses, the exact call's outputs, the group key"""

    def __init__(self, eng, c):
        self.eng, self.c, self.made = eng, c, {}

    def __getitem__(self, name):
        if name not in self.made:
            ks = TG.KeySet(self.eng, self.c, [s for s in TC.KEY_SETS if s[0] == name][0])
            ks.gk = TG.derive(self.eng, [ks.f0])[0] if ks.f0 is not None else None
            ks.exact = TG.combine(self.eng, ks.tuples, ks.bm_words, ks.t)
            TG.check(ks, ks.exact, name)
            self.made[name] = ks
        return self.made[name]


@pytest.fixture(scope="module")
def sets(eng, c):
    assert (E.OPT_TRIO_MAX_BATCH, E.OPT_NONET_MAX_BATCH, E.OPT_LM_MAX_BATCH) == (6, 13, 15)
    return Sets(eng, c)


def use(eng, ks, gk):
    """the set registered (which forgets the group key) and the group key named"""
    ks.register(eng)
    assert eng.set_group_key(gk) == 0


def model(c, eng, n_keys, tuples, gk, t, bm_words, share_exact=None):
    """tests/threshold_opt_model.py over the oracle -> (the model's dict, the group signatures it implies)"""
    msgs, shares, keys, sizes = TG.flat(tuples)
    pre = OM.precheck([c.g1_validate(s, 0) for s in shares], keys, [0] * n_keys, sizes, [0] * len(tuples))
    if share_exact is None:
        share_exact = TG.keyed(eng, tuples)

    def tuple_check(i, chosen):
        return c.verify(msgs[i], TM.group_signature(shares, chosen), gk, flags=0)

    m = OM.combine(keys, pre, sizes, [0] * len(tuples), bm_words, t, tuple_check, lambda s: share_exact[s])
    sigs = [TM.group_signature(shares, ch) if st == 0 else bytes(64) for st, ch in zip(m["tuple_status"], m["chosen"])]
    return m, sigs


def opt(eng, tuples, bm_words, t, opts=None, flags=0):
    """-> (the five outputs, the hook's counters), the route forced, plus opts"""
    o = dict(FORCE)
    o.update(opts or {})
    msgs, shares, keys, sizes = TG.flat(tuples)

    def call():
        out = eng.batch_threshold_combine_keyed_optimistic(msgs, b"".join(shares), keys, sizes, bm_words, t, flags=flags)
        return out, eng.debug_threshold_opt_last()
    return with_options(eng, o, call)


def hold(got, hook, m, sigs, label):
    """the five outputs and the counters against the model"""
    share_st, tuple_st, group, bits, counts = got
    print(label, "hook", hook, "model", m["hook"])
    assert hook == m["hook"], (label, hook, m["hook"])
    assert list(share_st) == m["share_status"], (label, [(s, a, b) for s, (a, b) in enumerate(zip(share_st, m["share_status"])) if a != b][:8])
    assert list(tuple_st) == m["tuple_status"], (label, list(tuple_st), m["tuple_status"])
    assert bits == [w for row in m["rows"] for w in row] and counts == m["counts"], (label, bits, counts, m["rows"], m["counts"])
    assert group == b"".join(sigs), (label, [i for i in range(len(sigs)) if group[64 * i:64 * i + 64] != sigs[i]])


def expectation(sets, c, eng, name, gk=None):
    """the model of a whole key set's tuples under gk (default: its true group key), computed once"""
    ks = sets[name]
    key = ("model", gk)
    if key not in ks.__dict__.setdefault("models", {}):
        ks.models[key] = model(c, eng, ks.n_keys, ks.tuples, gk or ks.gk, ks.t, ks.bm_words, ks.share_st)
    return ks.models[key]


def identity_a(ks, got, passing):
    """a passing tuple whose kept shares are all valid: tuple status, signature and row are the exact call's"""
    bm = ks.bm_words
    for i in passing:
        assert got[1][i] == ks.exact[1][i] == 0 and got[2][64 * i:64 * i + 64] == ks.exact[2][64 * i:64 * i + 64], i
        assert got[3][bm * i:bm * i + bm] == ks.exact[3][bm * i:bm * i + bm], i


def test_every_shape_of_the_dealt_set(eng, c, sets):
    """1. dealt9_t5, all 18 shapes, the true group key: which pass, which go exact, the counters, identity A, and (7.) the closed loop"""
    ks = sets["dealt9_t5"]
    use(eng, ks, ks.gk)
    m, sigs = expectation(sets, c, eng, "dealt9_t5")
    names = [s[0] for s in ks.shapes]
    assert sorted(names) == sorted(PASSING + GOING_EXACT) and len(names) == 18
    passing = [i for i, f in enumerate(m["flags"]) if f == OM.CHECK and m["verdicts"][i] == 0]
    assert sorted(names[i] for i in passing) == sorted(PASSING)
    assert m["hook"]["passed"] == len(PASSING) and m["hook"]["exact_tuples"] == len(GOING_EXACT)
    assert m["hook"]["checked"] == len(PASSING) + 2                       # low_wrong and low_wrong_short are checked, and fail
    got, hook = opt(eng, ks.tuples, ks.bm_words, ks.t)
    hold(got, hook, m, sigs, "dealt9_t5")
    identity_a(ks, got, passing)
    for i in range(len(names)):                                           # identity B: the tuples that went exact, all five outputs
        if i not in passing:
            lo, hi = sum(len(t[1]) for t in ks.tuples[:i]), sum(len(t[1]) for t in ks.tuples[:i + 1])
            assert (got[0][lo:hi], got[1][i], got[2][64 * i:64 * i + 64], got[3][i], got[4][i]) == \
                   (ks.exact[0][lo:hi], ks.exact[1][i], ks.exact[2][64 * i:64 * i + 64], ks.exact[3][i], ks.exact[4][i]), names[i]
    for i in passing:                                                     # the signature is THE group signature
        assert got[2][64 * i:64 * i + 64] == TM.signature_under(ks.tuples[i][0], ks.f0)
    closed_loop(eng, ks, got)


def closed_loop(eng, ks, got):
    """7. bn254_batch_verify of (m_i, group_sigs[i], GPK) is 0 for every status-0 tuple"""
    ok = [i for i in range(len(ks.tuples)) if got[1][i] == 0]
    assert ok
    st = eng.batch_verify([ks.tuples[i][0] for i in ok], b"".join(got[2][64 * i:64 * i + 64] for i in ok), ks.gk * len(ok), flags=0)
    assert st == bytes(len(ok)), list(st)


@pytest.mark.parametrize("name", ["dealt70_t63", "dealt70_t64", "dealt70_t65", "dealt9_t1", "dealt9_t9"])
def test_word_boundaries(eng, c, sets, name):
    """2. thresholds on both sides of a word boundary with three-word rows, threshold 1 and threshold = n"""
    ks = sets[name]
    use(eng, ks, ks.gk)
    m, sigs = expectation(sets, c, eng, name)
    got, hook = opt(eng, ks.tuples, ks.bm_words, ks.t)
    hold(got, hook, m, sigs, name)
    passing = [i for i, f in enumerate(m["flags"]) if f == OM.CHECK and m["verdicts"][i] == 0]
    assert len(passing) == 2 and hook["passed"] == 2                       # exactly_t and everybody; t_minus_1 (where there is one) goes exact
    identity_a(ks, got, passing)
    closed_loop(eng, ks, got)


def test_identity_group_key(eng, c, sets):
    """3. zero9_t5: f(0) = 0, the identity as group key — passing tuples give 64 zero bytes with status 0"""
    ks = sets["zero9_t5"]
    assert ks.gk == bytes(128)
    use(eng, ks, ks.gk)
    m, sigs = expectation(sets, c, eng, "zero9_t5")
    got, hook = opt(eng, ks.tuples, ks.bm_words, ks.t)
    hold(got, hook, m, sigs, "zero9_t5")
    passing = [i for i, f in enumerate(m["flags"]) if f == OM.CHECK and m["verdicts"][i] == 0]
    assert len(passing) >= 3 and hook["passed"] == len(passing)
    for i in passing:
        assert got[1][i] == 0 and got[2][64 * i:64 * i + 64] == bytes(64)
    identity_a(ks, got, passing)
    closed_loop(eng, ks, got)


@pytest.mark.parametrize("name", ["random9", "ident9", "dealt9_t5"])
def test_no_polynomial_or_the_wrong_key(eng, c, sets, name):
    """4. keys of no polynomial under some group key, and the dealt set under f(0) + 1: every accepted tuple goes exact — passed = 0 — and
    all five outputs are the exact call's, byte for byte"""
    ks = sets[name]
    wrong = TG.derive(eng, [(sets["dealt9_t5"].f0 + 1) % R])[0]
    use(eng, ks, wrong)
    m, sigs = expectation(sets, c, eng, name, gk=wrong)
    got, hook = opt(eng, ks.tuples, ks.bm_words, ks.t)
    hold(got, hook, m, sigs, name)
    assert hook["passed"] == 0 and hook["checked"] >= 3 and hook["exact_tuples"] == len(ks.tuples)
    assert got == ks.exact


def test_deviation_1_unverified_share_outside_the_kept_keys(eng, c, sets):
    """5. all nine keys, a wrong share at key 8: the tuple passes, that share reads 0 and n_valid = 9 — the exact call says 9 and 8"""
    ks = sets["dealt9_t5"]
    use(eng, ks, ks.gk)
    tuples = TG.plant(eng, c, "deviation 1", ks.secrets, [("nine", [(j, "ok") for j in range(8)] + [(8, "wrong")])], ks.n_keys)
    got, hook = opt(eng, tuples, 1, ks.t)
    assert hook == dict(checked=1, passed=1, exact_tuples=0, exact_shares=0)
    assert got[0] == bytes(9) and got[1] == b"\0" and got[3] == [0x1F] and got[4] == [9]
    assert got[2] == TM.signature_under(tuples[0][0], ks.f0)
    exact = TG.combine(eng, tuples, 1, ks.t)
    assert exact[0] == bytes(8) + b"\x09" and exact[4] == [8] and exact[1:4] == got[1:4]


def test_deviation_2_errors_that_cancel(eng, c, sets):
    """6. two shares of S' shifted by lambda_b D and -lambda_a D: the tuple passes with the true signature and both shares read 0; the exact
    call on the same tuple drops both keys"""
    ks = sets["dealt9_t5"]
    use(eng, ks, ks.gk)
    tuples = TG.plant(eng, c, "deviation 2", ks.secrets, [("six", [(j, "ok") for j in range(6)])], ks.n_keys)
    lam = TM.lagrange_at_zero([1, 2, 3, 4, 5])
    a, b = 1, 3
    d = c.g1_mul(c.g1_generator(), (0xD15EA5E).to_bytes(32, "big"))
    shift, st = eng.batch_g1_mul(d + d, lam[b].to_bytes(32, "big") + (R - lam[a]).to_bytes(32, "big"), 2)
    assert st == bytes(2)
    rows = list(tuples[0][1])
    rows[a] = (c.g1_add(rows[a][0], shift[:64]), a)
    rows[b] = (c.g1_add(rows[b][0], shift[64:]), b)
    tuples = [(tuples[0][0], rows)]
    got, hook = opt(eng, tuples, 1, ks.t)
    assert hook == dict(checked=1, passed=1, exact_tuples=0, exact_shares=0)
    assert got[0] == bytes(6) and got[1] == b"\0" and got[3] == [0x1F] and got[4] == [6]
    assert got[2] == TM.signature_under(tuples[0][0], ks.f0)
    exact = TG.combine(eng, tuples, 1, ks.t)
    assert list(exact[0]) == [0, 9, 0, 9, 0, 0] and exact[1] == b"\x09" and exact[3] == [0x35] and exact[4] == [4]


ROUTES = [("sliced", {E.OPT_MAX_CHUNK: 3}), ("all_waves", {E.OPT_COLLECT_WAVE_MIN_SHARES: 1}), ("lane_pairs", SMALL_OFF)]


@pytest.mark.parametrize("route", [r[0] for r in ROUTES])
def test_routes_give_the_same_bytes(eng, c, sets, route):
    """8. test 1's call with tuples and shares in pieces of 3, with every sum on a wave, and with the tuple check on lane pairs"""
    ks = sets["dealt9_t5"]
    use(eng, ks, ks.gk)
    m, sigs = expectation(sets, c, eng, "dealt9_t5")
    got, hook = opt(eng, ks.tuples, ks.bm_words, ks.t, opts=dict(ROUTES)[route])
    hold(got, hook, m, sigs, route)


@pytest.mark.parametrize("count", [1, 7, 14, 16])
def test_tuple_counts_of_every_layout(eng, c, sets, count):
    """8. the first `count` tuples of test 1: the tuple check on each layout of the routing table"""
    ks = sets["dealt9_t5"]
    use(eng, ks, ks.gk)
    m, sigs = expectation(sets, c, eng, "dealt9_t5")
    tuples = ks.tuples[:count]
    n_sh = sum(len(t[1]) for t in tuples)
    flags = m["flags"][:count]
    exact = [i for i in range(count) if flags[i] == OM.EXACT or (flags[i] == OM.CHECK and m["verdicts"][i] != 0)]
    part = dict(share_status=m["share_status"][:n_sh], tuple_status=m["tuple_status"][:count], rows=m["rows"][:count], counts=m["counts"][:count],
                hook=dict(checked=flags.count(OM.CHECK), passed=sum(1 for i in range(count) if flags[i] == OM.CHECK and m["verdicts"][i] == 0),
                          exact_tuples=len(exact), exact_shares=sum(1 for s in m["queue"] if s < n_sh)))
    got, hook = opt(eng, tuples, ks.bm_words, ks.t)
    hold(got, hook, part, sigs[:count], count)


def test_whole_call_routing(eng, c, sets):
    """9. below the default, with BN254_OPT_PAIR_LANES 0 and with no keys registered the call IS the exact call; no group key is a bad
    argument; a registration forgets the group key; a key off the curve reports the decoder's status and leaves none set"""
    ks = sets["dealt9_t5"]
    use(eng, ks, ks.gk)
    msgs, shares, keys, sizes = TG.flat(ks.tuples)
    call = lambda bm=ks.bm_words: eng.batch_threshold_combine_keyed_optimistic(msgs, b"".join(shares), keys, sizes, bm, ks.t)   # noqa: E731
    assert len(keys) < E.THRESHOLD_OPT_MIN_SHARES_DEFAULT or E.THRESHOLD_OPT_MIN_SHARES_DEFAULT == 0
    if len(keys) < E.THRESHOLD_OPT_MIN_SHARES_DEFAULT:
        assert call() == ks.exact and eng.debug_threshold_opt_last() == ZERO_HOOK
    got = with_options(eng, {E.OPT_THRESHOLD_OPT_MIN_SHARES: 0, E.OPT_PAIR_LANES: 0}, lambda: (call(), eng.debug_threshold_opt_last()))
    assert got == (ks.exact, ZERO_HOOK)
    got, hook = opt(eng, ks.tuples, ks.bm_words, ks.t)                     # the route does run on this context
    assert hook["passed"] == len(PASSING)
    assert TG.combine(eng, ks.tuples, ks.bm_words, ks.t) == ks.exact and eng.debug_threshold_opt_last() == ZERO_HOOK   # ... and the exact call resets the hook
    try:
        eng.register_keys(b"")
        assert eng.set_group_key(ks.gk) == 0
        got = with_options(eng, FORCE, lambda: (call(0), eng.debug_threshold_opt_last()))
        assert got == (TG.combine(eng, ks.tuples, 0, ks.t), ZERO_HOOK) and got[0][1] == bytes([9]) * len(msgs)
    finally:
        ks.register(eng)
    # the registration forgot the group key
    for forced in (FORCE, {}):
        with pytest.raises(E.NativeError) as e:
            with_options(eng, forced, call)
        assert e.value.rc == -10001
    assert eng.set_group_key(ks.gk) == 0 and call() is not None
    assert eng.set_group_key(None) == 0
    with pytest.raises(E.NativeError) as e:
        call()
    assert e.value.rc == -10001
    off_curve = bytearray(ks.gk); off_curve[100] ^= 2
    assert eng.set_group_key(ks.gk) == 0
    assert eng.set_group_key(bytes(off_curve)) == c.g2_validate(bytes(off_curve)) != 0
    with pytest.raises(E.NativeError) as e:
        call()
    assert e.value.rc == -10001


@pytest.mark.parametrize("name", ["dealt9_t5", "dealt70_t64", "dealt9_t9"])
def test_device_form(eng, c, sets, name):
    """10. the _device form on a caller's stream: the host form's bytes and counters; behind a larger call (a stale workspace); without the
    n_valid array; misaligned pointers refused; no group key refused"""
    from tests.hip_ctypes import DevBuf, Stream
    big = sets["dealt70_t64"]
    use(eng, big, big.gk)
    opt(eng, big.tuples, big.bm_words, big.t)                              # leaves a larger workspace and scratch behind
    ks = sets[name]
    use(eng, ks, ks.gk)
    m, sigs = expectation(sets, c, eng, name)
    msgs, shares, keys, sizes = TG.flat(ks.tuples)
    n, n_shares, bm = len(msgs), len(keys), ks.bm_words
    blob, off = E.pack_messages(msgs)
    soff = [sum(sizes[:i]) for i in range(n + 1)]
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    words = lambda raw, k: [int.from_bytes(raw[4 * j:4 * j + 4], "little") for j in range(k)]   # noqa: E731
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_msgs, d_moff, d_shares, d_keys, d_soff = dev(bytes(blob)), dev(u64(off)), dev(b"".join(shares)), dev(u32(keys) + bytes(4)), dev(u64(soff))
        d_sst, d_tst, d_sig, d_bits, d_cnt = dev(nbytes=n_shares + 4), dev(nbytes=n), dev(nbytes=64 * n + 4), dev(nbytes=4 * bm * n), dev(nbytes=4 * n)

        def run(with_counts=True, keys_ptr=None, sig_ptr=None):
            for b in (d_sst, d_tst, d_sig, d_bits, d_cnt):
                b.upload(b"\xEE" * b.nbytes)
            eng.batch_threshold_combine_keyed_optimistic_device(d_msgs.ptr, d_moff.ptr, d_shares.ptr, keys_ptr or d_keys.ptr, d_soff.ptr, n_shares, n, bm, ks.t,
                                                                d_sst.ptr, d_tst.ptr, sig_ptr or d_sig.ptr, d_bits.ptr, d_cnt.ptr if with_counts else None,
                                                                stream=stream.handle)
            stream.synchronize()
            return (d_sst.download(n_shares), d_tst.download(n), d_sig.download(64 * n), words(d_bits.download(4 * bm * n), bm * n),
                    words(d_cnt.download(4 * n), n)), eng.debug_threshold_opt_last()
        got, hook = with_options(eng, FORCE, run)
        hold(got, hook, m, sigs, (name, "device"))
        assert got == opt(eng, ks.tuples, bm, ks.t)[0]
        sliced, hook = with_options(eng, {**FORCE, E.OPT_MAX_CHUNK: 3}, run)
        hold(sliced, hook, m, sigs, (name, "device, sliced"))
        bare, hook = with_options(eng, FORCE, lambda: run(with_counts=False))
        assert bare[:4] == got[:4] and bare[4] == [0xEEEEEEEE] * n and hook == m["hook"]
        for kwargs in ({"keys_ptr": d_keys.ptr + 1}, {"sig_ptr": d_sig.ptr + 2}):
            with pytest.raises(E.NativeError) as e:
                with_options(eng, FORCE, lambda: run(**kwargs))
            assert e.value.rc == -10002, kwargs
        assert eng.set_group_key(None) == 0
        with pytest.raises(E.NativeError) as e:
            with_options(eng, FORCE, run)
        assert e.value.rc == -10001
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


def test_stage_intervals(eng, c, sets):
    """10. under profiling: four non-negative intervals; when nothing fails the exact fallback's interval is small beside the tuple check's
    (both run the Miller loop and final exponentiation kernels; the fallback's find an empty queue and leave at once)"""
    ks = sets["dealt9_t5"]
    use(eng, ks, ks.gk)
    names = [s[0] for s in ks.shapes]
    tuples = [ks.tuples[names.index(k)] for k in PASSING]
    try:
        eng.set_profiling(True)
        got, hook = opt(eng, tuples, ks.bm_words, ks.t)
        ms = eng.last_kernel_ms()
    finally:
        eng.set_profiling(False)
    print("threshold optimistic ms", ms)
    assert hook == dict(checked=len(PASSING), passed=len(PASSING), exact_tuples=0, exact_shares=0) and got[1] == bytes(len(PASSING))
    assert len(ms) == 4 and all(v >= 0 for v in ms.values())
    front, weighted, check_ms, fallback = ms["decode"], ms["hash_to_g1"], ms["miller_loop"], ms["final_exp"]
    assert check_ms > 0 and weighted > 0 and front > 0
    # nothing fails: every kernel of the fallback finds an empty queue or a closed gate and leaves at once, while the tuple check walks seven
    # Miller loops and final exponentiations — so the fallback's interval is held against the tuple check's, not against a constant
    assert fallback < check_ms, ms


def test_python_and_cpp_mirrors(eng, sets, tmp_path):
    """11. ECDSA.register_group_key / threshold_combine_keyed_optimistic on three tuples, and host/threshold_example.cpp (which runs the
    optimistic call through bn254.hpp) built with -Wall -Werror"""
    from bn254_amd import _native
    from bn254_amd.api import ECDSA, Error, ErrorKind, PrivateKey, PublicKey, Signature, threshold_deal
    secret = PrivateKey(0x5EDB << 200)
    sks = threshold_deal(secret.value, 3, 5, seed=2027)
    pks = [PublicKey(raw) for raw in TG.derive(eng, [k.value for k in sks])]
    try:
        assert ECDSA.register_keys(pks, engine=eng) == [None] * 5
        with pytest.raises(ValueError):
            ECDSA.threshold_combine_keyed_optimistic(b"m", [], [], 3, engine=eng)
        gk = ECDSA.threshold_group_key([0, 2, 4], [pks[0], pks[2], pks[4]], engine=eng)
        ECDSA.register_group_key(gk, engine=eng)
        msg = b"height 1001"
        sig_raw, st = eng.batch_sign([msg] * 5, b"".join(k.to_bytes() for k in sks))
        shares = [Signature(sig_raw[64 * j:64 * j + 64]) for j in range(5)]
        items = [(msg, shares, range(5)), (msg, [shares[4], shares[1], shares[0], shares[3]], [4, 1, 2, 3]), (b"other", [], [])]
        res = with_options(eng, FORCE, lambda: ECDSA.batch_threshold_combine_keyed_optimistic(items, 3, engine=eng))
        assert eng.debug_threshold_opt_last() == dict(checked=2, passed=1, exact_tuples=2, exact_shares=4)
        want = ECDSA.batch_threshold_combine_keyed(items, 3, engine=eng)
        assert res[0][0].raw == want[0][0].raw == TM.signature_under(msg, secret.value) and res[0][1] == [0, 1, 2] and res[0][2] == [None] * 5
        assert res[1][0].raw == want[1][0].raw and res[1][1] == want[1][1] == [1, 3, 4] and res[1][2] == want[1][2]
        assert res[2].kind == want[2].kind == ErrorKind.VerificationFailed and res[2].signers == []
        sigma = with_options(eng, FORCE, lambda: ECDSA.threshold_combine_keyed_optimistic(msg, shares, range(5), 3, engine=eng))
        assert sigma[0].raw == res[0][0].raw
        bad = bytearray(gk.raw); bad[100] ^= 2
        with pytest.raises(Error):
            ECDSA.register_group_key(PublicKey(bytes(bad)), engine=eng)
        with pytest.raises(ValueError):
            ECDSA.threshold_combine_keyed_optimistic(msg, shares, range(5), 3, engine=eng)
    finally:
        sets["dealt9_t5"].register(eng)
    host = os.path.join(ROOT, "bn254_amd", "host")
    exe = str(tmp_path / "threshold_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", host,
                           os.path.join(host, "threshold_example.cpp"), "-o", exe, _native.LIB_PATH, "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "threshold signatures: ok" in out.stdout and "optimistic: ok" in out.stdout
