"""The segmented scalar-weighted sum in G2 and the check of a dealing (include/bn254_hip.h: bn254_batch_g2_msm[_device],
bn254_ctx_check_dealing, bn254_debug_dealing_coefficients) on the GPU.
The sum: the defining identity — byte for byte bn254_batch_g2_mul followed by bn254_batch_g2_sum of the products — on a ragged batch of
segments of 0, 1, 2, 15, 16, 17, 63, 64, 65 and 129 terms (both layouts of the sum by size and forced by the option; the segments straddle
the term kernel's waves), with the scalars 0, 1, r - 1, r and 2^256 - 1 under both reduce_scalar values and identity points; the model's sum
on the short segments; a bad point first, in the middle and last; the _device form with a reversed and an over-long segment and misaligned
pointers; a workspace left by a verify.
The check: the whole case set of tests/dealing_cases.py under three seeds against tests/dealing_model.py, K against
ECDSA.threshold_group_key and the model; the coefficient hook against the model; the closed loop into the optimistic threshold combine; a
re-registration; argument errors; the Python and C++ mirrors.  Run on the MI355X box: -m gpu."""
import ctypes
import os
import random
import subprocess

import pytest

from bn254_amd import engine as E
from tests import dealing_cases as DC
from tests import dealing_model as DM
from tests import threshold_model as TM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = DC.R
SIZES = DC.SEGMENT_LENGTHS + [0, 3]
BAD_ARGUMENT, MISALIGNED = -10001, -10002


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


def be(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def derive(eng, secrets):
    """pk_j = s_j * G2::one() by the fixed-base route of bn254_batch_g2_mul (0 gives the identity: 128 zero bytes)"""
    out, st = eng.batch_g2_mul(None, be(s % R for s in secrets), len(secrets))
    assert st == bytes(len(secrets))
    return [out[128 * j:128 * j + 128] for j in range(len(secrets))]


def with_wave_min(eng, value, fn):
    try:
        eng.set_option(E.OPT_COLLECT_WAVE_MIN_SHARES, value)
        return fn()
    finally:
        eng.set_option(E.OPT_COLLECT_WAVE_MIN_SHARES, 16)


# ---- bn254_batch_g2_msm -------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def terms(eng):
    """every segment's points (multiples of the generator; every 11th the identity), their multipliers, and two scalar sets: below r with every
    7th zero, and the edge scalars in turn"""
    rnd = random.Random(32)
    m = sum(SIZES)
    a = [0 if s % 11 == 5 else rnd.randrange(1, R) for s in range(m)]
    pts = derive(eng, a)
    small = [0 if s % 7 == 3 else rnd.randrange(R) for s in range(m)]
    edge = [DC.EDGE_SCALARS[s % 5] for s in range(m)]
    seg = [0]
    for k in SIZES:
        seg.append(seg[-1] + k)
    return pts, a, small, edge, seg


def mul_then_sum(eng, pts, scalars, seg, reduce):
    prod, st = eng.batch_g2_mul(b"".join(pts), be(scalars), len(pts), reduce_scalar=reduce)
    assert st == bytes(len(pts))
    return eng.batch_g2_sum(prod, seg)


@pytest.mark.parametrize("scalars,reduce", [("small", False), ("small", True), ("edge", False), ("edge", True)])
def test_defining_identity_both_layouts(eng, terms, scalars, reduce):
    pts, a, small, edge, seg = terms
    ks = small if scalars == "small" else edge
    want = mul_then_sum(eng, pts, ks, seg, reduce)
    assert want[1] == bytes(len(SIZES)) and want[0][:128] == bytes(128) and want[0][128 * 10:128 * 11] == bytes(128)      # the empty segments
    got = eng.batch_g2_msm(b"".join(pts), be(ks), seg, reduce_scalar=reduce)
    assert got == want, [i for i in range(len(SIZES)) if got[0][128 * i:128 * i + 128] != want[0][128 * i:128 * i + 128]]
    assert with_wave_min(eng, 1, lambda: eng.batch_g2_msm(b"".join(pts), be(ks), seg, reduce_scalar=reduce)) == want
    assert with_wave_min(eng, 1 << 30, lambda: eng.batch_g2_msm(b"".join(pts), be(ks), seg, reduce_scalar=reduce)) == want
    # the points are multiples of the generator: every sum is (sum k_s a_s) * G2::one()
    sums = [sum(k * v for k, v in zip(ks[seg[i]:seg[i + 1]], a[seg[i]:seg[i + 1]])) % R for i in range(len(SIZES))]
    assert got[0] == b"".join(derive(eng, sums))


def test_against_the_model_and_degenerate_batches(eng, terms):
    """the segments of 1, 2 and 3 terms against group arithmetic in Python integers; all-zero scalars, all-identity points, no terms"""
    pts, _, small, edge, seg = terms
    got, st = eng.batch_g2_msm(b"".join(pts), be(small), seg)
    for i in (1, 2, 11):
        lo, hi = seg[i], seg[i + 1]
        assert got[128 * i:128 * i + 128] == DM.g2_weighted_sum(pts[lo:hi], small[lo:hi]), i
    n = len(SIZES)
    assert eng.batch_g2_msm(b"".join(pts), bytes(32 * len(pts)), seg) == (bytes(128 * n), bytes(n))
    assert eng.batch_g2_msm(bytes(128 * len(pts)), be(small), seg) == (bytes(128 * n), bytes(n))
    assert eng.batch_g2_msm(b"", b"", [0, 0, 0]) == (bytes(256), bytes(2))
    assert eng.batch_g2_msm(b"", b"", [0]) == (b"", b"")


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_bad_point_in_a_segment(eng, terms, where):
    """a point off the curve in every non-empty segment: status 4 and the identity; a second, different fault behind it does not change the
    status (the first in segment order wins) — in the lane layout and in the wave layout, where another lane meets the later fault first"""
    pts, _, small, _, seg = terms
    bad = list(pts)
    for i, k in enumerate(SIZES):
        if k == 0:
            continue
        at = seg[i] + {"first": 0, "middle": k // 2, "last": k - 1}[where]
        bad[at] = DC.plant(pts[at], "curve")
        if where != "last" and k > 2:
            bad[seg[i + 1] - 1] = DC.plant(pts[seg[i + 1] - 1], "big")          # a coordinate >= q: status 6, later in the segment
    want_st = bytes(4 if k else 0 for k in SIZES)
    for wave_min in (16, 1, 1 << 30):
        out, st = with_wave_min(eng, wave_min, lambda: eng.batch_g2_msm(b"".join(bad), be(small), seg))
        assert st == want_st and out == bytes(128 * len(SIZES)), (where, wave_min, list(st))
    # bn254_batch_g2_sum's own rule on the same points
    assert eng.batch_g2_sum(b"".join(bad), seg)[1] == want_st


def test_device_form_and_stale_workspace(eng, terms):
    """the host form's bytes on a caller's stream, behind a verify that left its workspace; a reversed segment and one past the terms read 2
    with the identity and leave the other segments alone; misaligned pointers are refused; n == 0 returns at once"""
    from tests.datagen import make_verify_batch
    from tests.hip_ctypes import DevBuf, Stream
    pts, _, small, _, seg = terms
    n, m = len(SIZES), len(pts)
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    host = eng.batch_g2_msm(b"".join(pts), be(small), seg)
    msgs, sigs, pks, expected = make_verify_batch(eng, 64, corrupt_every=8)
    assert eng.batch_verify(msgs, sigs, pks, flags=0) == bytes(expected)
    assert eng.batch_g2_msm(b"".join(pts), be(small), seg) == host
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_pts, d_k = dev(b"".join(pts) + bytes(4)), dev(be(small) + bytes(4))
        d_out, d_st = dev(nbytes=128 * n + 4), dev(nbytes=n)

        def run(offsets, p_ptr=None, k_ptr=None, o_ptr=None):
            d_seg = dev(u64(offsets))
            eng.batch_g2_msm_device(p_ptr or d_pts.ptr, k_ptr or d_k.ptr, d_seg.ptr, n, o_ptr or d_out.ptr, d_st.ptr, stream=stream.handle)
            stream.synchronize()
            return d_out.download(128 * n), d_st.download(n)
        assert run(seg) == host
        rev = list(seg)
        rev[3] = seg[2] - 1                          # segment 2 reversed; segment 3 then starts early and is the longer for it
        out, st = run(rev)
        assert st[2] == 2 and out[256:384] == bytes(128) and st[:2] == bytes(2) and st[4:] == bytes(n - 4) and out[:256] == host[0][:256]
        assert out[128 * 4:] == host[0][128 * 4:]
        past = list(seg)
        past[4] = m + 1                              # segment 3 runs past the terms, and segment 4 starts there: both refused
        out, st = run(past)
        assert st[3] == 2 and st[4] == 2 and out[128 * 3:128 * 5] == bytes(256) and out[:128 * 3] == host[0][:128 * 3]
        assert out[128 * 5:] == host[0][128 * 5:] and st[5:] == bytes(n - 5)
        for kw in ({"p_ptr": d_pts.ptr + 1}, {"k_ptr": d_k.ptr + 2}, {"o_ptr": d_out.ptr + 3}):
            with pytest.raises(E.NativeError) as e:
                run(seg, **kw)
            assert e.value.rc == MISALIGNED
        eng.batch_g2_msm_device(None, None, None, 0, None, None, stream=stream.handle)
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


# ---- bn254_ctx_check_dealing --------------------------------------------------------------------------------------------------------------------------
def register_case(eng, cs):
    """the case's keys registered as the case says -> (the keys' bytes, their registration statuses)"""
    keys = derive(eng, cs["secrets"])
    for at, kind in cs["faults"].items():
        keys[at] = DC.plant(keys[at], kind)
    if cs["pop_fail"] is None:
        return keys, eng.register_keys(b"".join(keys))
    pks, pops, st = eng.batch_pop_prove(be(cs["secrets"]))
    assert st == bytes(len(keys)) and pks == b"".join(keys)
    at = cs["pop_fail"]
    _, wrong, st = eng.batch_pop_prove(be([(cs["secrets"][at] + 1) % R]))          # a well-formed proof, of another key
    assert st == bytes(1)
    return keys, eng.register_keys_pop(pks, pops[:64 * at] + wrong + pops[64 * at + 64:])


@pytest.mark.parametrize("shape", DC.SHAPES + DC.DEVICE_ONLY_SHAPES, ids=lambda s: "%dof%d" % (s[1], s[0]))
def test_case_set(eng, shape):
    from bn254_amd.api import ECDSA, PublicKey
    n, t = shape
    seen = set()
    for cs in DC.cases_for(n, t):
        keys, key_st = register_case(eng, cs)
        answers = [eng.check_dealing(cs["t"], seed) for seed in DC.SEEDS]
        assert len(set(answers)) == 1, (cs["name"], [a[1:] for a in answers])
        pk, st, bad = answers[0]
        want_st, want_bad, k_scalar = DM.check_scalars(cs["secrets"], list(key_st), cs["t"], DC.SEEDS[0])
        assert (st, bad) == (want_st, want_bad), cs["name"]
        if cs["expect"] == "pass":
            assert st == 0 and bad == DM.NO_KEY and pk == derive(eng, [k_scalar])[0], cs["name"]
            assert pk == ECDSA.threshold_group_key(range(cs["t"]), [PublicKey(k) for k in keys[:cs["t"]]], engine=eng).raw, cs["name"]
            lam = TM.lagrange_at_zero(list(range(1, cs["t"] + 1)))
            assert pk == eng.batch_g2_msm(b"".join(keys[:cs["t"]]), be(lam), [0, cs["t"]])[0], cs["name"]
            if n <= 5:
                assert pk == DM.group_key(keys, cs["t"]), cs["name"]
        elif cs["expect"] == "fail":
            assert st == 9 and bad == DM.NO_KEY and pk == bytes(128), cs["name"]
        else:
            _, at, status = cs["expect"]
            assert key_st[at] != 0 and (status is None or key_st[at] == status), (cs["name"], list(key_st))
            assert (st, bad) == (key_st[at], at) and pk == bytes(128), cs["name"]
        seen.add(cs["name"])
    assert {"honest", "zero_polynomial", "threshold_1_equal_keys", "fault_lowest", "pop_failed", "threshold_n_plus_1"} <= seen
    if n > t:
        assert {"degree_t", "replaced_high", "replaced_low", "cancelling_pair"} <= seen


def test_coefficient_hook_against_the_model(eng):
    shapes = DC.SHAPES + DC.DEVICE_ONLY_SHAPES + [(n, 1) for n, _ in DC.SHAPES] + [(n, n) for n, _ in DC.SHAPES] + DC.random_shapes(6, 300, 43)
    for n, t in shapes:
        seed = DC.SEEDS[(n + t) % 3]
        raw = eng.debug_dealing_coefficients(n, t, seed)
        got = [int.from_bytes(raw[32 * j:32 * j + 32], "big") for j in range(n)]
        assert got == DM.coefficients(n, t, seed), (n, t)
    for n, t in ((0, 1), (3, 0), (3, 4)):
        with pytest.raises(E.NativeError) as e:
            eng.debug_dealing_coefficients(n, t, DC.SEEDS[0])
        assert e.value.rc == BAD_ARGUMENT


def test_closed_loop_into_the_optimistic_combine(eng):
    """a dealt committee: check_dealing(register=True) names the group key; the optimistic threshold combine then sends no tuple the exact
    way, and the group signature verifies under K"""
    from bn254_amd.api import ECDSA, PrivateKey, PublicKey, Signature, threshold_deal
    secret = PrivateKey(0xDEA1 << 190)
    sks = threshold_deal(secret.value, 5, 9, seed=2028)
    pks = [PublicKey(raw) for raw in derive(eng, [k.value for k in sks])]
    assert ECDSA.register_keys(pks, engine=eng) == [None] * 9
    assert not eng.group_key_set
    gk = ECDSA.check_dealing(5, engine=eng, register=True)                 # a seed from os.urandom
    assert eng.group_key_set and gk.raw == derive(eng, [secret.value])[0]
    msgs = [b"height %d" % h for h in range(3)]
    items = []
    for msg in msgs:
        sig_raw, st = eng.batch_sign([msg] * 9, b"".join(k.to_bytes() for k in sks))
        assert st == bytes(9)
        items.append((msg, [Signature(sig_raw[64 * j:64 * j + 64]) for j in range(9)], range(9)))
    try:
        eng.set_option(E.OPT_THRESHOLD_OPT_MIN_SHARES, 0)
        res = ECDSA.batch_threshold_combine_keyed_optimistic(items, 5, engine=eng)
        hook = eng.debug_threshold_opt_last()
    finally:
        eng.set_option(E.OPT_THRESHOLD_OPT_MIN_SHARES, E.THRESHOLD_OPT_MIN_SHARES_DEFAULT)
    assert hook == dict(checked=3, passed=3, exact_tuples=0, exact_shares=0)
    sigs = b"".join(r[0].raw for r in res)
    assert eng.batch_verify(msgs, sigs, gk.raw * 3, flags=0) == bytes(3)
    assert all(r[0].raw == TM.signature_under(m, secret.value) for r, m in zip(res, msgs))
    # the call does not install the key by itself, and a registration forgets it
    assert ECDSA.register_keys(pks, engine=eng) == [None] * 9 and not eng.group_key_set
    assert ECDSA.check_dealing(5, seed=DC.SEEDS[1], engine=eng).raw == gk.raw and not eng.group_key_set


def test_reregistration_profiling_and_argument_errors(eng):
    rnd = random.Random(5)
    a = TM.deal(DC.poly(rnd, 2), 7)
    b = list(a)
    b[5] = (b[5] + 1) % R
    c = TM.deal(DC.poly(rnd, 2), 4)
    seed = DC.SEEDS[1]
    assert eng.register_keys(b"".join(derive(eng, a))) == bytes(7)
    k_a = eng.check_dealing(3, seed)
    assert k_a[1:] == (0, DM.NO_KEY) and k_a[0] == derive(eng, [DM.check_scalars(a, [0] * 7, 3, seed)[2]])[0]
    assert eng.register_keys(b"".join(derive(eng, b))) == bytes(7)
    assert eng.check_dealing(3, seed) == (bytes(128), 9, DM.NO_KEY)
    assert eng.register_keys(b"".join(derive(eng, c))) == bytes(4)
    eng.set_profiling(True)
    try:
        k_c = eng.check_dealing(3, seed)
        ms = list(eng.last_kernel_ms().values())
    finally:
        eng.set_profiling(False)
    assert k_c[1:] == (0, DM.NO_KEY) and k_c[0] != k_a[0] and k_c[0] == derive(eng, [DM.check_scalars(c, [0] * 4, 3, seed)[2]])[0]
    assert len(ms) == 4 and all(v >= 0 for v in ms) and ms[1] > 0          # coefficients, terms, sums, verdict: the ladders take time
    # argument errors: threshold 0, flags, NULL seed / key / status; bad_key may be NULL; a context without keys
    lib, h = eng._lib, eng._h
    pk, st, bad = ctypes.create_string_buffer(128), ctypes.create_string_buffer(1), ctypes.c_uint32(7)
    call = lib.bn254_ctx_check_dealing
    assert call(h, 0, seed, 0, pk, st, ctypes.byref(bad)) == BAD_ARGUMENT
    assert call(h, 3, seed, 1, pk, st, ctypes.byref(bad)) == BAD_ARGUMENT
    assert call(h, 3, None, 0, pk, st, ctypes.byref(bad)) == BAD_ARGUMENT
    assert call(h, 3, seed, 0, None, st, ctypes.byref(bad)) == BAD_ARGUMENT
    assert call(h, 3, seed, 0, pk, None, ctypes.byref(bad)) == BAD_ARGUMENT
    assert bad.value == 7 and st.raw == b"\0" and pk.raw == bytes(128)     # nothing written by a refused call
    assert call(h, 3, seed, 0, pk, st, None) == 0 and st.raw == b"\0" and pk.raw == k_c[0]
    assert eng.register_keys(b"") == b""
    assert call(h, 1, seed, 0, pk, st, ctypes.byref(bad)) == BAD_ARGUMENT


def test_python_and_cpp_mirrors(eng, tmp_path):
    """ECDSA.g2_msm and ECDSA.check_dealing with their errors, and host/dealing_example.cpp (both calls through bn254.hpp) built with -Wall -Werror"""
    from bn254_amd import _native
    from bn254_amd.api import ECDSA, Error, ErrorKind, PublicKey, threshold_deal
    sks = threshold_deal(0x5EDC << 200, 3, 5, seed=2029)
    raw = derive(eng, [k.value for k in sks])
    pks = [PublicKey(r) for r in raw]
    assert ECDSA.register_keys(pks, engine=eng) == [None] * 5
    gk = ECDSA.check_dealing(3, seed=DC.SEEDS[2], engine=eng)
    assert gk.raw == derive(eng, [0x5EDC << 200])[0] == ECDSA.threshold_group_key([0, 2, 4], [pks[0], pks[2], pks[4]], engine=eng).raw
    assert ECDSA.g2_msm(pks[:3], [3, -3, 1], engine=eng).raw == gk.raw
    assert ECDSA.g2_msm([], [], engine=eng).raw == bytes(128)
    with pytest.raises(Error) as e:
        ECDSA.g2_msm([PublicKey(DC.plant(raw[0], "curve"))], [1], engine=eng)
    assert e.value.kind == ErrorKind.InvalidGroupPoint
    with pytest.raises(Error) as e:
        ECDSA.check_dealing(2, engine=eng)
    assert e.value.kind == ErrorKind.VerificationFailed and e.value.key is None
    with pytest.raises(ValueError):
        ECDSA.check_dealing(0, engine=eng)
    with pytest.raises(Error):
        ECDSA.check_dealing(3, seed=b"short", engine=eng)
    st = ECDSA.register_keys(pks[:2] + [PublicKey(DC.plant(raw[2], "curve"))] + pks[3:], engine=eng)
    assert st[2] is not None and st[:2] == [None, None]
    with pytest.raises(Error) as e:
        ECDSA.check_dealing(3, engine=eng, register=True)
    assert e.value.kind == st[2].kind and e.value.key == 2 and not eng.group_key_set
    host = os.path.join(ROOT, "bn254_amd", "host")
    exe = str(tmp_path / "dealing_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", host,
                           os.path.join(host, "dealing_example.cpp"), "-o", exe, _native.LIB_PATH, "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "dealing check: ok" in out.stdout
