"""The segmented scalar-weighted sum in G1 (include/bn254_hip.h: bn254_batch_g1_msm[_device]) on the GPU.  The defining identity — byte for
byte bn254_batch_g1_mul followed by bn254_batch_g1_sum of the products — on segments of 0, 1, 63, 64, 65 and 200 terms in both layouts of
the sum (by size and forced by the option), with zero scalars, scalars >= r with and without reduce_scalar, and identity points; the model's
sum (tests/threshold_model.py) on the short segments; a bad point first, in the middle and last in a segment; the _device form with a
refused segment.  Run on the MI355X box: -m gpu."""
import random

import pytest

from bn254_amd import engine as E
from tests import threshold_model as TM

pytestmark = pytest.mark.gpu
R = TM.R
SIZES = [0, 1, 63, 64, 65, 0, 200, 2]


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def terms(eng):
    """every segment's points (multiples of the generator; every 11th the identity) and three scalar sets: below r with every 7th zero,
    and at or above r"""
    rnd = random.Random(31)
    m = sum(SIZES)
    pts, st = eng.batch_g1_mul(None, b"".join(rnd.randrange(1, R).to_bytes(32, "big") for _ in range(m)), m, reduce_scalar=True)
    assert st == bytes(m)
    pts = [bytes(64) if s % 11 == 5 else pts[64 * s:64 * s + 64] for s in range(m)]
    small = [0 if s % 7 == 3 else rnd.randrange(R) for s in range(m)]
    big = [R + rnd.randrange(1000) if s % 2 else (1 << 256) - 1 - rnd.randrange(1000) for s in range(m)]
    seg = [0]
    for k in SIZES:
        seg.append(seg[-1] + k)
    return pts, small, big, seg


def be(values):
    return b"".join(v.to_bytes(32, "big") for v in values)


def mul_then_sum(eng, pts, scalars, seg, reduce):
    prod, st = eng.batch_g1_mul(b"".join(pts), be(scalars), len(pts), reduce_scalar=reduce)
    assert st == bytes(len(pts))
    return eng.batch_g1_sum(prod, seg)


def with_wave_min(eng, value, fn):
    try:
        eng.set_option(E.OPT_COLLECT_WAVE_MIN_SHARES, value)
        return fn()
    finally:
        eng.set_option(E.OPT_COLLECT_WAVE_MIN_SHARES, 16)


def test_defining_identity_both_layouts(eng, terms):
    pts, small, big, seg = terms
    for scalars, reduce in ((small, False), (small, True), (big, False), (big, True)):
        want = mul_then_sum(eng, pts, scalars, seg, reduce)
        assert want[1] == bytes(len(SIZES)) and want[0][:64] == bytes(64) and want[0][64 * 5:64 * 6] == bytes(64)      # the empty segments
        got = eng.batch_g1_msm(b"".join(pts), be(scalars), seg, reduce_scalar=reduce)
        assert got == want, [i for i in range(len(SIZES)) if got[0][64 * i:64 * i + 64] != want[0][64 * i:64 * i + 64]]
        assert with_wave_min(eng, 1, lambda: eng.batch_g1_msm(b"".join(pts), be(scalars), seg, reduce_scalar=reduce)) == want
        assert with_wave_min(eng, 1 << 30, lambda: eng.batch_g1_msm(b"".join(pts), be(scalars), seg, reduce_scalar=reduce)) == want
    # a raw scalar acts mod r: reduced or not, the same points
    assert eng.batch_g1_msm(b"".join(pts), be(big), seg) == eng.batch_g1_msm(b"".join(pts), be([k % R for k in big]), seg)


def test_against_the_model(eng, terms):
    """the segments of 1, 63 and 65 terms (one lane; a wave with one lane idle; a wave whose first lane takes two) against Python integers"""
    pts, small, big, seg = terms
    got, st = eng.batch_g1_msm(b"".join(pts), be(small), seg)
    for i in (1, 2, 4, 7):
        lo, hi = seg[i], seg[i + 1]
        assert got[64 * i:64 * i + 64] == TM.weighted_sum(pts[lo:hi], small[lo:hi]), i
    lo, hi = seg[1], seg[2]
    assert eng.batch_g1_msm(b"".join(pts[lo:hi]), be(big[lo:hi]), [0, 1])[0] == TM.weighted_sum(pts[lo:hi], [big[lo] % R])


def test_all_zero_scalars_and_all_identity_points(eng, terms):
    pts, small, _, seg = terms
    n = len(SIZES)
    assert eng.batch_g1_msm(b"".join(pts), bytes(32 * len(pts)), seg) == (bytes(64 * n), bytes(n))
    assert eng.batch_g1_msm(bytes(64 * len(pts)), be(small), seg) == (bytes(64 * n), bytes(n))
    assert eng.batch_g1_msm(b"", b"", [0, 0, 0]) == (bytes(128), bytes(2))
    assert eng.batch_g1_msm(b"", b"", [0]) == (b"", b"")


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_bad_point_in_a_segment(eng, terms, where):
    """a point off the curve in every non-empty segment: status 4 and the identity; a second, different fault behind it does not change the
    status (the first in segment order wins) — in the lane layout and in the wave layout, where another lane meets the later fault first"""
    pts, small, _, seg = terms
    bad = list(pts)
    for i, k in enumerate(SIZES):
        if k == 0:
            continue
        at = seg[i] + {"first": 0, "middle": k // 2, "last": k - 1}[where]
        p = bytearray(pts[at] if pts[at] != bytes(64) else pts[at - 1 if at > seg[i] else at + 1])
        p[40] ^= 4
        bad[at] = bytes(p)
        if where != "last" and k > 2:
            bad[seg[i + 1] - 1] = b"\xff" + bytes(pts[seg[i + 1] - 2][1:])          # a coordinate >= q: status 6, later in the segment
    want_st = bytes(4 if k else 0 for k in SIZES)
    for wave_min in (16, 1, 1 << 30):
        out, st = with_wave_min(eng, wave_min, lambda: eng.batch_g1_msm(b"".join(bad), be(small), seg))
        assert st == want_st and out == bytes(64 * len(SIZES)), (where, wave_min, list(st))
    # bn254_batch_g1_sum's own rule on the same points
    assert eng.batch_g1_sum(b"".join(bad), seg)[1] == want_st


def test_device_form(eng, terms):
    """the host form's bytes on a caller's stream; a reversed segment and one past the terms read 2 with the identity and leave the other
    segments alone; misaligned scalars are refused; n == 0 returns at once"""
    from tests.hip_ctypes import DevBuf, Stream
    pts, small, _, seg = terms
    n, m = len(SIZES), len(pts)
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    host = eng.batch_g1_msm(b"".join(pts), be(small), seg)
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_pts, d_k = dev(b"".join(pts)), dev(be(small) + bytes(4))
        d_out, d_st = dev(nbytes=64 * n), dev(nbytes=n)

        def run(offsets, k_ptr=None):
            d_seg = dev(u64(offsets))
            eng.batch_g1_msm_device(d_pts.ptr, k_ptr or d_k.ptr, d_seg.ptr, n, d_out.ptr, d_st.ptr, stream=stream.handle)
            stream.synchronize()
            return d_out.download(64 * n), d_st.download(n)
        assert run(seg) == host
        rev = list(seg)
        rev[3] = seg[2] - 1                          # segment 2 reversed; segment 3 then starts early and is the longer for it
        out, st = run(rev)
        assert st[2] == 2 and out[128:192] == bytes(64) and st[:2] == bytes(2) and st[4:] == bytes(n - 4) and out[:128] == host[0][:128]
        assert out[64 * 4:] == host[0][64 * 4:]
        past = list(seg)
        past[4] = m + 1                              # segment 3 runs past the terms, and segment 4 starts there: both refused
        out, st = run(past)
        assert st[3] == 2 and st[4] == 2 and out[64 * 3:64 * 5] == bytes(128) and out[:64 * 3] == host[0][:64 * 3]
        with pytest.raises(E.NativeError) as e:
            run(seg, k_ptr=d_k.ptr + 1)
        assert e.value.rc == -10002                  # BN254_E_MISALIGNED
        eng.batch_g1_msm_device(None, None, None, 0, None, None, stream=stream.handle)
    finally:
        for b in bufs:
            b.free()
        stream.destroy()
