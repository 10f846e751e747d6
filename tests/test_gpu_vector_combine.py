"""Vectors of G2 points combined column by column, one scalar per vector (include/bn254_hip.h: bn254_batch_g2_vector_combine[_device]) on the
GPU.  Every case of tests/reshare_cases.py — the shapes (d, len) from one term to 130 vectors, scalars 0, 1, r - 1 and >= r under both
reduce_scalar values, identity points, a column that sums through the identity, equal products, points outside the subgroup, decode faults in
the first, a middle and the last vector and two in one column — under the shipped split of the sums, the forced lane layout and the forced
wave layout (BN254_OPT_COLLECT_WAVE_MIN_SHARES): against tests/reshare_model.py (Python integers and the C oracle), byte for byte against
bn254_batch_g2_msm on the transposed input (the defining identity), and in the _device form on a caller's stream; d = 0 and len = 0; refused
arguments; the Python mirror.  Run on the MI355X box: -m gpu."""
import ctypes
import os
import re

import pytest

from bn254_amd import engine as E
from tests import reshare_cases as RC
from tests import reshare_model as RM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = RM.R
BAD_ARGUMENT, MISALIGNED = -10001, -10002
ZERO = bytes(128)
SPLITS = {"default": None, "lanes": 1 << 30, "waves": 1}


def split_default():
    text = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    return int(re.search(r"#define COLLECT_WAVE_MIN_SHARES_DEFAULT (\d+)", text).group(1))


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def be(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def chunks(raw, size=128):
    return [raw[i:i + size] for i in range(0, len(raw), size)]


@pytest.fixture(scope="module")
def cases(eng, c):
    """every case with its inputs as bytes and what the model says, computed once.  The points a * G2::one() come from the fixed-base route of
    bn254_batch_g2_mul, a call this feature does not touch; spot-checked against the oracle"""
    all_cases = RC.all_vc_cases()
    flat = [v for _, cs in all_cases if cs["points"] is None for row in cs["a"] for v in row]
    raw, st = eng.batch_g2_mul(None, be(flat), len(flat))
    assert st == bytes(len(flat))
    derived, at, out = chunks(raw), 0, []
    for shape, cs in all_cases:
        d, ln = shape
        if cs["points"] is None:
            pts = [derived[at + i * ln:at + (i + 1) * ln] for i in range(d)]
            at += d * ln
            assert pts[0][0] == RM.key_of(c, cs["a"][0][0])
        else:
            pts = [list(row) for row in cs["points"]]
        for (i, k), kind in cs["faults"].items():
            pts[i][k] = RM.DC.plant(pts[i][k], kind)
        out.append({"label": "%dx%d/%s" % (d, ln, cs["name"]), "d": d, "len": ln, "reduce": cs["reduce"], "vectors": b"".join(p for row in pts for p in row),
                    "transposed": b"".join(pts[i][k] for k in range(ln) for i in range(d)), "scalars": be(cs["scalars"]), "want": RM.vc_expected(c, cs)})
    return out


def with_split(eng, split, fn):
    try:
        if SPLITS[split] is not None:
            eng.set_option(E.OPT_COLLECT_WAVE_MIN_SHARES, SPLITS[split])
        return fn()
    finally:
        eng.set_option(E.OPT_COLLECT_WAVE_MIN_SHARES, split_default())


@pytest.mark.parametrize("split", list(SPLITS))
def test_case_set_model_identity_and_device_form(eng, cases, split):
    from tests.hip_ctypes import DevBuf, Stream
    biggest = max(len(cs["vectors"]) for cs in cases)
    stream = Stream()
    d_v, d_s, d_out, d_st = DevBuf(biggest + 4, fill=0), DevBuf(32 * 130 + 4, fill=0), DevBuf(128 * 50 + 4, fill=0xEE), DevBuf(64, fill=0xEE)

    def body():
        wrong, differ, device = [], [], []
        for cs in cases:
            d, ln = cs["d"], cs["len"]
            out, st = eng.batch_g2_vector_combine(cs["vectors"], cs["scalars"], d, ln, reduce_scalar=cs["reduce"])
            if [(s, v) for s, v in zip(st, chunks(out))] != cs["want"]:
                wrong.append(cs["label"])
            # the defining identity: ONE segment per column over the transposed points, the scalars 0 .. d-1 repeated
            if (out, st) != eng.batch_g2_msm(cs["transposed"], cs["scalars"] * ln, [k * d for k in range(ln + 1)], reduce_scalar=cs["reduce"]):
                differ.append(cs["label"])
            d_v.upload(cs["vectors"])
            d_s.upload(cs["scalars"])
            eng.batch_g2_vector_combine_device(d_v.ptr, d_s.ptr, d, ln, d_out.ptr, d_st.ptr, reduce_scalar=cs["reduce"], stream=stream.handle)
            stream.synchronize()
            if (d_out.download(128 * ln), d_st.download(ln)) != (out, st):
                device.append(cs["label"])
        return wrong, differ, device
    try:
        wrong, differ, device = with_split(eng, split, body)
    finally:
        for b in (d_v, d_s, d_out, d_st):
            b.free()
        stream.destroy()
    assert not wrong, (len(wrong), wrong[:8])
    assert not differ, (len(differ), differ[:8])
    assert not device, (len(device), device[:8])
    assert len(cases) >= 100 and {(cs["d"], cs["len"]) for cs in cases} == set(RC.VC_SHAPES)


def test_degenerate_and_refused(eng, cases):
    from tests.hip_ctypes import DevBuf, Stream
    lib, h = eng._lib, eng._h
    cs = next(x for x in cases if x["label"] == "3x50/random")
    # no vectors: every sum is empty — identities, status 0; no columns: nothing to do, nothing written
    assert eng.batch_g2_vector_combine(b"", b"", 0, 3) == (bytes(384), bytes(3))
    assert eng.batch_g2_vector_combine(b"", b"", 0, 0) == (b"", b"")
    call = lib.bn254_batch_g2_vector_combine
    out, st = ctypes.create_string_buffer(b"\xee" * 6400, 6400), ctypes.create_string_buffer(b"\xee" * 50, 50)
    assert call(h, None, None, 0, 2, 0, out, st) == 0 and out.raw[:256] == bytes(256) and st.raw[:2] == bytes(2) and out.raw[256:260] == b"\xee" * 4
    out, st = ctypes.create_string_buffer(b"\xee" * 6400, 6400), ctypes.create_string_buffer(b"\xee" * 50, 50)
    assert call(h, cs["vectors"], cs["scalars"], 3, 0, 0, None, None) == 0
    assert call(h, None, None, 3, 0, 0, None, None) == 0
    assert call(None, cs["vectors"], cs["scalars"], 3, 50, 0, out, st) == BAD_ARGUMENT
    assert call(h, None, cs["scalars"], 3, 50, 0, out, st) == BAD_ARGUMENT
    assert call(h, cs["vectors"], None, 3, 50, 0, out, st) == BAD_ARGUMENT
    assert call(h, cs["vectors"], cs["scalars"], 3, 50, 0, None, st) == BAD_ARGUMENT
    assert call(h, cs["vectors"], cs["scalars"], 3, 50, 0, out, None) == BAD_ARGUMENT
    assert call(h, cs["vectors"], cs["scalars"], 1 << 31, 2, 0, out, st) == BAD_ARGUMENT         # d * len = 2^32
    assert call(h, cs["vectors"], cs["scalars"], 1 << 32, 1, 0, out, st) == BAD_ARGUMENT
    assert call(h, cs["vectors"], cs["scalars"], 1, 1 << 32, 0, out, st) == BAD_ARGUMENT
    assert call(h, cs["vectors"], cs["scalars"], (1 << 64) - 1, 2, 0, out, st) == BAD_ARGUMENT   # the product wraps
    assert out.raw == b"\xee" * 6400 and st.raw == b"\xee" * 50                                  # nothing written by a refused call
    stream = Stream()
    d_v, d_s, d_out, d_st = DevBuf(len(cs["vectors"]) + 4, fill=0), DevBuf(100, fill=0), DevBuf(6404, fill=0xEE), DevBuf(50, fill=0xEE)
    try:
        dev = lib.bn254_batch_g2_vector_combine_device
        for ptrs in ((d_v.ptr + 1, d_s.ptr, d_out.ptr), (d_v.ptr, d_s.ptr + 2, d_out.ptr), (d_v.ptr, d_s.ptr, d_out.ptr + 3)):
            assert dev(h, ptrs[0], ptrs[1], 3, 50, 0, ptrs[2], d_st.ptr, stream.handle) == MISALIGNED
        assert dev(h, None, d_s.ptr, 3, 50, 0, d_out.ptr, d_st.ptr, stream.handle) == BAD_ARGUMENT
        assert dev(h, d_v.ptr, d_s.ptr, 3, 50, 0, None, d_st.ptr, stream.handle) == BAD_ARGUMENT
        assert dev(h, d_v.ptr, d_s.ptr, 1 << 31, 2, 0, d_out.ptr, d_st.ptr, stream.handle) == BAD_ARGUMENT
        assert dev(h, None, None, 3, 0, 0, None, None, stream.handle) == 0
        assert dev(h, None, None, 0, 2, 0, d_out.ptr, d_st.ptr, stream.handle) == 0
        stream.synchronize()
        assert d_out.download(260) == bytes(256) + b"\xee" * 4 and d_st.download(3) == bytes(2) + b"\xee"
    finally:
        for b in (d_v, d_s, d_out, d_st):
            b.free()
        stream.destroy()
    # no option was added for this call: 0 .. 46 are the numbers, as before
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    assert sorted(int(v) for v in re.findall(r"#define BN254_OPT_\w+ (\d+)\b", hdr)) == list(range(47))


def test_python_mirror(eng, c):
    from bn254_amd.api import ECDSA, Error, ErrorKind, PublicKey
    a, scalars = [[5, 7, 0], [11, R - 3, 2]], [3, R + 4]
    vectors = [[PublicKey(RM.key_of(c, v)) for v in row] for row in a]
    got = ECDSA.g2_vector_combine(vectors, scalars, engine=eng)
    assert [p.raw for p in got] == [RM.key_of(c, v) for v in RM.combine_scalars(a, [s % R for s in scalars])]
    vectors[1][2] = PublicKey(RM.DC.plant(vectors[1][2].raw, "curve"))
    with pytest.raises(Error) as e:
        ECDSA.g2_vector_combine(vectors, scalars, engine=eng)
    assert e.value.kind == ErrorKind.InvalidGroupPoint
    with pytest.raises(Error):
        ECDSA.g2_vector_combine([vectors[0], vectors[1][:2]], scalars, engine=eng)
