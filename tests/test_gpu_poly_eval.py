"""Polynomials with G2 coefficients at small integer points (include/bn254_hip.h: bn254_batch_g2_poly_eval[_device]) on the GPU.
The case set of tests/polyeval_cases.py as ONE call — every polynomial once, every (polynomial, point) an evaluation, sorted and shuffled,
with evaluations that name no polynomial — under the shipped split, the forced lane layout and the forced wave layout, against
tests/polyeval_model.py (Python integers and the C oracle); batches of 1, 63, 64 and 65 evaluations; one wave that mixes polynomials of 0, 1,
17 and 200 coefficients and points of 1 and of 32 bits; the defining identity against bn254_batch_g2_msm with scalars from Python integers;
the _device form on a caller's stream (misaligned pointers, a reversed and an over-long polynomial, a small call in the scratch a large one
left); refused arguments; the Python and C++ mirrors; a DKG round's share check and the sum of commitment vectors.  Run on the MI355X box: -m gpu."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from bn254_amd import engine as E
from tests import dealing_cases as DC
from tests import polyeval_cases as PC
from tests import polyeval_model as PM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = PM.R
BAD_ARGUMENT, MISALIGNED = -10001, -10002
ZERO = bytes(128)


def split_default():
    text = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    return int(re.search(r"#define POLY_EVAL_WAVE_MIN_COEFFS_DEFAULT (\d+)", text).group(1))


SPLITS = {"default": None, "lanes": 1 << 30, "waves": 1}


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def with_split(eng, split, fn):
    try:
        if SPLITS[split] is not None:
            eng.set_option(E.OPT_POLY_EVAL_WAVE_MIN_COEFFS, SPLITS[split])
        return fn()
    finally:
        eng.set_option(E.OPT_POLY_EVAL_WAVE_MIN_COEFFS, split_default())


def be(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def derive(eng, scalars):
    """a_k * G2::one() by the fixed-base route of bn254_batch_g2_mul, a call this feature does not touch: the INPUTS of the tests (0 gives the
    identity); every expectation is the model's"""
    if not scalars:
        return []
    out, st = eng.batch_g2_mul(None, be(s % R for s in scalars), len(scalars))
    assert st == bytes(len(scalars))
    return [out[128 * j:128 * j + 128] for j in range(len(scalars))]


def chunks(raw, size=128):
    return [raw[i:i + size] for i in range(0, len(raw), size)]


@pytest.fixture(scope="module")
def batch(eng, c):
    """the case set as one call: coefficients, offsets, the evaluations in polynomial order and what the model says of each"""
    cases = PC.all_cases()
    flat = derive(eng, [v for _, cs in cases if cs["points"] is None for v in cs["a"]])
    coeffs, off, evals, want, at = [], [0], [], [], 0
    for i, (n, cs) in enumerate(cases):
        if cs["points"] is None:
            pts = flat[at:at + n]
            at += n
        else:
            pts = list(cs["points"])
        for where, kind in cs["faults"].items():
            pts[where] = DC.plant(pts[where], kind)
        coeffs += pts
        off.append(off[-1] + n)
        for x in cs["xs"]:
            evals.append((i, x))
            want.append(PM.expected(c, cs, x))
    # evaluations that name no polynomial: the first index past the end, and the largest
    for poly in (len(cases), 0xFFFFFFFF):
        evals.append((poly, 3))
        want.append((PM.ST_INDEX_OOB, ZERO))
    assert coeffs[off[1]:off[2]] == [c.public_key_g2(cases[1][1]["a"][0].to_bytes(32, "big"))]      # the inputs are what the model assumes
    return {"coeffs": b"".join(coeffs), "off": off, "evals": evals, "want": want, "cases": cases}


def run(eng, batch, order):
    out, st = eng.batch_g2_poly_eval(batch["coeffs"], batch["off"], [batch["evals"][e][0] for e in order], [batch["evals"][e][1] for e in order])
    return [(st[k], out[128 * k:128 * k + 128]) for k in range(len(order))]


def label(batch, e):
    poly, x = batch["evals"][e]
    return (poly, x) if poly >= len(batch["cases"]) else (batch["cases"][poly][0], batch["cases"][poly][1]["name"], x)


@pytest.mark.parametrize("split", list(SPLITS))
def test_case_set(eng, batch, split):
    q = len(batch["evals"])
    order = list(range(q))
    got = with_split(eng, split, lambda: run(eng, batch, order))
    wrong = [label(batch, e) for e in order if got[e] != batch["want"][e]]
    assert not wrong, (len(wrong), wrong[:8])
    shuffled = list(order)
    random.Random(11).shuffle(shuffled)
    got = with_split(eng, split, lambda: run(eng, batch, shuffled))
    wrong = [label(batch, e) for k, e in enumerate(shuffled) if got[k] != batch["want"][e]]
    assert not wrong, (len(wrong), wrong[:8])


@pytest.mark.parametrize("q", [1, 63, 64, 65])
def test_batch_shapes(eng, batch, q):
    """one evaluation, a wave short of one, a full wave, one more; drawn from the whole set, so every batch mixes lengths and layouts"""
    order = list(range(len(batch["evals"])))
    random.Random(q).shuffle(order)
    order = order[:q]
    for split in ("default", "lanes"):
        got = with_split(eng, split, lambda: run(eng, batch, order))
        assert got == [batch["want"][e] for e in order], (q, split)


def test_one_wave_mixing_lengths_and_widths(eng, c):
    """64 evaluations in the lane layout: polynomials of 0, 1, 17 and 200 coefficients side by side, x of one bit beside x of 32 bits — the
    loop bounds are the wave's, the values each lane's own"""
    rnd = random.Random(64)
    lengths = [0, 1, 17, 200]
    polys = [[rnd.randrange(1, R) for _ in range(n)] for n in lengths]
    off = [0]
    for n in lengths:
        off.append(off[-1] + n)
    coeffs = b"".join(derive(eng, [v for a in polys for v in a]))
    evals = [(e % 4, 1 if (e // 4) % 2 == 0 else (1 << 32) - 1) for e in range(64)]
    want = b"".join(PM.key_of(c, PM.eval_scalar(polys[p], x)) for p, x in evals)
    for split in ("lanes", "default", "waves"):
        got = with_split(eng, split, lambda: eng.batch_g2_poly_eval(coeffs, off, [p for p, _ in evals], [x for _, x in evals]))
        assert got == (want, bytes(64)), split


@pytest.mark.parametrize("split", list(SPLITS))
def test_defining_identity_against_g2_msm(eng, split):
    """byte for byte bn254_batch_g2_msm over one segment of the polynomial's coefficients with the scalars x^k mod r from Python integers,
    reduce_scalar = 0: random coefficients with the identity among them, and a polynomial with a fault (its status and the identity)"""
    rnd = random.Random(171)
    xs = [0, 1, 257, (1 << 32) - 1]
    for n in (1, 17, 65, 171):
        pts = derive(eng, [0 if k % 13 == 5 else rnd.randrange(1, R) for k in range(n)])
        faulty = list(pts)
        faulty[n // 2] = DC.plant(pts[n // 2], "curve")
        for coeffs in (pts, faulty):
            raw = b"".join(coeffs)
            want = [eng.batch_g2_msm(raw, be(PM.powers(x, n)), [0, n], reduce_scalar=False) for x in xs]
            got = with_split(eng, split, lambda: eng.batch_g2_poly_eval(raw, [0, n], [0] * len(xs), xs))
            assert got == (b"".join(w[0] for w in want), b"".join(w[1] for w in want)), (n, coeffs is faulty)
            assert (got[1] == bytes(len(xs))) == (coeffs is pts)


def test_device_form_and_stale_scratch(eng, batch):
    """the host form's bytes on a caller's stream; a reversed polynomial and one that runs past the coefficients read 2 with the identity and
    leave the other evaluations alone; misaligned pointers are refused; a small call after the large one computes in the scratch it left"""
    from tests.hip_ctypes import DevBuf, Stream
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    off, evals = batch["off"], batch["evals"]
    p, q, m = len(off) - 1, len(evals), off[-1]
    host = eng.batch_g2_poly_eval(batch["coeffs"], off, [e[0] for e in evals], [e[1] for e in evals])
    assert [(s, v) for s, v in zip(host[1], chunks(host[0]))] == batch["want"]
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_c, d_poly, d_x = dev(batch["coeffs"] + bytes(4)), dev(u32(e[0] for e in evals) + bytes(4)), dev(u32(e[1] for e in evals) + bytes(4))
        d_out, d_st = dev(nbytes=128 * q + 4), dev(nbytes=q)

        def run_dev(offsets, **ptr):
            d_off = dev(u64(offsets) + bytes(8))
            eng.batch_g2_poly_eval_device(ptr.get("c", d_c.ptr), ptr.get("off", d_off.ptr), p, ptr.get("poly", d_poly.ptr), ptr.get("x", d_x.ptr), q,
                                          ptr.get("out", d_out.ptr), d_st.ptr, stream=stream.handle)
            stream.synchronize()
            return d_out.download(128 * q), d_st.download(q)
        assert run_dev(off) == host
        # polynomial `hit` (17 random coefficients) reversed: its evaluations read 2; its neighbour, which now starts early, is ANOTHER polynomial
        # and is left out of the comparison; everything else stands
        hit = next(i for i, (n, cs) in enumerate(batch["cases"]) if n == 17 and cs["name"] == "random")
        rev = list(off)
        rev[hit + 1] = off[hit] - 1
        out, st = run_dev(rev)
        for e, (poly, _) in enumerate(evals):
            if poly == hit:
                assert st[e] == 2 and out[128 * e:128 * e + 128] == ZERO
            elif poly != hit + 1:
                assert (st[e], out[128 * e:128 * e + 128]) == batch["want"][e], e
        past = list(off)
        past[hit + 1] = m + 1                               # it runs past the coefficients, and its neighbour starts there: both refused
        out, st = run_dev(past)
        for e, (poly, _) in enumerate(evals):
            if poly in (hit, hit + 1):
                assert st[e] == 2 and out[128 * e:128 * e + 128] == ZERO
            else:
                assert (st[e], out[128 * e:128 * e + 128]) == batch["want"][e], e
        for name, ptr in (("c", d_c.ptr + 1), ("poly", d_poly.ptr + 2), ("x", d_x.ptr + 3), ("out", d_out.ptr + 2), ("off", dev(bytes(8 * p + 24)).ptr + 4)):
            with pytest.raises(E.NativeError) as e:
                run_dev(off, **{name: ptr})
            assert e.value.rc == MISALIGNED, name
        eng.batch_g2_poly_eval_device(None, None, 0, None, None, 0, None, None, stream=stream.handle)
        # a small call in the scratch the large one left: 3 coefficients where 146 B x thousands were decoded
        lo = next(i for i, (n, cs) in enumerate(batch["cases"]) if n == 3 and cs["name"] == "random")
        small = batch["coeffs"][128 * off[lo]:128 * off[lo + 1]]
        d_small, d_soff, d_sp, d_sx = dev(small), dev(u64([0, 3])), dev(u32([0, 0])), dev(u32([2, 65536]))
        eng.batch_g2_poly_eval_device(d_small.ptr, d_soff.ptr, 1, d_sp.ptr, d_sx.ptr, 2, d_out.ptr, d_st.ptr, stream=stream.handle)
        stream.synchronize()
        for k, x in enumerate((2, 65536)):
            e = evals.index((lo, x))
            assert (d_st.download(2)[k], d_out.download(256)[128 * k:128 * k + 128]) == batch["want"][e]
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


def test_refused_arguments_and_degenerate_calls(eng, batch):
    lib, h = eng._lib, eng._h
    call = lib.bn254_batch_g2_poly_eval
    coeffs = batch["coeffs"][:256]
    off = (ctypes.c_uint64 * 2)(0, 2)
    poly, x = (ctypes.c_uint32 * 2)(0, 0), (ctypes.c_uint32 * 2)(1, 2)
    out, st = ctypes.create_string_buffer(b"\xee" * 256, 256), ctypes.create_string_buffer(b"\xee\xee", 2)
    assert call(None, coeffs, off, 1, poly, x, 2, out, st) == BAD_ARGUMENT
    assert call(h, None, off, 1, poly, x, 2, out, st) == BAD_ARGUMENT               # coefficients to stage, no buffer
    assert call(h, coeffs, None, 1, poly, x, 2, out, st) == BAD_ARGUMENT
    assert call(h, coeffs, off, 1, None, x, 2, out, st) == BAD_ARGUMENT
    assert call(h, coeffs, off, 1, poly, None, 2, out, st) == BAD_ARGUMENT
    assert call(h, coeffs, off, 1, poly, x, 2, None, st) == BAD_ARGUMENT
    assert call(h, coeffs, off, 1, poly, x, 2, out, None) == BAD_ARGUMENT
    assert call(h, coeffs, off, 1 << 32, poly, x, 2, out, st) == BAD_ARGUMENT
    assert call(h, coeffs, off, 1, poly, x, 1 << 32, out, st) == BAD_ARGUMENT
    assert call(h, coeffs, (ctypes.c_uint64 * 3)(0, 2, 1), 2, poly, x, 2, out, st) == BAD_ARGUMENT      # offsets step back (host form)
    assert out.raw == b"\xee" * 256 and st.raw == b"\xee\xee"                          # nothing written by a refused call
    assert call(h, None, None, 0, None, None, 0, None, None) == 0
    # no polynomials at all: every evaluation names one that is not there; an empty polynomial: the identity, status 0
    assert eng.batch_g2_poly_eval(b"", [0], [0, 5], [1, 2]) == (bytes(256), b"\x02\x02")
    assert eng.batch_g2_poly_eval(b"", [0, 0], [0, 1], [1, 2]) == (bytes(256), b"\x00\x02")
    assert eng.batch_g2_poly_eval(coeffs, [0, 2], [], []) == (b"", b"")
    for value in (0, -1):
        with pytest.raises(E.NativeError):
            eng.set_option(E.OPT_POLY_EVAL_WAVE_MIN_COEFFS, value)
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    number = int(re.search(r"#define BN254_OPT_POLY_EVAL_WAVE_MIN_COEFFS (\d+)\b", hdr).group(1))
    assert number == E.OPT_POLY_EVAL_WAVE_MIN_COEFFS and len(re.findall(r"#define BN254_OPT_\w+ %d\b" % number, hdr)) == 1


def test_dealt_shares_and_combined_commitments(eng, c):
    """a DKG round among 5 dealers, threshold 4: the holder of key 6 checks the share every dealer sent it against that dealer's commitments
    — one share is wrong, one dealer's vector has a faulty commitment; and the sum of 3 dealers' vectors is the commitment vector of the
    summed polynomial"""
    from bn254_amd.api import ECDSA, ErrorKind, PrivateKey, PublicKey, threshold_commitments, threshold_deal
    rnd = random.Random(5)
    index, t = 6, 4
    polys = [[rnd.randrange(1, R) for _ in range(t)] for _ in range(5)]
    vectors = [[PublicKey(b) for b in derive(eng, a)] for a in polys]
    assert [v.raw for v in vectors[0]] == [PM.key_of(c, v) for v in polys[0]]
    shares = [PrivateKey(PM.eval_scalar(a, index + 1)) for a in polys]
    assert ECDSA.batch_verify_dealt_shares(vectors, index, shares, engine=eng) == [None] * 5
    shares[2] = PrivateKey((shares[2].value + 1) % R)
    vectors[4][1] = PublicKey(DC.plant(vectors[4][1].raw, "big"))
    res = ECDSA.batch_verify_dealt_shares(vectors, index, shares, engine=eng)
    assert res[0] is None and res[1] is None and res[3] is None
    assert res[2].kind == ErrorKind.VerificationFailed and res[4].kind == ErrorKind.NotMemberError
    assert ECDSA.batch_verify_dealt_shares(vectors[:4], index + 1, shares[:4], engine=eng)[0].kind == ErrorKind.VerificationFailed      # another index
    assert ECDSA.batch_verify_dealt_shares([], 0, [], engine=eng) == []
    summed = [sum(a[k] for a in polys[:3]) % R for k in range(t)]
    both = ECDSA.combine_commitments(vectors[:3], engine=eng)
    assert [v.raw for v in both] == [PM.key_of(c, v) for v in summed]
    # threshold_commitments commits to the polynomial threshold_deal shares: its values at 1 .. n are the share keys, C_0 the group key
    secret = 0xC0FFEE << 200
    sks = threshold_deal(secret, 3, 5, seed=77)
    cs = threshold_commitments(secret, 3, seed=77)
    assert len(cs) == 3 and cs[0].raw == PM.key_of(c, secret)
    vals = ECDSA.commitments_eval(cs, range(0, 6), engine=eng)
    assert vals[0].raw == cs[0].raw and [v.raw for v in vals[1:]] == [PM.key_of(c, k.value) for k in sks]
    assert ECDSA.batch_verify_dealt_shares([cs] * 5, 3, [sks[3]] * 5, engine=eng) == [None] * 5
    assert [v.raw for v in ECDSA.commitments_eval([], [0, 7], engine=eng)] == [ZERO, ZERO]
    with pytest.raises(Exception) as e:
        ECDSA.commitments_eval([cs[0], PublicKey(DC.plant(cs[1].raw, "curve"))], [1], engine=eng)
    assert e.value.kind == ErrorKind.InvalidGroupPoint
    with pytest.raises(Exception):
        ECDSA.commitments_eval(cs, [1 << 32], engine=eng)


def test_cpp_mirror(eng, tmp_path):
    """host/commitments_example.cpp (every new call through bn254.hpp) built with -Wall -Werror"""
    from bn254_amd import _native
    host = os.path.join(ROOT, "bn254_amd", "host")
    exe = str(tmp_path / "commitments_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", host,
                           os.path.join(host, "commitments_example.cpp"), "-o", exe, _native.LIB_PATH, "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "commitments: ok" in out.stdout
