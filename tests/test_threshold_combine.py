"""Threshold signatures and the scalar-weighted sum (include/bn254_hip.h: bn254_batch_threshold_combine_keyed[_device],
bn254_batch_g1_msm[_device]) without a GPU: the four entry points are declared with the stated arity, exported with matching argtypes,
bound in INTEGRATION.md's extern block and mirrored in bn254.hpp (which compiles, with its example, against the library); the two debug
hooks are declared and exported; both new sources are in the build list and the Fr constants come from gen_constants.py; the Python mirrors
refuse mismatched lengths and a zero threshold before they touch a device; threshold_deal deals what the model's polynomial gives."""
import os
import re
import subprocess

import pytest

from bn254_amd import _native
from tests import threshold_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254_batch_threshold_combine_keyed", "bn254_batch_threshold_combine_keyed_device", "bn254_batch_g1_msm", "bn254_batch_g1_msm_device"]
ARITY = {NAMES[0]: 16, NAMES[1]: 17, NAMES[2]: 8, NAMES[3]: 9}
HOOKS = {"bn254_debug_fr_op": 6, "bn254_debug_lagrange_at_zero": 5}
R = TM.R


def _arity(decl):
    return len([a for a in decl.split(",") if a.strip()])


def _header_decls(names):
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {name: re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr) for name in names}


def test_declared_and_registered():
    decls = _header_decls(NAMES + list(HOOKS))
    for name, arity in list(ARITY.items()) + list(HOOKS.items()):
        assert decls[name], name
        assert _arity(decls[name].group(1)) == arity, name
        assert name in _native.EXPORTED_SYMBOLS
    assert "uint32_t threshold" in decls[NAMES[0]].group(1) and "uint32_t *n_valid" in decls[NAMES[0]].group(1)
    assert "uint32_t *d_used_bits" in decls[NAMES[1]].group(1) and "void *stream" in decls[NAMES[1]].group(1)
    assert "int reduce_scalar" in decls[NAMES[2]].group(1) and "const uint64_t *d_seg_off" in decls[NAMES[3]].group(1)
    units = _native.translation_units()
    assert os.path.join(ROOT, "bn254_amd", "csrc", "bn254_threshold.hip") in units
    deps = _native._dependencies()
    for h in ("bn254_fr.h", "bn254_threshold.h"):
        assert os.path.join(ROOT, "bn254_amd", "csrc", h) in deps, h
    # the header says what the library does not check about a threshold key set, and what is out of scope
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    assert "lie on one polynomial" in hdr and "dealer's or the DKG's job" in hdr and "an optimistic form that interpolates first" in hdr


def test_fr_constants_are_generated():
    """R^2 mod r, -r^-1 mod 2^32 and one in Montgomery form stand in bn254_constants.h as gen_constants.py computes them"""
    text = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_constants.h")).read()
    gen = open(os.path.join(ROOT, "bn254_amd", "csrc", "gen_constants.py")).read()
    assert "C_FR_R2" in gen and "BN_FR_N0" in gen and "C_FR_ONE" in gen

    def words(name):
        m = re.search(r"%s\[8\] = \{([^}]*)\}" % name, text)
        return sum(int(w.strip().rstrip("u"), 16) << (32 * i) for i, w in enumerate(m.group(1).split(",")))
    assert words("C_FR_R2") == pow(1 << 256, 2, R) and words("C_FR_ONE") == (1 << 256) % R and words("C_ORDER_R") == R
    n0 = int(re.search(r"#define BN_FR_N0 0x([0-9a-f]+)u", text).group(1), 16)
    assert (n0 * R + 1) % (1 << 32) == 0


def test_exported_by_the_library():
    _native.build()
    lib = _native.load()
    decls = _header_decls(NAMES + list(HOOKS))
    for name in NAMES + list(HOOKS):
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == _arity(decls[name].group(1)), name


def test_integration_extern_block_matches_header():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    decls = _header_decls(NAMES)
    for name in NAMES:
        m = re.search(r"\bfn\s+%s\s*\(([^)]*)\)\s*->\s*c_int;" % name, doc)
        assert m, name
        assert _arity(m.group(1)) == _arity(decls[name].group(1)), name
    assert "does **not** check" in doc


def test_cpp_mirror_and_example_compile(tmp_path):
    """bn254.hpp calls both entry points; a program that uses the mirrors, and host/threshold_example.cpp, build with -Wall -Werror and link"""
    _native.build()
    host = os.path.join(ROOT, "bn254_amd", "host")
    hpp = open(os.path.join(host, "bn254.hpp")).read()
    assert "bn254_batch_threshold_combine_keyed(e.raw()" in hpp and "bn254_batch_g1_msm(e.raw()" in hpp
    assert "threshold_combine_keyed(" in hpp and "static Signature g1_msm(" in hpp
    common = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", host]
    link = [_native.LIB_PATH, "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)]
    subprocess.check_call(common + [os.path.join(host, "threshold_example.cpp"), "-o", str(tmp_path / "threshold_example")] + link)


def test_api_rejects_malformed_items_before_the_device(monkeypatch):
    from bn254_amd import api, engine

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(engine, "default_engine", no_device)
    sig = api.Signature(bytes(64))
    for items in ([(b"a", [sig], [0]), (b"b", [sig])], [(b"a", [sig], [0], [1])], [(b"a", [sig, sig], [0])], [(b"a", [], [3])]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.batch_threshold_combine_keyed(items, 1)
        assert e.value.kind == api.ErrorKind.InvalidLength
    for idx in ([0, -1], [1 << 32, 0]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.threshold_combine_keyed(b"a", [sig, sig], idx, 1)
        assert e.value.kind == api.ErrorKind.IndexOutOfBounds
    for t in (0, -3, 1 << 32):
        with pytest.raises(ValueError):
            api.ECDSA.threshold_combine_keyed(b"a", [sig], [0], t)
    class Blind:
        pass
    with pytest.raises(ValueError):
        api.ECDSA.threshold_combine_keyed(b"a", [sig], [0], 1, engine=Blind())
    # the engine mirrors: sizes must add up to the shares, the threshold must be positive, points and scalars must match the segments
    with pytest.raises(AssertionError):
        engine.Engine.batch_threshold_combine_keyed(None, [b"a", b"b"], bytes(128), [0, 1], [1, 2], 1, 1)
    with pytest.raises(AssertionError):
        engine.Engine.batch_threshold_combine_keyed(None, [b"a"], bytes(64), [0], [1], 1, 0)
    with pytest.raises(AssertionError):
        engine.Engine.batch_g1_msm(None, bytes(128), bytes(32), [0, 2])
    # g1_msm and threshold_group_key: lengths that differ, repeated indices
    with pytest.raises(api.Error) as e:
        api.ECDSA.g1_msm([sig, sig], [1])
    assert e.value.kind == api.ErrorKind.InvalidLength
    pk = api.PublicKey(bytes(128))
    for idx, pks in (([0, 1], [pk]), ([], []), ([2, 2], [pk, pk])):
        with pytest.raises(api.Error) as e:
            api.ECDSA.threshold_group_key(idx, pks)
        assert e.value.kind == api.ErrorKind.InvalidLength


def test_threshold_deal_and_lagrange():
    """the dealing helper against the model's polynomial arithmetic: any t shares interpolate to the secret, t - 1 do not (for this seed)"""
    from bn254_amd import api
    secret = 0x1234567890ABCDEF << 100
    shares = [k.value for k in api.threshold_deal(secret, 5, 9, seed=7)]
    assert len(shares) == 9 and len(set(shares)) == 9
    for subset in ([0, 1, 2, 3, 4], [8, 2, 4, 6, 7], [4, 5, 6, 7, 8]):
        lam = TM.lagrange_at_zero([j + 1 for j in subset])
        assert lam == api._lagrange_at_zero([j + 1 for j in subset])
        assert sum(l * shares[j] for l, j in zip(lam, subset)) % R == secret
    lam4 = TM.lagrange_at_zero([1, 2, 3, 4])
    assert sum(l * shares[j] for l, j in zip(lam4, range(4))) % R != secret
    assert [k.value for k in api.threshold_deal(secret + R, 1, 3, seed=1)] == [secret] * 3
    with pytest.raises(ValueError):
        api.threshold_deal(1, 4, 3, seed=0)
