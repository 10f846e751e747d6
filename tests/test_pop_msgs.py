"""Proofs of possession without a GPU (include/bn254_hip.h: bn254_batch_pop_prove / _verify, bn254_ctx_register_keys_pop):
- the golden vectors tests/golden/pop_vectors.json — (sk, pk, pop) with pop = sk * H(TAG || pk), produced by oracle.bn254_model
  (tests/golden/gen_pop_vectors.py), sk = 1, r - 1 and two sk >= r among them — are reproduced by the model and by oracle.c_oracle, verify,
  and stop verifying for the untagged message, a neighbouring key's proof and a tag with one byte changed: the tag and the wire format are pinned;
- the tag has one spelling: header, engine.py, bn254.hpp;
- the device code of the front end (bn254_amd/csrc/bn254_pop.h), compiled for the host (tests/hostsim/hostsim_pop.cpp) and walked as the
  launch walks it, whole workgroups included: the composer against a three-line restatement at n = 0, 1, 63, 64, 65, 130 (messages, offsets,
  the last message's end, key indices, not a byte past 144 n), the fold over all 12 x 12 status pairs;
- the same source with its own main under AddressSanitizer and UBSan, run directly, on exact-size heap buffers;
- the entry points are declared, exported with matching argtypes, bound in INTEGRATION.md; the translation unit is registered."""
import ctypes
import json
import os
import re
import subprocess

import pytest

from oracle import bn254_model as M
from oracle import c_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_pop.cpp")
TAG = b"BN254G2_POP_V01:"
SIZES = [0, 1, 63, 64, 65, 130]
NAMES = ["bn254_batch_pop_prove", "bn254_batch_pop_prove_device", "bn254_batch_pop_verify", "bn254_batch_pop_verify_device",
         "bn254_ctx_register_keys_pop", "bn254_mgpu_register_keys_pop"]


def vectors():
    doc = json.load(open(os.path.join(ROOT, "tests", "golden", "pop_vectors.json")))
    assert doc["tag"].encode() == TAG
    return [(bytes.fromhex(v["sk"]), bytes.fromhex(v["pk"]), bytes.fromhex(v["pop"])) for v in doc["vectors"]]


def test_golden_vectors_model_and_oracle():
    vs = vectors()
    sks = [int.from_bytes(sk, "big") for sk, _, _ in vs]
    assert 1 in sks and M.R - 1 in sks and any(s >= M.R for s in sks)
    for i, (sk, pk, pop) in enumerate(vs):
        assert len(sk) == 32 and len(pk) == 128 and len(pop) == 64
        k = M.private_key_from_bytes(sk)
        assert M.g2_to_uncompressed(M.public_key(k)) == pk
        assert M.g1_to_uncompressed(M.sign(TAG + pk, k)) == pop
        assert c_oracle.public_key_g2(sk) == pk
        assert c_oracle.sign(TAG + pk, sk) == pop
        assert c_oracle.verify(TAG + pk, pop, pk) == 0
        assert c_oracle.verify(pk, pop, pk) == 9                                   # the untagged message
        assert c_oracle.verify(TAG + pk, vs[(i + 1) % len(vs)][2], pk) == 9         # a neighbouring key's proof
        for at in (0, 7, 15):                                                       # a tag with one byte changed
            bad = bytearray(TAG)
            bad[at] ^= 1
            assert c_oracle.verify(bytes(bad) + pk, pop, pk) == 9
    # sk and sk mod r are the same key and the same proof (Fr::from_slice reduces)
    by_key = {}
    for sk, pk, pop in vs + [((int.from_bytes(vs[0][0], "big") + M.R).to_bytes(32, "big"), vs[0][1], vs[0][2])]:
        assert by_key.setdefault(int.from_bytes(sk, "big") % M.R, (pk, pop)) == (pk, pop)
    assert c_oracle.public_key_g2((1 + M.R).to_bytes(32, "big")) == vs[sks.index(1)][1]


def test_tag_has_one_spelling():
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    m = re.search(r'#define BN254_POP_TAG "([^"]*)"', hdr)
    assert m and m.group(1).encode() == TAG and len(TAG) == 16
    assert re.search(r"#define BN254_POP_TAG_LEN 16\b", hdr)
    from bn254_amd import engine
    assert engine.POP_TAG == TAG
    hpp = open(os.path.join(ROOT, "bn254_amd", "host", "bn254.hpp")).read()
    assert "BN254_POP_TAG" in hpp and '"BN254G2_POP_V01:"' not in hpp.replace("//", "")     # the C++ mirror takes the header's macro, no second literal


def test_abi_wiring():
    from bn254_amd import _native
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    arity = {"bn254_batch_pop_prove": 6, "bn254_batch_pop_prove_device": 7, "bn254_batch_pop_verify": 6, "bn254_batch_pop_verify_device": 7,
             "bn254_ctx_register_keys_pop": 6, "bn254_mgpu_register_keys_pop": 6}
    _native.build()
    lib = _native.load()
    for name in NAMES:
        m = re.search(r"\bint %s\(([^;]*)\);" % name, hdr)
        assert m, name
        assert len(m.group(1).split(",")) == arity[name], name
        assert name in _native.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == arity[name], name
        assert "fn %s(" % name in integ, name
    units = {os.path.basename(p) for p in _native.translation_units()}
    deps = {os.path.basename(p) for p in _native._dependencies()}
    assert "bn254_pop.hip" in units and {"bn254_pop.hip", "bn254_pop.h"} <= deps


@pytest.fixture(scope="module")
def hp(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("hostsim_pop") / "libhp.so")
    p = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-shared", "-fPIC", "-Wall", "-Werror", "-Wno-unknown-pragmas",
                        "-Wno-unused-function", "-o", so, SRC], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    L = ctypes.CDLL(so)
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    L.hp_compose.argtypes = [vp, sz, vp, vp, vp]
    L.hp_compose.restype = None
    L.hp_fold.argtypes = [sz, vp, vp]
    L.hp_fold.restype = None
    L.hp_tag.restype = ctypes.c_char_p
    return L


def key_bytes(n):
    return bytes((i * 131 + 7 * (i >> 7) + 1) & 0xFF for i in range(128 * n))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("with_idx", [True, False])
def test_composer_against_restatement(hp, n, with_idx):
    assert hp.hp_tag() == TAG and hp.hp_msg_bytes() == 144
    pks = key_bytes(n)
    # the restatement
    want_msgs = b"".join(TAG + pks[128 * j:128 * j + 128] for j in range(n))
    want_off = [144 * j for j in range(n + 1)]
    want_idx = list(range(n))
    guard = 64                                        # canary bytes behind every output: nothing is written past its end
    msgs = ctypes.create_string_buffer(b"\xA5" * (144 * n + guard), 144 * n + guard)
    off = (ctypes.c_uint64 * (n + 1 + 8))(*([0xA5A5A5A5A5A5A5A5] * (n + 1 + 8)))
    idx = (ctypes.c_uint32 * (n + 8))(*([0xA5A5A5A5] * (n + 8)))
    src = ctypes.create_string_buffer(pks, max(len(pks), 1))
    hp.hp_compose(src, n, msgs, off, idx if with_idx else None)
    assert msgs.raw[:144 * n] == want_msgs
    assert msgs.raw[144 * n:] == b"\xA5" * guard
    assert list(off)[:n + 1] == want_off and off[n] == 144 * n == len(want_msgs)       # the last message ends where the buffer does
    assert list(off)[n + 1:] == [0xA5A5A5A5A5A5A5A5] * 8
    assert list(idx)[:n] == (want_idx if with_idx else [0xA5A5A5A5] * n)
    assert list(idx)[n:] == [0xA5A5A5A5] * 8
    assert src.raw[:len(pks)] == pks


def test_fold_precedence_all_pairs(hp):
    pairs = [(a, b) for a in range(12) for b in range(12)]
    assert all(hp.hp_fold_one(a, b) == (a if a else b) for a, b in pairs)
    for n in SIZES + [144]:
        first = bytes(pairs[j % 144][0] for j in range(n))
        second = bytes(pairs[j % 144][1] for j in range(n))
        a = ctypes.create_string_buffer(first + b"\xA5" * 16, n + 16)
        b = ctypes.create_string_buffer(second + b"\x5A" * 16, n + 16)
        hp.hp_fold(n, a, b)
        assert a.raw[:n] == bytes(x if x else y for x, y in zip(first, second))
        assert a.raw[n:] == b"\xA5" * 16 and b.raw == second + b"\x5A" * 16


def test_stand_alone_under_sanitizers(tmp_path):
    """hostsim_pop.cpp with its own main, under AddressSanitizer and UBSan, run directly: exact-size heap buffers (an offset n + 1, an index n
    or a byte past 144 n is a heap overflow), sizes 0 .. 257 with and without key indices; the program checks its results itself"""
    exe = str(tmp_path / "hostsim_pop_san")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DHP_MAIN",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and "hostsim_pop ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
