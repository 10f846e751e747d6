"""Same-message aggregates as signer bitmaps over registered keys (include/bn254_hip.h: bn254_batch_verify_keyed_bitmap[_device]), without a GPU:
- the two entry points are declared with the stated arity, exported, bound in INTEGRATION.md's extern block; the option mirror agrees;
- the Python mirrors refuse malformed items before they touch a device;
- the device code of the aggregate key (bn254_amd/csrc/bn254_bitmap.h: table builder, bitmap walk with and without tables, rule-2 scan),
  compiled for the host (tests/hostsim/hostsim_bitmap.cpp; pair layout plain and under -DBN_TRACK_BOUNDS, one-lane layout plain), against
  the oracle's g2_add / g2_mul / pairing_check: random bitmaps over sets of 1, 7, 8, 9 and 20 keys, a key registered twice (doubling), a
  key and its negation (inside one window and across two), a registered identity key, a refused key, the empty bitmap, and rule 2 against
  a restatement in a few lines of Python (bad keys, bits at or above n_keys, bm_words too small and too large)."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from bn254_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254_batch_verify_keyed_bitmap", "bn254_batch_verify_keyed_bitmap_device"]
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_bitmap.cpp")
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def _arity(decl):
    return len([a for a in decl.split(",") if a.strip()])


def _header_decls():
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {name: re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr) for name in NAMES}


def test_declared_and_registered():
    from bn254_amd import engine
    decls = _header_decls()
    for name in NAMES:
        assert decls[name], name
        assert name in _native.EXPORTED_SYMBOLS
    assert _arity(decls[NAMES[0]].group(1)) == 9 and _arity(decls[NAMES[1]].group(1)) == 10
    assert "const uint32_t *signer_bits" in decls[NAMES[0]].group(1) and "size_t bm_words" in decls[NAMES[0]].group(1)
    assert "const uint32_t *d_signer_bits" in decls[NAMES[1]].group(1) and "void *stream" in decls[NAMES[1]].group(1)
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    assert re.search(r"#define BN254_OPT_BITMAP_TABLE_MAX_KEYS 28\b", hdr) and engine.OPT_BITMAP_TABLE_MAX_KEYS == 28
    assert re.search(r"#define BN254_OPT_BITMAP_ROUTE 29\b", hdr) and engine.OPT_BITMAP_ROUTE == 29
    assert os.path.join(ROOT, "bn254_amd", "csrc", "bn254_bitmap.hip") in _native.translation_units()


def test_exported_by_the_library():
    _native.build()
    lib = _native.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == _arity(_header_decls()[name].group(1))


def test_integration_extern_block_matches_header():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    decls = _header_decls()
    for name in NAMES:
        m = re.search(r"\bfn\s+%s\s*\(([^)]*)\)\s*->\s*c_int;" % name, doc)
        assert m, name
        assert _arity(m.group(1)) == _arity(decls[name].group(1)), name


def test_api_rejects_mismatched_lengths_before_the_device(monkeypatch):
    from bn254_amd import api, engine

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(engine, "default_engine", no_device)
    sig = api.Signature(bytes(64))
    with pytest.raises(api.Error) as e:
        api.ECDSA.batch_verify_keyed_signers([(b"a", sig, [0]), (b"b", sig)])
    assert e.value.kind == api.ErrorKind.InvalidLength
    with pytest.raises(api.Error) as e:
        api.ECDSA.batch_verify_keyed_signers([(b"a", sig, [0], [1])])
    assert e.value.kind == api.ErrorKind.InvalidLength
    with pytest.raises(api.Error) as e:
        api.ECDSA.verify_keyed_signers(b"a", sig, [0, -1])
    assert e.value.kind == api.ErrorKind.IndexOutOfBounds
    # ... and the engine mirror: the bitmap array must hold n * bm_words words
    with pytest.raises(AssertionError):
        engine.Engine.batch_verify_keyed_bitmap(None, [b"a", b"b"], bytes(128), [0, 0, 0], 2)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    """the harness with the flags of the Makefile's libhostsim_pair.so and libhostsim_pair_bounds.so, and the one-lane layout, side by side"""
    out = tmp_path_factory.mktemp("hb")
    common = ["-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"], "one_lane": ["-O2", "-DBM_ONE_LANE"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libhb_%s.so" % name))
        procs[name] = (so, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + common + ["-o", so, SRC], stderr=subprocess.PIPE, text=True))
    for name, (so, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: so for name, (so, _) in procs.items()}


BUILDS = ["plain", "bounds", "one_lane"]


class Harness:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        self.lib.hb_sum.argtypes = [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
        self.lib.hb_table_bytes_per_key.restype = ctypes.c_size_t

    def register(self, pks, sts):
        self.lib.hb_register(len(pks), b"".join(pks) or bytes(128), bytes(sts) or b"\0")

    def sum(self, words, tables):
        row = (ctypes.c_uint32 * max(len(words), 1))(*words)
        out = ctypes.create_string_buffer(128)
        gen = ctypes.c_int(0)
        st = self.lib.hb_sum(row, len(words), int(tables), out, ctypes.byref(gen))
        return out.raw, st, gen.value


def rule2(words, sts):
    """rule 2 restated: the lowest set bit that is bad — 2 at or above n_keys, else the key's non-zero registration status"""
    for j in range(32 * len(words)):
        if (words[j // 32] >> (j % 32)) & 1:
            if j >= len(sts):
                return 2
            if sts[j]:
                return sts[j]
    return 0


def oracle_sum(c, words, pks, sts):
    acc = bytes(128)
    for j in range(min(32 * len(words), len(pks))):
        if (words[j // 32] >> (j % 32)) & 1 and not sts[j]:
            acc = c.g2_add(acc, pks[j])
    return acc


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def make_keys(c, rnd, n):
    g2 = c.g2_generator()
    return [c.g2_mul(g2, rnd.randrange(1, R).to_bytes(32, "big")) for _ in range(n)]


def neg(c, p):
    return c.g2_mul(p, (R - 1).to_bytes(32, "big"))


def check(h, c, words, pks, sts):
    want, want_st = oracle_sum(c, words, pks, sts), rule2(words, sts)
    for tables in (1, 0):
        got, st, gen = h.sum(words, tables)
        assert got == want, (tables, words)
        assert st == want_st, (tables, words, st, want_st)
        assert gen == (want == bytes(128)), (tables, words)     # an identity sum carries the generator's coordinates under the flag


@pytest.mark.parametrize("build", BUILDS)
def test_random_bitmaps_against_the_oracle(libs, c, build):
    h = Harness(libs[build])
    rnd = random.Random(20261017)
    for n in (1, 7, 8, 9, 20):
        pks = make_keys(c, rnd, n)
        sts = [0] * n
        h.register(pks, sts)
        assert h.lib.hb_table_bytes_per_key() == 5152
        nw = (n + 31) // 32
        cases = [[0] * nw, [(1 << n) - 1], [1], [1 << (n - 1)]]
        cases += [[rnd.getrandbits(n)] for _ in range(3 if build == "bounds" else 8)]
        cases += [[], [rnd.getrandbits(n), 0, 0], [rnd.getrandbits(32), rnd.getrandbits(32)]]      # bm_words 0, too large, bits above n_keys
        for words in cases:
            check(h, c, words, pks, sts)


@pytest.mark.parametrize("build", BUILDS)
def test_exceptional_sums(libs, c, build):
    """doubling (a key registered twice, both selected — inside one window and across two), a key and its negation (the identity sum; inside
    one window, across two, and with more keys around), a registered identity key, refused keys (identity in the sum, status from rule 2)"""
    h = Harness(libs[build])
    rnd = random.Random(7)
    k = make_keys(c, rnd, 12)
    pks = [k[0], k[1], k[0], neg(c, k[1]), k[2], bytes(128), k[3], k[4], k[0], neg(c, k[4]), k[5], k[6], neg(c, k[6]), k[7]]
    sts = [0] * len(pks)
    sts[10] = 4
    sts[11] = 6
    h.register(pks, sts)
    bit = lambda *js: [sum(1 << j for j in js)]      # noqa: E731
    assert h.sum(bit(0, 2), 1)[0] == c.g2_add(k[0], k[0]) == h.sum(bit(0, 2), 0)[0]          # doubling inside window 0
    assert h.sum(bit(0, 8), 1)[0] == c.g2_add(k[0], k[0]) == h.sum(bit(2, 8), 0)[0]          # ... across windows 0 and 1
    for js in [(1, 3), (7, 9), (1, 3, 7, 9), (5,), (), (1, 3, 5), (10, 11)]:                  # identity sums
        for tables in (1, 0):
            got, _, gen = h.sum(bit(*js), tables)
            assert got == bytes(128) and gen == 1, (js, tables)
    assert h.sum(bit(0, 1, 3), 1)[0] == k[0] and h.sum(bit(7, 9, 13), 1)[0] == k[7] and h.sum(bit(1, 9, 3, 7, 4), 0)[0] == k[2]
    for js in [(0, 10), (10, 11), (11, 0, 13), (0, 5, 6), (4, 14), (10, 14), (15, 31)]:
        check(h, c, bit(*js), pks, sts)
    assert h.sum(bit(0, 10), 1)[1] == 4 and h.sum(bit(11, 10 + 32), 1)[1] == 6 and h.sum(bit(14), 0)[1] == 2
    for _ in range(4 if build == "bounds" else 24):
        check(h, c, [rnd.getrandbits(32) & rnd.getrandbits(32)] + [rnd.getrandbits(32) & rnd.getrandbits(32) & rnd.getrandbits(32)] * rnd.randrange(2), pks, sts)


def test_table_entries_and_pairing(libs, c):
    """a table entry IS the subset sum; and a signature aggregated over a bitmap verifies against the walk's key (pairing_check)"""
    h = Harness(libs["plain"])
    rnd = random.Random(99)
    sks = [rnd.randrange(1, R) for _ in range(9)]
    g2 = c.g2_generator()
    pks = [c.g2_mul(g2, s.to_bytes(32, "big")) for s in sks]
    h.register(pks, [0] * 9)
    out = ctypes.create_string_buffer(128)
    for window, mask in [(0, 0), (0, 1), (0, 0xA5), (0, 255), (1, 1), (1, 254)]:
        h.lib.hb_table_entry(window, mask, out)
        assert out.raw == oracle_sum(c, [mask << (8 * window)], pks, [0] * 9), (window, mask)
    st, hm, _ = c.hash_to_g1(b"bitmap/host")
    assert st == 0
    words = [0b101100101]
    sk_sum = sum(s for j, s in enumerate(sks) if (words[0] >> j) & 1) % R
    sigma = c.g1_mul(hm, sk_sum.to_bytes(32, "big"))
    apk, st2, _ = h.sum(words, 1)
    assert st2 == 0
    assert c.pairing_check(hm + sigma, apk + neg(c, g2), 2) == 0
    assert c.pairing_check(hm + sigma, h.sum([0b101100100], 1)[0] + neg(c, g2), 2) == 9
