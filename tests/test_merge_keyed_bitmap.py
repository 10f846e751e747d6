"""Merging partial signer-bitmap aggregates (include/bn254_hip.h: bn254_batch_merge_keyed_bitmap[_device]), without a GPU:
- the two entry points are declared with the stated arity, exported with matching argtypes, bound in INTEGRATION.md's extern block; the
  option has a number of its own, mirrored in engine.py; the translation unit is registered;
- the Python mirrors refuse malformed items before they touch a device;
- the device code of the first-fit select-and-sum (bn254_amd/csrc/bn254_merge.h), compiled for the host (tests/hostsim/hostsim_merge.cpp,
  plain and under -DBN_TRACK_BOUNDS), over GIVEN status arrays: both layouts (the wave layout as 64 lanes' select, their partial sums and
  the tree) against tests/merge_model.py and the oracle's g1_add — tuples of 0 .. 130 partials at rows of 0 .. 130 words, the overlap cases
  of the contract, refused tuples, and a key set that repeats keys (tests/collect_repeat_cases.py as one-bit partials): equal and opposite
  partial sums at every level of the tree and in a lane's own stride; one-bit partials against the collect's model (identity 3);
- the same source as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from bn254_amd import _native
from tests import collect_model, merge_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254_batch_merge_keyed_bitmap", "bn254_batch_merge_keyed_bitmap_device"]
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_merge.cpp")
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130]
WIDTHS = [0, 1, 2, 3, 64, 65, 130]


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
    assert _arity(decls[NAMES[0]].group(1)) == 16 and _arity(decls[NAMES[1]].group(1)) == 17
    assert "const uint32_t *part_bits" in decls[NAMES[0]].group(1) and "uint8_t *part_taken" in decls[NAMES[0]].group(1)
    assert "uint32_t *n_signers" in decls[NAMES[0]].group(1)
    assert "const uint64_t *d_part_off" in decls[NAMES[1]].group(1) and "void *stream" in decls[NAMES[1]].group(1)
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    assert re.search(r"#define BN254_OPT_MERGE_WAVE_MIN_PARTS 43\b", hdr) and engine.OPT_MERGE_WAVE_MIN_PARTS == 43
    numbers = [int(x) for x in re.findall(r"#define BN254_OPT_\w+ (\d+)\b", hdr)]
    assert numbers.count(43) == 1 and len(numbers) == len(set(numbers))       # a number of its own
    ws = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    assert int(re.search(r"#define MERGE_WAVE_MIN_PARTS_DEFAULT (\d+)", ws).group(1)) == engine.MERGE_WAVE_MIN_PARTS_DEFAULT
    mirrored = [v for k, v in vars(engine).items() if k.startswith("OPT_")]
    assert mirrored.count(43) == 1
    assert os.path.join(ROOT, "bn254_amd", "csrc", "bn254_merge.hip") in _native.translation_units()
    assert hasattr(engine.Engine, "merge_keyed_bitmap") and hasattr(engine.Engine, "merge_keyed_bitmap_device")


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


def test_api_rejects_malformed_items_before_the_device(monkeypatch):
    from bn254_amd import api, engine

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(engine, "default_engine", no_device)
    sig = api.Signature(bytes(64))
    short = api.Signature(bytes(64))
    short.raw = bytes(63)
    for items in ([(b"a", [(sig, [0])]), (b"b",)],                # an item that is not a pair
                  [(b"a", [(sig, [0])], [1])],
                  [b"ab"],
                  [(b"a", [(sig, [0], 1)])],                      # a part that is not a pair
                  [(b"a", [(sig,)])],
                  [(b"a", [(sig, [0]), (short, [1])])]):          # a signature of the wrong length
        with pytest.raises(api.Error) as e:
            api.ECDSA.batch_merge_keyed_signers(items)
        assert e.value.kind == api.ErrorKind.InvalidLength, items
    for idx in ([0, -1], [1 << 32, 0]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.merge_keyed_signers(b"a", [(sig, [3]), (sig, idx)])
        assert e.value.kind == api.ErrorKind.IndexOutOfBounds
    # ... and the engine mirror: sizes must add up to the partials, rows to the bitmap width
    with pytest.raises(AssertionError):
        engine.Engine.merge_keyed_bitmap(None, [b"a", b"b"], bytes(128), [1, 2], [1, 2], 1)
    with pytest.raises(AssertionError):
        engine.Engine.merge_keyed_bitmap(None, [b"a"], bytes(128), [1, 2, 3], [2], 2)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    out = tmp_path_factory.mktemp("hm")
    common = ["-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libhm_%s.so" % name))
        procs[name] = (so, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + common + ["-o", so, SRC], stderr=subprocess.PIPE, text=True))
    for name, (so, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: so for name, (so, _) in procs.items()}


BUILDS = ["plain", "bounds"]


class Harness:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        vp, sz = ctypes.c_void_p, ctypes.c_size_t
        self.lib.hm_merge.argtypes = [vp, vp, vp, vp, vp, sz, sz, ctypes.c_int, vp, vp, vp, vp]
        self.lib.hm_merge.restype = None

    def merge(self, parts, rows, sizes, part_st, tuple_st, bm_words, layout):
        """exact-size inputs (plus one word so that an empty array has an address) -> (taken, bits, counts, agg)"""
        n, ends = len(sizes), [0]
        for k in sizes:
            ends.append(ends[-1] + k)
        n_parts = ends[-1]
        assert len(parts) == n_parts == len(rows) == len(part_st) and all(len(r) == bm_words for r in rows)
        off = (ctypes.c_uint64 * (n + 1))(*ends)
        words = (ctypes.c_uint32 * (n_parts * bm_words + 1))(*[w for r in rows for w in r])
        taken = ctypes.create_string_buffer(n_parts + 1)
        bits = (ctypes.c_uint32 * (n * bm_words + 1))()
        agg = ctypes.create_string_buffer(64 * n + 1)
        counts = (ctypes.c_uint32 * (n + 1))()
        self.lib.hm_merge(b"".join(parts) + bytes(4), words, off, bytes(part_st) + b"\0", bytes(tuple_st) + b"\0", n, bm_words, layout, taken, bits, agg, counts)
        assert bits[n * bm_words] == 0 and counts[n] == 0 and taken.raw[n_parts:] == b"\0" and agg.raw[64 * n:] == b"\0"
        return list(taken.raw[:n_parts]), list(bits)[:n * bm_words], list(counts)[:n], agg.raw[:64 * n]


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def expected(c, parts, rows, sizes, part_st, tuple_st, bm_words):
    urows, counts, taken = merge_model.select(rows, part_st, sizes, tuple_st, bm_words)
    return taken, [w for r in urows for w in r], counts, b"".join(merge_model.aggregates(c, parts, sizes, taken))


def check(h, c, parts, rows, sizes, part_st, tuple_st, bm_words):
    want = expected(c, parts, rows, sizes, part_st, tuple_st, bm_words)
    for layout in (0, 1):
        got = h.merge(parts, rows, sizes, part_st, tuple_st, bm_words, layout)
        assert got[0] == want[0], (layout, bm_words, [p for p in range(len(parts)) if got[0][p] != want[0][p]][:8])
        assert got[1] == want[1] and got[2] == want[2], (layout, bm_words)
        assert got[3] == want[3], (layout, bm_words, [i for i in range(len(sizes)) if got[3][64 * i:64 * i + 64] != want[3][64 * i:64 * i + 64]])
    return want


def row_of(bits, bm_words):
    row = [0] * bm_words
    for b in bits:
        row[b // 32] |= 1 << (b % 32)
    return row


@pytest.fixture(scope="module")
def points(c):
    """multiples of one base (the statuses are given, so any point serves as a partial's signature); [0] = the identity"""
    rnd = random.Random(20261018)
    st_h, base, _ = c.hash_to_g1(b"merge/host")
    assert st_h == 0
    return [bytes(64)] + [c.g1_mul(base, rnd.randrange(1, R).to_bytes(32, "big")) for _ in range(sum(SIZES))]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("bm_words", WIDTHS)
def test_select_and_sum_both_layouts(libs, c, points, build, bm_words):
    """tuples of 0 .. 130 partials with rows of one to four random bits (narrow rows fill up and refuse most, wide ones take most), statuses
    0, 9, 2, 4, 6 and 1 given, not computed; then a tuple whose hash failed and one the range rule refused"""
    h = Harness(libs[build])
    rnd = random.Random(1000 + bm_words)
    n_bits = 32 * bm_words
    parts, rows, part_st = [], [], []
    for i, k in enumerate(SIZES):
        for t in range(k):
            parts.append(points[1 + len(parts)])
            rows.append(row_of([rnd.randrange(n_bits) for _ in range(rnd.randrange(1, 5))] if n_bits else [], bm_words))
            part_st.append(0 if k <= 2 else [0, 0, 0, 9, 0, 2, 0, 4, 0, 6, 0, 1, 0][t % 13])
    if bm_words:
        rows[sum(SIZES[:-1])][-1] |= 1 << 31                                   # the first partial of the longest tuple: the row's last bit
    tuple_st = [0] * len(SIZES)
    taken, bits, counts, agg = check(h, c, parts, rows, SIZES, part_st, tuple_st, bm_words)
    at = sum(SIZES[:-1])
    if bm_words == 0:                                                          # empty rows are disjoint: every status-0 partial is taken
        assert taken == [int(s == 0) for s in part_st] and counts == [0] * len(SIZES)
    elif bm_words <= 3:
        assert 0 < sum(taken[at:]) < part_st[at:].count(0)                     # the row fills up: later partials overlap
    else:
        assert sum(taken[at:]) > 32 and bits[len(SIZES) * bm_words - 1] >> 31
    tuple_st2 = [0] * len(SIZES)
    tuple_st2[3], tuple_st2[4] = 1, 2
    st2 = list(part_st)
    at3 = sum(SIZES[:3])
    st2[at3:at3 + SIZES[3]] = [1] * SIZES[3]
    want2 = check(h, c, parts, rows, SIZES, st2, tuple_st2, bm_words)
    at4 = at3 + SIZES[3]
    assert want2[2][3] == 0 and want2[2][4] == 0 and want2[3][64 * 3:64 * 5] == bytes(128) and not any(want2[0][at3:at4 + SIZES[4]])


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("bm_words", [3, 65, 130])
def test_overlap_cases(libs, c, points, build, bm_words):
    h = Harness(libs[build])
    last = 32 * bm_words - 1
    far = [32 * 64 + 5, 32 * (bm_words - 1) + 9] if bm_words > 64 else [40, 70]      # words >= 64 where the row has them
    P = lambda j: points[1 + j]     # noqa: E731
    # distance 1 and distance 64: 66 partials with a bit of their own each (bit k), partial 1 also holding partial 0's, partial 65 partial 1's
    # (not taken, so no overlap: taken) and partial 66 — a 67th — partial 2's (taken 64 places before, the same lane's in the wave layout)
    own = [[k] for k in range(67)]
    own[1] = [1, 0]
    own[65] = [65, 1]
    own[66] = [66, 2]
    tuples = [
        [(P(1), [0, 1], 0), (P(2), [1, 2], 0)],                                        # an overlap with a taken partial
        [(P(3), [0, 1], 9), (P(4), [1, 2], 0)],                                        # an overlap with a refused partial only: taken
        [(P(5), [0, 1], 0), (P(6), [1, 2], 0), (P(7), [2, 3], 0)],                     # a chain: A and C
        [(P(8), [4, 9], 0), (P(8), [4, 9], 0)],                                        # the same partial twice
        [(P(9), [0, last], 0), (P(10), [1, last], 0), (P(11), [2], 0)],                # an overlap in the last bit of the last word only
        [(P(12), [0, far[0]], 0), (P(13), [1, far[0]], 0), (P(14), [2, far[1]], 0), (P(15), [3, far[1]], 0)],      # ... in a high word only
        [(P(16 + k), own[k], 0) for k in range(67)],
        [(points[0], [], 0), (P(90), [7], 0), (points[0], [], 0)],                     # a status-0 empty row (the identity): taken, adds nothing
        [(P(91), [0], 9), (P(92), [1], 2), (P(93), [2], 4), (P(94), [3], 6), (P(95), [4], 1)],      # every partial refused
        [(P(96 + k), [5 * k], [0, 1, 0, 2, 0, 4, 0, 6, 0, 9][k % 10]) for k in range(19)],        # statuses mixed in
        [(P(120), [0], 0), (P(121), [1], 0)],                                          # a refused tuple (below)
        [],
    ]
    parts = [p for t in tuples for p, _, _ in t]
    rows = [row_of(b, bm_words) for t in tuples for _, b, _ in t]
    part_st = [s for t in tuples for _, _, s in t]
    sizes = [len(t) for t in tuples]
    tuple_st = [0] * len(tuples)
    tuple_st[10] = 2
    taken, bits, counts, agg = check(h, c, parts, rows, sizes, part_st, tuple_st, bm_words)
    T = lambda i: taken[sum(sizes[:i]):sum(sizes[:i + 1])]      # noqa: E731
    A = lambda i: agg[64 * i:64 * i + 64]                       # noqa: E731
    assert T(0) == [1, 0] and T(1) == [0, 1] and T(2) == [1, 0, 1] and T(3) == [1, 0] and T(4) == [1, 0, 1] and T(5) == [1, 0, 1, 0]
    assert T(6) == [1, 0] + [1] * 64 + [0] and T(7) == [1, 1, 1] and T(8) == [0] * 5 and T(10) == [0, 0]
    assert counts[:6] == [2, 2, 4, 2, 3, 4] and counts[6] == 66 and counts[7] == 1 and counts[8] == 0 and counts[9] == 10 and counts[10:] == [0, 0]
    assert A(0) == P(1) and A(1) == P(4) and A(2) == c.g1_add(P(5), P(7)) and A(3) == P(8) and A(7) == P(90)
    assert A(8) == A(10) == A(11) == bytes(64)


@pytest.mark.parametrize("build", BUILDS)
def test_repeated_keys_and_the_collect_inside(libs, c, build):
    """tests/collect_repeat_cases.py as ONE-BIT partials (a key set that lists one key 128 times and its negation 64 times): a doubling and a
    cancellation at every level of the tree, all 64 slots doubling at all six levels, a lane's own stride adding sigma to sigma and to -sigma.
    Every valid share names an index of its own, so all are taken; both layouts against the model, the oracle's g1_add and the net multiple
    through g1_mul.  Then shares that DO repeat indices: rows, counts, aggregates and taken equal the collect's model (identity 3)."""
    from tests import collect_repeat_cases as rc
    h = Harness(libs[build])
    rnd = random.Random(17)
    st_h, base, _ = c.hash_to_g1(b"merge/repeated")
    assert st_h == 0
    a = rnd.randrange(1, R)
    sigma, neg = c.g1_mul(base, a.to_bytes(32, "big")), c.g1_mul(base, (R - a).to_bytes(32, "big"))
    b = [c.g1_mul(base, rnd.randrange(1, R).to_bytes(32, "big")) for _ in range(rc.N_B)]
    wrong = c.g1_add(sigma, base)
    cases = rc.shapes()
    shares, keys, sizes, status = rc.plant(cases, lambda i, kind, key: {"A": sigma, "N": neg, "W": wrong}.get(kind) or b[key - rc.K_B])
    rows = [row_of([k], rc.BM) for k in keys]
    taken, bits, counts, agg = check(h, c, shares, rows, sizes, status, [0] * len(sizes), rc.BM)
    assert taken == [int(s == 0) for s in status]
    for i, (name, sh) in enumerate(cases):
        m, bs, count = rc.net(sh)
        point = c.g1_mul(sigma, (m % R).to_bytes(32, "big")) if m % R else bytes(64)
        for j in bs:
            point = c.g1_add(point, b[j])
        assert agg[64 * i:64 * i + 64] == point and counts[i] == count, name
    # identity 3: shares over 40 keys in tuples of 0 .. 130, indices repeating, a valid and an invalid share of one key in both orders
    sig = [c.g1_mul(base, rnd.randrange(1, R).to_bytes(32, "big")) for _ in range(40)]
    shares, keys, st = [], [], []
    for i, k in enumerate(SIZES):
        for t in range(k):
            key = (7 * i + 3 * t) % 40 if t % 11 else (t // 11) % 40
            s = 0 if k <= 2 else [0, 0, 9, 0, 2, 0, 0, 4][(t + i) % 8]
            shares.append(sig[key] if s == 0 else c.g1_add(sig[key], base))
            keys.append(key)
            st.append(s)
    crow, ccount, chosen = collect_model.select(keys, st, SIZES, [0] * len(SIZES), 2)
    want_agg = b"".join(collect_model.aggregates(c, shares, chosen))
    first = [int(p in {s for pick in chosen for s in pick}) for p in range(len(keys))]
    for layout in (0, 1):
        got = h.merge(shares, [row_of([k], 2) for k in keys], SIZES, st, [0] * len(SIZES), 2, layout)
        assert got == (first, [w for r in crow for w in r], ccount, want_agg), layout
    assert 0 < sum(first) < st.count(0)


def test_stand_alone_under_sanitizers(tmp_path):
    """hostsim_merge.cpp with its own main, under AddressSanitizer and UBSan, run directly: exact-size buffers, both layouts, rows of 0 .. 130
    words, tuples of 0 .. 130 partials; the program checks its results itself (multiples of the generator)"""
    exe = str(tmp_path / "hostsim_merge_san")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DHM_MAIN",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "hostsim_merge ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
