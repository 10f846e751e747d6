"""bn254_batch_merge_keyed_bitmap_optimistic[_device] (include/bn254_hip.h), without a GPU:
- the two entry points and the debug hook are declared with the stated arity and the exact merge's arguments, exported with matching
  argtypes, bound in INTEGRATION.md's extern block; option 45 has a number of its own and an engine mirror;
- the Python mirrors refuse malformed items before they touch a device;
- tests/merge_opt_model.py end to end over the oracle (hash_to_g1, g1_add, g2_add, pairing_check): a passing tuple, a wrong partial, a pair
  of partials whose errors cancel, a key and its negation, an overlap, a non-identity partial with an empty row, a tuple with no candidate;
- the device code of the route (bn254_amd/csrc/bn254_merge.h: mgo_*), compiled for the host (tests/hostsim/hostsim_merge_opt.cpp, plain and
  under -DBN_TRACK_BOUNDS), over GIVEN arrays against the model in both layouts: the pre-check statuses, the overlap report (adjacent
  partials, at distance 64, only in a word >= 64), an empty-row candidate counted as a candidate, the queue whole and sliced, and the masked
  re-select, which leaves a marker in a passing tuple's row, aggregate and part_taken alone.  Tuples of 0 .. 130 partials, rows of 0 .. 130
  words;
- the same source as a stand-alone program under AddressSanitizer and UBSan."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from bn254_amd import _native
from tests import merge_model
from tests import merge_opt_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254_batch_merge_keyed_bitmap_optimistic", "bn254_batch_merge_keyed_bitmap_optimistic_device"]
EXACT_NAMES = ["bn254_batch_merge_keyed_bitmap", "bn254_batch_merge_keyed_bitmap_device"]
HOOK = "bn254_debug_merge_opt_last"
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_merge_opt.cpp")
R = M.R
SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130]
WIDTHS = [0, 1, 2, 3, 64, 65, 130]


def _arity(decl):
    return len([a for a in decl.split(",") if a.strip()])


def _header():
    return open(os.path.join(ROOT, "include", "bn254_hip.h")).read()


def _header_decls(names=NAMES):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr) for name in names}


def test_declared_like_the_exact_pair():
    both = _header_decls(NAMES + EXACT_NAMES + [HOOK])
    for name in NAMES + [HOOK]:
        assert both[name], name
        assert name in _native.EXPORTED_SYMBOLS
    assert _arity(both[NAMES[0]].group(1)) == 16 and _arity(both[NAMES[1]].group(1)) == 17

    def squash(t):
        return re.sub(r"\s+", " ", t).strip()
    assert squash(both[NAMES[0]].group(1)) == squash(both[EXACT_NAMES[0]].group(1))          # the exact call's arguments, no seed
    assert squash(both[NAMES[1]].group(1)) == squash(both[EXACT_NAMES[1]].group(1))
    assert re.search(r"uint64_t\s+out\[4\]", both[HOOK].group(1))


def test_option_45():
    from bn254_amd import engine
    hdr = _header()
    assert re.search(r"#define BN254_OPT_MERGE_OPT_MIN_PARTS 45\b", hdr) and engine.OPT_MERGE_OPT_MIN_PARTS == 45
    numbers = [int(x) for x in re.findall(r"#define BN254_OPT_\w+ (\d+)\b", hdr)]
    assert numbers.count(45) == 1 and len(numbers) == len(set(numbers))       # used once in the header
    mirrored = [v for k, v in vars(engine).items() if k.startswith("OPT_")]
    assert mirrored.count(45) == 1                                            # ... and once in the mirror
    ws = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    assert int(re.search(r"#define MERGE_OPT_MIN_PARTS_DEFAULT (\d+)", ws).group(1)) == engine.MERGE_OPT_MIN_PARTS_DEFAULT
    hpp = open(os.path.join(ROOT, "bn254_amd", "host", "bn254.hpp")).read()
    assert "BN254_OPT_MERGE_OPT_MIN_PARTS" in hpp and "bn254_batch_merge_keyed_bitmap_optimistic" in hpp
    for name in ("merge_keyed_bitmap_optimistic", "merge_keyed_bitmap_optimistic_device", "debug_merge_opt_last"):
        assert hasattr(engine.Engine, name), name


def test_exported_by_the_library():
    _native.build()
    lib = _native.load()
    decls = _header_decls(NAMES + [HOOK])
    for name in NAMES + [HOOK]:
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == _arity(decls[name].group(1))


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
    for items in ([(b"a", [(sig, [0])]), (b"b",)], [(b"a", [(sig, [0])], [1])], [b"ab"], [(b"a", [(sig, [0], 1)])], [(b"a", [(sig,)])],
                  [(b"a", [(sig, [0]), (short, [1])])]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.batch_merge_keyed_signers_optimistic(items)
        assert e.value.kind == api.ErrorKind.InvalidLength, items
    for idx in ([0, -1], [1 << 32, 0]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.merge_keyed_signers_optimistic(b"a", [(sig, [3]), (sig, idx)])
        assert e.value.kind == api.ErrorKind.IndexOutOfBounds
    with pytest.raises(AssertionError):
        engine.Engine.merge_keyed_bitmap_optimistic(None, [b"a", b"b"], bytes(128), [1, 2], [1, 2], 1)
    with pytest.raises(AssertionError):
        engine.Engine.merge_keyed_bitmap_optimistic(None, [b"a"], bytes(128), [1, 2, 3], [2], 2)
    assert "cancel" in api.ECDSA.merge_keyed_signers_optimistic.__doc__ and "cancel" in api.ECDSA.batch_merge_keyed_signers_optimistic.__doc__


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def row_of(bits, bm_words):
    row = [0] * bm_words
    for b in bits:
        row[b // 32] |= 1 << (b % 32)
    return row


def test_model_over_the_oracle(c):
    """six keys (key 5 = the negation of key 1), real partial aggregates (sum of the secrets) * H(m): every step of the model with the
    oracle's pairing as both checks"""
    rnd = random.Random(45)
    sks = [rnd.randrange(1, R) for _ in range(5)]
    sks.append(R - sks[1])
    pks = [c.g2_mul(c.g2_generator(), s.to_bytes(32, "big")) for s in sks]
    msgs = [b"merge-opt/model/%d" % i for i in range(7)]
    h = [c.hash_to_g1(m)[1] for m in msgs]
    g1 = c.g1_generator()
    neg_g1 = c.g1_mul(g1, (R - 1).to_bytes(32, "big"))

    def sig(i, keys):
        s = sum(sks[k] for k in keys) % R
        return c.g1_mul(h[i], s.to_bytes(32, "big")) if s else bytes(64)
    tuples = [
        [(sig(0, [0, 2]), [0, 2]), (sig(0, [3]), [3]), (bytes(64), [])],                              # passes; the empty-row identity is taken
        [(sig(1, [0]), [0]), (c.g1_add(sig(1, [2, 3]), g1), [2, 3]), (sig(1, [4]), [4])],               # one wrong partial: the exact way
        [(c.g1_add(sig(2, [0]), g1), [0]), (c.g1_add(sig(2, [3, 4]), neg_g1), [3, 4]), (sig(2, [2]), [2])],      # errors that cancel: passes, all taken
        [(sig(3, [1]), [1]), (sig(3, [5]), [5])],                                                   # a key and its negation: identity sum, identity key
        [(sig(4, [0, 2]), [0, 2]), (sig(4, [2, 3]), [2, 3]), (sig(4, [4]), [4])],                     # an overlap: the exact way
        [(sig(5, [0]), [0]), (g1, [])],                                                             # a non-identity partial with an empty row: fails
        [(sig(6, [0]), [0, 9]), (b"\xff" + sig(6, [1])[1:], [1])],                                  # no candidate: FINAL
    ]
    parts = [p for t in tuples for p, _ in t]
    rows = [row_of(b, 1) for t in tuples for _, b in t]
    sizes = [len(t) for t in tuples]
    n = len(tuples)
    pre = M.precheck([c.g1_validate(p, 0) for p in parts], rows, [0] * 6, sizes, [0] * n)
    assert pre == [0] * 16 + [2, 6]
    tuple_check, part_check = M.oracle_checks(c, msgs, parts, rows, sizes, pks)
    out = M.merge(rows, pre, sizes, [0] * n, 1, tuple_check, part_check)
    assert out["flags"] == [M.CHECK, M.CHECK, M.CHECK, M.CHECK, M.EXACT, M.CHECK, M.FINAL]
    assert out["verdicts"] == [0, 9, 0, 0, None, 9, None]
    assert out["hook"] == dict(checked=5, passed=3, exact_tuples=3, exact_parts=3 + 3 + 2)
    assert out["part_status"] == [0, 0, 0, 0, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 9, 2, 6] and out["queue"] == [3, 4, 5, 11, 12, 13, 14, 15]
    assert out["taken"] == [1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 0, 0, 0]
    assert [r[0] for r in out["rows"]] == [0b1101, 0b10001, 0b11101, 0b100010, 0b10101, 0b1, 0] and out["counts"] == [3, 2, 4, 2, 3, 1, 0]
    agg = merge_model.aggregates(c, parts, sizes, out["taken"])
    assert agg[2] == sig(2, [0, 3, 4, 2]) and agg[3] == bytes(64) and agg[6] == bytes(64)        # the deviation: still the honest sum
    rng = M.ranges(sizes)
    for i in range(n):                                                       # identity 2 by the oracle
        assert tuple_check(i, out["rows"][i], [p for p in range(*rng[i]) if out["taken"][p]]) == 0, i
    # the exact call on the same input (step 7, every partial by the pairing): the cancelling pair reads 9, 9 and is left out
    exact = M.merge(rows, pre, sizes, [0] * n, 1, tuple_check, part_check, routed=False)
    assert exact["part_status"][6:8] == [9, 9] and exact["taken"][6:9] == [0, 0, 1] and exact["hook"] == dict(checked=0, passed=0, exact_tuples=0, exact_parts=0)
    differ = [p for p in range(len(parts)) if exact["part_status"][p] != out["part_status"][p]]
    assert differ == [6, 7]
    for i in (0, 1, 3, 4, 5, 6):                                             # every tuple without a cancelling pair: the exact call's outputs
        assert exact["rows"][i] == out["rows"][i] and exact["taken"][rng[i][0]:rng[i][1]] == out["taken"][rng[i][0]:rng[i][1]], i


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    out = tmp_path_factory.mktemp("hmo")
    common = ["-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libhmo_%s.so" % name))
        procs[name] = (so, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + common + ["-o", so, SRC], stderr=subprocess.PIPE, text=True))
    for name, (so, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: so for name, (so, _) in procs.items()}


BUILDS = ["plain", "bounds"]


def _offsets(sizes):
    ends = [0]
    for k in sizes:
        ends.append(ends[-1] + k)
    return ends


class Harness:
    def __init__(self, path):
        self.lib = ctypes.CDLL(path)
        vp, sz, u32, u64 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_uint64
        self.lib.hmo_precheck.argtypes = [vp, vp, vp, vp, vp, sz, u64, sz, u32, vp, u32, vp]
        self.lib.hmo_precheck.restype = None
        self.lib.hmo_select.argtypes = [vp, vp, vp, vp, vp, sz, sz, ctypes.c_int, vp, vp, vp, vp, vp, vp]
        self.lib.hmo_select.restype = None
        self.lib.hmo_settle.argtypes = [sz, sz, vp, vp, vp, vp]
        self.lib.hmo_settle.restype = None
        self.lib.hmo_queue.argtypes = [vp, vp, sz, u64, u64, vp, vp, vp, vp]
        self.lib.hmo_queue.restype = u64

    @staticmethod
    def _arrays(parts, rows, sizes, bm_words):
        n = len(sizes)
        return (b"".join(parts) + bytes(4), (ctypes.c_uint32 * (len(rows) * bm_words + 1))(*[w for r in rows for w in r]), (ctypes.c_uint64 * (n + 1))(*_offsets(sizes)))

    def precheck(self, parts, rows, sizes, tuple_st, hash_st, bm_words, flags, key_st):
        blob, words, off = self._arrays(parts, rows, sizes, bm_words)
        out = ctypes.create_string_buffer(b"\x02" * len(parts), len(parts) + 1)
        self.lib.hmo_precheck(blob, words, off, bytes(tuple_st) + b"\0", bytes(hash_st) + b"\0", len(sizes), len(parts), bm_words, flags, bytes(key_st) + b"\0",
                              len(key_st), out)
        return list(out.raw[:len(parts)])

    def select(self, parts, rows, sizes, part_st, tuple_st, bm_words, layout, state=None):
        """state None: the provisional select-and-sum on zeroed rows and part_taken -> (taken, bits, counts, agg, flags).  state = (verdict,
        flag, taken, bits, counts, agg): the re-select on those arrays -> the same five"""
        n, n_parts = len(sizes), len(parts)
        blob, words, off = self._arrays(parts, rows, sizes, bm_words)
        if state is None:
            verdict, flag = None, ctypes.create_string_buffer(b"\xEE" * n, n + 1)
            taken = ctypes.create_string_buffer(n_parts + 1)
            bits, counts, agg = (ctypes.c_uint32 * (n * bm_words + 1))(), (ctypes.c_uint32 * (n + 1))(), ctypes.create_string_buffer(64 * n + 1)
        else:
            verdict, flag = bytes(state[0]) + b"\0", ctypes.create_string_buffer(bytes(state[1]), n + 1)
            taken = ctypes.create_string_buffer(bytes(state[2]), n_parts + 1)
            bits, counts = (ctypes.c_uint32 * (n * bm_words + 1))(*state[3]), (ctypes.c_uint32 * (n + 1))(*state[4])
            agg = ctypes.create_string_buffer(state[5], 64 * n + 1)
        self.lib.hmo_select(blob, words, off, bytes(part_st) + b"\0", bytes(tuple_st) + b"\0", n, bm_words, layout, verdict, flag, taken, bits, agg, counts)
        assert bits[n * bm_words] == 0 and counts[n] == 0 and taken.raw[n_parts:] == b"\0" and agg.raw[64 * n:] == b"\0" and flag.raw[n:] == b"\0"
        return list(taken.raw[:n_parts]), list(bits)[:n * bm_words], list(counts)[:n], agg.raw[:64 * n], list(flag.raw[:n])

    def settle(self, bm_words, flag, verdict, bits):
        n = len(flag)
        b = (ctypes.c_uint32 * (n * bm_words + 1))(*bits)
        stats = (ctypes.c_uint32 * 3)()
        self.lib.hmo_settle(n, bm_words, bytes(flag) + b"\0", bytes(verdict) + b"\0", b, stats)
        return list(b)[:n * bm_words], list(stats)

    def queue(self, sizes, tuple_st, part_st, flag, verdict, base, length):
        n = len(sizes)
        out = (ctypes.c_uint32 * max(length, 1))()
        cnt = self.lib.hmo_queue((ctypes.c_uint64 * (n + 1))(*_offsets(sizes)), bytes(tuple_st) + b"\0", n, base, length, bytes(part_st) + b"\0",
                                 bytes(flag) + b"\0", bytes(verdict) + b"\0", out)
        return [base + j for j in list(out)[:cnt]]


@pytest.fixture(scope="module")
def points(c):
    """multiples of one base (the checks are given, so any point serves as a partial's signature); [0] = the identity"""
    rnd = random.Random(20261019)
    st_h, base, _ = c.hash_to_g1(b"merge-opt/host")
    assert st_h == 0
    return [bytes(64)] + [c.g1_mul(base, rnd.randrange(1, R).to_bytes(32, "big")) for _ in range(sum(SIZES) + 140)]


@pytest.mark.parametrize("build", BUILDS)
def test_precheck_statuses(libs, c, points, build):
    """decode statuses 6 (a coordinate >= q) and 4 (off the curve; the identity under REJECT_IDENTITY), rule 2 with the LOWEST bad bit
    deciding (a refused key below a bit beyond the set, and the other way round), hash status 1 and 5, a refused tuple (every partial keeps the
    2 of the fill), empty rows: the first of the three rules, at rows of 2 and of 66 words"""
    h = Harness(libs[build])
    for bm_words, n_keys in ((2, 40), (66, 2100), (1, 32), (0, 0)):
        key_st = [0] * n_keys
        if n_keys >= 40:
            key_st[7], key_st[8], key_st[9], key_st[n_keys - 1] = 4, 6, 3, 4
        big = bytearray(points[2]); big[0] = 0xFF
        off_curve = bytearray(points[3]); off_curve[40] ^= 4
        parts, rows = [], []
        for i, k in enumerate(SIZES):
            for t in range(k):
                kind = t % 13
                parts.append(bytes(big) if kind == 3 else bytes(off_curve) if kind == 5 else bytes(64) if kind == 7 else points[1 + len(parts)])
                bits = [] if not n_keys else [(7 * i + 3 * t) % n_keys] + ([n_keys - 1] if kind == 2 else []) + ([32 * bm_words - 1] if kind == 9 and 32 * bm_words > n_keys else [])
                rows.append(row_of([] if kind == 11 else bits, bm_words))
        tuple_st = [0] * len(SIZES)
        tuple_st[3], tuple_st[4], tuple_st[6] = 1, 2, 5
        for flags in (0, 2):
            got = h.precheck(parts, rows, SIZES, tuple_st, tuple_st, bm_words, flags, key_st)
            want = M.precheck([c.g1_validate(p, flags) for p in parts], rows, key_st, SIZES, tuple_st)
            assert got == want, (bm_words, flags, [(p, a, b) for p, (a, b) in enumerate(zip(got, want)) if a != b][:8])
            lo = sum(SIZES[:4])
            assert got[lo:lo + SIZES[4]] == [2] * SIZES[4]
            if n_keys == 40:
                assert {0, 1, 2, 3, 4, 5, 6} <= set(got)
        assert h.precheck(parts, rows, SIZES, tuple_st, tuple_st, bm_words, 2, key_st) != h.precheck(parts, rows, SIZES, tuple_st, tuple_st, bm_words, 0, key_st)


def _case(points, bm_words):
    """the ten sizes — partial t of a tuple holds bit t where the row has it (so a tuple within the row's width is pairwise disjoint: CHECK),
    pre-check statuses given (0, 2, 3, 4, 6, 1 mixed in) — then the named tuples: an overlap between adjacent partials, at distance 64 (the
    same lane's partial sum in the wave layout), only in a word >= 64 (where the row has one), an overlap with a non-candidate only (none),
    empty-row candidates alone and among others, and a tuple of non-candidates only.  truth[p]: what the exact verify gives candidate p"""
    n_bits = 32 * bm_words
    P = lambda j: points[1 + j]      # noqa: E731
    tuples = []
    at = 0
    for i, k in enumerate(SIZES):
        t = []
        for j in range(k):
            st = 0 if k <= 2 else [0, 0, 0, 4, 0, 2, 0, 3, 0, 6, 0, 1, 0][j % 13]
            t.append([P(at), [j % n_bits] if n_bits else [], st, 0])
            at += 1
        tuples.append(t)
    for i, j in ((3, 2), (8, 4)):                                          # one wrong candidate in the 15-partial tuple and in the 65-partial one
        assert tuples[i][j][2] == 0
        tuples[i][j][3] = 9
    hi = [32 * 64 + 5, n_bits - 1] if bm_words > 64 else [n_bits - 1, n_bits - 2] if n_bits > 8 else [0, 0]
    if n_bits:
        w = min(n_bits, 70)
        far = [[P(300 + k), [k % w], 0, 0] for k in range(70)]
        far[66][1] = [66 % w, 2 % w]                                       # partial 66 meets partial 2: 64 places apart
        tuples += [
            [[P(200), [0, 1], 0, 0], [P(201), [1, 2 % n_bits], 0, 0]],                              # adjacent
            far,
            [[P(202), [0, hi[0]], 0, 0], [P(203), [1, hi[0]], 0, 0], [P(204), [2, hi[1]], 0, 9]],   # only in a high word; a wrong one behind it
            [[P(205), [0, 1], 9, 0], [P(206), [1, 2 % n_bits], 0, 0]],                              # meets a non-candidate only: CHECK
        ]
    tuples += [
        [[points[0], [], 0, 0]],                                            # an empty-row candidate alone: a candidate (CHECK), the row stays empty
        [[P(207), [], 0, 9]],                                               # ... a point: its check fails
        [[points[0], [], 0, 0], [P(208), [0] if n_bits else [], 0, 0], [points[0], [], 0, 0]],
        [[P(209), [0] if n_bits else [], 4, 0], [P(210), [], 2, 0]],        # no candidate: FINAL
    ]
    parts = [x[0] for t in tuples for x in t]
    rows = [row_of(x[1], bm_words) for t in tuples for x in t]
    pre = [x[2] for t in tuples for x in t]
    truth = [x[3] for t in tuples for x in t]
    return parts, rows, pre, truth, [len(t) for t in tuples]


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("bm_words", WIDTHS)
def test_overlaps_queue_and_masked_reselect(libs, c, points, build, bm_words):
    h = Harness(libs[build])
    parts, rows, pre, truth, sizes = _case(points, bm_words)
    assert sizes[:len(SIZES)] == SIZES
    n, n0 = len(sizes), len(SIZES)
    tuple_st = [0] * n
    flags_want = [f for f, _ in M.tuple_flags(rows, pre, sizes, tuple_st, bm_words)]
    if bm_words:
        assert flags_want[n0:] == [M.EXACT, M.EXACT, M.EXACT, M.CHECK, M.CHECK, M.CHECK, M.CHECK, M.FINAL], flags_want[n0:]
        assert flags_want[:3] == [M.FINAL, M.CHECK, M.CHECK]
        assert all(f == (M.CHECK if k <= 32 * bm_words else M.EXACT) for f, k in zip(flags_want[1:n0], SIZES[1:]))
    else:
        assert flags_want == [M.FINAL] + [M.CHECK] * 9 + [M.CHECK, M.CHECK, M.CHECK, M.FINAL]      # empty rows never overlap
    # the tuple check as given: a CHECK tuple fails iff it holds a wrong candidate — and one all-valid tuple fails all the same (index 5)
    ranges = M.ranges(sizes)

    def tuple_check(i, row, taken_parts):
        return 9 if i == 5 or any(truth[p] for p in range(*ranges[i]) if pre[p] == 0) else 0
    want = M.merge(rows, pre, sizes, tuple_st, bm_words, tuple_check, lambda p: truth[p])
    assert want["flags"] == flags_want
    want_agg = b"".join(merge_model.aggregates(c, parts, sizes, want["taken"]))
    verdict = [0xEE if v is None else v for v in want["verdicts"]]         # read for CHECK tuples only
    pro_rows, pro_counts, pro_taken = merge_model.select(rows, pre, sizes, tuple_st, bm_words)
    pro_agg = merge_model.aggregates(c, parts, sizes, pro_taken)
    seen = []
    for layout in (0, 1):
        taken, bits, counts, agg, flag = h.select(parts, rows, sizes, pre, tuple_st, bm_words, layout)
        assert flag == flags_want, (layout, [(i, a, b) for i, (a, b) in enumerate(zip(flag, flags_want)) if a != b])
        assert taken == pro_taken and bits == [w for r in pro_rows for w in r] and counts == pro_counts and agg == b"".join(pro_agg), layout
        settled, stats = h.settle(bm_words, flag, verdict, bits)
        assert stats == [want["hook"]["checked"], want["hook"]["passed"], want["hook"]["exact_tuples"]]
        for i in range(n):
            exact = flag[i] == M.EXACT or (flag[i] == M.CHECK and verdict[i] != 0)
            assert settled[bm_words * i:bm_words * i + bm_words] == ([0] * bm_words if exact else bits[bm_words * i:bm_words * i + bm_words]), i
        # the queue, whole and in slices of 64 and 37 partials
        n_parts = len(parts)
        assert h.queue(sizes, tuple_st, pre, flag, verdict, 0, n_parts) == want["queue"] and len(want["queue"]) == want["hook"]["exact_parts"]
        for chunk in (64, 37):
            got = [p for lo in range(0, n_parts, chunk) for p in h.queue(sizes, tuple_st, pre, flag, verdict, lo, min(chunk, n_parts - lo))]
            assert got == want["queue"], chunk
        # the exact verify of the queued candidates as given, then the re-select in either layout on the settled rows
        queued = set(want["queue"])
        status = [truth[p] if p in queued else pre[p] for p in range(n_parts)]
        assert status == want["part_status"]
        passing = [i for i in range(n) if not (flag[i] == M.EXACT or (flag[i] == M.CHECK and verdict[i] != 0))]
        # markers: a passing tuple's row, aggregate, count and part_taken must survive; a fallback tuple's part_taken is rewritten throughout
        m_taken, m_bits, m_counts, m_agg = list(taken), list(settled), list(counts), bytearray(agg)
        for i in range(n):
            lo, hi = ranges[i]
            if i in passing:
                m_agg[64 * i:64 * i + 64] = b"\xA5" * 64
                m_taken[lo:hi] = [0xA5] * (hi - lo)
                m_counts[i] = 0xA5A5
                if bm_words:
                    m_bits[bm_words * i] ^= 0x80000000
            else:
                m_taken[lo:hi] = [0x55] * (hi - lo)
        for relayout in (0, 1):
            t2, b2, c2, a2, f2 = h.select(parts, rows, sizes, status, tuple_st, bm_words, relayout, state=(verdict, flag, m_taken, m_bits, m_counts, bytes(m_agg)))
            assert f2 == flag                                               # the re-select writes no flags
            for i in range(n):
                lo, hi = ranges[i]
                if i in passing:
                    assert (t2[lo:hi], b2[bm_words * i:bm_words * i + bm_words], c2[i], a2[64 * i:64 * i + 64]) == \
                        (m_taken[lo:hi], m_bits[bm_words * i:bm_words * i + bm_words], m_counts[i], bytes(m_agg[64 * i:64 * i + 64])), (layout, relayout, i)
                else:
                    assert (t2[lo:hi], b2[bm_words * i:bm_words * i + bm_words], c2[i], a2[64 * i:64 * i + 64]) == \
                        (want["taken"][lo:hi], want["rows"][i], want["counts"][i], want_agg[64 * i:64 * i + 64]), (layout, relayout, i)
            seen.append((t2, b2, c2, a2))
    assert all(s == seen[0] for s in seen)
    # the fallback tuples are the exact call's: first fit over the final statuses
    rows_x, counts_x, taken_x = merge_model.select(rows, want["part_status"], sizes, tuple_st, bm_words)
    for i in range(n):
        if i not in passing:
            assert want["rows"][i] == rows_x[i] and want["counts"][i] == counts_x[i] and want["taken"][ranges[i][0]:ranges[i][1]] == taken_x[ranges[i][0]:ranges[i][1]]
    # a refused tuple (status 2) has no partials on this route either
    tuple_st2 = list(tuple_st)
    tuple_st2[7] = 2
    pre2 = list(pre)
    lo, hi = ranges[7]
    pre2[lo:hi] = [2] * (hi - lo)
    taken, bits, counts, agg, flag = h.select(parts, rows, sizes, pre2, tuple_st2, bm_words, 1)
    assert flag[7] == M.FINAL and counts[7] == 0 and agg[64 * 7:64 * 8] == bytes(64) and bits[bm_words * 7:bm_words * 8] == [0] * bm_words and not any(taken[lo:hi])


def test_stand_alone_under_sanitizers(tmp_path):
    """hostsim_merge_opt.cpp with its own main, under AddressSanitizer and UBSan, run directly: exact-size buffers, both layouts, rows of
    0 .. 130 words, tuples of 0 .. 130 partials, pre-check, select, queue and re-select; the program checks its results itself"""
    exe = str(tmp_path / "hostsim_merge_opt_san")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DHMO_MAIN",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "hostsim_merge_opt ok" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
