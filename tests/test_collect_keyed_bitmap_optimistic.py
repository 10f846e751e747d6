"""bn254_batch_collect_keyed_bitmap_optimistic[_device] (include/bn254_hip.h), without a GPU:
- the two entry points and the debug hook are declared with the stated arity, exported with matching argtypes, bound in INTEGRATION.md's
  extern block; options 40 and 41 have numbers of their own and engine mirrors;
- the Python mirrors refuse malformed items before they touch a device;
- tests/collect_opt_model.py end to end over the oracle (hash_to_g1, g1_add, g2_add, pairing_check): a passing tuple, a wrong share, a pair
  of shares whose errors cancel, a key and its negation, a duplicate;
- the device code of the route (bn254_amd/csrc/bn254_collect.h: clo_*), compiled for the host (tests/hostsim/hostsim_collect_opt.cpp, plain
  and under -DBN_TRACK_BOUNDS), over GIVEN arrays against the model: the pre-check statuses, duplicate detection in both sum layouts (in one
  lane's stride and across lanes), the queue from a given verdict array and given flags, and the masked re-sum, which leaves the rows and
  aggregates of passing tuples untouched.  Tuples of 0 .. 130 shares."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from bn254_amd import _native
from tests import collect_model
from tests import collect_opt_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254_batch_collect_keyed_bitmap_optimistic", "bn254_batch_collect_keyed_bitmap_optimistic_device"]
HOOK = "bn254_debug_collect_opt_last"
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_collect_opt.cpp")
R = M.R
SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130]


def _arity(decl):
    return len([a for a in decl.split(",") if a.strip()])


def _header():
    return open(os.path.join(ROOT, "include", "bn254_hip.h")).read()


def _header_decls(names=NAMES):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr) for name in names}


def test_declared_like_the_exact_pair():
    both = _header_decls(NAMES + ["bn254_batch_collect_keyed_bitmap", "bn254_batch_collect_keyed_bitmap_device", HOOK])
    for name in NAMES + [HOOK]:
        assert both[name], name
        assert name in _native.EXPORTED_SYMBOLS
    assert _arity(both[NAMES[0]].group(1)) == 15 and _arity(both[NAMES[1]].group(1)) == 16

    def squash(t):
        return re.sub(r"\s+", " ", t).strip()
    assert squash(both[NAMES[0]].group(1)) == squash(both["bn254_batch_collect_keyed_bitmap"].group(1))          # the exact call's arguments, no seed
    assert squash(both[NAMES[1]].group(1)) == squash(both["bn254_batch_collect_keyed_bitmap_device"].group(1))
    assert re.search(r"uint64_t\s+out\[4\]", both[HOOK].group(1))


def test_options_40_and_41():
    from bn254_amd import engine
    hdr = _header()
    assert re.search(r"#define BN254_OPT_COLLECT_OPT_MIN_SHARES 40\b", hdr) and engine.OPT_COLLECT_OPT_MIN_SHARES == 40
    assert re.search(r"#define BN254_OPT_COLLECT_OPT_MIN_TUPLE_SHARES 41\b", hdr) and engine.OPT_COLLECT_OPT_MIN_TUPLE_SHARES == 41
    numbers = [int(x) for x in re.findall(r"#define BN254_OPT_\w+ (\d+)\b", hdr)]
    assert numbers.count(40) == 1 and numbers.count(41) == 1 and len(numbers) == len(set(numbers))
    ws = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    assert int(re.search(r"#define COLLECT_OPT_MIN_SHARES_DEFAULT (\d+)", ws).group(1)) == engine.COLLECT_OPT_MIN_SHARES_DEFAULT
    assert int(re.search(r"#define COLLECT_OPT_MIN_TUPLE_SHARES_DEFAULT (\d+)", ws).group(1)) == engine.COLLECT_OPT_MIN_TUPLE_SHARES_DEFAULT


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
    for items in ([(b"a", [sig], [0]), (b"b", [sig])], [(b"a", [sig], [0], [1])], [(b"a", [sig, sig], [0])], [(b"a", [], [3])]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.batch_aggregate_keyed_signers_optimistic(items)
        assert e.value.kind == api.ErrorKind.InvalidLength
    for idx in ([0, -1], [1 << 32, 0]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.aggregate_keyed_signers_optimistic(b"a", [sig, sig], idx)
        assert e.value.kind == api.ErrorKind.IndexOutOfBounds

    class Blind:
        pass
    with pytest.raises(ValueError):
        api.ECDSA.aggregate_keyed_signers_optimistic(b"a", [sig], [0], engine=Blind())
    with pytest.raises(AssertionError):
        engine.Engine.batch_collect_keyed_bitmap_optimistic(None, [b"a", b"b"], bytes(128), [0, 1], [1, 2], 1)
    with pytest.raises(AssertionError):
        engine.Engine.batch_collect_keyed_bitmap_optimistic(None, [b"a"], bytes(64), [0, 1], [2], 1)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def test_model_over_the_oracle(c):
    """six keys (key 5 = the negation of key 1), real signatures sk * H(m): every step of the model with the oracle's pairing as both checks"""
    rnd = random.Random(40)
    sks = [rnd.randrange(1, R) for _ in range(5)]
    sks.append(R - sks[1])
    pks = [c.g2_mul(c.g2_generator(), s.to_bytes(32, "big")) for s in sks]
    msgs = [b"collect-opt/model/%d" % i for i in range(6)]
    h = [c.hash_to_g1(m)[1] for m in msgs]
    g1 = c.g1_generator()
    neg_g1 = c.g1_mul(g1, (R - 1).to_bytes(32, "big"))
    sig = lambda i, k: c.g1_mul(h[i], sks[k].to_bytes(32, "big"))     # noqa: E731
    tuples = [
        [(sig(0, 0), 0), (sig(0, 2), 2), (sig(0, 3), 3)],                                   # passes
        [(sig(1, 0), 0), (c.g1_add(sig(1, 2), g1), 2), (sig(1, 4), 4)],                     # one wrong share: the exact way
        [(c.g1_add(sig(2, 0), g1), 0), (c.g1_add(sig(2, 3), neg_g1), 3), (sig(2, 4), 4)],   # errors that cancel: passes, both counted
        [(sig(3, 1), 1), (sig(3, 5), 5)],                                                   # a key and its negation: identity aggregate, identity key
        [(sig(4, 2), 2), (sig(4, 2), 2), (sig(4, 3), 3)],                                   # a duplicate: the exact way
        [(sig(5, 0), 0), (sig(5, 1), 9)],                                                   # one candidate: below the minimum of 2
    ]
    shares = [s for t in tuples for s, _ in t]
    keys = [k for t in tuples for _, k in t]
    sizes = [len(t) for t in tuples]
    pre = M.precheck([c.g1_validate(s, 0) for s in shares], keys, [0] * 6, sizes, [0] * 6)
    assert pre == [0] * 14 + [0, 2]
    tuple_check, share_check = M.oracle_checks(c, msgs, shares, keys, sizes, pks)
    out = M.collect(keys, pre, sizes, [0] * 6, 1, 2, tuple_check, share_check)
    assert out["flags"] == [M.CHECK, M.CHECK, M.CHECK, M.CHECK, M.EXACT, M.EXACT]
    assert out["verdicts"] == [0, 9, 0, 0, None, None]
    assert out["hook"] == dict(checked=4, passed=3, exact_tuples=3, exact_shares=3 + 3 + 1)
    assert out["share_status"] == [0, 0, 0, 0, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 2] and out["queue"] == [3, 4, 5, 11, 12, 13, 14]
    assert [r[0] for r in out["rows"]] == [0b1101, 0b10001, 0b11001, 0b100010, 0b1100, 0b1] and out["counts"] == [3, 2, 3, 2, 2, 1]
    agg = collect_model.aggregates(c, shares, out["chosen"])
    assert agg[2] == c.g1_add(c.g1_add(sig(2, 0), sig(2, 3)), sig(2, 4)) and agg[3] == bytes(64)      # the deviation: still the honest sum
    # identity 2 by the oracle: every aggregate verifies against the sum of its row's keys
    for i in range(6):
        assert tuple_check(i, out["rows"][i], out["chosen"][i]) == 0, i
    # the exact call on the same input (every share by the pairing): the cancelling pair reads 9, 9 and is left out
    exact_st = [st or share_check(s) for s, st in enumerate(pre)]
    assert exact_st[6:8] == [9, 9] and [a == b for a, b in zip(exact_st, out["share_status"])].count(False) == 2
    # with the per-tuple minimum above every tuple the model IS the exact call
    all_exact = M.collect(keys, pre, sizes, [0] * 6, 1, 4, tuple_check, share_check)
    assert all_exact["share_status"] == exact_st and all_exact["hook"] == dict(checked=0, passed=0, exact_tuples=6, exact_shares=15)
    assert all_exact["rows"] == collect_model.select(keys, exact_st, sizes, [0] * 6, 1)[0]


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    out = tmp_path_factory.mktemp("hco")
    common = ["-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libhco_%s.so" % name))
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
        self.lib.hco_precheck.argtypes = [vp, vp, vp, vp, vp, sz, u64, u32, vp, u32, vp]
        self.lib.hco_precheck.restype = None
        self.lib.hco_sum.argtypes = [vp, vp, vp, vp, vp, sz, sz, ctypes.c_int, u32, vp, vp, vp, vp, vp]
        self.lib.hco_sum.restype = None
        self.lib.hco_settle.argtypes = [sz, sz, vp, vp, vp, vp]
        self.lib.hco_settle.restype = None
        self.lib.hco_queue.argtypes = [vp, vp, sz, u64, u64, vp, vp, vp, vp]
        self.lib.hco_queue.restype = u64

    @staticmethod
    def _arrays(shares, keys, sizes):
        n = len(sizes)
        return (b"".join(shares) + bytes(4), (ctypes.c_uint32 * max(len(keys), 1))(*keys), (ctypes.c_uint64 * (n + 1))(*_offsets(sizes)))

    def precheck(self, shares, keys, sizes, tuple_st, hash_st, flags, key_st):
        blob, k32, off = self._arrays(shares, keys, sizes)
        out = ctypes.create_string_buffer(b"\x02" * len(keys), len(keys) + 1)
        self.lib.hco_precheck(blob, k32, off, bytes(tuple_st) + b"\0", bytes(hash_st) + b"\0", len(sizes), len(keys), flags, bytes(key_st) + b"\0", len(key_st), out)
        return list(out.raw[:len(keys)])

    def sum(self, shares, keys, sizes, share_st, tuple_st, bm_words, layout, min_tuple, state=None):
        """state None: the provisional sum on zeroed rows -> (bits, counts, agg, flags).  state = (verdict, flag, bits, counts, agg): the re-sum
        on those arrays -> the same four"""
        n = len(sizes)
        blob, k32, off = self._arrays(shares, keys, sizes)
        if state is None:
            verdict, flag = None, ctypes.create_string_buffer(b"\xEE" * n, n + 1)
            bits, counts, agg = (ctypes.c_uint32 * max(n * bm_words, 1))(), (ctypes.c_uint32 * max(n, 1))(), ctypes.create_string_buffer(64 * n + 1)
        else:
            verdict, flag = bytes(state[0]) + b"\0", ctypes.create_string_buffer(bytes(state[1]), n + 1)
            bits, counts = (ctypes.c_uint32 * max(n * bm_words, 1))(*state[2]), (ctypes.c_uint32 * max(n, 1))(*state[3])
            agg = ctypes.create_string_buffer(state[4], 64 * n + 1)
        self.lib.hco_sum(blob, k32, off, bytes(share_st) + b"\0", bytes(tuple_st) + b"\0", n, bm_words, layout, min_tuple, verdict, flag, bits, agg, counts)
        return list(bits)[:n * bm_words], list(counts)[:n], agg.raw[:64 * n], list(flag.raw[:n])

    def settle(self, bm_words, flag, verdict, bits):
        n = len(flag)
        b = (ctypes.c_uint32 * max(n * bm_words, 1))(*bits)
        stats = (ctypes.c_uint32 * 3)()
        self.lib.hco_settle(n, bm_words, bytes(flag) + b"\0", bytes(verdict) + b"\0", b, stats)
        return list(b)[:n * bm_words], list(stats)

    def queue(self, sizes, tuple_st, share_st, flag, verdict, base, length):
        n = len(sizes)
        out = (ctypes.c_uint32 * max(length, 1))()
        cnt = self.lib.hco_queue((ctypes.c_uint64 * (n + 1))(*_offsets(sizes)), bytes(tuple_st) + b"\0", n, base, length, bytes(share_st) + b"\0",
                                 bytes(flag) + b"\0", bytes(verdict) + b"\0", out)
        return [base + j for j in list(out)[:cnt]]


@pytest.fixture(scope="module")
def points(c):
    """46 keys as multiples of one base (the valid share of key k is sk_k * base): key 45 = the negation of key 1, key 43 the identity key"""
    rnd = random.Random(20261018)
    st_h, base, _ = c.hash_to_g1(b"collect-opt/host")
    assert st_h == 0
    sks = [rnd.randrange(1, R) for _ in range(46)]
    sks[45] = R - sks[1]
    sig = [c.g1_mul(base, s.to_bytes(32, "big")) for s in sks]
    sig[43] = bytes(64)
    return base, sig


@pytest.mark.parametrize("build", BUILDS)
def test_precheck_statuses(libs, c, points, build):
    """decode statuses 6 (a coordinate >= q) and 4 (off the curve; the identity under REJECT_IDENTITY), key statuses 2 (index >= n_keys), 3, 4
    and 6 as registration left them, hash status 1 and 5, a refused tuple (every share keeps the 2 of the fill): the first of the three rules"""
    h = Harness(libs[build])
    base, sig = points
    n_keys = 40
    key_st = [0] * n_keys
    key_st[7], key_st[8], key_st[9] = 4, 6, 3
    big = bytearray(sig[2]); big[0] = 0xFF
    off_curve = bytearray(sig[3]); off_curve[40] ^= 4
    shares, keys, sizes = [], [], SIZES
    for i, k in enumerate(sizes):
        for t in range(k):
            key = (7 * i + 3 * t) % 46                                     # 40 .. 45: outside the set
            kind = t % 11
            shares.append(bytes(big) if kind == 3 else bytes(off_curve) if kind == 5 else bytes(64) if kind == 7 else sig[key])
            keys.append(key if kind != 9 else n_keys + 20)
    tuple_st = [0] * len(sizes)
    tuple_st[3], tuple_st[4], tuple_st[6] = 1, 2, 5
    for flags in (0, 2):
        got = h.precheck(shares, keys, sizes, tuple_st, tuple_st, flags, key_st)
        want = M.precheck([c.g1_validate(s, flags) for s in shares], keys, key_st, sizes, tuple_st)
        assert got == want, (flags, [(s, a, b) for s, (a, b) in enumerate(zip(got, want)) if a != b][:8])
        assert {0, 1, 2, 3, 4, 5, 6} <= set(got)
        lo = sum(sizes[:4])
        assert got[lo:lo + sizes[4]] == [2] * sizes[4]
    assert h.precheck(shares, keys, sizes, tuple_st, tuple_st, 2, key_st) != h.precheck(shares, keys, sizes, tuple_st, tuple_st, 0, key_st)


def _case(points, c):
    """tuples of 0 .. 130 shares, pre-check statuses given (0, 2, 3, 4, 6, 1 mixed in), distinct keys within a tuple while it has at most 46
    candidates — plus tuples with a duplicate: adjacent shares (two lanes of the wave), shares 64 apart (one lane's stride), 128 apart, a
    duplicate of the last share, and a tuple of two shares of one key.  truth[s]: what the exact verify gives candidate s (9 for a wrong share)"""
    base, sig = points
    tuples = []
    for i, k in enumerate(SIZES):
        t = []
        for j in range(k):
            key = (5 * i + j) % 46
            st = 0 if k <= 2 or j >= 46 - 6 else [0, 0, 0, 4, 0, 2, 0, 3, 0, 6, 0, 1, 0][j % 13]
            if j >= 46:
                st = [2, 4, 6, 3][j % 4]                                   # a key cannot be a candidate twice here: the later shares are refused
            t.append([sig[key], key, st, 0])
        tuples.append(t)
    wrong = lambda key: c.g1_add(sig[key] if sig[key] != bytes(64) else base, base)      # noqa: E731
    for i, j in ((3, 2), (8, 4)):                                          # one wrong candidate in the 15-share tuple and in the 65-share one
        assert tuples[i][j][2] == 0
        tuples[i][j] = [wrong(tuples[i][j][1]), tuples[i][j][1], 0, 9]

    def dup(length, a, b):
        t = [[sig[j % 46], j % 46, 0 if j < 46 else 2, 0] for j in range(length)]
        t[b] = [t[a][0], t[a][1], 0, 0]
        return t
    tuples += [dup(17, 3, 4), dup(70, 2, 66), dup(130, 1, 129), dup(130, 0, 128), [[sig[9], 9, 0, 0]] * 2, dup(16, 14, 15),
               [[sig[1], 1, 0, 0], [sig[45], 45, 0, 0]],                   # a key and its negation
               [[sig[43], 43, 0, 0], [sig[4], 4, 0, 0]],                   # the identity key's share
               [[wrong(2), 2, 0, 9], [sig[2], 2, 0, 0]],                   # invalid, then valid, of one key
               [[sig[2], 2, 0, 0], [wrong(2), 2, 0, 9]]]
    shares = [x[0] for t in tuples for x in t]
    keys = [x[1] for t in tuples for x in t]
    pre = [x[2] for t in tuples for x in t]
    truth = [x[3] for t in tuples for x in t]
    return shares, keys, pre, truth, [len(t) for t in tuples]


@pytest.mark.parametrize("build", BUILDS)
def test_duplicates_queue_and_masked_resum(libs, c, points, build):
    h = Harness(libs[build])
    shares, keys, pre, truth, sizes = _case(points, c)
    assert sizes[:len(SIZES)] == SIZES
    n, bm_words, min_tuple = len(sizes), 2, 2
    tuple_st = [0] * n
    flags_want = [f for f, _ in M.tuple_flags(keys, pre, sizes, min_tuple)]
    n0 = len(SIZES)
    assert flags_want[:n0] == [M.FINAL, M.EXACT] + [M.CHECK] * 8 and flags_want[n0:] == [M.EXACT] * 6 + [M.CHECK] * 2 + [M.EXACT] * 2
    # the tuple check as given: a CHECK tuple fails iff it holds a wrong candidate — and one all-valid tuple fails all the same (index 5)
    ranges = M.ranges(sizes)

    def tuple_check(i, row, chosen):
        return 9 if i == 5 or any(truth[s] for s in range(*ranges[i]) if pre[s] == 0) else 0
    want = M.collect(keys, pre, sizes, tuple_st, bm_words, min_tuple, tuple_check, lambda s: truth[s])
    assert want["flags"] == flags_want and [i for i, v in enumerate(want["verdicts"]) if v == 9] == [3, 5, 8]
    want_agg = b"".join(collect_model.aggregates(c, shares, want["chosen"]))
    verdict = [0xEE if v is None else v for v in want["verdicts"]]         # read for CHECK tuples only
    pro_rows, pro_counts, pro_chosen = collect_model.select(keys, pre, sizes, tuple_st, bm_words)
    pro_agg = collect_model.aggregates(c, shares, pro_chosen)
    seen = []
    for layout in (0, 1):
        bits, counts, agg, flag = h.sum(shares, keys, sizes, pre, tuple_st, bm_words, layout, min_tuple)
        assert flag == flags_want, (layout, [(i, a, b) for i, (a, b) in enumerate(zip(flag, flags_want)) if a != b])
        for i in range(n):                                                  # the provisional outputs of every tuple without a duplicate
            if i < n0 or flags_want[i] == M.CHECK:
                assert bits[bm_words * i:bm_words * i + bm_words] == pro_rows[i] and counts[i] == pro_counts[i] and agg[64 * i:64 * i + 64] == pro_agg[i], (layout, i)
        # with the minimum at 0 and at 3 only the flags move
        assert h.sum(shares, keys, sizes, pre, tuple_st, bm_words, layout, 0)[3] == [f for f, _ in M.tuple_flags(keys, pre, sizes, 0)]
        assert h.sum(shares, keys, sizes, pre, tuple_st, bm_words, layout, 3)[3] == [f for f, _ in M.tuple_flags(keys, pre, sizes, 3)]
        settled, stats = h.settle(bm_words, flag, verdict, bits)
        assert stats == [want["hook"]["checked"], want["hook"]["passed"], want["hook"]["exact_tuples"]]
        for i in range(n):
            exact = flag[i] == M.EXACT or (flag[i] == M.CHECK and verdict[i] != 0)
            assert settled[bm_words * i:bm_words * i + bm_words] == ([0] * bm_words if exact else bits[bm_words * i:bm_words * i + bm_words]), i
        # the queue, whole and in slices of 64 and 37 shares
        n_shares = len(keys)
        assert h.queue(sizes, tuple_st, pre, flag, verdict, 0, n_shares) == want["queue"] and len(want["queue"]) == want["hook"]["exact_shares"]
        for chunk in (64, 37):
            got = [s for lo in range(0, n_shares, chunk) for s in h.queue(sizes, tuple_st, pre, flag, verdict, lo, min(chunk, n_shares - lo))]
            assert got == want["queue"], chunk
        # the exact verify of the queued candidates as given, then the re-sum in either layout on the settled rows
        status = [truth[s] if s in set(want["queue"]) else pre[s] for s in range(n_shares)]
        assert status == want["share_status"]
        poisoned = bytearray(agg)
        passing = [i for i in range(n) if flag[i] == M.CHECK and verdict[i] == 0]
        for relayout in (0, 1):
            b2, c2, a2, f2 = h.sum(shares, keys, sizes, status, tuple_st, bm_words, relayout, min_tuple, state=(verdict, flag, settled, counts, bytes(poisoned)))
            assert f2 == flag                                               # the re-sum writes no flags
            assert b2 == [w for r in want["rows"] for w in r] and c2 == want["counts"], (layout, relayout)
            assert a2 == want_agg, (layout, relayout, [i for i in range(n) if a2[64 * i:64 * i + 64] != want_agg[64 * i:64 * i + 64]])
            seen.append((b2, c2, a2))
        # ... which leaves a passing tuple alone: a marker in its aggregate and its row survives
        i = passing[-1]
        poisoned[64 * i:64 * i + 64] = b"\xA5" * 64
        marked = list(settled)
        marked[bm_words * i] ^= 0x80000000
        b3, c3, a3, _ = h.sum(shares, keys, sizes, status, tuple_st, bm_words, 1 - layout, min_tuple, state=(verdict, flag, marked, counts, bytes(poisoned)))
        assert a3[64 * i:64 * i + 64] == b"\xA5" * 64 and b3[bm_words * i] == marked[bm_words * i] and c3[i] == counts[i]
    assert all(s == seen[0] for s in seen)
    # the fallback tuples are the exact call's: select over the final statuses
    rows_x, counts_x, chosen_x = collect_model.select(keys, want["share_status"], sizes, tuple_st, bm_words)
    assert want["rows"] == rows_x and want["counts"] == counts_x
    # a refused tuple (status 2) has no shares on this route either
    tuple_st2 = list(tuple_st)
    tuple_st2[7] = 2
    pre2 = list(pre)
    lo, hi = ranges[7]
    pre2[lo:hi] = [2] * (hi - lo)
    bits, counts, agg, flag = h.sum(shares, keys, sizes, pre2, tuple_st2, bm_words, 1, min_tuple)
    assert flag[7] == M.FINAL and counts[7] == 0 and agg[64 * 7:64 * 8] == bytes(64) and bits[2 * 7:2 * 8] == [0, 0]
