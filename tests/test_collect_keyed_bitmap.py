"""Building signer-bitmap aggregates from individual signatures (include/bn254_hip.h: bn254_batch_collect_keyed_bitmap[_device]), without a GPU:
- the two entry points are declared with the stated arity, exported with matching argtypes, bound in INTEGRATION.md's extern block; the
  option mirror agrees; the translation unit is registered;
- the Python mirrors refuse malformed items before they touch a device;
- the device code of the select-and-sum and of the range rule (bn254_amd/csrc/bn254_collect.h), compiled for the host
  (tests/hostsim/hostsim_collect.cpp, plain and under -DBN_TRACK_BOUNDS), over GIVEN status arrays: both layouts (the wave layout as 64
  partial sums plus the tree) against tests/collect_model.py and the oracle's g1_add, tuples of 0 .. 130 shares, duplicates of a valid share,
  a valid and an invalid share of one key in both orders, a key and its negation, a registered identity key, all shares refused, statuses
  2, 4, 6, 9 and 1 mixed in; and a key set that repeats keys (tests/collect_repeat_cases.py): equal and opposite partial sums at every level
  of the tree and in a lane's own stride."""
import ctypes
import os
import random
import re
import subprocess

import pytest

from bn254_amd import _native
from tests import collect_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254_batch_collect_keyed_bitmap", "bn254_batch_collect_keyed_bitmap_device"]
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_collect.cpp")
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130]


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
    assert _arity(decls[NAMES[0]].group(1)) == 15 and _arity(decls[NAMES[1]].group(1)) == 16
    assert "const uint32_t *share_key" in decls[NAMES[0]].group(1) and "uint32_t *n_signers" in decls[NAMES[0]].group(1)
    assert "const uint64_t *d_share_off" in decls[NAMES[1]].group(1) and "void *stream" in decls[NAMES[1]].group(1)
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    assert re.search(r"#define BN254_OPT_COLLECT_WAVE_MIN_SHARES 37\b", hdr) and engine.OPT_COLLECT_WAVE_MIN_SHARES == 37
    numbers = [int(x) for x in re.findall(r"#define BN254_OPT_\w+ (\d+)\b", hdr)]
    assert numbers.count(37) == 1 and len(numbers) == len(set(numbers))       # a number of its own
    assert os.path.join(ROOT, "bn254_amd", "csrc", "bn254_collect.hip") in _native.translation_units()


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
    for items in ([(b"a", [sig], [0]), (b"b", [sig])], [(b"a", [sig], [0], [1])], [(b"a", [sig, sig], [0])], [(b"a", [], [3])]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.batch_aggregate_keyed_signers(items)
        assert e.value.kind == api.ErrorKind.InvalidLength
    for idx in ([0, -1], [1 << 32, 0]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.aggregate_keyed_signers(b"a", [sig, sig], idx)
        assert e.value.kind == api.ErrorKind.IndexOutOfBounds
    # an engine that does not know its key count cannot size the bitmaps: the count must be given
    class Blind:
        pass
    with pytest.raises(ValueError):
        api.ECDSA.aggregate_keyed_signers(b"a", [sig], [0], engine=Blind())
    # ... and the engine mirror: sizes must add up to the shares
    with pytest.raises(AssertionError):
        engine.Engine.batch_collect_keyed_bitmap(None, [b"a", b"b"], bytes(128), [0, 1], [1, 2], 1)
    with pytest.raises(AssertionError):
        engine.Engine.batch_collect_keyed_bitmap(None, [b"a"], bytes(64), [0, 1], [2], 1)


@pytest.fixture(scope="module")
def libs(tmp_path_factory):
    out = tmp_path_factory.mktemp("hc")
    common = ["-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libhc_%s.so" % name))
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
        self.lib.hc_sum.argtypes = [vp, vp, vp, vp, vp, sz, sz, ctypes.c_int, vp, vp, vp]
        self.lib.hc_sum.restype = None
        self.lib.hc_plan.argtypes = [vp, sz, ctypes.c_uint64, vp, vp]
        self.lib.hc_plan.restype = None

    def sum(self, shares, keys, sizes, share_st, tuple_st, bm_words, layout):
        n, ends = len(sizes), [0]
        for k in sizes:
            ends.append(ends[-1] + k)
        off = (ctypes.c_uint64 * (n + 1))(*ends)
        k32 = (ctypes.c_uint32 * max(len(keys), 1))(*keys)
        bits = (ctypes.c_uint32 * max(n * bm_words, 1))()
        agg = ctypes.create_string_buffer(64 * n + 1)
        counts = (ctypes.c_uint32 * max(n, 1))()
        self.lib.hc_sum(b"".join(shares) + bytes(4), k32, off, bytes(share_st) + b"\0", bytes(tuple_st) + b"\0", n, bm_words, layout, bits, agg, counts)
        return list(bits)[:n * bm_words], list(counts)[:n], agg.raw[:64 * n]

    def plan(self, off, n_shares):
        n = len(off) - 1
        ok = ctypes.create_string_buffer(n + 1)
        tuple_of = (ctypes.c_uint64 * max(n_shares, 1))()
        self.lib.hc_plan((ctypes.c_uint64 * (n + 1))(*off), n, n_shares, ok, tuple_of)
        return list(ok.raw[:n]), list(tuple_of)[:n_shares]


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def check(h, c, shares, keys, sizes, share_st, tuple_st, bm_words):
    rows, counts, chosen = collect_model.select(keys, share_st, sizes, tuple_st, bm_words)
    want = ([w for r in rows for w in r], counts, b"".join(collect_model.aggregates(c, shares, chosen)))
    lane = h.sum(shares, keys, sizes, share_st, tuple_st, bm_words, 0)
    wave = h.sum(shares, keys, sizes, share_st, tuple_st, bm_words, 1)
    assert lane == want, [i for i in range(len(sizes)) if lane[2][64 * i:64 * i + 64] != want[2][64 * i:64 * i + 64]]
    assert wave == want, [i for i in range(len(sizes)) if wave[2][64 * i:64 * i + 64] != want[2][64 * i:64 * i + 64]]
    return want


@pytest.mark.parametrize("build", BUILDS)
def test_select_and_sum_both_layouts(libs, c, build):
    """tuples of 0 .. 130 shares over 46 keys; points are multiples of one base (the valid signature of a key is unique: share = sk_key * H);
    statuses 0, 2, 4, 6, 9 and 1 given, not computed"""
    h = Harness(libs[build])
    rnd = random.Random(20261018)
    n_keys, bm_words = 46, 2
    st_h, base, _ = c.hash_to_g1(b"collect/host")
    assert st_h == 0
    sks = [rnd.randrange(1, R) for _ in range(n_keys)]
    sks[45] = R - sks[1]                                                   # key 45 = the negation of key 1
    sig = [c.g1_mul(base, s.to_bytes(32, "big")) for s in sks]
    sig[43] = bytes(64)                                                    # key 43 = a registered identity key: its valid share is the identity
    sizes = SIZES
    shares, keys, share_st = [], [], []
    for i, k in enumerate(sizes):
        for t in range(k):
            key = (7 * i + 3 * t) % n_keys
            st = 0 if k <= 2 else [0, 0, 0, 9, 0, 2, 0, 4, 0, 6, 0, 1, 0][t % 13]
            shares.append(sig[key] if st in (0, 2, 1) else c.g1_add(sig[key] if sig[key] != bytes(64) else base, base))
            keys.append(key)
            share_st.append(st)
    tuple_st = [0] * len(sizes)
    want = check(h, c, shares, keys, sizes, share_st, tuple_st, bm_words)
    assert want[1][sizes.index(65)] > 32                                   # both words of a row in use
    # a tuple whose hash failed (every share reads 1), one the range rule refused (status 2: no shares, whatever their statuses), the rest as before
    tuple_st2 = [0] * len(sizes)
    tuple_st2[3], tuple_st2[4] = 1, 2
    st2 = list(share_st)
    at3 = sum(sizes[:3])
    st2[at3:at3 + sizes[3]] = [1] * sizes[3]
    want2 = check(h, c, shares, keys, sizes, st2, tuple_st2, bm_words)
    assert want2[1][3] == 0 and want2[1][4] == 0 and want2[2][64 * 4:64 * 5] == bytes(64)


@pytest.mark.parametrize("build", BUILDS)
def test_select_and_sum_exceptional_cases(libs, c, build):
    h = Harness(libs[build])
    rnd = random.Random(3)
    st_h, base, _ = c.hash_to_g1(b"collect/exceptional")
    sks = [rnd.randrange(1, R) for _ in range(8)]
    sks[7] = R - sks[1]
    sig = [c.g1_mul(base, s.to_bytes(32, "big")) for s in sks]
    sig[6] = bytes(64)
    bad = [c.g1_add(s if s != bytes(64) else base, base) for s in sig]
    tuples = [
        [(sig[2], 2, 0)] * 3,                                              # duplicates of a valid share: once
        [(sig[3], 3, 0), (bad[3], 3, 9)],                                  # valid, then invalid, for one key
        [(bad[3], 3, 9), (sig[3], 3, 0)],                                  # ... and the other order
        [(sig[1], 1, 0), (sig[7], 7, 0)],                                  # a key and its negation: two bits, the identity
        [(sig[1], 1, 0), (sig[2], 2, 0), (sig[7], 7, 0)],
        [(sig[6], 6, 0)],                                                  # the identity key's (identity) share: one bit, the identity
        [(sig[6], 6, 0), (sig[4], 4, 0)],
        [(bad[0], 0, 9), (sig[1], 9, 2), (bad[2], 2, 4), (sig[3], 3, 6), (sig[4], 4, 1)],      # all refused
        [(sig[0], 0, 0), (sig[0], 0, 0), (sig[5], 5, 0), (sig[0], 0, 0)] * 20,                 # 80 shares of two keys: the wave layout's claims
        [(sig[j % 6], j % 6, 0 if j % 3 else 9) for j in range(66)],
    ]
    shares = [s for t in tuples for s, _, _ in t]
    keys = [k for t in tuples for _, k, _ in t]
    share_st = [st for t in tuples for _, _, st in t]
    sizes = [len(t) for t in tuples]
    bits, counts, agg = check(h, c, shares, keys, sizes, share_st, [0] * len(tuples), 1)
    assert counts == [1, 1, 1, 2, 3, 1, 2, 0, 2, 4]
    assert bits[:8] == [4, 8, 8, 0x82, 0x86, 0x40, 0x50, 0]
    A = lambda i: agg[64 * i:64 * i + 64]     # noqa: E731
    assert A(0) == sig[2] and A(1) == sig[3] == A(2) and A(3) == bytes(64) and A(4) == sig[2] and A(5) == bytes(64) and A(6) == sig[4] and A(7) == bytes(64)
    assert A(8) == c.g1_add(sig[0], sig[5])
    # a wider bitmap than the key set needs: the words past it stay zero
    bits3, _, agg3 = check(h, c, shares, keys, sizes, share_st, [0] * len(tuples), 3)
    assert agg3 == agg and all(bits3[3 * i + 1] == 0 and bits3[3 * i + 2] == 0 for i in range(len(tuples)))


@pytest.fixture(scope="module")
def repeated(c):
    """tests/collect_repeat_cases.py as multiples of one base: sigma = a base, -sigma = (r - a) base, B_j's share b_j base, a wrong share
    sigma + base.  -> (cases, (shares, keys, sizes, statuses), sigma, the B shares, the expectation by the model and the oracle's g1_add)"""
    from tests import collect_repeat_cases as rc
    rnd = random.Random(17)
    st_h, base, _ = c.hash_to_g1(b"collect/repeated")
    assert st_h == 0
    a = rnd.randrange(1, R)
    sigma, neg = c.g1_mul(base, a.to_bytes(32, "big")), c.g1_mul(base, (R - a).to_bytes(32, "big"))
    assert c.g1_add(sigma, neg) == bytes(64) and sigma[:32] == neg[:32]
    b = [c.g1_mul(base, rnd.randrange(1, R).to_bytes(32, "big")) for _ in range(rc.N_B)]
    wrong = c.g1_add(sigma, base)
    cases = rc.shapes()
    flat = rc.plant(cases, lambda i, kind, key: {"A": sigma, "N": neg, "W": wrong}.get(kind) or b[key - rc.K_B])
    shares, keys, sizes, status = flat
    rows, counts, chosen = collect_model.select(keys, status, sizes, [0] * len(sizes), rc.BM)
    want = ([w for r in rows for w in r], counts, b"".join(collect_model.aggregates(c, shares, chosen)))
    return cases, flat, sigma, b, want


@pytest.mark.parametrize("build", BUILDS)
def test_select_and_sum_repeated_keys(libs, c, repeated, build):
    """a key set that lists one key 128 times and its negation 64 times (tests/collect_repeat_cases.py), statuses given: a doubling and a
    cancellation at every level of the tree with every other slot the identity, all 64 slots doubling at all six levels (the last one
    32 sigma + 32 sigma), a cancellation at the first level only and at the last only, one level whose slots double, cancel, add ordinarily
    and add identities, the same one position on, and a lane's own stride adding sigma to sigma and to -sigma.  Both layouts against the
    model and the oracle's g1_add; every aggregate again as (the net multiple) sigma + the B shares, through g1_mul.  Under
    -DBN_TRACK_BOUNDS the interval tracker aborts the process on a violated bound."""
    from tests import collect_repeat_cases as rc
    cases, (shares, keys, sizes, status), sigma, b, want = repeated
    h = Harness(libs[build])
    bits, counts, agg = want
    for layout in (0, 1):
        got = h.sum(shares, keys, sizes, status, [0] * len(sizes), rc.BM, layout)
        assert got[0] == bits and got[1] == counts, layout
        assert got[2] == agg, "layout %d: %s" % (layout, " ".join(cases[i][0] for i in range(len(cases)) if got[2][64 * i:64 * i + 64] != agg[64 * i:64 * i + 64]))
    by_name = {}
    for i, (name, sh) in enumerate(cases):
        m, bs, count = rc.net(sh)
        point = c.g1_mul(sigma, (m % R).to_bytes(32, "big")) if m % R else bytes(64)
        for j in bs:
            point = c.g1_add(point, b[j])
        assert agg[64 * i:64 * i + 64] == point and counts[i] == count, name
        assert sum(bin(w).count("1") for w in bits[rc.BM * i:rc.BM * i + rc.BM]) == count, name
        by_name[name] = (m, bs, count)
    assert by_name["double_every_level"] == (64, [], 64) and by_name["own_stride_128"] == (128, [], 128)
    assert by_name["own_stride_sss"] == (128, [0, 1], 130) and by_name["own_stride_sns"] == (126, [], 130)
    assert all(by_name["double_at_%d" % s] == (2, [], 2) and by_name["cancel_at_%d" % s] == (0, [], 2) for s in rc.STRIDES)
    assert by_name["cancel_first_level"] == by_name["cancel_last_level"] == (0, [], 64) and by_name["mixed_vote"] == (16, list(range(16)), 48)
    assert by_name["cancel_at_8+1"] == (0, [], 2) and by_name["double_every_level+2"] == (64, [62, 63], 66)


def range_rule(off, n_shares):
    """the range rule restated: accepted iff lo <= hi <= n_shares and no earlier offset exceeds lo; a share belongs to the accepted tuple that holds it
    (the earlier offsets as their running maximum, so that tests/test_gpu_collect_many_tuples.py can ask it about 65 900 tuples)"""
    n = len(off) - 1
    ok, before = [], 0
    for i in range(n):
        ok.append(int(off[i] <= off[i + 1] <= n_shares and before <= off[i]))
        before = max(before, off[i])
    tuple_of = [n] * n_shares
    for i in range(n):
        if ok[i]:
            for s in range(off[i], off[i + 1]):
                assert tuple_of[s] == n                      # accepted ranges are disjoint
                tuple_of[s] = i
    return ok, tuple_of


def test_range_rule_and_share_map(libs):
    h = Harness(libs["plain"])
    rnd = random.Random(9)
    fixed = [([0, 3, 3, 7, 10], 10), ([0, 3, 2, 7, 10], 10), ([0, 5, 3, 8, 10], 10), ([0, 4, 8, 12], 10), ([2, 4, 9], 10), ([0, 0, 0], 0), ([0, 11], 10),
             ([5, 2, 2, 6], 8), ([0, 9, 1, 3, 9, 10], 10)]
    for off, n_shares in fixed:
        assert h.plan(off, n_shares) == tuple(range_rule(off, n_shares)), off
    for _ in range(300):
        n = rnd.randrange(1, 12)
        n_shares = rnd.randrange(0, 40)
        off = sorted(rnd.randrange(0, n_shares + 1) for _ in range(n + 1))
        for _ in range(rnd.randrange(0, 3)):
            off[rnd.randrange(0, n + 1)] = rnd.randrange(0, n_shares + 3)
        assert h.plan(off, n_shares) == tuple(range_rule(off, n_shares)), off
