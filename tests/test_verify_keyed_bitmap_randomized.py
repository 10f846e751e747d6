"""The randomised signer-bitmap call without a device: the argument errors of ECDSA.batch_verify_keyed_signers_randomized, the model's own
fold and grouping rules on small cases, and the conditions the GPU tests' plans rely on."""
import pytest

from bn254_amd import api
from tests import bitmap_rand_model as BM


class NoEngine:
    n_registered_keys = 4

    def __getattr__(self, name):
        raise AssertionError("the device was reached: " + name)


class Sig:
    def __init__(self, n=64):
        self.raw = bytes(n)


def test_argument_errors_before_any_device_work():
    f = api.ECDSA.batch_verify_keyed_signers_randomized
    with pytest.raises(api.Error) as e:
        f([(b"m", Sig())], engine=NoEngine())
    assert e.value.kind == api.ErrorKind.InvalidLength
    with pytest.raises(api.Error) as e:
        f([(b"m", Sig(63), [0])], engine=NoEngine())
    assert e.value.kind == api.ErrorKind.InvalidLength
    with pytest.raises(api.Error) as e:
        f([(b"m", Sig(), [0, -1])], engine=NoEngine())
    assert e.value.kind == api.ErrorKind.IndexOutOfBounds
    with pytest.raises(ValueError):
        f([(b"m", Sig(), [0])], seed=bytes(31), engine=NoEngine())


def test_the_call_reaches_the_engine_with_seed_and_flags():
    from bn254_amd import engine as E
    seen = {}

    class Eng:
        n_registered_keys = 40

        def batch_verify_keyed_bitmap_randomized(self, msgs, sigs, bits, bm_words, seed, flags):
            seen.update(msgs=msgs, bits=bits, bm_words=bm_words, seed=seed, flags=flags)
            return bytes([0, 9])
    out = api.ECDSA.batch_verify_keyed_signers_randomized([(b"a", Sig(), [0, 33]), (b"b", Sig(), [77])], seed=bytes(32), engine=Eng(), rand64=True)
    assert out[0] is None and out[1].kind == api.ErrorKind(9)
    assert seen["bm_words"] == 2 and seen["bits"] == [1, 2, 0, 1 << 8] and seen["flags"] == E.FLAG_RAND64 and seen["seed"] == bytes(32)


def test_grouping_rules():
    sets = [[0, 1], [1, 9], [], [3], [2], [40]]
    at = [True, True, True, False, True, True]
    inf = [False] * 41
    inf[9] = True
    w = BM.grouping(sets, at, [False, True, False, False, False, False], inf, 2, 2)
    # groups {0, 1} (keys 0, 1; fails), {2} (one, no key), {4, 5} (keys 2, 40)
    assert w == dict(groups=3, table_pairs=3 + 1 + 3, failed_groups=1, rechecked=2, single_groups=1)
    assert BM.grouping(sets, at, [False] * 6, inf, 2, 1)["table_pairs"] == 3 + 1 + 2      # key 40 does not fit one word
    assert BM.r_model(bytes(32), 5, 1) < 1 << 64 <= BM.r_model(bytes(32), 5, 0) < 1 << 128


def test_plan_conditions_of_the_gpu_tests():
    """the plans whose counters and sums the GPU tests compare (the passing batch, the ragged plan), from their own generators: at least
    half of the groups hold two or more tuples at the check, and at most a quarter of the tuples are off the check.  (The mixed plan of the
    parity test is the exact call's, three quarters of it wrong on purpose: it is compared byte for byte, and its counters whatever they are.)"""
    n = 301
    assert len(BM.passing_sets(n)) == n
    for G in (7, 64, 512):
        members = BM.groups_of(n, [True] * n, G)
        assert 2 * len([g for g in members.values() if len(g) >= 2]) >= len(members)
    kinds = [k for _, k in BM.ragged_sets()]
    assert {"ok", "refused", "oob", "curve"} == set(kinds) and 4 * len([k for k in kinds if k != "ok"]) <= len(kinds)
    for G in (7, 16, 32):
        members = BM.groups_of(len(kinds), [k == "ok" for k in kinds], G)
        assert 2 * len([g for g in members.values() if len(g) >= 2]) >= len(members)


# ---- the device functions of bn254_amd/csrc/bn254_bitmap_rand.h, compiled for the host (tests/hostsim/hostsim_bitmap_rand.cpp) ------------
import ctypes  # noqa: E402
import os  # noqa: E402
import random  # noqa: E402
import subprocess  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_bitmap_rand.cpp")
O = BM.O


class Harness:
    def __init__(self, path):
        L = self.lib = ctypes.CDLL(path)
        u32, u64, sz, vp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p
        L.hbr_bucket.argtypes, L.hbr_bucket.restype = [u64, u32, u32, u32], u64
        L.hbr_sig_bucket.argtypes, L.hbr_sig_bucket.restype = [u64, u32], u64
        L.hbr_byte.argtypes, L.hbr_byte.restype = [vp, sz, u32], u32
        L.hbr_window_keys.argtypes, L.hbr_window_keys.restype = [u32, u32, vp, vp], u32
        L.hbr_pair_rank.argtypes, L.hbr_pair_rank.restype = [u32, u32], u32
        L.hbr_window.argtypes = [sz, vp, vp, sz, u32, u32, vp, vp, vp]

    def window(self, pts, byte_values, w, mask, bm_words=2):
        """entries pts[i] whose bitmap has byte w = byte_values[i] -> (the eight key sums, [(key, point)] of the keys in mask)"""
        n = len(pts)
        rows = (ctypes.c_uint32 * max(n * bm_words, 1))()
        for i, v in enumerate(byte_values):
            rows[i * bm_words + w // 4] = v << (8 * (w % 4))
        keys, pp, all_t = (ctypes.c_uint32 * 8)(), ctypes.create_string_buffer(8 * 64), ctypes.create_string_buffer(8 * 64)
        k = self.lib.hbr_window(n, b"".join(pts), rows, bm_words, w, mask, keys, pp, all_t)
        return [all_t.raw[64 * b:64 * b + 64] for b in range(8)], [(int(keys[t]), pp.raw[64 * t:64 * t + 64]) for t in range(k)]


@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    """both layouts of Fq2, the pair layout also under the bound tracker"""
    out = tmp_path_factory.mktemp("hbr")
    common = ["-std=c++17", "-shared", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    builds = {"plain": ["-O2"], "bounds": ["-O1", "-DBN_TRACK_BOUNDS"], "one_lane": ["-O2", "-DBM_ONE_LANE"], "one_lane_bounds": ["-O1", "-DBM_ONE_LANE", "-DBN_TRACK_BOUNDS"]}
    procs = {}
    for name, flags in builds.items():
        so = str(out / ("libhbr_%s.so" % name))
        procs[name] = (so, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + common + ["-o", so, SRC], stderr=subprocess.PIPE, text=True))
    libs = {}
    for name, (so, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, (name, err[-2000:])
        libs[name] = Harness(so)
    return libs


@pytest.fixture(scope="module")
def oracle():
    from oracle import c_oracle
    return c_oracle


def points(c, n, seed=1):
    rnd = random.Random(seed)
    g = c.g1_generator()
    return [c.g1_mul(g, rnd.randrange(1, BM.R).to_bytes(32, "big")) for _ in range(n)]


def want_window(c, pts, byte_values, w, mask):
    buckets = {}
    for p, v in zip(pts, byte_values):
        if v:
            buckets[v] = c.g1_add(buckets.get(v, O), p)
    t = BM.fold_model(c, buckets)
    return t, [(8 * w + b, t[b]) for b in range(8) if (mask >> b) & 1]


def test_numbering_bytes_and_window_keys(harnesses):
    h = harnesses["plain"].lib
    for n_keys in (1, 8, 9, 46, 257):
        nW = (n_keys + 7) // 8
        per = 255 * nW + 1
        seen = set()
        for g in (0, 1, 5):
            for w in range(nW):
                for v in range(1, 256):
                    b = h.hbr_bucket(g, w, v, n_keys)
                    assert b == g * per + 255 * w + v - 1
                    seen.add(b)
            assert h.hbr_sig_bucket(g, n_keys) == g * per + per - 1 and h.hbr_sig_bucket(g, n_keys) not in seen
        st, inf = bytearray(n_keys), bytearray(n_keys)
        if n_keys > 3:
            st[1], inf[3] = 4, 1
        for w in range(nW):
            want = sum(1 << b for b in range(8) if 8 * w + b < n_keys and not st[8 * w + b] and not inf[8 * w + b])
            assert h.hbr_window_keys(w, n_keys, bytes(st), bytes(inf)) == want
    row = (ctypes.c_uint32 * 2)(0x04030201, 0xFF00A5C3)
    assert [h.hbr_byte(row, 2, w) for w in range(10)] == [1, 2, 3, 4, 0xC3, 0xA5, 0, 0xFF, 0, 0]
    assert [h.hbr_byte(row, 1, w) for w in range(6)] == [1, 2, 3, 4, 0, 0] and h.hbr_byte(None, 0, 0) == 0
    for mask in (0, 1, 0x80, 0xA5, 0xFF):
        assert [h.hbr_pair_rank(mask, b) for b in range(8)] == [bin(mask & ((1 << b) - 1)).count("1") for b in range(8)]


def test_fold_every_byte_value_and_empty_buckets(harnesses, oracle):
    """one entry per byte value 1 .. 255 (every bucket one point); a sparse window (most buckets empty); an all-identity fold"""
    pts = points(oracle, 255)
    for name, h in harnesses.items():
        for w, mask in ((0, 0xFF), (5, 0xA5)):
            vals = list(range(1, 256))
            assert h.window(pts, vals, w, mask) == want_window(oracle, pts, vals, w, mask), name
        vals = [0x80, 0x01, 0x81, 0x10, 0, 0]
        assert h.window(pts[:6], vals, 3, 0x91) == want_window(oracle, pts[:6], vals, 3, 0x91), name
        t, pairs = h.window(pts[:4], [0, 0, 0, 0], 2, 0)
        assert t == [O] * 8 and pairs == [], name
        t, pairs = h.window([O, O, O], [0xFF, 0x0F, 0xF0], 1, 0xFF)       # identity entries in live buckets: pairs that carry the identity
        assert t == [O] * 8 and pairs == [(8 + b, O) for b in range(8)], name


def test_fold_equal_and_opposite_points(harnesses, oracle):
    """P + P and P + (-P) inside a bucket and inside the fold (between buckets, on the halving and on the tree side)"""
    c = oracle
    p, q = points(c, 2, seed=7)
    neg = lambda x: c.g1_mul(x, (BM.R - 1).to_bytes(32, "big"))  # noqa: E731
    cases = [([p, p], [0x03, 0x03]),                   # a bucket that doubles
             ([p, neg(p)], [0x03, 0x03]),              # a bucket that cancels: its keys' sums are the identity, the pairs stay
             ([p, neg(p), q], [0x05, 0x05, 0x04]),
             ([p, p], [0x81, 0x01]),                   # equal points meet on the halving (B[1] + B[129])
             ([p, neg(p)], [0x81, 0x01]),
             ([p, p], [0x80, 0x81]),                   # ... and in the tree of the upper half
             ([p, neg(p)], [0x80, 0x81]),
             ([p, p, p, p], [0xFF, 0xFE, 0x7F, 0x01]),
             ([p, neg(p), q, neg(q)], [0xC0, 0xC1, 0x41, 0x40]),
             ([p] * 9, [0xFF] * 9)]
    for name, h in harnesses.items():
        for pts, vals in cases:
            mask = 0
            for v in vals:
                mask |= v
            got, want = h.window(pts, vals, 1, mask), want_window(c, pts, vals, 1, mask)
            assert got == want, (name, vals)
    t, pairs = harnesses["plain"].window([p, neg(p)], [0x03, 0x03], 0, 0x03)
    assert pairs == [(0, O), (1, O)]
