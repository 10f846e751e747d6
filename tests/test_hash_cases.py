"""Hash-to-G1 on the case set of tests/hash_cases.py: the set itself (every kind, every boundary length, the hard messages as hard as
they claim), the two oracles against each other — the C oracle with its own SHA-256, the big-integer model with hashlib's — and the
one-lane body compiled for the host (tests/hostsim/hostsim.cpp: hs_hash_to_g1 — hash_state_init, load_block / padded_byte, hash_try as
the kernels inline them) on EVERY case, the 2^20 + 1 byte message included, in the plain and in the bound-tracking build.  CPU only;
tests/test_gpu_hash_cases.py runs the same cases through every schedule of the device and through its callers."""
import os
import subprocess
import sys

from tests import hash_cases as hc
from tests import hostsim_binding as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_builder_imports_nothing_from_the_library():
    src = open(os.path.join(ROOT, "tests", "hash_cases.py")).read()
    assert "bn254_amd" not in src and "hostsim" not in src
    p = subprocess.run([sys.executable, "-c", "import sys; from tests import hash_cases as k; k.cases(); k.expected(k.cases()[70].msg); k.filler(5); "
                        "print([n for n in sys.modules if n.startswith('bn254_amd') or 'hostsim' in n])"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "[]", (p.stdout, p.stderr[-500:])


def test_every_kind_and_every_boundary_length_is_present():
    cs = hc.cases() + [hc.huge_case()]
    assert {x.kind for x in cs} == set(hc.KINDS)
    assert len({x.name + x.kind for x in cs}) == len(cs)
    assert [len(x.msg) for x in hc.of_kind("every length")] == list(range(201))
    assert [len(x.msg) for x in hc.of_kind("longer")] == list(hc.LONGER) and len(hc.huge_case().msg) == (1 << 20) + 1
    # around every block edge: the length field leaves the counter's block, then the 0x80 byte, then the counter byte
    assert {54, 55, 62, 63, 64, 118, 119, 126, 127, 128, 182, 183, 191, 192} <= set(hc.BOUNDARY) and set(hc.HARD17_LENGTHS) <= set(hc.BOUNDARY)
    contents = hc.of_kind("contents")
    for n in hc.BOUNDARY:
        mine = {x.name.split(": ", 1)[1]: x.msg for x in contents if x.name.startswith("length %d: " % n)}
        assert len(mine) == (8 if n else 7), n
        m = mine["m"]
        assert len(m) == n and mine["all 0x00"] == bytes(n) and mine["all 0xFF"] == b"\xff" * n and mine["all 0x80"] == b"\x80" * n
        assert mine["m || 0x00"] == m + b"\0" and (n == 0 or mine["m[:-1]"] == m[:-1])
        p = mine["padded stream of m"]
        assert len(p) % 64 == 0 and len(p) == 64 * ((n + 10 + 63) // 64) and p[:n] == m and p[n:n + 2] == b"\x00\x80"
        assert int.from_bytes(p[-8:], "big") == 8 * (n + 1) and not any(p[n + 2:-8]) and mine["padded stream of m without its length field"] == p[:-8]
        assert [len(x.msg) for x in hc.of_kind("hard9")].count(n) == (1 if n else 0)             # the one empty message takes a single try
    assert sorted(len(x.msg) for x in hc.of_kind("hard17")) == sorted(hc.HARD17_LENGTHS)
    assert [len(hc.padded_stream(bytes(n), 7)) for n in (0, 54, 55, 63, 64, 118, 119)] == [64, 64, 128, 128, 128, 128, 192]
    s = hc.caller_set()
    assert 60 <= len(s) <= 80 and {len(x.msg) for x in s} >= set(hc.BOUNDARY) | set(hc.LONGER) and len(hc.contents_pairs()) == 2 * len(hc.BOUNDARY) - 1
    f = hc.filler(500)
    assert [len(m) for m in f] == [i % 201 for i in range(500)] and len(set(f[1:201])) == 200 and f[201] == b"" and f[202] != f[1]
    blob, offs = hc.pack(f[:9])
    assert offs[0] == 13 and len(offs) == 10 and offs[-1] == len(blob) and all(blob[offs[i]:offs[i + 1]] == f[i] for i in range(9))


def test_the_two_oracles_agree_on_every_case_they_share():
    shared = [x for x in hc.cases() if len(x.msg) <= hc.MODEL_MAX_LEN]
    assert len(shared) == len(hc.cases()) >= 390
    for x in shared:
        a, b = hc.expectation(x.msg), hc.expectation(x.msg, "model")
        assert (a.src, b.src) == ("c_oracle", "model") and a[:3] == b[:3], x.name
        assert a.status == 0 and 1 <= a.tries <= 255 and a.point != bytes(64), x.name
    big = hc.expectation(hc.huge_case().msg)
    assert big.src == "c_oracle" and big.status == 0
    assert hc.expected(hc.huge_case().msg) == tuple(big[:3])


def test_hard_messages_have_exactly_the_tries_they_claim():
    """by both oracles, not by the filter that found them; the filter itself agrees with the oracles on every case"""
    fx = hc.fixture()
    assert sorted(e["length"] for e in fx) == sorted(hc.HARD17_LENGTHS) and all(e["tag"] == hc.HARD_TAG and e["tries"] >= 17 for e in fx)
    for e in fx:
        m = hc.hard_candidate(e["index"], e["length"])
        assert len(m) == e["length"]
        assert hc.expectation(m).tries == e["tries"] == hc.expectation(m, "model").tries, e
    for x in hc.of_kind("hard9", "hard17"):
        assert hc.expectation(x.msg).tries == hc.claimed_tries(x) >= (9 if x.kind == "hard9" else 17), x.name
    for x in hc.cases():
        assert hc.filter_tries(x.msg) == hc.expectation(x.msg).tries, x.name
    # a counter budget below the try count: HashToPointError, no point, the budget
    x = hc.of_kind("hard9")[3]
    assert hc.expected(x.msg, 8) == (1, bytes(64), 8) and hc.expected(x.msg, hc.claimed_tries(x)) == hc.expected(x.msg)


def test_distinct_messages_of_the_contents_class_have_distinct_points():
    """a stream builder that dropped, doubled or misplaced a byte near the end of the message would make two of these collide: m and m ||
    0x00 (the counter byte of 0 behind m), m and m[:-1], the uniform fills against each other across lengths, and m's own padded stream"""
    point = {}
    for x in hc.of_kind("contents"):
        point[x.msg] = hc.expectation(x.msg).point
    assert len(point) >= 8 * len(hc.BOUNDARY) - 12 and len(set(point.values())) == len(point)
    by_name = {x.name: x.msg for x in hc.of_kind("contents")}
    for n in hc.BOUNDARY:
        m = by_name["length %d: m" % n]
        for what in ("padded stream of m", "padded stream of m without its length field", "m || 0x00"):
            assert point[by_name["length %d: %s" % (n, what)]] != point[m], (n, what)


def test_host_build_of_the_one_lane_body_vs_oracle_on_every_case():
    for x in hc.cases() + [hc.huge_case()]:
        assert hs.hash_to_g1(x.msg) == hc.expected(x.msg), (x.kind, x.name)


def test_first_difference_reports_the_item():
    msgs = [x.msg for x in hc.caller_set()[:20]]
    want = [hc.expected(m) for m in msgs]
    got = (b"".join(w[1] for w in want), bytes(w[0] for w in want), bytes(w[2] for w in want))
    assert hc.first_difference(msgs, got) is None
    bad = bytearray(got[0]); bad[64 * 7 + 5] ^= 1
    assert hc.first_difference(msgs, (bytes(bad), got[1], got[2])).startswith("item 7 (%d bytes)" % len(msgs[7]))
    assert hc.first_difference(msgs, (bytes(bad), got[1], got[2]), only=[0, 3, 6]) is None
    bad = bytearray(got[2]); bad[11] += 1
    assert "points equal" in hc.first_difference(msgs, (got[0], got[1], bytes(bad)))


BOUNDS_DRIVER = r'''
import ctypes, sys
root = sys.argv[1]
sys.path.insert(0, root)
from tests import hash_cases as hc
hs = ctypes.CDLL(root + "/tests/hostsim/libhostsim_bounds.so")
hs.hs_hash_to_g1.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.POINTER(ctypes.c_int)]
ran = 0
for x in hc.cases():
    o, t = ctypes.create_string_buffer(64), ctypes.c_int(0)
    st = hs.hs_hash_to_g1(x.msg, len(x.msg), o, ctypes.byref(t))
    assert (st, o.raw, t.value) == hc.expected(x.msg), x.name
    ran += 1
print("ok", ran)
'''


def test_bound_tracking_host_build_vs_oracle_on_every_case():
    """the interval bookkeeping of tests/test_bounds.py under the same cases: x^3 + 3 and the square root for candidates of every length"""
    hs.build_all()
    p = subprocess.run([sys.executable, "-c", BOUNDS_DRIVER, ROOT], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip() == "ok %d" % len(hc.cases()), (p.stdout[-500:], p.stderr[-2000:])
