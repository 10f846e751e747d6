"""The case set of hash-to-G1 (csrc/bn254_hash.h), shared by tests/test_hash_cases.py (host builds) and tests/test_gpu_hash_cases.py
(every schedule of launch_hash_rounds and its callers).  The stage branches on the message LENGTH: padded_byte / load_block build
msg || ctr || 0x80 || 0.. || be64(8 (len + 1)) byte by byte, hash_state_init splits the stream at block len / 64 (the block of the counter
byte) and pre-compresses the blocks in front of it.  What changes where: 54 -> 55 the length field leaves the counter's block, 62 -> 63 the
0x80 byte does, 63 -> 64 the counter byte itself (first_block = 1, the midstate is no longer the IV); the same at 118/119, 126/127/128,
182/183, 190/191/192.

Messages, deterministic from tests.datagen.D, each with a kind:
  every length   one message of every length 0 .. 200
  longer         LONGER; HUGE (2^20 + 1 bytes) is for the direct route only
  contents       at every BOUNDARY length L: all 0x00, all 0xFF, all 0x80, a base message m, m || 0x00, m[:-1], and m's own padded stream for
                 counter 0 with and without its length field (a message that LOOKS like padding must hash differently)
  hard9          at every BOUNDARY length but 0 (the one empty message takes a single try) a message whose first passing counter is >= 8, found
                 here by a restated filter (hashlib, the range rules, Euler's criterion) — a survivor of every narrow filter round with a
                 multi-block state
  hard17         at HARD17_LENGTHS a message whose first passing counter is >= 16: tests/golden/hash_hard_messages.json (tag, index, length
                 and claimed tries; written by tests/golden/gen_hash_hard.py, the search takes minutes).  The fixture is never trusted:
                 every expectation is recomputed from the oracles.

Expectations are (status, point, tries) from oracle.c_oracle.hash_to_g1 (src "c_oracle", every case) and from
oracle.bn254_model.hash_to_try_and_increment_ex (src "model": SHA-256 from hashlib, independent of the C oracle's own; every case up to
MODEL_MAX_LEN bytes), cached per message.  This module imports nothing from the library under test or its host build."""
import hashlib
import json
import os
from collections import namedtuple

from tests.datagen import D

Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
BOUNDARY = (0, 1, 54, 55, 56, 62, 63, 64, 65, 118, 119, 120, 126, 127, 128, 182, 183, 191, 192)
EVERY = tuple(range(201))
LONGER = (247, 248, 255, 256, 257, 511, 512, 1000, 4096, 65535, 65536, 65537)
HUGE = (1 << 20) + 1
HARD9_LENGTHS = BOUNDARY[1:]
HARD17_LENGTHS = (54, 55, 56, 62, 63, 64, 118, 119, 120, 128, 183)
MODEL_MAX_LEN = 65537
KINDS = ("every length", "longer", "huge", "contents", "hard9", "hard17")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hash_hard_messages.json")
HARD_TAG = "hash-cases/hard"
HARD9_SEARCH = 4000                      # candidates per length at most: 0.5274^8 = 0.6 % of them need nine tries or more

Case = namedtuple("Case", "name kind msg")
Expect = namedtuple("Expect", "status point tries src")


def message(tag, i, length):
    """`length` bytes: D(tag / i, 0) || D(tag / i, 1) || .. cut to size"""
    t = "%s/%d" % (tag, i)
    return b"".join(D(t, b) for b in range((length + 31) // 32))[:length]


def hard_candidate(i, length):
    """candidate i of the searches for hard messages of `length` bytes (here and in tests/golden/gen_hash_hard.py)"""
    return message("%s/%d" % (HARD_TAG, length), i, length)


def padded_stream(msg, ctr=0):
    """what SHA-256 compresses for counter `ctr` (FIPS 180-4 section 5.1.1 on msg || ctr)"""
    v = bytes(msg) + bytes([ctr])
    return v + b"\x80" + bytes((55 - len(v)) % 64) + (8 * len(v)).to_bytes(8, "big")


def filter_tries(msg, limit=255):
    """the try loop restated: counters consumed until the first one that yields a point (limit + 1 if none does).  The digest of msg || ctr
    read big-endian is skipped if >= 5q, reduced by repeated subtraction while > q (so a multiple of q stops AT q and is refused), and
    yields a point iff x^3 + 3 is a square mod q (Euler's criterion; 0 is one)."""
    h0 = hashlib.sha256(bytes(msg))
    for ctr in range(limit):
        h = h0.copy()
        h.update(bytes([ctr]))
        x = int.from_bytes(h.digest(), "big")
        if x >= 5 * Q:
            continue
        while x > Q:
            x -= Q
        if x == Q:
            continue
        rhs = (x * x * x + 3) % Q
        if rhs == 0 or pow(rhs, (Q - 1) // 2, Q) == 1:
            return ctr + 1
    return limit + 1


def find_hard(length, min_tries, start=0, stop=None):
    """(index, tries) of the first candidate of `length` bytes that needs at least min_tries tries"""
    i = start
    while stop is None or i < stop:
        t = filter_tries(hard_candidate(i, length))
        if t >= min_tries:
            return i, t
        i += 1
    raise LookupError((length, min_tries, start, stop))


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)["messages"]


def _contents(length):
    m = message("hash-cases/contents", length, length)
    out = [("all 0x00", bytes(length)), ("all 0xFF", b"\xff" * length), ("all 0x80", b"\x80" * length), ("m", m), ("m || 0x00", m + b"\x00")]
    if length:
        out.append(("m[:-1]", m[:-1]))
    p = padded_stream(m)
    return out + [("padded stream of m", p), ("padded stream of m without its length field", p[:-8])]


_CASES = None
_HUGE = None


def cases():
    """every case but the HUGE one"""
    global _CASES
    if _CASES is None:
        out = [Case("length %d" % n, "every length", message("hash-cases/len", n, n)) for n in EVERY]
        out += [Case("length %d" % n, "longer", message("hash-cases/len", n, n)) for n in LONGER]
        for n in BOUNDARY:
            out += [Case("length %d: %s" % (n, what), "contents", msg) for what, msg in _contents(n)]
        for n in HARD9_LENGTHS:
            i, t = find_hard(n, 9, stop=HARD9_SEARCH)
            out.append(Case("length %d: candidate %d, %d tries" % (n, i, t), "hard9", hard_candidate(i, n)))
        for e in fixture():
            assert e["tag"] == HARD_TAG
            out.append(Case("length %d: candidate %d, %d tries" % (e["length"], e["index"], e["tries"]), "hard17", hard_candidate(e["index"], e["length"])))
        _CASES = out
    return _CASES


def huge_case():
    global _HUGE
    if _HUGE is None:
        _HUGE = Case("length %d" % HUGE, "huge", message("hash-cases/len", HUGE, HUGE))
    return _HUGE


def of_kind(*kinds):
    return [x for x in cases() if x.kind in kinds]


def claimed_tries(case):
    """the try count in the name of a hard case"""
    assert case.kind in ("hard9", "hard17")
    return int(case.name.rsplit(", ", 1)[1].split()[0])


def caller_set():
    """S: one message per boundary length, the hard ones, the longer ones — what the verify-shaped callers are fed"""
    by_len = {len(x.msg): x for x in of_kind("every length")}
    return [by_len[n] for n in BOUNDARY] + of_kind("hard9", "hard17", "longer")


def contents_pairs():
    """[(m, other)] for other = m || 0x00 and m[:-1] at every boundary length: messages that differ in their last byte position only"""
    by_name = {x.name: x.msg for x in of_kind("contents")}
    out = []
    for n in BOUNDARY:
        m = by_name["length %d: m" % n]
        out.append((m, by_name["length %d: m || 0x00" % n]))
        if n:
            out.append((m, by_name["length %d: m[:-1]" % n]))
    return out


_WANT = {}


def _from_c_oracle(msg):
    from oracle import c_oracle
    st, pt, tries = c_oracle.hash_to_g1(msg)
    return Expect(st, pt, tries, "c_oracle")


def _from_model(msg):
    from oracle import bn254_model as model
    try:
        p, tries = model.hash_to_try_and_increment_ex(msg)
    except model.Bn254Error as e:
        return Expect(e.code, bytes(64), 255, "model")
    return Expect(model.OK, model.g1_to_uncompressed(p), tries, "model")


def expectation(msg, src="c_oracle"):
    """the cached Expect of a message from one of the two oracles"""
    msg = bytes(msg)
    if (src, msg) not in _WANT:
        _WANT[src, msg] = {"c_oracle": _from_c_oracle, "model": _from_model}[src](msg)
    return _WANT[src, msg]


def expected(msg, max_tries=255):
    """(status, point, tries) of the C oracle; with a counter budget below the message's try count: HashToPointError, no point, the budget
    (hash.rs:62)"""
    e = expectation(msg)
    if e.tries > max_tries:
        return (1, bytes(64), max_tries)
    return tuple(e[:3])


def filler(n):
    """n messages whose lengths run through 0 .. 200"""
    return [message("hash-cases/filler", i, i % 201) for i in range(n)]


def pack(msgs, prefix=13):
    """(blob, offsets): the messages back to back behind `prefix` junk bytes, offsets[0] = prefix"""
    blob = message("hash-cases/junk", prefix, prefix) + b"".join(msgs)
    offs = [prefix]
    for m in msgs:
        offs.append(offs[-1] + len(m))
    assert len(blob) == offs[-1]
    return blob, offs


def first_difference(msgs, got, max_tries=255, only=None):
    """None if (points, statuses, tries) equal the C oracle's on every message (or on the indices `only`), else a description of the first
    item that differs"""
    pts, st, tries = got
    assert len(st) == len(tries) == len(msgs) and len(pts) == 64 * len(msgs), (len(msgs), len(pts), len(st), len(tries))
    for i in (range(len(msgs)) if only is None else only):
        want = expected(msgs[i], max_tries)
        have = (st[i], pts[64 * i:64 * i + 64], tries[i])
        if have != want:
            return "item %d (%d bytes): status %d tries %d, want status %d tries %d%s" % (
                i, len(msgs[i]), have[0], have[2], want[0], want[2], "" if have[1] != want[1] else ", points equal")
    return None
