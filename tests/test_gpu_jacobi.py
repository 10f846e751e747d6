"""The Jacobi symbol of the hash filter ON THE DEVICE — the hand-written borrow chains of u32xw_sub<8/6/4/2> and the wave votes that end a
phase, which the host build does not compile — element-wise through bn254_debug_jacobi (include/bn254_hip.h) against Python integers: the
whole case set of tests/jacobi_cases.py in all three modes, fp_sqrt on the same values (non-residues included), the same values in wave
arrangements that change which lanes vote together, the existing bn254_debug_hash_candidate hook against mode 1, and the refused arguments.
tests/test_jacobi_cases.py proves on the CPU that the set covers what it claims.  Run on the MI355X box: -m gpu."""
import ctypes
import hashlib
import random

import pytest

from tests import jacobi_cases as J

pytestmark = pytest.mark.gpu
Q = J.Q


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def want():
    """the references on the whole set, computed once: value -> flag (mode 0), x -> (value, flags) (mode 1), (a, b) -> flag (mode 2; over
    q by Euler's criterion, which tests/test_jacobi_cases.py shows to agree with the textbook symbol and which is five times quicker)"""
    w0 = {c.a: J.want0(c.a) for c in J.mode0_cases()}
    w2 = {(c.a, c.b): (2 if c.a == 0 else 1 - w0[c.a]) if c.b == Q else J.want2(c.a, c.b) for c in J.mode2_cases()}
    return w0, {c.a: J.want1(c.a) for c in J.mode1_cases()}, w2


def run(eng, mode, a, b=None):
    """-> (values handed to the passes, flag bytes) of one call"""
    value, flags = eng.debug_jacobi(mode, J.be(a), None if b is None else J.be(b), len(a))
    return J.ints(value), list(flags)


def check0(eng, want, values, what):
    got_v, got_f = run(eng, 0, values)
    wrong = [(i, hex(a), f) for i, (a, f) in enumerate(zip(values, got_f)) if f != want[0][a]]
    assert not wrong, (what, len(wrong), wrong[:4])
    assert got_v == list(values), what


def check2(eng, want, pairs, what):
    got_v, got_f = run(eng, 2, [a for a, _ in pairs], [b for _, b in pairs])
    wrong = [(i, hex(p[0]), hex(p[1]), f) for i, (p, f) in enumerate(zip(pairs, got_f)) if f != want[2][p]]
    assert not wrong, (what, len(wrong), wrong[:4])
    assert got_v == [a for a, _ in pairs], what


# ---- a. the whole set against the references -------------------------------------------------------------------------------------------
def test_mode_0_whole_set(eng, want):
    check0(eng, want, [c.a for c in J.mode0_cases()], "case order")


def test_mode_1_whole_set(eng, want):
    xs = [c.a for c in J.mode1_cases()]
    got_v, got_f = run(eng, 1, xs)
    assert got_v == [want[1][x][0] for x in xs] == [(x ** 3 + 3) % Q for x in xs]
    assert all(f in (0, 3) for f in got_f), [(hex(x), f) for x, f in zip(xs, got_f) if f not in (0, 3)][:4]      # filter and square root agree
    assert got_f == [want[1][x][1] for x in xs]


def test_mode_2_whole_set(eng, want):
    check2(eng, want, [(c.a, c.b) for c in J.mode2_cases()], "case order")


def test_mode_2_over_q_equals_mode_0(eng):
    values = [c.a for c in J.mode0_cases()]
    sym, sq = run(eng, 2, values, [Q] * len(values))[1], run(eng, 0, values)[1]
    assert all(s in (0, 1, 2) and (s != 1) == bool(f) and (s == 2) == (a == 0) for a, s, f in zip(values, sym, sq))


def test_fp_sqrt_on_the_mode_0_set(eng, want):
    """the square root the filter guards, on the same values: status 6 exactly on the non-residues, a root of a otherwise"""
    values = [c.a for c in J.mode0_cases()]
    out, st = eng.debug_fp_op(5, J.be(values), None, len(values))
    roots = J.ints(out)
    assert [s for s in st] == [0 if want[0][a] else 6 for a in values]
    assert all(r < Q and r * r % Q == a for a, r, s in zip(values, roots, st) if s == 0)
    assert 1000 < sum(s == 6 for s in st) < len(values) - 1000


# ---- b. wave arrangements: phases end on votes, so who shares a wave must not matter ----------------------------------------------------
def test_mode_0_sorted_and_shuffled(eng, want):
    values = [c.a for c in J.mode0_cases()]
    passes = {a: J.mirror(a, Q).passes for a in set(values)}
    check0(eng, want, sorted(values, key=lambda a: (passes[a], a)), "sorted by pass count: homogeneous waves")
    check0(eng, want, sorted(values), "sorted by value")
    shuffled = list(values)
    random.Random(0x5eed).shuffle(shuffled)
    check0(eng, want, shuffled, "shuffled")


def test_mode_0_one_slow_lane_among_idle_ones_and_one_zero_among_busy_ones(eng, want):
    slow = [v for _, v in J.slow_values()]
    busy = [c.a for c in J.mode0_cases() if c.cls == "random"]
    idle = (0, 1, 2, 3, 5)
    batch = []
    for k, lane in enumerate((0, 63, 17, 32)):                       # a wave of finished and tiny lanes around one that needs 200 passes
        wave = [idle[(i + k) % len(idle)] for i in range(64)]
        wave[lane] = slow[k % len(slow)]
        batch += wave
    for k, lane in enumerate((0, 31, 63)):                           # a wave of full-size lanes around one that never starts
        wave = busy[64 * k:64 * k + 64]
        wave[lane] = 0
        batch += wave
    batch += [0] * 64 + [1] * 64                                     # ... and waves in which nobody works, or everybody one pass
    known = dict(want[0])
    known.update({a: J.want0(a) for a in idle})
    check0(eng, (known,), batch, "mixed waves")


def test_mode_2_arrangements(eng, want):
    cases = [c for c in J.mode2_cases() if c.cls != "mode-0 set over q"]
    by_width = {w: [(c.a, c.b) for c in cases if c.b.bit_length() == w] for w in J.WIDTHS}
    count = min(len(v) for v in by_width.values())
    assert count >= 256
    mixed = [by_width[w][i] for i in range(count) for w in J.WIDTHS]           # every wave holds all four modulus widths, lane by lane
    check2(eng, want, mixed, "all four widths in every wave")
    pairs = [(c.a, c.b) for c in cases]
    check2(eng, want, sorted(pairs, key=lambda p: (p[1].bit_length(), p[0].bit_length(), p)), "sorted by width: homogeneous waves")
    shuffled = list(pairs)
    random.Random(0x5eee).shuffle(shuffled)
    check2(eng, want, shuffled, "shuffled")
    for w in (64, 128, 192):                                                   # one narrow lane in a wide wave, one wide lane in a narrow wave
        wave = by_width[254][:64]
        wave[w % 61] = by_width[w][5]
        check2(eng, want, wave, "a %d-bit lane among 254-bit ones" % w)
        wave = by_width[w][:64]
        wave[w % 59] = by_width[254][7]
        check2(eng, want, wave, "a 254-bit lane among %d-bit ones" % w)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 64 * 3 + 17])
def test_batch_lengths(eng, want, n):
    values = [c.a for c in J.mode0_cases()]
    random.Random(n).shuffle(values)
    check0(eng, want, values[:n], "n = %d" % n)
    pairs = [(c.a, c.b) for c in J.mode2_cases() if c.cls != "mode-0 set over q"]
    random.Random(n + 1).shuffle(pairs)
    check2(eng, want, pairs[:n], "n = %d" % n)
    xs = [c.a for c in J.mode1_cases()][:n]
    assert run(eng, 1, xs) == ([want[1][x][0] for x in xs], [want[1][x][1] for x in xs])


# ---- c. the existing hook agrees with mode 1 --------------------------------------------------------------------------------------------
def test_hash_candidate_hook_agrees_with_mode_1(eng):
    """bn254_debug_hash_candidate on 512 digests: no disagreement bit, and its verdict is mode 1's on the reduced x"""
    hs = [int.from_bytes(hashlib.sha256(b"jacobi digest %d" % i).digest(), "big") for i in range(512)]
    pts, st = eng.debug_hash_candidate(J.be(hs), len(hs))
    assert not any(s & 0x80 for s in st)
    cand = [(i, h % Q) for i, h in enumerate(hs) if h < 5 * Q and h % Q]       # 5q <= h: no candidate (about one digest in nineteen)
    assert 0 < len(hs) - len(cand) < 64 and all(st[i] == 1 for i in set(range(len(hs))) - {i for i, _ in cand})
    xs = [x for _, x in cand]
    got_v, got_f = run(eng, 1, xs)
    assert got_v == [J.curve_rhs(x) for x in xs]
    for (i, x), f in zip(cand, got_f):
        assert f == J.want1(x)[1] and st[i] == (0 if f & 1 else 1), (i, hex(x), f, st[i])
        if st[i] == 0:
            px, py = int.from_bytes(pts[64 * i:64 * i + 32], "big"), int.from_bytes(pts[64 * i + 32:64 * i + 64], "big")
            assert px == x and py * py % Q == J.curve_rhs(x) and py % 2 == 0


# ---- d. refused arguments ----------------------------------------------------------------------------------------------------------------
def test_refused_arguments(eng, want):
    from bn254_amd.engine import NativeError
    for mode, b in ((3, bytes(32)), (-1, bytes(32)), (2, None)):
        with pytest.raises(NativeError) as e:
            eng.debug_jacobi(mode, bytes(32), b, 1)
        assert e.value.rc == -10001
    buf, one = ctypes.create_string_buffer(32), ctypes.create_string_buffer(1)
    for a, v, f in ((None, buf, one), (bytes(32), None, one), (bytes(32), buf, None)):
        assert eng._lib.bn254_debug_jacobi(eng._h, 0, a, None, 1, v, f) == -10001
    for mode in (0, 1, 2):
        assert eng.debug_jacobi(mode, b"", b"", 0) == (b"", b"")
    assert eng._lib.bn254_debug_jacobi(eng._h, 0, None, None, 0, None, None) == 0


def test_out_of_range_operands_set_bit_7_and_leave_their_neighbours_alone(eng, want):
    top = (1 << 256) - 1
    good = [c.a for c in J.mode0_cases() if c.cls == "random"][:8]
    batch = [good[0], Q, good[1], Q + 1, top, good[2], 5 * Q, good[3]]
    got_v, got_f = run(eng, 0, batch)
    assert got_f == [0x80 if a >= Q else want[0][a] for a in batch] and got_v == [0 if a >= Q else a for a in batch]
    got_v, got_f = run(eng, 1, batch)
    assert got_f == [0x80 if x >= Q else J.want1(x)[1] for x in batch] and got_v == [0 if x >= Q else J.curve_rhs(x) for x in batch]
    bad = [(1, 4), (0, 1), (0, 0), (1, 2), (3, 3), (7, 5), (Q, Q), (1, 1 << 255), (top, top)]
    pairs = []
    for k, p in enumerate(bad):
        pairs += [(good[k % 8], Q), p]
    pairs += [(2, 3), (top - 1, top)]                                          # the least and the widest modulus the hook accepts
    got_v, got_f = run(eng, 2, [a for a, _ in pairs], [b for _, b in pairs])
    assert got_f == [0x80 if p in bad else J.want2(*p) for p in pairs]
    assert got_v == [0 if p in bad else p[0] for p in pairs]
