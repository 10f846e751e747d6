"""The Jacobi symbol of the hash filter on the case set of tests/jacobi_cases.py, CPU only: the mirror of the passes and the host build of the
header (tests/hostsim/hostsim.cpp: hs_jacobi — the plain-C++ borrow loop, no wave votes) against the references on every case, and the
COVERAGE the set claims, asserted from the mirror's counters.  tests/test_gpu_jacobi.py runs the same cases through the device's own borrow
chains and votes (bn254_debug_jacobi)."""
import os
import subprocess
import sys

import pytest

from tests import hostsim_binding as hs
from tests import jacobi_cases as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = J.Q


@pytest.fixture(scope="module")
def traces():
    """the mirror's trace of every mode-0 and mode-2 case, once"""
    return ([J.mirror(c.a, Q) for c in J.mode0_cases()], [J.mirror(c.a, c.b) for c in J.mode2_cases()])


def by_class(cases, verdicts):
    seen = {}
    for c, v in zip(cases, verdicts):
        seen.setdefault(c.cls, set()).add(v)
    return seen


def test_builder_imports_nothing_from_the_library():
    p =subprocess.run([sys.executable, "-c", "import sys; from tests import jacobi_cases as k; k.mode2_cases(); k.mode1_cases(); "
                        "print([n for n in sys.modules if n.startswith('bn254_amd') or 'hostsim' in n])"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "[]", (p.stdout, p.stderr[-500:])


def test_the_set_holds_what_it_claims():
    c0, c1, c2 = J.mode0_cases(), J.mode1_cases(), J.mode2_cases()
    v0 = {c.a for c in c0}
    assert {0, 1, 2, 3, 4, Q - 1, Q - 2, (Q - 1) // 2, (Q + 1) // 2} <= v0
    for k in range(257):
        assert all(v in v0 for v in (1 << k, Q - (1 << k), (1 << k) - 1) if 0 <= v < Q), k
    assert {1 << 253, (1 << 253) - 1, Q - (1 << 253)} <= v0 and 1 << 254 > Q
    odd = [c.a for c in c0 if c.cls == "odd << s"]
    assert {(a & -a).bit_length() - 1 for a in odd} == set(range(1, 32))
    words = [c.a for c in c0 if c.cls == "k << 32j"]
    assert {((a & -a).bit_length() - 1) // 32 for a in words} >= set(range(1, 7)) and all(a % (1 << 32) == 0 for a in words)
    assert [c.a for c in c0 if c.cls == "slow"] == [v for _, v in J.slow_values()]
    assert sum(c.cls == "random" for c in c0) == J.N_RANDOM == sum(c.cls == "random" for c in c1) == 4096
    assert all(0 <= c.a < Q for c in c0 + c1)
    x1 = {c.a for c in c1}
    assert {0, 1, 2, Q - 1, Q - 2} <= x1 and all({1 << (29 * k), (1 << (29 * k)) - 1} <= x1 for k in range(1, 9)) and 1 << (29 * 9) > Q
    # mode 2: moduli of every width, each with its word shifts, edges, shared factors and random pairs; the mode-0 set again over q
    assert all(c.b & 1 and c.b >= 3 and 0 <= c.a < c.b for c in c2)
    for width in J.WIDTHS:
        mine = [c for c in c2 if c.cls.startswith("%d bits: " % width)]
        assert {c.b.bit_length() for c in mine} == {width}
        assert {c.cls.split(": ")[1] for c in mine} == {"k << 32j", "edges", "shared factor", "random"}
        for b in {c.b for c in mine if c.cls.endswith("edges")}:
            assert {1, b - 1} <= {c.a for c in mine if c.b == b}
            assert {((c.a & -c.a).bit_length() - 1) // 32 for c in mine if c.b == b and c.cls.endswith("k << 32j")} == set(range(1, (width - 1) // 32 + 1))
    assert {c.a for c in c2 if c.b == 3} == {0, 1, 2}
    assert [c.a for c in c2 if c.cls == "mode-0 set over q"] == [c.a for c in c0] and all(c.b == Q for c in c2 if c.cls == "mode-0 set over q")


def test_references_agree_with_each_other():
    """Euler's criterion and the textbook symbol are independent of each other: over the prime q they must say the same"""
    for c in J.mode0_cases():
        assert J.want0(c.a) == (0 if J.jacobi(c.a, Q) == -1 else 1), hex(c.a)
    assert [J.jacobi(a, 15) for a in range(15)] == [0, 1, 1, 0, 1, 0, 0, -1, 1, 0, 0, -1, 0, -1, -1]
    assert J.jacobi(1001, 9907) == -1 and J.jacobi(19, 45) == 1 and J.jacobi(8, 21) == -1 and J.jacobi(5, 21) == 1


def test_mirror_equals_the_references_on_the_whole_set(traces):
    t0, t2 = traces
    for c, tr in zip(J.mode0_cases(), t0):
        assert (tr.symbol != 1) == J.is_square(c.a) and tr.left == 0, hex(c.a)
        assert (tr.symbol == 2) == (c.a == 0)
    for c, tr in zip(J.mode2_cases(), t2):
        assert tr.symbol == J.want2(c.a, c.b) and tr.left == 0, (hex(c.a), hex(c.b))
    for c in J.mode1_cases():
        v, fl = J.want1(c.a)
        assert J.mirror_is_square(v) == (fl == 3), hex(c.a)


def test_host_build_equals_the_references_on_the_whole_set():
    for c in J.mode0_cases():
        assert hs.jacobi(0, c.a) == (c.a, J.want0(c.a)), hex(c.a)
    for c in J.mode1_cases():
        assert hs.jacobi(1, c.a) == J.want1(c.a), hex(c.a)
    for c in J.mode2_cases():
        assert hs.jacobi(2, c.a, c.b) == (c.a, J.want2(c.a, c.b)), (hex(c.a), hex(c.b))


def test_mode_2_over_q_equals_mode_0():
    for c in J.mode0_cases():
        sym = hs.jacobi(2, c.a, Q)[1]
        assert sym in (0, 1, 2) and (sym != 1) == bool(hs.jacobi(0, c.a)[1]) and (sym == 2) == (c.a == 0), hex(c.a)


def test_host_build_refuses_what_the_hook_refuses():
    for a in (Q, Q + 1, (1 << 256) - 1):
        assert hs.jacobi(0, a) == (0, 0x80) and hs.jacobi(1, a) == (0, 0x80)
    for a, b in ((1, 4), (0, 1), (0, 0), (1, 2), (3, 3), (7, 5), (Q, Q), (1, 1 << 255)):
        assert hs.jacobi(2, a, b) == (0, 0x80), (a, b)
    top = (1 << 256) - 1                                             # the widest modulus the operand format holds is still accepted
    assert hs.jacobi(2, 2, 3) == (2, 1) and hs.jacobi(2, top - 1, top) == (top - 1, J.want2(top - 1, top))


def test_coverage_conditions(traces):
    """conditions, not measurements: what the set exists for is there, by the mirror's own counters"""
    t0, t2 = traces
    c0, c1, c2 = J.mode0_cases(), J.mode1_cases(), J.mode2_cases()
    # both verdicts in every class (mode 2: both signs; symbol 0 wherever a class is built to share a factor)
    for cls, seen in by_class(c0, [J.want0(c.a) for c in c0]).items():
        assert seen == {0, 1}, cls
    for cls, seen in by_class(c1, [J.want1(c.a)[1] for c in c1]).items():
        assert seen == {0, 3}, cls
    for cls, seen in by_class(c2, [J.want2(c.a, c.b) for c in c2]).items():
        assert {0, 1} <= seen, cls
        assert 2 in seen or not cls.endswith(("shared factor", "edges", "tiny modulus")), cls
    both = t0 + t2
    # a whole-word shift in each of the four phases
    for w in J.PHASES:
        assert any(tr.shifts[w] for tr in t2), w
    assert any(tr.shifts[8] for tr in t0)                           # ... and under q itself
    assert max(sum(tr.shifts.values()) for tr in t0) >= 6           # k << 192: six shifts in one run
    # every strip count, swaps and passes without one, each sign rule flipping and not flipping
    assert set().union(*(tr.strips for tr in t0)) == set(range(32))
    assert any(tr.swaps for tr in both) and any(tr.stays for tr in both)
    rule2 = set().union(*(tr.rule2 for tr in t0))
    assert rule2 == {(s, n) for s in (0, 1) for n in (1, 3, 5, 7)}   # flips iff s odd and n = 3, 5 (mod 8): two of the eight
    recip = set().union(*(tr.recip for tr in t0))
    assert recip == {(o, n) for o in (1, 3) for n in (1, 3)}         # flips iff both are 3 (mod 4): one of the four
    # lanes that enter phases 6, 4 and 2 with no pass in a wider one — and, under q, none does
    for w, width in ((6, 192), (4, 128), (2, 64)):
        direct = [c for c, tr in zip(c2, t2) if tr.entered_directly(w)]
        assert direct and any(c.b.bit_length() == width for c in direct), w
    assert all(tr.per_phase[8] > 0 for c, tr in zip(c0, t0) if c.a)
    # every phase runs passes under q as well (the operands shrink through all four)
    assert all(any(tr.per_phase[w] for tr in t0) for w in J.PHASES)


def test_pass_counts_stay_below_the_budget(traces):
    t0, t2 = traces
    slowest = max(tr.passes for tr in t0 + t2)
    assert slowest < J.BUDGET
    assert slowest <= 508                                            # each pass removes at least one bit of |a| + |n| <= 2 * 254
    # the figures of the module's docstring
    assert J.slow_values()[0][0] == max(tr.passes for c, tr in zip(J.mode0_cases(), t0) if c.cls == "slow") == 207
    assert "207 passes" in J.__doc__ and "with %d" % slowest in J.__doc__
    # a run out of budget is visible in the mirror as an operand left over: the check above would catch it
    assert J.mirror(J.slow_values()[0][1], Q, budget=100).left != 0
