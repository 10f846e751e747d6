"""Fr on the device (bn254_amd/csrc/bn254_fr.h) and the Lagrange coefficients at zero (bn254_threshold.h) through their debug hooks
(include/bn254_hip.h: bn254_debug_fr_op, bn254_debug_lagrange_at_zero), against Python integers (tests/threshold_model.py): the case set of
tests/threshold_cases.py and 4 096 random operands per operation.  Run on the MI355X box: -m gpu."""
import pytest

from tests import threshold_cases as TC
from tests import threshold_model as TM

pytestmark = pytest.mark.gpu
R = TC.R


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


def be(values):
    return b"".join(v.to_bytes(32, "big") for v in values)


def run_op(eng, op, pairs):
    a, b = be(p[0] for p in pairs), be(p[1] for p in pairs)
    out = eng.debug_fr_op(op, a, b if op <= 2 else None, len(pairs))
    return [int.from_bytes(out[32 * i:32 * i + 32], "big") for i in range(len(pairs))]


@pytest.mark.parametrize("op", [0, 1, 2, 3, 4, 5])
def test_fr_case_set_and_random_operands(eng, op):
    pairs = TC.fr_pairs() + [(a, 0) for a in TC.FR_INVERSES] + TC.fr_random(4096, 100 + op)
    got = run_op(eng, op, pairs)
    want = [TM.fr_op(op, a, b) for a, b in pairs]
    wrong = [(hex(a), hex(b)) for (a, b), g, w in zip(pairs, got, want) if g != w]
    assert not wrong, (len(wrong), wrong[:3])
    assert all(g < R for g in got)
    if op == 0:
        at = len(TC.FR_OPERANDS) ** 2
        assert got[at:at + len(TC.FR_PRODUCT_PAIRS)] == [0, 0, 1, 1, 1, R - 1, R - 1, R - 1]
    if op == 4:                                                         # a * a^-1 == 1 on the device as well
        inv = run_op(eng, 0, [(a, g) for (a, _), g in zip(pairs, got)])
        assert all(v == (1 if a % R else 0) for (a, _), v in zip(pairs, inv))


def test_fr_u32_load(eng):
    """op 6: the operand's low 32 bits through the uint32_t load, whatever stands above them"""
    values = TC.FR_OPERANDS + TC.FR_INVERSES + TC.FR_U32_LOADS + [a for a, _ in TC.fr_random(4096, 106)]
    assert run_op(eng, 6, [(a, 0) for a in values]) == [TM.fr_load_u32(a) for a in values]


def test_fr_refused_arguments(eng):
    from bn254_amd.engine import NativeError
    for op, b in ((7, bytes(32)), (-1, bytes(32)), (0, None)):
        with pytest.raises(NativeError) as e:
            eng.debug_fr_op(op, bytes(32), b, 1)
        assert e.value.rc == -10001
    assert eng.debug_fr_op(0, b"", b"", 0) == b""


def test_lagrange_at_zero(eng):
    """every point set of the case set as a segment of ONE call (so a lane has to find its segment), with an empty segment among them"""
    sets = TC.lagrange_sets()
    sets.insert(3, [])
    xs, seg = [], [0]
    for s in sets:
        xs += s
        seg.append(len(xs))
    out = eng.debug_lagrange_at_zero(xs, seg)
    got = [int.from_bytes(out[32 * i:32 * i + 32], "big") for i in range(len(xs))]
    want = [v for s in sets for v in TM.lagrange_at_zero(s)]
    assert got == want, [i for i, (g, w) in enumerate(zip(got, want)) if g != w][:8]
    assert got[0] == 1 and got[1] == 1                                  # t = 1: the coefficient is one, whatever the point
    # order does not matter: the descending and the shuffled nine points carry the ascending set's coefficients
    asc, desc, shuf = sets[5], sets[6], sets[7]
    assert asc == sorted(desc) == sorted(shuf)
    lam = dict(zip(asc, TM.lagrange_at_zero(asc)))
    at = seg[6]
    assert [lam[x] for x in desc] == got[at:at + 9] and [lam[x] for x in shuf] == got[seg[7]:seg[7] + 9]
    # the coefficients of a set sum to one (the constant polynomial interpolates to itself)
    for k, s in enumerate(sets):
        if s:
            assert sum(got[seg[k]:seg[k + 1]]) % R == 1, s[:4]
    # offsets that do not start at zero or decrease are refused
    import ctypes
    x = (ctypes.c_uint32 * 4)(1, 2, 3, 4)
    buf = ctypes.create_string_buffer(128)
    for bad in ([1, 4], [0, 3, 2]):
        rc = eng._lib.bn254_debug_lagrange_at_zero(eng._h, x, (ctypes.c_uint64 * len(bad))(*bad), len(bad) - 1, buf)
        assert rc == -10001, bad
