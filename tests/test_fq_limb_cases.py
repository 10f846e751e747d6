"""The case set of tests/fq_limb_cases.py against the four HOST twins of bn254_debug_fq2_limbs: the classic layout's fp2_* (hs_fq2_limbs) and the
pair layout's host branches (hp_fq2_limbs), each in the plain build and in the interval-tracking build with the operands' intervals set from the
limbs handed over.  Output limbs equal the Python-integer model word for word, flags are equal, and the tracking builds accept every case —
which ties the contract predicates of the case module to the tracker's own.  CPU only; the device meets the same cases in
tests/test_gpu_fq_limbs.py."""
import math

import pytest

from tests import fq_limb_cases as F
from tests import hostsim_binding as hs

TARGETS = [(0, False), (0, True), (1, False), (1, True)]      # (layout, tracking build)


@pytest.fixture(scope="module")
def twin_outputs():
    """{(op, layout, bounds): ([(limbs, flag)], violated)}: every op's whole case set through every twin, once"""
    hs.build_all()
    out = {}
    for op in F.OPS:
        cs = F.cases(op)
        ops_b, k_b = F.pack(cs)
        for layout, bounds in TARGETS:
            o, fl, violated = hs.fq2_limbs(layout, F.OPS[op], ops_b, k_b, len(cs), bounds=bounds)
            out[op, layout, bounds] = (F.unpack(o, fl, len(cs)), violated)
    return out


def test_op_numbers_match_the_header():
    """the op numbers of the case module are the enum of bn254_fq2_hook.h, and every op is in both"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bn254_amd", "csrc", "bn254_fq2_hook.h")).read()
    enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"FQ2_([A-Z0-9_]+) = (\d+)", text)}
    count = enum.pop("op_count")
    assert enum == F.OPS and sorted(enum.values()) == list(range(count))


@pytest.mark.parametrize("op", list(F.OPS))
def test_cases_lie_inside_the_contract(op):
    """every generated case satisfies its primitive's contract as the case module restates it, and is exercised at all"""
    cs = F.cases(op)
    assert len(cs) >= 200 and len({(c.a, c.k) for c in cs}) > len(cs) * 9 // 10
    for c in cs:
        F.check_contract(c)


@pytest.mark.parametrize("op", list(F.OPS))
def test_case_set_is_not_tame(op):
    """every product op reaches accumulator values beyond +-2^62, every accumulator value fits int64 (asserted inside the model), and every
    op with a value bound has a case within 1 % of it"""
    st = F.op_stats(op)
    F.check_tameness(op, st)
    print("%-12s cases %5d  largest column %s  smallest %s  largest bounded quantity %.2f  largest |value / q| %.2f" % (
        op, st["cases"], _log2(st.get("col_hi", 0)), _log2(st.get("col_lo", 0)), float(st["reach"]), float(st["max_voq"])))


def _log2(x):
    return "-" if x == 0 else "%s2^%.2f" % ("-" if x < 0 else "", math.log2(abs(x)))


@pytest.mark.parametrize("layout,bounds", TARGETS)
@pytest.mark.parametrize("op", list(F.OPS))
def test_twin_equals_model(twin_outputs, op, layout, bounds):
    got, violated = twin_outputs[op, layout, bounds]
    cs = F.cases(op)
    assert len(got) == len(cs)
    if violated:                                   # name the case: one by one through the same build
        for c in cs:
            ops_b, k_b = F.pack([c])
            assert not hs.fq2_limbs(layout, F.OPS[op], ops_b, k_b, 1, bounds=True)[2], ("BOUND VIOLATION", op, c.tag, c.a, c.k)
    assert not violated
    for c, (limbs, flag) in zip(cs, got):
        want, want_flag = F.expected(c)
        if want is None:
            F.check_inv(c, limbs)
        else:
            assert limbs == want, (op, c.tag, c.a, c.k, limbs, want)
        assert flag == want_flag, (op, c.tag, c.a, c.k, flag, want_flag)


@pytest.mark.parametrize("op", list(F.OPS))
def test_twins_agree_word_for_word(twin_outputs, op):
    """the four twins return the same words — the inverse's included, whose limbs the model does not predict"""
    ref = twin_outputs[op, 0, False][0]
    for layout, bounds in TARGETS[1:]:
        assert twin_outputs[op, layout, bounds][0] == ref, (op, layout, bounds)


@pytest.mark.parametrize("layout", [0, 1])
def test_tracker_rejects_what_the_contract_excludes(layout):
    """the tie between the predicates and the tracker is not vacuous: cases just outside a contract trip the tracking build (recorded, not
    aborted) and the case module's predicate alike"""
    lazy = F.lazy_limbs(3, 0, F.SIGN_PATTERNS[0])
    outside = [F._mk("mul", "column", a=(lazy, lazy), b=(lazy, lazy)),
               F._mk("reduce_weak", "value", a=(F.rep(601 * F.Q, 1, F._rng("outside")), F.ZERO)),
               F._mk("norm", "limb", a=((F.I32 - F.HALF - 64,) * 8 + (0,), F.ZERO)),
               F._mk("canon", "value", a=(F.rep(81 * F.Q, 1, F._rng("outside")), F.ZERO))]
    for c in outside:
        with pytest.raises(AssertionError):
            F.check_contract(c)
        ops_b, k_b = F.pack([c])
        assert hs.fq2_limbs(layout, F.OPS[c.op], ops_b, k_b, 1, bounds=True)[2], c.tag


def test_twins_refuse_unknown_ops():
    import ctypes
    ops_b, k_b = F.pack([F._mk("add", "x")])
    for layout in (0, 1):
        hs.fq2_limbs(layout, 0, ops_b, k_b, 1)
        L, f = hs._fq2[layout, False]
        o, fl = ctypes.create_string_buffer(72), ctypes.create_string_buffer(1)
        assert f(len(F.OPS), ops_b, k_b, 1, o, fl) == -1 and f(-1, ops_b, k_b, 1, o, fl) == -1
        assert f(0, None, k_b, 1, o, fl) == -1 and f(0, None, None, 0, None, None) == 0
