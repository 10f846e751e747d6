"""The Fq / Fq2 primitives ON THE DEVICE, limb for limb, in both layouts — through bn254_debug_fq2_limbs (include/bn254_hip.h) on the case set of
tests/fq_limb_cases.py: raw in-contract limb vectors at the contract's edge, which no byte decoder produces.  Layout 0 runs the classic fp2_* /
fp_* one lane per item; layout 1 runs the pair layout's DEVICE source — the DPP partner fetches and the (p ^ mask) + one negation of
fp_pair_mul_impl, the asm prologue of bn254_pair_sqr_body.inc, the folded negation of fp2_mul_xi, bn_pair_and and the DPP decision of
fp2_u512_greater — which the host builds (and so the interval tracker) never compile.  Every output must equal the Python-integer model and
the host twin word for word; flags must be equal; there is no tolerance anywhere.  tests/test_fq_limb_cases.py proves on the CPU that the
cases lie inside the contracts and are not tame.  Run on the MI355X box: -m gpu."""
import ctypes

import pytest

from tests import fq_limb_cases as F
from tests import hostsim_binding as hs

pytestmark = pytest.mark.gpu
LAYOUTS = (0, 1)
BATCHES = (1, 63, 64, 65, 129)                      # items (layout 1: lane pairs); 129 crosses the 128-pair workgroup
POSITION_OPS = ("mul", "sqr", "mul_fp", "mul_xi", "mul_xi_n", "inv")   # ops whose device form reads the partner lane through quad_perm selectors
E_BAD_ARGUMENT = -10001


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def ref():
    """{op: (cases, [(limbs, flag)] by layout)}: the host twins' words, checked against the model here — computed once, never changed"""
    out = {}
    for op in F.OPS:
        cs = F.cases(op)
        ops_b, k_b = F.pack(cs)
        twins = []
        for layout in LAYOUTS:
            o, fl, _ = hs.fq2_limbs(layout, F.OPS[op], ops_b, k_b, len(cs))
            twins.append(tuple(F.unpack(o, fl, len(cs))))
        for c, t0, t1 in zip(cs, twins[0], twins[1]):
            want, want_flag = F.expected(c)
            if want is None:
                F.check_inv(c, t0[0])
                want = t0[0]
            assert t0 == t1 == (want, want_flag), (op, c.tag)
        out[op] = (cs, twins)
    return out


def run(eng, layout, op, cs):
    ops_b, k_b = F.pack(cs)
    o, fl = eng.debug_fq2_limbs(layout, F.OPS[op], ops_b, k_b, len(cs))
    return F.unpack(o, fl, len(cs))


def assert_same(got, want, cs, what):
    wrong = [(i, c.tag, c.a, c.k, g, w) for i, (c, g, w) in enumerate(zip(cs, got, want)) if g != w]
    assert not wrong, (what, len(wrong), wrong[:2])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("op", list(F.OPS))
def test_whole_set(eng, ref, op, layout):
    """every case of the op in one call: model, host twin and device agree on all 18 words and the flag"""
    cs, twins = ref[op]
    assert_same(run(eng, layout, op, cs), twins[layout], cs, (op, layout))


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n", BATCHES)
def test_batch_sizes(eng, ref, n, layout):
    """partial waves and the workgroup boundary: every op on n consecutive cases (a different window per op and size)"""
    for op in F.OPS:
        cs, twins = ref[op]
        lo = (F.OPS[op] * 37 + n) % (len(cs) - n)
        assert_same(run(eng, layout, op, cs[lo:lo + n]), twins[layout][lo:lo + n], cs[lo:lo + n], (op, layout, n, lo))


@pytest.mark.parametrize("op", POSITION_OPS)
def test_pair_result_ignores_position_and_neighbour(eng, ref, op):
    """layout 1: a lane pair shares its quad of lanes with ONE other pair, and the partner fetches are quad_perm selectors — each case at the even
    and at the odd pair index of its quad, beside an extreme-limb case and beside zero, gives the same words as alone"""
    cs, twins = ref[op]
    weight = lambda c: sum(abs(x) for o in c.a for half in o for x in half[:8])
    loud = max(range(len(cs)), key=lambda i: weight(cs[i]))
    zero = F._mk(op, "zero")
    F.check_contract(zero)
    ops_b, k_b = F.pack([zero])
    zero_want = F.unpack(*hs.fq2_limbs(1, F.OPS[op], ops_b, k_b, 1)[:2], 1)[0]            # the host twin's words, checked against the model
    model, model_flag = F.expected(zero)
    assert zero_want == ((0,) * 18 if model is None else model, model_flag)
    for neighbour, n_want in ((cs[loud], twins[1][loud]), (zero, zero_want)):
        for case_first in (True, False):
            batch, want = [], []
            for c, w in zip(cs, twins[1]):
                batch += [c, neighbour] if case_first else [neighbour, c]
                want += [w, n_want] if case_first else [n_want, w]
            assert_same(run(eng, 1, op, batch), want, batch, (op, neighbour.tag, "even" if case_first else "odd"))


def test_refused_arguments(eng):
    lib, h = eng._lib, eng._h
    cs = F.cases("add")[:4]
    ops_b, k_b = F.pack(cs)
    out, fl = ctypes.create_string_buffer(72 * 4), ctypes.create_string_buffer(4)
    call = lambda layout, op, a, k, n, o, f: lib.bn254_debug_fq2_limbs(h, layout, op, a, k, n, o, f)
    assert call(0, 0, ops_b, k_b, 4, out, fl) == 0 and call(1, 0, ops_b, k_b, 4, out, fl) == 0
    for layout in (-1, 2, 3):
        assert call(layout, 0, ops_b, k_b, 4, out, fl) == E_BAD_ARGUMENT
    for layout in LAYOUTS:
        for op in (-1, len(F.OPS), 1000):
            assert call(layout, op, ops_b, k_b, 4, out, fl) == E_BAD_ARGUMENT
        assert call(layout, 0, None, k_b, 4, out, fl) == E_BAD_ARGUMENT
        assert call(layout, 0, ops_b, None, 4, out, fl) == E_BAD_ARGUMENT
        assert call(layout, 0, ops_b, k_b, 4, None, fl) == E_BAD_ARGUMENT
        assert call(layout, 0, ops_b, k_b, 4, out, None) == E_BAD_ARGUMENT
        assert call(layout, 0, None, None, 0, None, None) == 0             # n == 0 returns at once
        assert call(layout, len(F.OPS), None, None, 0, None, None) == E_BAD_ARGUMENT
    assert lib.bn254_debug_fq2_limbs(None, 0, 0, ops_b, k_b, 4, out, fl) == E_BAD_ARGUMENT
    assert eng.debug_fq2_limbs(1, 0, b"", b"", 0) == (b"", b"")
