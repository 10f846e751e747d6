"""Every case of tests/group_cases.py through the device source compiled for the host (tests/hostsim): jac_add, jac_mul, jac_accumulate
and the one-lane Fq12 tower, composed as k_g1_add / k_g2_add / k_g2_mul / k_g1_sum / k_g2_sum / k_debug_fp12_op compose them, against
the model's expectations — outputs and statuses of every item, bit-exact.  On the host BN_WAVE_ANY(x) is (x): what is checked here is
the arithmetic and the select logic; the wave vote itself is checked by the same cases in tests/test_gpu_group_ops.py."""
import pytest

from tests import group_cases as gc
from tests import hostsim_binding as hs

GROUPS = [gc.G1, gc.G2]


@pytest.mark.parametrize("G", GROUPS, ids=lambda G: G.name)
def test_additions(G):
    add = hs.g2_add if G is gc.G2 else hs.g1_add
    n = 0
    for batch in gc.add_batches(G.name):
        for lane, it in enumerate(batch):
            st, out = add(it["a"], it["b"])
            assert (st, out) == (it["status"], it["want"]), (len(batch), lane, it["kind"])
            n += 1
    assert n == sum(len(b) for b in gc.add_batches(G.name)) > 1700


@pytest.mark.parametrize("G", GROUPS, ids=lambda G: G.name)
def test_jac_add_on_jacobian_operands(G):
    """jac_add below the byte decoders: every Z = 0 triple is the identity (also one whose X and Y make the P = -Q test fire: the
    identity overrides come last), and points with Z != 1"""
    cases = gc.jacobian_add_cases(G.name)
    kinds = [cs["kind"] for cs in cases]
    assert {k: kinds.count(k) for k in set(kinds)} == {"O + P": 16, "P + O": 16, "O + O": 8, "P + Q": 12, "P + P": 6, "P + (-P)": 6}
    for i, cs in enumerate(cases):
        assert hs.jac_add_raw(G is gc.G2, cs["p"], cs["q"]) == cs["want"], (i, cs["kind"])


def test_g2_multiplication_raw_and_reduced():
    mc = gc.g2_mul_cases()
    for reduce in (False, True):
        for i, it in enumerate(mc["items"]):
            st, out = hs.g2_mul(mc["bases"][it["base"]], gc.be(it["k"]), reduce=reduce)
            assert (st, out) == (it["status"], it["want", reduce]), (i, it["kind"], hex(it["k"]), reduce)
    # the generator passed explicitly and the built-in one (points = NULL) are the same base
    for it in mc["items"]:
        if it["kind"] == "generator" and it["set"] == "edge":
            assert hs.g2_mul(None, gc.be(it["k"]))[1] == it["want", False]


@pytest.mark.parametrize("G", GROUPS, ids=lambda G: G.name)
def test_segmented_sums(G):
    msum = hs.g2_msum if G is gc.G2 else hs.g1_msum
    for call in gc.sum_calls(G.name):
        for i, seg in enumerate(call.segments):
            st, out = msum(seg)
            assert (st, out) == (call.status[i], call.want[i]), (call.name, i, len(seg), call.notes.get(i))


def test_fp12_ops_vs_model():
    seen = set()
    for cs in gc.fp12_cases():
        got = hs.fp12_op(gc.FP12_OPS[cs["op"]], cs["a"], cs["b"])
        assert got == cs["want"], (cs["op"], cs["kind"])
        seen.add(cs["op"])
    assert seen == set(gc.FP12_OPS)
