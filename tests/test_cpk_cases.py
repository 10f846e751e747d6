"""check_public_keys on the case set of tests/cpk_cases.py: the set itself (anchors, what makes it discriminating), the one-lane kernel
body compiled for the host (tests/hostsim/hostsim.cpp: hs_check_public_keys — bn254_io.h decoders, miller_loop<true, true> with
G1::one() as pair A's point, the final exponentiation) under every flags value against the oracle, and the same cases once under the
bound-tracking build.  CPU only; tests/test_gpu_check_public_keys.py runs the same cases on every layout of the device."""
import os
import subprocess
import sys

import pytest

from oracle import bn254_model as m
from oracle import c_oracle as c
from tests import cpk_cases as ck
from tests import hostsim_binding as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_builder_imports_nothing_from_the_library():
    src = open(os.path.join(ROOT, "tests", "cpk_cases.py")).read()
    assert "bn254_amd" not in src and "hostsim" not in src
    p = subprocess.run([sys.executable, "-c", "import sys; from tests import cpk_cases as k; k.expected(3); "
                        "print([n for n in sys.modules if n.startswith('bn254_amd') or 'hostsim' in n])"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "[]", (p.stdout, p.stderr[-500:])


def test_anchors_and_what_makes_the_set_discriminating(derived, kats):
    cs, names = ck.cases(), ck.names()
    ln = ck.length()
    assert ln >= 40 and all(ln % d for d in range(2, ln))      # prime: tiling walks every case through every slot
    assert len({(x.pk_g2, x.pk_g1) for x in cs}) == ln
    exp = {f: ck.expected(f) for f in ck.FLAGS}
    for name, want in ck.ANCHORS.items():
        i = names.index(name)
        assert tuple(exp[f][i] for f in ck.FLAGS) == want, name
    assert {0, 4, 6, 9} <= set(exp[0])
    assert sum(a != b for a, b in zip(exp[0], exp[1])) >= 2
    assert sum(a != b for a, b in zip(exp[0], exp[2])) >= 3
    # the decode order is observable: the single-operand codes differ, and the pair reports pk_g2's
    codes = ck.order_pair_codes()
    assert len(codes) >= 3
    for name, (flags, only_g2, only_g1, both) in codes.items():
        assert only_g2 not in (0, 9) and only_g1 not in (0, 9) and only_g2 != only_g1 and both == only_g2, (name, flags, only_g2, only_g1, both)
        assert exp[flags][names.index(name)] == only_g2
    # in both assignments of the codes 4 and 6, and one with each flag
    assert {(g2, g1) for flags, g2, g1, _ in codes.values() if flags == 0} == {(4, 6), (6, 4)}
    assert {flags for flags, _, _, _ in codes.values()} == {0, 1, 2}
    # the golden point outside the subgroup is the one the fixtures hand out, and the reference's two vectors are in the set's classes
    assert cs[names.index("off-subgroup pk_g2, valid pk_g1")].pk_g2 == bytes.fromhex(derived["g2_not_in_subgroup"])
    assert sorted(v["status"] for v in kats["check_public_keys"]) == [0, 9]
    for v in kats["check_public_keys"]:
        pair = c.public_key_g2(bytes.fromhex(v["sk_g2"])), c.public_key_g1(bytes.fromhex(v["sk_g1"]))
        assert all(c.check_public_keys(*pair, flags=f) == v["status"] for f in ck.FLAGS)


def test_tiled_walks_the_set():
    ln = ck.length()
    g2, g1, want = ck.tiled(2 * ln + 3, 1, shift=5)
    assert len(g2) == 128 * len(want) and len(g1) == 64 * len(want) == 64 * (2 * ln + 3)
    for i in (0, 1, ln - 6, ln - 5, 2 * ln + 2):
        cs = ck.cases()[(i + 5) % ln]
        assert (g2[128 * i:128 * i + 128], g1[64 * i:64 * i + 64], want[i]) == (cs.pk_g2, cs.pk_g1, ck.expected(1)[(i + 5) % ln])
        assert ck.case_at(i, 5) is cs
    assert ck.tiled(0, 0) == (b"", b"", b"")
    assert ck.first_difference(want, want) is None
    wrong = bytearray(want); wrong[7] ^= 1; wrong[20] ^= 1
    assert ck.first_difference(bytes(wrong), want, 5).startswith("item 7 of %d (%s)" % (len(want), ck.case_at(7, 5).name))


def _point(group, b):
    st, p = group.decode(b)
    assert st == m.OK
    return p


def test_big_integer_model_agrees_where_both_keys_decode():
    """the C oracle's 0 / 9 against oracle/bn254_model.py (affine big-integer pairing) on the cases that reach the pairing with an
    identity on either side, keys off the subgroup or negated keys — the statuses no reference vector pins"""
    from tests import group_cases as gc
    picked = [cs for cs in ck.cases() if "identity" in cs.name or "off-subgroup" in cs.name or "negated" in cs.name or "2 sk" in cs.name]
    ran = 0
    for cs in picked:
        i = ck.names().index(cs.name)
        if ck.expected(0)[i] not in (0, 9):
            continue
        want = m.check_public_keys_status(_point(gc.G2, cs.pk_g2), _point(gc.G1, cs.pk_g1))
        assert want == ck.expected(0)[i], cs.name
        ran += 1
    assert ran >= 10


@pytest.mark.parametrize("flags", ck.FLAGS)
def test_host_build_of_the_one_lane_kernel_body_vs_oracle(flags):
    want = ck.expected(flags)
    got = bytes(hs.check_public_keys(cs.pk_g2, cs.pk_g1, flags) for cs in ck.cases())
    assert got == want, ck.first_difference(got, want)


BOUNDS_DRIVER = r'''
import ctypes, sys
root = sys.argv[1]
sys.path.insert(0, root)
from tests import cpk_cases as ck
hs = ctypes.CDLL(root + "/tests/hostsim/libhostsim_bounds.so")
hs.hs_check_public_keys.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint32]
for flags in ck.FLAGS:
    want = ck.expected(flags)
    got = bytes(hs.hs_check_public_keys(cs.pk_g2, cs.pk_g1, flags) for cs in ck.cases())
    assert got == want, (flags, ck.first_difference(got, want))
print("ok", ck.length())
'''


def test_bounds_hold_on_the_check_public_keys_flow():
    """a flow of its own for the interval bookkeeping (tests/test_bounds.py): an identity on either side, G1::one() as pair A's point
    and the substituted generators of failed decodes are operation sequences its "verify" flow never walks.  Every case under every
    flags value; the statuses are compared with the oracle's there too."""
    hs.build_all()
    p = subprocess.run([sys.executable, "-c", BOUNDS_DRIVER, ROOT], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip() == "ok %d" % ck.length(), (p.stdout[-500:], p.stderr[-2000:])
