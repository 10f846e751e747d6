"""The pairing products on the case set of tests/pairing_cases.py: the set itself (anchors, what makes it discriminating), the one-lane
kernel body compiled for the host (tests/hostsim/hostsim.cpp: hs_pairing — bn254_io.h decoders with the generator substituted for a
failed operand, one miller_loop<true, false> per pair, the product, the exact final exponentiation) under every flags value against the
oracle, the pair-layout and small-batch bodies (tests/hostsim/hostsim_pair.cpp) on the cases that decode, the big-integer model on a
sample, items longer than the oracle's MAX_PAIRS, and one flow under the bound-tracking build.  CPU only;
tests/test_gpu_pairing.py runs the same cases on every route of the device."""
import ctypes
import os
import subprocess
import sys

import pytest

from oracle import bn254_model as m
from oracle import c_oracle as c
from tests import group_cases as gc
from tests import hostsim_binding as hs
from tests import pairing_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_builder_imports_nothing_from_the_library():
    src = open(os.path.join(ROOT, "tests", "pairing_cases.py")).read()
    assert "bn254_amd" not in src and "hostsim" not in src
    p = subprocess.run([sys.executable, "-c", "import sys; from tests import pairing_cases as k; k.expected(2, 3); k.long_item(3, 1); "
                        "print([n for n in sys.modules if n.startswith('bn254_amd') or 'hostsim' in n])"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "[]", (p.stdout, p.stderr[-500:])


def test_anchors_and_what_makes_the_set_discriminating(derived):
    assert pc.KS == (1, 2, 3, 4)
    for k in pc.KS:
        cs = pc.cases_of(k)
        ln = len(cs)
        assert ln >= 29 and all(ln % d for d in range(2, ln))  # prime: tiling walks every case through every slot
        assert len({(x.g1, x.g2) for x in cs}) == ln
        assert all(x.k == k and len(x.g1) == 64 * k and len(x.g2) == 128 * k and x.name.startswith("k=%d: " % k) for x in cs)
    names = pc.names()
    exp = {f: b"".join(pc.expected(k, f)[0] for k in pc.KS) for f in pc.FLAGS}
    for name, want in pc.ANCHORS.items():
        i = names.index(name)
        assert tuple(exp[f][i] for f in pc.FLAGS) == want, name
    assert {int(n[2]) for n in pc.ANCHORS} == set(pc.KS)
    for f in pc.FLAGS:
        assert {0, 4, 6, 9} <= set(exp[f]), f
        for k in pc.KS:
            want = {4, 6, 9} if k == 1 and f & 2 else {0, 4, 6, 9}     # one pair without an identity is never one
            assert want <= set(pc.expected(k, f)[0]), (k, f)
    assert sum(a != b for a, b in zip(exp[0], exp[1])) >= 8 and sum(a != b for a, b in zip(exp[0], exp[2])) >= 12
    # every kind of single fault sits in the first, a middle and the last pair of every k, and reports its own code
    for k in pc.KS:
        nm, st = pc.names(k), pc.expected(k, 0)[0]
        for kind in list(pc.FAULTS)[:8]:
            for j in pc.placements(k):
                assert st[nm.index("k=%d: %s in pair %d" % (k, kind, j))] == (6 if ">= q" in kind else 4), (k, kind, j)
        for j in pc.placements(k):
            i = nm.index("k=%d: G2 off the subgroup in pair %d" % (k, j))
            assert [pc.expected(k, f)[0][i] for f in pc.FLAGS] == [9, 4, 9, 4]
            for what, code in (("identity G1", 9 if k > 1 else 0), ("identity G2", 9 if k > 1 else 0)):
                i = nm.index("k=%d: %s in pair %d" % (k, what, j))
                assert [pc.expected(k, f)[0][i] for f in pc.FLAGS] == [code, code, 4, 4]
        i = nm.index("k=%d: every pair both identities" % k)
        assert [pc.expected(k, f) [0][i] for f in pc.FLAGS] == [0, 0, 4, 4] and pc.expected(k, 0)[1][i].hex() == derived["gt_one"]
    assert pc.placements(4) == [0, 2, 3] and pc.placements(1) == [0]
    # products that are one have the Gt one, the others do not; the oracle writes no Gt for a failed item
    for k in pc.KS:
        for f in pc.FLAGS:
            st, gt = pc.expected(k, f)
            for i in range(len(st)):
                assert (gt[i].hex() == derived["gt_one"]) == (st[i] == 0) and (gt[i] == bytes(384)) == (st[i] not in (0, 9)), (k, f, i)
            full = pc.full_gt(k, f)
            assert all(len(g) == 384 and g != bytes(384) for g in full) and set(pc.gt_of_failed(k, f)) == {i for i in range(len(st)) if st[i] not in (0, 9)}
    assert pc.outside_subgroup()[0] == bytes.fromhex(derived["g2_not_in_subgroup"])


def test_every_ordering_case_has_two_different_codes_and_reports_the_earlier():
    codes, table = pc.order_pair_codes(), pc.order_pairs()
    assert set(codes) == set(table) and len(codes) >= 40
    for name, (flags, first, second, both) in codes.items():
        assert flags == table[name]
        assert first not in (0, 9) and second not in (0, 9) and first != second and both == first, (name, flags, first, second, both)
    for k in pc.KS:
        mine = {n: v for n, v in codes.items() if n.startswith("k=%d: " % k)}
        # in both assignments of the codes 4 and 6 under no flag, and one with each flag
        assert {(a, b) for flags, a, b, _ in mine.values() if flags == 0} == {(4, 6), (6, 4)}
        assert {flags for flags, _, _, _ in mine.values()} == {0, 1, 2}
        for j in pc.placements(k):                             # G1 and G2 of the same pair
            assert mine["k=%d: order: G1 x >= q in pair %d, G2 off the twist in pair %d" % (k, j, j)][1:3] == (6, 4)
            assert mine["k=%d: order: G1 off the curve in pair %d, G2 x.im >= q in pair %d" % (k, j, j)][1:3] == (4, 6)
        if k > 1:                                              # G2 of an earlier pair against G1 of a later one; identity before and behind x >= q
            assert any(n.split(": order: ")[1].startswith("G2") and ", G1" in n for n in mine)
            assert "k=%d: order: identity G1 in pair 0, G1 x >= q in pair %d" % (k, k - 1) in mine
            assert "k=%d: order: G1 x >= q in pair 0, identity G1 in pair %d" % (k, k - 1) in mine
            assert mine["k=%d: order: G2 off the subgroup in pair 0, G1 x >= q in pair 1" % k][:3] == (1, 4, 6)


def test_tile_walks_the_set():
    for k in pc.KS:
        cs = pc.cases_of(k)
        ln = len(cs)
        g1, g2, st, gt, idx = pc.tiled(k, 2 * ln + 3, 1, shift=5)
        assert (g1, g2, list(idx)) == pc.tile(cs, 2 * ln + 3, 5)
        assert len(g1) == 64 * k * len(idx) and len(g2) == 128 * k * len(idx) and len(st) == len(idx) == 2 * ln + 3 and len(gt) == 384 * len(idx)
        assert set(idx) == set(range(ln))
        for i in (0, 1, ln - 6, ln - 5, 2 * ln + 2):
            j = (i + 5) % ln
            assert idx[i] == j and g1[64 * k * i:64 * k * (i + 1)] == cs[j].g1 and g2[128 * k * i:128 * k * (i + 1)] == cs[j].g2
            assert st[i] == pc.expected(k, 1)[0][j] and gt[384 * i:384 * i + 384] == pc.full_gt(k, 1)[j]
        assert pc.tile(cs, 0) == (b"", b"", [])
        assert pc.first_difference(k, idx, st, st) is None
        wrong = bytearray(st); wrong[7] ^= 1; wrong[20] ^= 1
        assert pc.first_difference(k, idx, bytes(wrong), st).startswith("item 7 of %d (%s)" % (len(idx), cs[idx[7]].name))
        wrong = bytearray(gt); wrong[384 * 9 + 383] ^= 1
        assert pc.first_difference(k, idx, bytes(wrong), gt, 384).startswith("item 9 of %d (%s): Gt differs; 1 items" % (len(idx), cs[idx[9]].name))


@pytest.mark.parametrize("flags", pc.FLAGS)
def test_host_build_of_the_one_lane_kernel_body_vs_oracle(flags):
    """hs_pairing gives the oracle's status on every case and the oracle's Gt wherever the status is 0 or 9; on a failed item it gives
    the product of the substituted item (include/bn254_hip.h), which the oracle computes from the substituted bytes"""
    for k in pc.KS:
        cs = pc.cases_of(k)
        want_st, want_gt, full = pc.expected(k, flags) + (pc.full_gt(k, flags),)
        got = [hs.pairing(x.g1, x.g2, k, flags) for x in cs]
        idx = list(range(len(cs)))
        got_st = bytes(st for st, _ in got)
        assert got_st == want_st, (k, pc.first_difference(k, idx, got_st, want_st))
        for i, (st, gt) in enumerate(got):
            if st in (0, 9):
                assert gt == want_gt[i], (k, cs[i].name)
            assert gt == full[i], (k, cs[i].name)


def _points(cs):
    out = []
    for j in range(cs.k):
        s1, p = gc.G1.decode(cs.g1[64 * j:64 * j + 64])
        s2, q = gc.G2.decode(cs.g2[128 * j:128 * j + 128])
        if s1 != m.OK or s2 != m.OK:
            return None
        out.append((p, q))
    return out


def test_big_integer_model_agrees_on_a_sample():
    """the C oracle's Gt against oracle/bn254_model.py (affine big-integer Miller loops, one plain power for the final exponentiation)
    on 57 cases, about 120 Miller loops of the model at a fifth of a second each: every case of one and of two pairs whose operands all
    decode and lie in the subgroup (status 0 or 9 under the subgroup check), every third such case of three and of four pairs, and the
    named ones below"""
    named = ["k=3: e(aP,Q) e(bP,Q) e(-(a+b)P,Q)", "k=3: cancelling pairs around an identity pair", "k=3: identity G1 in pair 2",
             "k=4: e(aP,Q) e(-aP,Q) e(bP',Q') e(P',-bQ')", "k=4: both identities in pair 3", "k=4: cancelling pairs around two identity pairs"]
    picked = []
    for k in pc.KS:
        good = [n for n, st in zip(pc.names(k), pc.expected(k, 1)[0]) if st in (0, 9)]
        picked += good if k <= 2 else good[::3] + [n for n in named if n.startswith("k=%d" % k) and n not in good[::3]]
    assert 50 <= len(picked) <= 60, len(picked)
    ones = 0
    for name in picked:
        k = int(name[2])
        i = pc.names(k).index(name)
        cs = pc.cases_of(k)[i]
        pairs = _points(cs)
        assert pairs is not None and all(q is None or m.g2_in_subgroup(q) for _, q in pairs), name
        gt = m.pairing_batch(pairs)
        st, want = pc.expected(k, 0)
        assert m.f12_to_bytes(gt) == want[i], name
        assert (gt == m.F12_ONE) == (st[i] == 0), name
        ones += st[i] == 0
    assert ones >= 12


def _decodable(k):
    """[(case, Gt)] of the cases of k whose every operand decodes under flags 0 (points off the subgroup included)"""
    st, gt = pc.expected(k, 0)
    return [(cs, gt[i]) for i, cs in enumerate(pc.cases_of(k)) if st[i] in (0, 9)]


def test_pair_layout_and_small_batch_bodies_on_the_cases_that_decode():
    """hp_pairing (the lane-pair Miller loop and the accumulator machine's exact program), hp_pairing_small_batch (the lane machine's
    schedule with the fixed pair skipped, C_FE_EXACT in the nonet schedule) on every decodable case of one pair; hp_pairing_product4
    (two two-pair Miller loops, their product, the final exponentiation) on every decodable case of four.  An identity operand is
    all-zero bytes there too."""
    L = hs.pair_lib()
    ran = 0
    for cs, want in _decodable(1):
        for fn in (L.hp_pairing, L.hp_pairing_small_batch):
            out = ctypes.create_string_buffer(384)
            fn(cs.g1, cs.g2, out)
            assert out.raw == want, (fn.__name__, cs.name)
        ran += 1
    assert ran >= 12
    ran = 0
    for cs, want in _decodable(4):
        out = ctypes.create_string_buffer(384)
        L.hp_pairing_product4(cs.g1, cs.g2, out)
        assert out.raw == want, cs.name
        ran += 1
    assert ran >= 25


def test_long_items_on_the_host_build(derived):
    """40 pairs, beyond the oracle's 16 per item: the expectation is one oracle pairing by bilinearity"""
    g1, g2, st, gt = pc.long_item(40, 7)
    assert (len(g1), len(g2), st) == (40 * 64, 40 * 128, 9) and hs.pairing(g1, g2, 40, 0) == (9, gt)
    h1, h2, st, one = pc.long_item(40, 7, one=True)
    assert (len(h1), len(h2), st) == (40 * 64, 40 * 128, 0) and one.hex() == derived["gt_one"] and hs.pairing(h1, h2, 40, 3) == (0, one)
    assert h1[:39 * 64] == g1[:39 * 64] and h2[:39 * 128] == g2[:39 * 128] and h1[39 * 64:] != g1[39 * 64:]
    # the helper's shortcut against the oracle itself where the oracle can follow: 16 pairs
    for one_ in (False, True):
        a1, a2, st, gt = pc.long_item(16, 3, one=one_)
        assert c.batch_pairing(a1, a2, 1, 16, 3) == (gt, bytes([st]))
    # dropping the last pair of either changes the product
    assert hs.pairing(g1[:39 * 64], g2[:39 * 128], 39, 0)[1] != gt and hs.pairing(h1[:39 * 64], h2[:39 * 128], 39, 0)[0] == 9


BOUNDS_DRIVER = r'''
import ctypes, sys
root = sys.argv[1]
sys.path.insert(0, root)
from tests import pairing_cases as pc
hs = ctypes.CDLL(root + "/tests/hostsim/libhostsim_bounds.so")
hs.hs_pairing.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_char_p, ctypes.c_int]
names = pc.names(4)
ran = 0
for name in ("k=4: cancelling pairs around two identity pairs", "k=4: identity G1 in pair 2", "k=4: identity G2 in pair 2", "k=4: both identities in pair 2",
             "k=4: G1 x >= q in pair 2"):
    i = names.index(name)
    cs = pc.cases_of(4)[i]
    for flags in pc.FLAGS:
        out = ctypes.create_string_buffer(384)
        st = hs.hs_pairing(cs.g1, cs.g2, 4, flags, out, 0)
        assert st == pc.expected(4, flags)[0][i] and out.raw == pc.full_gt(4, flags)[i], (name, flags, st)
        ran += 1
print("ok", ran)
'''


def test_bounds_hold_on_the_pairing_product_flow():
    """a flow of its own for the interval bookkeeping (tests/test_bounds.py): its "pairing" flow multiplies two Miller values of
    ordinary pairs.  Here: four-pair products with an identity G1, an identity G2 and both in the MIDDLE pair (a Miller value of one
    between ordinary ones), two identity pairs inside a product that is one, and the substituted generator of a failed decode, under
    every flags value; statuses and Gt are compared with the oracle's there too."""
    hs.build_all()
    p = subprocess.run([sys.executable, "-c", BOUNDS_DRIVER, ROOT], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.strip() == "ok 20", (p.stdout[-500:], p.stderr[-2000:])
