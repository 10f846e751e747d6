"""The case builder of the group-operation tests (tests/group_cases.py) checked on its own, CPU only: every named kind of case is
present (counts asserted, so a kind that goes missing fails here), the model and the C oracle agree on every expected value both
can compute, and no expected value can have come from the library under test."""
import ast
import os

import pytest

from oracle import bn254_model as m
from oracle import c_oracle as c
from tests import group_cases as gc

GROUPS = [gc.G1, gc.G2]


def test_the_builder_never_touches_the_library_under_test():
    tree = ast.parse(open(os.path.join(os.path.dirname(__file__), "group_cases.py")).read())
    mods = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            mods |= {a.name for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            mods |= {"%s.%s" % (node.module, a.name) for a in node.names}
    assert mods == {"functools", "hashlib", "random", "oracle.bn254_model", "oracle.c_oracle"}
    assert {it["src", r] for it in gc.g2_mul_cases()["items"] for r in (False, True)} == {"model", "c_oracle"}


@pytest.mark.parametrize("G", GROUPS, ids=lambda G: G.name)
def test_addition_matrix_layouts_and_oracle_agreement(G):
    batches = gc.add_batches(G.name)
    assert sorted({len(b) for b in batches}) == [1, 63, 64, 65, 200]
    items = [it for b in batches for it in b]
    count = lambda kind: sum(1 for it in items if it["kind"] == kind)     # noqa: E731
    for kind in gc.ADD_KINDS:
        assert count(kind) >= 8, kind                                     # n = 1, 63, 65, the all-exceptional wave (5+), the big batch
    assert count("ordinary") + count("ordinary, outside the subgroup") >= 1500
    assert G is gc.G2 or count("ordinary, outside the subgroup") == 0
    if G is gc.G2:
        assert count("ordinary, outside the subgroup") >= 100
        out = [it for it in items if it["kind"] == "ordinary, outside the subgroup"][0]
        assert not m.g2_in_subgroup(G.decode(out["a"])[1]) and not m.g2_in_subgroup(G.decode(out["b"])[1]) and out["status"] == 0
    # the statuses the issue names: a's code wins, a coordinate equal to q is not a member
    want_status = {"a>=q": 6, "b off curve": 4, "a>=q, b off curve": 6, "a off curve, b>=q": 4, "coordinate == q": 6}
    for it in items:
        if it["kind"] in want_status:
            assert it["status"] == want_status[it["kind"]] and it["want"] == G.zero, it["kind"]
        if it["kind"] in ("P+(-P)", "O+O"):
            assert it["want"] == G.zero and it["status"] == 0
        if it["kind"] == "P+P":
            assert it["a"] == it["b"] and it["want"] not in (G.zero, it["a"]) and it["status"] == 0
        if it["kind"] == "O+P":
            assert it["want"] == it["b"] != G.zero
        if it["kind"] == "P+O":
            assert it["want"] == it["a"] != G.zero
    assert len({it["status"] for it in items if it["kind"] == "x == 0, y != 0"}) == 1            # 0 if (0, sqrt b) exists, else 4
    # wave layouts: some wave with exactly one exceptional lane, one with only exceptional lanes, one with none
    profiles = [(len(b), gc.wave_profile(b, lambda it: gc.is_exceptional(G, it))) for b in batches]
    waves = [(n, w, k, min(64, n - 64 * w)) for n, prof in profiles for w, k in enumerate(prof)]
    assert sum(1 for n, w, k, lanes in waves if k == 0 and lanes == 64) >= 10
    assert sum(1 for n, w, k, lanes in waves if k == 64 and lanes == 64) >= 2
    assert sum(1 for n, w, k, lanes in waves if k == 1 and lanes == 63) == len(gc.ADD_KINDS)
    assert sum(1 for n, w, k, lanes in waves if k == 1 and lanes == 1 and n == 65) == len(gc.ADD_KINDS)
    assert dict(profiles)[200] == [0, 64, 1, 1]
    for it in items:
        assert gc.is_exceptional(G, it) == (not it["kind"].startswith("ordinary") and not (it["kind"] == "x == 0, y != 0" and it["status"] == 0))
    # the C oracle on the same bytes: same sum, or the same error
    for it in items:
        try:
            got = (G.c_add(it["a"], it["b"]), 0)
        except c.OracleError as e:
            got = (G.zero, e.code)
        assert got == (it["want"], it["status"]), it["kind"]


def test_g2_multiplication_cases():
    mc = gc.g2_mul_cases()
    items, G = mc["items"], gc.G2
    n = len(items)
    assert n % 64 != 0 and len(mc["points"]) == 128 * n and len(mc["scalars"]) == 32 * n
    for k in {it["k"] for it in items if it["set"] == "edge"}:
        assert {it["base"] for it in items if it["set"] == "edge" and it["k"] == k} == set(range(7))     # every base under every edge scalar
    assert {it["kind"] for it in items} == set(gc.MUL_BASE_KINDS)
    assert mc["bases"][0] == c.g2_generator() and mc["bases"][5] == bytes(128)
    for b in (1, 2):
        assert m.g2_in_subgroup(G.decode(mc["bases"][b])[1])
    for b in (3, 4):
        assert G.decode(mc["bases"][b])[0] == 0 and not m.g2_in_subgroup(G.decode(mc["bases"][b])[1])
    assert G.decode(mc["bases"][6])[0] == 4
    ks = {it["k"] for it in items if it["set"] == "edge"}
    R = m.R
    named = {0, 1, 2, 7, 8, 9, 15, 16, 17, int("8" * 64, 16), int("9" * 64, 16), int("7" * 64, 16), 1 << 128, 1 << 253, (1 << 256) - 1, (1 << 256) - 16,
             R - 2, R - 1, R, R + 1} | {mm * R for mm in range(2, 6)} | {mm * R - 2 * mm for mm in range(2, 6)}
    assert named <= ks
    hits = gc.ladder_hit_scalars()
    assert set(hits) <= ks
    assert sum(1 for h in hits.values() if h[0][1] == "doubling") >= 1 and sum(1 for h in hits.values() if h[0][1] == "cancellation") >= 1
    for mm in range(1, 6):          # the scalars the analysis of the ladder predicts, found again by the restated recoding
        assert gc.ladder_hits(mm * R - 2 * mm) == [(0, "doubling")] and gc.ladder_hits(mm * R) == [(0, "cancellation")]
    assert gc.ladder_hits(12345) == [] and gc.ladder_hits(R - 1) == []
    assert sum(1 for it in items if it["set"] == "random 256-bit") >= 150 and sum(1 for it in items if it["set"] == "random < r") >= 50
    for w in range(0, n, 64):
        assert len({it["base"] for it in items[w:w + 64]}) == 7                  # every wave mixes all the bases
    # reduce_scalar is observable: some (point outside the subgroup, k >= r) has two different answers; on the subgroup it never has
    assert mc["observable"] >= 1
    assert any(it["want", False] != it["want", True] for it in items if it["kind"] == "outside the subgroup" and it["set"] == "edge" and it["k"] == R + 1)
    for it in items:
        if it["kind"] in ("generator", "subgroup", "identity", "invalid") or it["k"] < R:
            assert it["want", False] == it["want", True]
        if it["kind"] in ("identity", "invalid"):
            assert it["want", False] == bytes(128) and it["status"] == (4 if it["kind"] == "invalid" else 0)
    # model and C oracle agree on every expected value (the invalid base: both refuse it with the same code)
    cache = {}
    for it in items:
        base = mc["bases"][it["base"]]
        for reduce in (False, True):
            k = it["k"] % R if reduce else it["k"]
            if it["status"] != 0:
                with pytest.raises(c.OracleError) as e:
                    c.g2_mul(base, gc.be(k))
                assert e.value.code == it["status"]
                continue
            if it["src", reduce] == "model":
                other = c.g2_mul(base, gc.be(k))
            else:
                if (it["base"], k) not in cache:
                    cache[it["base"], k] = G.enc(m.g2_mul(G.decode(base)[1], k))
                other = cache[it["base"], k]
            assert other == it["want", reduce], (it["kind"], hex(it["k"]), reduce)


@pytest.mark.parametrize("G", GROUPS, ids=lambda G: G.name)
def test_segmented_sum_cases(G):
    calls = gc.sum_calls(G.name)
    assert [cl.name for cl in calls] == ["ragged", "single long", "empty ends"]
    rag, one, ends = calls
    lens = [len(s) for s in rag.segments]
    assert len(lens) >= 130 and len(lens) % 64 != 0 and set(lens) == set(gc.SUM_LENGTHS)
    for w in (0, 64):
        assert {0, 1, 2, 3} <= set(lens[w:w + 64]) and max(lens[w:w + 64]) == 1000       # every full wave mixes empty, short and long
    notes = set(rag.notes.values())
    for text in ("doubling, neighbours mid-loop", "cancellation then O + P, neighbours mid-loop",
                 "cancellation then O + P, then a doubling, in the only lane still looping", "P, -P, Q", "P, P", "identity terms around a point",
                 "identity terms only", "identity terms mid-segment", "one invalid point in the middle", "two invalid points, codes 6 then 4",
                 "two invalid points, codes 4 then 6", "invalid points only", "invalid point first", "doubling at the last step, in the ragged wave"):
        assert text in notes, text
    # the planted steps are where they are said to be, and nowhere else
    assert rag.exceptional[10] == [(30, "doubling")] and min(lens[9], lens[11]) >= 63
    assert rag.exceptional[12] == [(31, "cancellation")]
    assert rag.exceptional[84] == [(500, "cancellation"), (700, "doubling")]
    assert all(n <= 65 for i, n in enumerate(lens[64:128]) if i != 20)                    # lane 84 loops alone from step 65 on
    assert rag.exceptional[35] == [(1, "cancellation")] and rag.want[35] == rag.segments[35][2]
    assert rag.exceptional[36] == [(1, "doubling")]
    assert sum(1 for ex in rag.exceptional if ex) == len(rag.planted) == 8
    assert rag.identity_terms[37] == 2 and rag.want[37] == rag.segments[37][1] and rag.identity_terms[38] == 3 and rag.want[38] == G.zero
    assert rag.identity_terms[90] == 2 and sum(rag.identity_terms) == 7
    faulty = {20: 4, 22: 6, 28: 4, 30: 4, 32: 6, 132: 6}
    assert {i: s for i, s in enumerate(rag.status) if s} == faulty
    for i in faulty:
        assert rag.want[i] == G.zero and rag.status[i + 1] == 0 and rag.want[i + 1] != G.zero and lens[i + 1] >= 1
    assert [G.decode(p)[0] for p in rag.segments[30]] == [4, 6, 4] and [G.decode(rag.segments[22][j])[0] for j in (5, 40)] == [6, 4]
    assert [G.decode(rag.segments[28][j])[0] for j in (60, 61)] == [4, 6]
    assert rag.want[134] == G.zero and rag.status[134] == 0
    assert [len(s) for s in one.segments] == [5000] and one.exceptional[0] == [(2500, "doubling")]
    elens = [len(s) for s in ends.segments]
    assert elens[:70] == [0] * 70 and elens[-70:] == [0] * 70 and elens[70:75] == [3, 64, 1, 2, 65] and ends.exceptional[74] == [(33, "doubling")]
    assert ends.seg_off[0] == ends.seg_off[70] == 0 and ends.seg_off[75] == ends.seg_off[-1] == 135
    # the C oracle folds every fault-free segment to the same point
    for call in calls:
        for seg, want, st in zip(call.segments, call.want, call.status):
            if st == 0:
                acc = G.zero
                for p in seg:
                    acc = G.c_add(acc, p)
                assert acc == want, call.name
        assert len(call.points) == G.size * call.seg_off[-1]


def test_fp12_cases():
    els = gc.fp12_elements()
    kinds = [k for k, _ in els]
    assert {k: kinds.count(k) for k in set(kinds)} == {"zero": 1, "one": 1, "basis 1": 12, "basis q-1": 12, "subfield Fq": 1, "subfield Fq2": 1,
                                                      "subfield Fq6": 1, "sparse line": 3, "miller": 4, "gt": 4, "random": 40}
    for kind, e in els:
        flat = [x for f2 in e for x in f2]
        if kind.startswith("basis"):
            assert sorted(flat)[:11] == [0] * 11 and max(flat) == (1 if kind == "basis 1" else m.Q - 1)
        if kind == "sparse line":
            assert sum(1 for f2 in e if f2 != (0, 0)) == 3
        if kind == "gt":
            assert m.f12_pow(list(e), m.R) == m.F12_ONE
    assert len({tuple(e) for k, e in els if k.startswith("basis")}) == 24
    # bytes <-> model coefficients: the inverse of f12_to_bytes, and the tower order it undoes
    e = [(2 * i + 1, 2 * i + 2) for i in range(6)]
    assert gc.f12_from_bytes(m.f12_to_bytes(e)) == e
    assert m.f12_to_bytes(e)[64:96] == (5).to_bytes(32, "big")              # the second Fq2 of the tower is the coefficient of w^2
    cases = gc.fp12_cases()
    per_op = {op: [cs for cs in cases if cs["op"] == op] for op in gc.FP12_OPS}
    assert len(per_op["mul"]) >= 90 and all(cs["a"] != cs["b"] for cs in per_op["mul"])
    assert {"0 * x", "x * 0", "1 * x", "x * 1", "sparse * dense", "dense * sparse", "basis * basis", "distinct random"} <= {cs["kind"] for cs in per_op["mul"]}
    assert len(per_op["sqr"]) == len(per_op["conj"]) == len(els)
    for p in ("frob1", "frob2", "frob3"):
        assert sum(1 for cs in per_op[p] if cs["kind"].startswith("basis")) == 24 and sum(1 for cs in per_op[p] if cs["kind"] == "random") >= 6
        assert any(cs["want"] != cs["a"] for cs in per_op[p])
    assert 20 <= len(per_op["inv"]) <= 48 and all(cs["a"] != bytes(384) for cs in per_op["inv"])
    assert len(per_op["cyclotomic_sqr"]) == 4
    assert any(cs["want"] != cs["a"] for cs in per_op["conj"] if cs["kind"] == "random")
    # a Gt element: conjugation is inversion there — the model's conj and its power agree (ties the conj convention to the arithmetic)
    g = [cs for cs in per_op["conj"] if cs["kind"] == "gt"][0]
    assert m.f12_mul(gc.f12_from_bytes(g["a"]), gc.f12_from_bytes(g["want"])) == m.F12_ONE
