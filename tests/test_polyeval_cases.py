"""The bodies of the evaluation of polynomials with G2 coefficients (bn254_amd/csrc/bn254_polyeval.h over bn254_dealing.h, bn254_threshold.h
and bn254_fr.h), compiled for the host as a stand-alone program (tests/hostsim/hostsim_polyeval.cpp) and run on the case set of
tests/polyeval_cases.py against tests/polyeval_model.py — without a GPU.  Three builds of the one source: plain, with
-fsanitize=address,undefined (an executable of its own: nothing sanitised is loaded into this process), and under -DBN_TRACK_BOUNDS, where
the interval tracker aborts the program on a violated limb or value bound of the jac_* arithmetic.  The plain build runs every case of up to 65 coefficients at
every one of its points; the instrumented builds run every pattern at the lengths polyeval_cases.LIGHT_LENGTHS (up to 65 coefficients: chunks of
one and of two, a ragged last chunk, empty lanes) and at the first point of each case — 64 ladders of 256 steps per evaluation under the
tracker are slow.  Above 65 coefficients the plain build, too, takes the first point of each case (the random polynomial: all of its points)."""
import os
import subprocess

import pytest

from tests import polyeval_cases as PC
from tests import polyeval_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_polyeval.cpp")
R = PM.R
BUILDS = {"plain": ["-O2"], "san": ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
          "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("hpe")
    common = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    procs = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("hostsim_polyeval_%s" % name))
        procs[name] = (exe, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + common + ["-o", exe, SRC], stderr=subprocess.PIPE, text=True))
    for name, (exe, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: exe for name, (exe, _) in procs.items()}


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def run(exe, lines, tmp_path):
    """one command per line -> one answer per line; a sanitizer report or a tracker abort fails the run"""
    path = tmp_path / "commands.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=1800)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])
    got = p.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    return got


@pytest.fixture(scope="module")
def evaluations(c):
    """every (case, point) -> (command, expected answer of ONE layout, label, light), the model computed once for all three builds.  The lane
    walks alone (its own bounds), and on the short polynomials also as in a wave beside a polynomial 3 longer and a 32-bit x"""
    out = []
    for n, cs in PC.all_cases():
        body = " ".join(p.hex() for p in PM.coefficients(c, cs))
        for i, x in enumerate(cs["xs"]):
            if n > 65 and i > 0 and cs["name"] != "random":
                continue
            st, value = PM.expected(c, cs, x)
            want = "%d %s" % (st, value.hex())
            for more_len, more_bits in ((0, 0), (3, 32)) if n <= 17 and i == 0 else ((0, 0),):
                out.append(("eval %d %d %d %d %s" % (x, more_len, more_bits, n, body), want, "%d/%s/%d/%d" % (n, cs["name"], x, more_len),
                            PC.is_light(n, cs) and i == 0))
    return out


def test_model_cross_check(c):
    """the model against itself: the oracle's key derivation of sum a_k x^k against group arithmetic in Python integers, at every point"""
    checked = 0
    for n, cs in PC.all_cases():
        if 1 <= n <= PM.GROUP_MAX_COEFFS and not cs["faults"] and cs["points"] is None:
            for x in cs["xs"]:
                assert PM.cross_check(c, cs, x), (n, cs["name"], x)
                checked += 1
    assert checked >= 30
    assert PM.eval_scalar([5, 7, 11], 0) == 5 and PM.eval_scalar([], 3) == 0 and PM.powers(0, 3) == [1, 0, 0]
    assert not PM.M.g2_in_subgroup(PM.DM.g2_point(PM.off_subgroup_point(7)))


def test_case_set_is_the_one_the_header_names():
    names = {cs["name"] for _, cs in PC.all_cases()}
    assert {"random", "all_identity", "identity_top", "identity_bottom", "identity_middle", "equal_neighbours", "through_identity", "root_at_x",
            "chunk_root", "tree_equal", "tree_opposite", "fault_first", "fault_middle", "fault_last", "two_faults", "off_subgroup"} <= names
    assert {n for n, _ in PC.all_cases()} == set(PC.LENGTHS) and {PC.chunk_len(n) for n in PC.LENGTHS if n} == {1, 2, 3, 4}
    assert {x for _, cs in PC.all_cases() for x in cs["xs"]} == set(PC.POINTS)
    # the patterns are what they say: a root gives the identity's scalar, the equal / opposite pair meets in the tree
    for n, cs in PC.all_cases():
        if cs["name"] == "root_at_x":
            assert PM.eval_scalar(cs["a"], cs["xs"][0]) == 0, n
        if cs["name"] == "through_identity":                 # Horner's accumulator is the identity after every second coefficient from the top
            assert all(PM.eval_scalar(cs["a"][n - k:], cs["xs"][0]) == 0 for k in range(2, n + 1, 2)), n
        if cs["name"] in ("tree_equal", "tree_opposite"):
            L, part, x = PC.chunk_len(n), PC.tree_partner(n), cs["xs"][0]
            mine = PM.eval_scalar(cs["a"][:L], x)
            theirs = PM.eval_scalar(cs["a"][part * L:(part + 1) * L], x) * pow(x, part * L, R) % R
            assert mine == (theirs if cs["name"] == "tree_equal" else -theirs % R) and mine != 0, (n, cs["name"])
        if cs["name"] == "chunk_root":
            L = PC.chunk_len(n)
            assert PM.eval_scalar(cs["a"][L:2 * L], cs["xs"][0]) == 0 and PM.eval_scalar(cs["a"], cs["xs"][0]) != 0


@pytest.mark.parametrize("build", list(BUILDS))
def test_both_layouts_on_the_case_set(exes, evaluations, build, tmp_path):
    cases = [e for e in evaluations if build == "plain" or e[3]]
    got = run(exes[build], [cmd for cmd, _, _, _ in cases], tmp_path)
    wrong, differ = [], []
    for (_, want, label, _), g in zip(cases, got):
        words = g.split(" ")
        lane, wave = " ".join(words[:2]), " ".join(words[2:])
        if lane != wave:
            differ.append(label)
        if lane != want or wave != want:
            wrong.append(label)
    assert not differ, differ[:8]                            # the two layouts give identical bytes
    assert not wrong, wrong[:8]
    assert len({label.split("/")[1] for _, _, label, _ in cases}) >= 16


@pytest.mark.parametrize("build", list(BUILDS))
def test_spans_and_chunk_scalars(exes, build, tmp_path):
    off = [0, 3, 3, 10, 7, 12]                               # polynomial 3 is reversed; with 11 coefficients polynomial 4 runs past the end
    lines = ["span 5 12 %d %s" % (i, " ".join(map(str, off))) for i in (0, 1, 2, 3, 4, 5, 0xFFFFFFFF)]
    lines += ["span 5 11 4 %s" % " ".join(map(str, off)), "span 0 0 0 0"]
    want = ["0 0 3", "0 3 0", "0 3 7", "2 0 0", "0 7 5", "2 0 0", "2 0 0", "2 0 0", "2 0 0"]
    pows = [(x, e) for x in (0, 1, 2, 257, (1 << 32) - 1) for e in (0, 1, 2, 63, 64, 252, 12600, (1 << 32) - 1)]
    lines += ["pow %d %d" % xe for xe in pows]
    want += ["%064x" % pow(x, e, R) for x, e in pows]
    assert run(exes[build], lines, tmp_path) == want
