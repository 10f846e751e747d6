"""The bodies of the vector combine and of the reshare (bn254_amd/csrc/bn254_reshare.h over bn254_polyeval.h, bn254_dealing.h, bn254_threshold.h
and bn254_fr.h), compiled for the host as a stand-alone program (tests/hostsim/hostsim_reshare.cpp) and run on the case sets of
tests/reshare_cases.py against tests/reshare_model.py — without a GPU.  Three builds of the one source: plain, with
-fsanitize=address,undefined (an executable of its own: nothing sanitised is loaded into this process), and under -DBN_TRACK_BOUNDS, where
the interval tracker aborts the program on a violated limb or value bound of the jac_* arithmetic.  The plain build runs every case (at the
committee of 70 a selection: 2 209 ladders a case); the instrumented builds run every pattern at the shapes reshare_cases.VC_LIGHT (up to 65
vectors) and the committees reshare_cases.RS_LIGHT."""
import os
import subprocess

import pytest

from tests import reshare_cases as RC
from tests import reshare_model as RM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_reshare.cpp")
R = RM.R
BUILDS = {"plain": ["-O2"], "san": ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
          "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}
LARGE_SELECTION = {"honest_all", "honest_spread", "index_out_of_range", "refused_key", "too_few_qualified"}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("hrs")
    common = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    procs = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("hostsim_reshare_%s" % name))
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


def columns(expected):
    return " ".join("%d %s" % (st, v.hex()) for st, v in expected)


def vc_command(c, cs):
    pts = RM.vc_points(c, cs)
    return "vc %d %d %d %s %s" % (cs["reduce"], cs["d"], cs["len"], " ".join("%064x" % s for s in cs["scalars"]),
                                  " ".join(p.hex() for row in pts for p in row))


def rs_command(c, cs, bm_words):
    keys, key_st = RM.registered_keys(c, cs)
    vecs = RM.dealer_vectors(c, cs)
    return "rs %d %d %d %d %d %s %s %s" % (len(keys), cs["threshold"], cs["t_new"], len(vecs), bm_words, " ".join("%d %s" % (s, k.hex()) for s, k in zip(key_st, keys)),
                                           " ".join(str(k) for k, _ in cs["dealers"]), " ".join(p.hex() for row in vecs for p in row))


def rs_answer(c, cs, bm_words):
    """what the program must print: the head, and the commitments in both layouts of the sums"""
    status, dealer_st, used, taken, lam, scalars = RM.reshare_expected(cs)
    head = [status, len([s for s in dealer_st if s == 0])] + dealer_st + RM.bits_of(used, bm_words)
    words = [str(v) for v in head]
    if status == 0:
        words += [str(i) for i in taken] + ["%064x" % v for v in lam]
        cols = columns([(0, RM.key_of(c, v)) for v in scalars])
    else:
        cols = columns([(0, RM.IDENTITY)] * cs["t_new"])
    return " ".join(words + [cols, cols])


@pytest.fixture(scope="module")
def vc_runs(c):
    """(command, expected answer, label, light), the model computed once for all three builds"""
    out = []
    for shape, cs in RC.all_vc_cases():
        cols = columns(RM.vc_expected(c, cs))
        out.append((vc_command(c, cs), "vc %s %s" % (cols, cols), "%dx%d/%s" % (shape + (cs["name"],)), shape in RC.VC_LIGHT))
    out.append(("vc 0 0 3", "vc " + " ".join([columns([(0, RM.IDENTITY)] * 3)] * 2), "0x3/no_vectors", True))     # d = 0: every sum is empty
    return out


@pytest.fixture(scope="module")
def rs_runs(c):
    out = []
    for (old, new), cs in RC.all_rs_cases():
        if old[0] > 7 and cs["name"] not in LARGE_SELECTION:
            continue
        n = len(cs["secrets"])
        bm_words = (n + 31) // 32 + (1 if cs["name"] == "honest_all" else 0)          # a row wider than the key set: the words behind stay zero
        out.append((rs_command(c, cs, bm_words), rs_answer(c, cs, bm_words), "%dof%d/%s" % (old[1], old[0], cs["name"]), (old, new) in RC.RS_LIGHT))
    return out


def test_model_cross_check(c):
    """the model against itself: the oracle's key derivation of a scalar sum against group arithmetic in Python integers; the textbook
    coefficients interpolate; a reshare of honest sub-dealings keeps f(0) and gives a polynomial of degree t' - 1 whose shares combine"""
    a = [[5, 7], [11, R - 3], [R - 1, 2]]
    assert RM.cross_check(c, a, [3, R - 2, 9]) and RM.cross_check(c, a[:1], [R - 1])
    f, secrets = RC.old_committee(7, 5)
    for keys in ([0, 1, 2, 3, 4], [2, 3, 4, 5, 6], [0, 2, 3, 5, 6]):
        lam = RM.lagrange_at_zero(keys)
        assert sum(l * secrets[k] for l, k in zip(lam, keys)) % R == f[0]
        new = RM.combine_scalars([RC.sub_dealing(secrets[k], 4, k) for k in keys], lam)
        assert new[0] == f[0] and len(new) == 4
        # new member j's share: the combination of the sub-shares it received is the new polynomial at j + 1
        for j in range(6):
            assert sum(l * RM.evaluate(RC.sub_dealing(secrets[k], 4, k), j + 1) for l, k in zip(lam, keys)) % R == RM.evaluate(new, j + 1)
    assert not RM.M.g2_in_subgroup(RM.DM.g2_point(RM.PM.off_subgroup_point(7)))


def test_case_sets_are_the_ones_the_header_names():
    names = {cs["name"] for _, cs in RC.all_vc_cases()}
    assert {"random", "edge_scalars_taken", "edge_scalars_reduced", "identity_points", "through_identity", "equal_products", "fault_first", "fault_middle",
            "fault_last", "two_faults_one_column", "off_subgroup"} <= names
    assert {shape for shape, _ in RC.all_vc_cases()} == set(RC.VC_SHAPES)
    for _, cs in RC.all_vc_cases():
        if cs["name"] in ("through_identity", "equal_products"):
            prod = [s * row[0] % R for s, row in zip(cs["scalars"], cs["a"])]
            assert all(p == prod[0] for p in prod) if cs["name"] == "equal_products" else all((prod[i] + prod[i + 1]) % R == 0 for i in range(len(prod) - 1))
    names = {cs["name"] for _, cs in RC.all_rs_cases()}
    assert {"honest_all", "honest_exactly_t_high", "honest_spread", "threshold_above_d", "threshold_above_n", "index_out_of_range", "refused_key", "pop_failed",
            "fault_commitment_0", "fault_commitment_middle", "fault_commitment_last", "two_decode_faults", "d0_other_key", "d0_negated_key", "d0_identity",
            "key_status_before_decode", "decode_before_d0", "identity_key_qualifies", "too_few_qualified"} <= names
    # what the cases say they are: a disqualified low index moves S up; too few leaves Q in the row; the honest ones keep f(0)
    for (old, new), cs in RC.all_rs_cases():
        status, dealer_st, used, taken, lam, scalars = RM.reshare_expected(cs)
        if cs["name"].startswith("honest"):
            assert status == 0 and scalars[0] == RC.old_committee(*old)[0][0] and len(scalars) == new[1], cs["name"]
        if cs["name"] in ("refused_key", "pop_failed", "fault_commitment_0", "d0_other_key", "d0_negated_key", "d0_identity"):
            assert status == 0 and dealer_st[0] != 0 and used == list(range(1, old[1] + 1)) and scalars[0] == RC.old_committee(*old)[0][0]
        if cs["name"] in ("too_few_qualified", "threshold_above_d", "threshold_above_n"):
            assert status == 9 and len(used) < cs["threshold"] and scalars is None


@pytest.mark.parametrize("build", list(BUILDS))
def test_vector_combine_on_the_case_set(exes, vc_runs, build, tmp_path):
    cases = [e for e in vc_runs if build == "plain" or e[3]]
    got = run(exes[build], [cmd for cmd, _, _, _ in cases], tmp_path)
    wrong = [label for (_, want, label, _), g in zip(cases, got) if g != want]
    assert not wrong, wrong[:8]
    assert len({label.split("/")[1] for _, _, label, _ in cases}) >= 12


@pytest.mark.parametrize("build", list(BUILDS))
def test_reshare_on_the_case_set(exes, rs_runs, build, tmp_path):
    cases = [e for e in rs_runs if build == "plain" or e[3]]
    got = run(exes[build], [cmd for cmd, _, _, _ in cases], tmp_path)
    wrong = [label for (_, want, label, _), g in zip(cases, got) if g != want]
    assert not wrong, wrong[:8]
    assert len({label.split("/")[1] for _, _, label, _ in cases}) >= 19
