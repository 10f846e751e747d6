"""The bodies of the G2 weighted sum and of the dealing check (bn254_amd/csrc/bn254_dealing.h over bn254_threshold.h and bn254_fr.h), compiled
for the host as a stand-alone program (tests/hostsim/hostsim_dealing.cpp) and run on the case set of tests/dealing_cases.py against
tests/dealing_model.py — without a GPU.  Three builds of the one source: plain, with -fsanitize=address,undefined (an executable of its own:
nothing sanitised is loaded into this process), and under -DBN_TRACK_BOUNDS, where the interval tracker aborts the program on a violated limb
or value bound of the jac_* arithmetic the G2Jac sums use.  The instrumented builds run the whole case set on the shapes up to 33 keys and
the honest, degree-t and cancelling-pair cases under one seed on the larger ones (a 256-step G2 ladder per term under the tracker is slow)."""
import os
import random
import subprocess

import pytest

from tests import dealing_cases as DC
from tests import dealing_model as DM
from tests import threshold_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_dealing.cpp")
R = DC.R
BUILDS = {"plain": ["-O2"], "san": ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
          "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("hdl")
    common = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    procs = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("hostsim_dealing_%s" % name))
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


def h32(v):
    return "%064x" % v


def key_of(c, secret):
    return c.public_key_g2(secret.to_bytes(32, "big")) if secret else bytes(128)


def coefficient_shapes():
    shapes = list(DC.SHAPES) + [(n, 1) for n, _ in DC.SHAPES] + [(n, n) for n, _ in DC.SHAPES] + DC.random_shapes(12, 300, 41) + [(300, 299), (300, 1), (257, 129)]
    return sorted(set(shapes))


@pytest.fixture(scope="module")
def coefficient_model():
    """(n, t, seed) -> the model's coefficients, computed once for all three builds"""
    seed = DC.SEEDS[1]
    return {(n, t): DM.coefficients(n, t, seed) for n, t in coefficient_shapes()}


@pytest.mark.parametrize("build", list(BUILDS))
def test_coefficients(exes, coefficient_model, build, tmp_path):
    seed = DC.SEEDS[1]
    shapes = list(coefficient_model)
    got = run(exes[build], ["coef %d %d %s" % (n, t, seed.hex()) for n, t in shapes], tmp_path)
    rnd = random.Random(9)
    for (n, t), line in zip(shapes, got):
        words = [int(w, 16) for w in line.split(" ")]
        cs, lam = words[:n], words[n:]
        assert len(lam) == t and all(v < R for v in words)
        assert cs == coefficient_model[(n, t)], (n, t)
        assert lam == TM.lagrange_at_zero(list(range(1, t + 1))), (n, t)
        if n <= 33:
            assert cs == DM.coefficients_by_definition(n, t, seed), (n, t)
        assert cs[t:] == [DM.rho(seed, j) for j in range(t, n)]
        # what the coefficients are for: they annihilate every polynomial of degree below t, and not one of degree t
        for degree in sorted({0, t - 1, rnd.randrange(t)}):
            f = DC.poly(rnd, degree)
            assert sum(cj * DM.evaluate(f, j + 1) for j, cj in enumerate(cs)) % R == 0, (n, t, degree)
        if n > t:
            f = DC.poly(rnd, t)
            assert sum(cj * DM.evaluate(f, j + 1) for j, cj in enumerate(cs)) % R != 0, (n, t)
    # under another seed the weights change and the property holds all the same
    other = run(exes[build], ["coef 5 3 %s" % DC.SEEDS[2].hex()], tmp_path)[0].split(" ")
    assert [int(w, 16) for w in other[:5]] == DM.coefficients(5, 3, DC.SEEDS[2]) != coefficient_model[(5, 3)]


def msm_cases(c):
    """every segment length x variant -> (command, expected answer, label).  The points are multiples a_s of the generator, so the expected
    sum is (sum k_s a_s) * G2::one(): one multiplication by the C oracle; on the short segments also by group arithmetic in Python integers"""
    rnd = random.Random(78)
    gen = c.g2_generator()
    out = []
    for m in DC.SEGMENT_LENGTHS:
        for variant in ("plain", "edge_scalars", "zero_and_identity", "bad_first", "bad_middle", "bad_last"):
            if m == 0 and variant != "plain":
                continue
            a = [rnd.randrange(1, R) for _ in range(m)]
            ks = [rnd.randrange(R) for _ in range(m)]
            bad = None
            if variant == "edge_scalars":
                ks = [DC.EDGE_SCALARS[i % 5] if i % 2 == 0 or m < 6 else k for i, k in enumerate(ks)]
            elif variant == "zero_and_identity":
                ks = [0 if i % 3 == 0 else k for i, k in enumerate(ks)]
                a = [0 if i % 3 == 1 else v for i, v in enumerate(a)]
            pts = [key_of(c, v) for v in a]
            if variant.startswith("bad"):
                bad = {"bad_first": 0, "bad_middle": m // 2, "bad_last": m - 1}[variant]
                pts[bad] = DC.plant(pts[bad], "curve")
                if m > 2 and variant == "bad_first":                   # a second, different fault behind it: the first one wins
                    pts[m - 1] = DC.plant(pts[m - 1], "big")
            body = " ".join("%s %s" % (p.hex(), h32(k)) for p, k in zip(pts, ks))
            for reduce in ((0, 1) if variant == "edge_scalars" else (0,)):
                if bad is not None:
                    one = "4 " + "00" * 128
                else:
                    total = sum(k * v for k, v in zip(ks, a)) % R
                    want = key_of(c, total)
                    if m <= 2:
                        assert DM.g2_weighted_sum(pts, [k % R for k in ks]) == want
                    one = "0 " + want.hex()
                out.append(("msm %d %d %s" % (reduce, m, body), one + " " + one, "%d/%s/%d" % (m, variant, reduce)))
    return out


@pytest.fixture(scope="module")
def msm(c):
    return msm_cases(c)


@pytest.mark.parametrize("build", list(BUILDS))
def test_weighted_sum_both_layouts(exes, msm, build, tmp_path):
    got = run(exes[build], [cmd for cmd, _, _ in msm], tmp_path)
    wrong = [label for (_, want, label), g in zip(msm, got) if g != want]
    assert not wrong, wrong[:8]


def check_cases(c, full):
    """the case set as `check` commands -> (command, expected answer, label, passes).  full: every case under every seed; else the whole set on
    the shapes up to 33 keys and three cases under one seed on the larger ones"""
    out = []
    for n, t in DC.SHAPES:
        for cs in DC.cases_for(n, t):
            small = n <= 33
            if not full and not small and cs["name"] not in ("honest", "degree_t", "cancelling_pair"):
                continue
            keys = [key_of(c, s) for s in cs["secrets"]]
            status = [0] * n
            for at, kind in cs["faults"].items():
                keys[at] = DC.plant(keys[at], kind)
                status[at] = DC.FAULT_STATUS[kind]
            if cs["pop_fail"] is not None:
                status[cs["pop_fail"]] = 9
            body = " ".join("%s %d" % (k.hex(), s) for k, s in zip(keys, status))
            for seed in (DC.SEEDS if full or small else DC.SEEDS[:1]):
                st, bad, k_scalar = DM.check_scalars(cs["secrets"], status, cs["t"], seed)
                pk = key_of(c, k_scalar) if st == 0 else bytes(128)
                if n <= 5 and not cs["faults"]:
                    assert DM.check(keys, status, cs["t"], seed) == (st, bad, pk), (n, t, cs["name"])
                if cs["expect"] == "pass":
                    assert st == 0 and bad == DM.NO_KEY
                elif cs["expect"] == "fail":
                    assert st == 9 and bad == DM.NO_KEY, (n, t, cs["name"])
                else:
                    assert (st, bad) == (cs["expect"][2] or 9, cs["expect"][1])
                want = "%d %d %s" % (st, bad, pk.hex())
                for layout in ((0, 1) if n <= 5 else (1,)):
                    out.append(("check %d %d %s %d %s" % (layout, cs["t"], seed.hex(), n, body), want, "%d/%d/%s/%d" % (n, t, cs["name"], layout),
                                cs["expect"] == "pass"))
    return out


@pytest.fixture(scope="module")
def checks(c):
    return {True: check_cases(c, True), False: check_cases(c, False)}


@pytest.mark.parametrize("build", list(BUILDS))
def test_check_dealing_case_set(exes, checks, build, tmp_path):
    cases = checks[build == "plain"]
    got = run(exes[build], [cmd for cmd, _, _, _ in cases], tmp_path)
    wrong = [label for (_, want, label, _), g in zip(cases, got) if g != want]
    assert not wrong, wrong[:8]
    # a passing case gives the same bytes under every seed; a failing one reads 9 (or its key's status) under each, with a zeroed key
    by_label = {}
    for (_, _, label, passes), g in zip(cases, got):
        by_label.setdefault((label, passes), set()).add(g)
    for (label, passes), answers in by_label.items():
        assert len(answers) == 1, label
        st, _, pk = next(iter(answers)).split(" ")
        assert (st == "0") == passes and (passes or pk == "00" * 128), label
    names = {label.split("/")[2] for label, _ in by_label}
    assert {"honest", "degree_t", "cancelling_pair"} <= names
    if build == "plain":
        assert {"degree_t_minus_2", "replaced_high", "replaced_low", "root_at_3", "zero_polynomial", "threshold_1_equal_keys",
                "fault_lowest", "fault_higher", "pop_failed", "threshold_n_plus_1"} <= names
