"""Fr, the Lagrange coefficients and the rank / select / coefficient / term / sum bodies of the threshold call and the scalar-weighted sum
(bn254_amd/csrc/bn254_fr.h, bn254_threshold.h), compiled for the host as a stand-alone program (tests/hostsim/hostsim_threshold.cpp) and run
on the case set of tests/threshold_cases.py against tests/threshold_model.py — without a GPU.  Three builds of the one source: plain, with
-fsanitize=address,undefined (an executable of its own: nothing sanitised is loaded into this process), and under -DBN_TRACK_BOUNDS, where
the interval tracker aborts the program on a violated limb or value bound of the jac_* arithmetic the sums use."""
import os
import random
import subprocess

import pytest

from tests import threshold_cases as TC
from tests import threshold_model as TM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_threshold.cpp")
R = TC.R
BUILDS = {"plain": ["-O2"], "san": ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
          "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("hth")
    common = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    procs = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("hostsim_threshold_%s" % name))
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
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])
    got = p.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    return got


def h32(v):
    return "%064x" % v


def fr_commands():
    """(command, expected hex) for every operation on the case set and 200 random operands each"""
    out = []
    pairs = TC.fr_pairs() + TC.fr_random(200, 11)
    singles = TC.FR_OPERANDS + TC.FR_INVERSES + [a for a, _ in TC.fr_random(200, 12)]
    for op in (0, 1, 2):
        out += [("fr %d %s %s" % (op, h32(a), h32(b)), h32(TM.fr_op(op, a, b))) for a, b in pairs]
    for op in (3, 4, 5):
        out += [("fr %d %s %s" % (op, h32(a), h32(0)), h32(TM.fr_op(op, a))) for a in singles]
    out += [("fr 6 %s %s" % (h32(a), h32(0)), h32(TM.fr_load_u32(a))) for a in singles + TC.FR_U32_LOADS]
    return out


@pytest.mark.parametrize("build", list(BUILDS))
def test_fr_and_lagrange(exes, build, tmp_path):
    cmds = fr_commands()
    for xs in TC.lagrange_sets():
        cmds.append(("lag %d %s" % (len(xs), " ".join(str(x) for x in xs)), " ".join(h32(v) for v in TM.lagrange_at_zero(xs))))
    rnd = random.Random(5)
    for _ in range(60):                                                 # the t lowest bits of a three-word row, t across the word boundaries
        row = [rnd.randrange(1 << 32) & rnd.randrange(1 << 32) for _ in range(3)]
        bits = [j for j in range(96) if (row[j // 32] >> (j % 32)) & 1]
        for t in (1, 2, 31, 32, 33, len(bits) - 1, len(bits), len(bits) + 1, 96, rnd.randrange(1, 97)):
            if t < 1:
                continue
            kept = [0, 0, 0]
            for j in bits[:t]:
                kept[j // 32] |= 1 << (j % 32)
            cmds.append(("trim 3 %d %s" % (t, " ".join("%x" % w for w in row)), " ".join("%x" % w for w in kept)))
    got = run(exes[build], [cmd for cmd, _ in cmds], tmp_path)
    wrong = [(cmd[:40], g[:20], w[:20]) for (cmd, w), g in zip(cmds, got) if g != w]
    assert not wrong, wrong[:5]
    # the identities the case set is built around
    assert TM.fr_op(0, *TC.FR_PRODUCT_PAIRS[2]) == 1 and TM.fr_op(0, *TC.FR_PRODUCT_PAIRS[6]) == R - 1 and TM.fr_op(0, *TC.FR_PRODUCT_PAIRS[1]) == 0
    assert TM.lagrange_at_zero([7]) == [1] and sum(TM.lagrange_at_zero(list(range(1, 66)))) % R == 1


def plant(c, base, secrets, shape, n_keys):
    """one tuple of the case set as multiples of one base: -> (shares, keys, statuses)"""
    shares, keys, status = [], [], []
    for key, kind in shape:
        if kind == "again":
            shares.append(shares[-1]); keys.append(keys[-1]); status.append(status[-1])
            continue
        sk = secrets[key]
        sg = c.g1_mul(base, sk.to_bytes(32, "big")) if sk else bytes(64)
        if kind == "wrong":
            sg = c.g1_add(sg, base)
        elif kind == "curve":
            sg = bytearray(sg); sg[40] ^= 4; sg = bytes(sg)
        elif kind == "big":
            sg = b"\xff" + sg[1:]
        elif kind == "oob":
            key = n_keys + 3
        shares.append(sg); keys.append(key); status.append(TC.KIND_STATUS[kind])
    return shares, keys, status


def comb_cases(c):
    """every key set and tuple shape of the case set -> (command per layout, expected answer, a label)"""
    out = []
    for name, n_keys, dealt_t, secret in TC.KEY_SETS:
        t = TC.threshold_of(name, dealt_t)
        secrets, f0 = TC.secrets_of(name, n_keys, dealt_t, secret)
        st_h, base, _ = c.hash_to_g1(("threshold/host/" + name).encode())
        assert st_h == 0
        bm_words = (n_keys + 31) // 32
        for shape_name, shape in TC.shapes_for(name, n_keys, t):
            shares, keys, status = plant(c, base, secrets, shape, n_keys)
            st, count, row, chosen = TM.select(keys, status, [len(keys)], [0], bm_words, t)[0]
            if st:
                sig = bytes(64)
            elif f0 is not None:                                       # dealt keys: expectation 2, f(0) times the base
                sig = TM.weighted_sum([base], [f0])
                if n_keys <= 9:                                        # ... and expectation 1 where it is cheap
                    assert TM.group_signature(shares, chosen) == sig, (name, shape_name)
            else:
                sig = TM.group_signature(shares, chosen)
            claim = row if st == 0 else [0] * bm_words                 # every kept key is claimed by exactly one share
            want = " ".join([str(st), str(count)] + ["%x" % w for w in row] + ["%x" % w for w in claim] + [sig.hex()])
            body = " ".join("%s %d %d" % (s.hex(), k, x) for s, k, x in zip(shares, keys, status))
            for layout in ((0, 1) if n_keys <= 9 else (1,)):
                out.append(("comb %d %d %d %d %s" % (layout, bm_words, t, len(keys), body), want, "%s/%s/%d" % (name, shape_name, layout)))
    return out


@pytest.fixture(scope="module")
def comb(c):
    return comb_cases(c)


@pytest.mark.parametrize("build", list(BUILDS))
def test_rank_select_coefficients_and_sum(exes, comb, build, tmp_path):
    got = run(exes[build], [cmd for cmd, _, _ in comb], tmp_path)
    wrong = [label for (_, want, label), g in zip(comb, got) if g != want]
    assert not wrong, wrong[:8]
    by = {label: want.split(" ") for _, want, label in comb}
    assert by["dealt9_t5/t_minus_1/0"][:2] == ["9", "4"] and by["dealt9_t5/t_minus_1/0"][-1] == "00" * 64
    assert by["dealt9_t5/more_than_t/1"][:3] == ["0", "9", "1f"] and by["dealt9_t5/low_wrong/0"][:3] == ["0", "5", "3d"]
    assert by["dealt9_t5/low_oob_short/0"][:3] == ["9", "4", "1d"] and by["dealt9_t5/empty/0"][:3] == ["9", "0", "0"]
    assert by["dealt9_t5/exactly_t/0"][-1] == by["dealt9_t5/more_than_t/0"][-1] == by["dealt9_t5/upper_keys/1"][-1] == by["dealt9_t5/descending/0"][-1]
    assert by["zero9_t5/exactly_t/0"][-1] == "00" * 64 and by["zero9_t5/exactly_t/0"][0] == "0"
    assert by["dealt70_t63/everybody/1"][2:5] == ["ffffffff", "7fffffff", "0"] and by["dealt70_t65/everybody/1"][2:5] == ["ffffffff", "ffffffff", "1"]
    assert by["dealt70_t64/t_minus_1/1"][:2] == ["9", "63"]


def msm_cases(c):
    rnd = random.Random(77)
    base = c.g1_generator()
    out = []
    for m in (0, 1, 3, 17, 65):
        for variant in ("plain", "big_scalars", "zero_and_identity", "bad_first", "bad_middle", "bad_last"):
            if m == 0 and variant != "plain":
                continue
            pts = [c.g1_mul(base, rnd.randrange(1, R).to_bytes(32, "big")) for _ in range(m)]
            ks = [rnd.randrange(R) for _ in range(m)]
            bad = None
            if variant == "big_scalars":
                ks = [R + k % 1000 if i % 2 else (1 << 256) - 1 - k % 1000 for i, k in enumerate(ks)]
            elif variant == "zero_and_identity":
                ks = [0 if i % 3 == 0 else k for i, k in enumerate(ks)]
                pts = [bytes(64) if i % 3 == 1 else p for i, p in enumerate(pts)]
            elif variant.startswith("bad"):
                bad = {"bad_first": 0, "bad_middle": m // 2, "bad_last": m - 1}[variant]
                flipped = bytearray(pts[bad]); flipped[40] ^= 4
                pts[bad] = bytes(flipped)
                if m > 2 and variant == "bad_first":                   # a second, different fault behind it: the first one wins
                    pts[m - 1] = b"\xff" + pts[m - 1][1:]
            want = "4 " + "00" * 64 if bad is not None else "0 " + TM.weighted_sum(pts, [k % R for k in ks]).hex()
            body = " ".join("%s %s" % (p.hex(), h32(k)) for p, k in zip(pts, ks))
            for layout in (0, 1):
                for reduce in ((0, 1) if variant == "big_scalars" else (0,)):
                    out.append(("msm %d %d %d %s" % (layout, reduce, m, body), want, "%d/%s/%d/%d" % (m, variant, layout, reduce)))
    return out


@pytest.fixture(scope="module")
def msm(c):
    return msm_cases(c)


@pytest.mark.parametrize("build", list(BUILDS))
def test_weighted_sum_both_layouts(exes, msm, build, tmp_path):
    got = run(exes[build], [cmd for cmd, _, _ in msm], tmp_path)
    wrong = [label for (_, want, label), g in zip(msm, got) if g != want]
    assert not wrong, wrong[:8]
