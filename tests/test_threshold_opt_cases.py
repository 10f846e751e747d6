"""The bookkeeping of the optimistic threshold call (bn254_amd/csrc/bn254_threshold.h: candidate row and duplicate byte, the optimistic
settle, the gates of both interpolations, the second claim pass and settle), compiled for the host as a stand-alone program
(tests/hostsim/hostsim_threshold_opt.cpp) and held to tests/threshold_opt_model.py — without a GPU.  Three builds of the one source: plain,
under -DBN_TRACK_BOUNDS, and with -fsanitize=address,undefined as an executable of its own (nothing sanitised is loaded into this
process).  Cases: rows of 1 and 3 words; thresholds 1, 5, 63, 64, 65 (the cut on both sides of a word boundary); a duplicate in the first
and in the last position; |C| = t - 1, t, t + 1; every verdict; what the exact verify leaves of the candidates (all, t, t - 1, none)."""
import os
import random
import subprocess

import pytest

from tests import threshold_opt_model as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_threshold_opt.cpp")
BUILDS = {"plain": ["-O2"], "san": ["-O1", "-g1", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
          "bounds": ["-O1", "-DBN_TRACK_BOUNDS"]}


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    out = tmp_path_factory.mktemp("htho")
    common = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
    procs = {}
    for name, flags in BUILDS.items():
        exe = str(out / ("hostsim_threshold_opt_%s" % name))
        procs[name] = (exe, subprocess.Popen([os.environ.get("CXX", "g++")] + flags + common + ["-o", exe, SRC], stderr=subprocess.PIPE, text=True))
    for name, (exe, p) in procs.items():
        _, err = p.communicate(timeout=900)
        assert p.returncode == 0, err[-3000:]
    return {name: exe for name, (exe, _) in procs.items()}


def run(exe, lines, tmp_path):
    path = tmp_path / "commands.txt"
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0 and not p.stderr, (p.returncode, p.stderr[-3000:])
    got = p.stdout.split("\n")[:-1]
    assert len(got) == len(lines)
    return got


def expect(bm_words, t, tuple_st, verdict, keys, pre, exact):
    """the answer of `opt` from the model: the first half from the candidate set alone, the second from OM.combine"""
    m = OM.combine(keys, pre, [len(keys)], [tuple_st], bm_words, t, lambda i, chosen: verdict, lambda s: exact[s])
    flag = m["flags"][0]
    cand = sorted({k for k, p in zip(keys, pre) if p == 0}) if tuple_st == 0 else []
    row1 = OM.row_of(cand[:t] if flag == OM.CHECK else cand, bm_words)
    first = [str(flag), "0" if flag == OM.CHECK else "255", str(len(cand))] + ["%x" % w for w in row1] + ["0" if flag == OM.CHECK else "1"]
    goes = m["hook"]["exact_tuples"] == 1
    st = m["tuple_status"][0]
    count = m["counts"][0] if (goes or flag == OM.CHECK) else 0
    row2 = m["rows"][0]
    second = ["1" if goes else "0", "0" if goes and st == 0 else "255", str(st), str(count)] + ["%x" % w for w in row2] + ["1" if goes and st != 0 else "0"]
    return " ".join(first) + " | " + " ".join(second), m


def command(bm_words, t, tuple_st, verdict, keys, pre, exact):
    return "opt %d %d %d %d %d %s" % (bm_words, t, tuple_st, verdict, len(keys), " ".join("%d %d %d" % x for x in zip(keys, pre, exact)))


def cases():
    """-> [(label, bm_words, t, tuple status, verdict, keys, pre-check statuses, exact statuses)]"""
    out = []
    rnd = random.Random(20261020)
    for bm_words, n_keys, thresholds in ((1, 9, (1, 5)), (1, 32, (1, 5)), (3, 70, (1, 5, 63, 64, 65)), (3, 96, (63, 64, 65))):
        for t in thresholds:
            for size in (t - 1, t, t + 1):
                if size < 0 or size > n_keys:
                    continue
                for pick in ("lowest", "highest", "random"):
                    ks = {"lowest": list(range(size)), "highest": list(range(n_keys - size, n_keys)), "random": sorted(rnd.sample(range(n_keys), size))}[pick]
                    rnd.shuffle(ks)
                    ok = [0] * size
                    label = "w%d/k%d/t%d/c%d/%s" % (bm_words, n_keys, t, size, pick)
                    for verdict in (0, 9):
                        out.append((label + "/v%d/all valid" % verdict, bm_words, t, 0, verdict, ks, ok, ok))
                        # what the exact verify leaves: the lowest candidate bad, the highest bad, all bad
                        if size:
                            low, high = ks.index(min(ks)), ks.index(max(ks))
                            for name, bad in (("low bad", [low]), ("high bad", [high]), ("all bad", list(range(size)))):
                                ex = [9 if s in bad else 0 for s in range(size)]
                                out.append((label + "/v%d/%s" % (verdict, name), bm_words, t, 0, verdict, ks, ok, ex))
                    if size:
                        # non-candidates between the candidates keep their status and never claim; a duplicate first and last
                        mixed_keys = ks + [n_keys + 3, ks[0]]
                        mixed_pre = ok + [2, 4]
                        out.append((label + "/non-candidates", bm_words, t, 0, 0, mixed_keys, mixed_pre, mixed_pre))
                        for name, keys2 in (("dup first", [ks[0]] + ks), ("dup last", ks + [ks[-1]]), ("dup of the highest key", ks + [max(ks)])):
                            pre2 = [0] * len(keys2)
                            for ex2 in (pre2, [9] + pre2[1:], pre2[:-1] + [9]):
                                out.append((label + "/" + name + "/%d%d" % (ex2[0], ex2[-1]), bm_words, t, 0, 0, keys2, pre2, ex2))
                    # a tuple refused by the range rule or the hash: final, whatever the rest says
                    for st in (2, 5):
                        out.append((label + "/tuple status %d" % st, bm_words, t, st, 0, ks, [st] * size, [st] * size))
    return out


@pytest.fixture(scope="module")
def table():
    return [(label, command(*args), expect(*args)) for label, *args in cases()]


@pytest.mark.parametrize("build", list(BUILDS))
def test_bookkeeping_against_the_model(exes, table, build, tmp_path):
    got = run(exes[build], [cmd for _, cmd, _ in table], tmp_path)
    wrong = [(label, g, want) for (label, _, (want, _)), g in zip(table, got) if g != want]
    assert not wrong, wrong[:5]


def test_the_cases_cover_what_they_claim(table):
    """the case set itself: every flag, both verdicts, both gates of both passes, cuts on both sides of the word boundaries"""
    by = {label: (want.split(" "), m) for label, _, (want, m) in table}
    assert len(by) == len(table) > 600
    flags = {m["flags"][0] for _, m in by.values()}
    assert flags == {OM.FINAL, OM.CHECK, OM.EXACT}
    # |C| = t passes under verdict 0 with S' = C; t + 1 drops the highest key; t - 1 goes exact and fails with row V = C
    a, m = by["w3/k70/t64/c64/lowest/v0/all valid"]
    assert a[:3] == ["1", "0", "64"] and a[3:6] == ["ffffffff", "ffffffff", "0"] and a[8:] == ["0", "255", "0", "64", "ffffffff", "ffffffff", "0", "0"]
    a, m = by["w3/k70/t64/c65/lowest/v0/all valid"]
    assert a[2] == "65" and a[3:6] == ["ffffffff", "ffffffff", "0"] and a[11] == "65"
    a, m = by["w3/k70/t65/c65/lowest/v0/all valid"]
    assert a[3:6] == ["ffffffff", "ffffffff", "1"]
    a, m = by["w3/k70/t63/c64/lowest/v0/all valid"]
    assert a[3:6] == ["ffffffff", "7fffffff", "0"]
    a, m = by["w3/k70/t64/c63/lowest/v0/all valid"]
    assert a[:3] == ["2", "255", "63"] and a[6] == "1" and a[8:] == ["1", "255", "9", "63", "ffffffff", "7fffffff", "0", "1"]
    # a failed check with every share valid: the exact call's answer, S again, through the open second gate
    a, m = by["w1/k9/t5/c6/lowest/v9/all valid"]
    assert a[:4] == ["1", "0", "6", "1f"] and a[6:] == ["1", "0", "0", "6", "1f", "0"] and m["hook"] == dict(checked=1, passed=0, exact_tuples=1, exact_shares=6)
    # ... with the lowest key bad the next one moves up; in a PASSING tuple the same bad share is never looked at (deviation 1 and 2)
    a, m = by["w1/k9/t5/c6/lowest/v9/low bad"]
    assert a[6:] == ["1", "0", "0", "5", "3e", "0"] and m["share_status"].count(9) == 1
    a, m = by["w1/k9/t5/c6/lowest/v0/low bad"]
    assert a[6:] == ["0", "255", "0", "6", "1f", "0"] and m["share_status"] == [0] * 6 and m["hook"]["exact_shares"] == 0
    # a duplicate sends the tuple exact without a check, whichever position it stands in
    for name in ("dup first", "dup last"):
        a, m = by["w1/k9/t5/c5/lowest/%s/00" % name]
        assert a[0] == "2" and a[2] == "5" and m["hook"] == dict(checked=0, passed=0, exact_tuples=1, exact_shares=6) and a[6:] == ["1", "0", "0", "5", "1f", "0"]
    a, m = by["w1/k9/t5/c5/lowest/tuple status 5"]
    assert a == ["0", "255", "0", "0", "1", "|", "0", "255", "5", "0", "0", "0"] and m["hook"] == dict(checked=0, passed=0, exact_tuples=0, exact_shares=0)
