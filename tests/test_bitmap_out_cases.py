"""The emit, settle and weight bodies behind bn254_batch_aggregate_keys_bitmap, bn254_batch_verify_keyed_bitmap_export and
bn254_batch_bitmap_weights (bn254_amd/csrc/bn254_bitmap_out.h), compiled for the host as the stand-alone program
tests/hostsim/hostsim_bitmap_out.cpp — in both layouts of Fq2, each plain, under AddressSanitizer + UBSan and with the interval tracker
(-DBN_TRACK_BOUNDS) — and run over tests/bitmap_out_cases.py behind a registered set and subset tables built by bn254_bitmap.h.
Expectations are the oracle's (g2_add over the set keys, hash_to_g1) and Python integers.  CPU only; nothing sanitised is loaded into
Python and nothing is preloaded."""
import os
import struct
import subprocess
from concurrent.futures import ThreadPoolExecutor

import pytest

from tests import bitmap_out_cases as B
from tests.datagen import D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_bitmap_out.cpp")
COMMON = ["-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-Wno-unused-function"]
LAYOUTS = {"pair": [], "one_lane": ["-DBM_ONE_LANE"]}
BUILDS = {"plain": ["-O2"],
          "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
          "bounds": ["-O1", "-g", "-DBN_TRACK_BOUNDS"]}
VARIANTS = [(layout, build) for layout in sorted(LAYOUTS) for build in sorted(BUILDS)]


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostsim_bitmap_out")

    def compile_one(v):
        exe = str(d / ("hostsim_bitmap_out_%s_%s" % v))
        p = subprocess.run([os.environ.get("CXX", "g++")] + COMMON + LAYOUTS[v[0]] + BUILDS[v[1]] + ["-o", exe, SRC], capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, (v, p.stderr[-3000:])
        return v, exe
    with ThreadPoolExecutor(6) as ex:
        return dict(ex.map(compile_one, VARIANTS)), d


def run(programs, variant, pks, reg, weights, items, bm_words, tables):
    """items: (set bits, H(m) bytes, hash status, sigma's decode status, final status)"""
    exes, d = programs
    n, n_keys = len(items), len(pks)
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    with open(fin, "wb") as f:
        f.write(struct.pack("<4Q", n_keys, n, bm_words, 1 if tables else 0))
        f.write(b"".join(pks) + bytes(reg) + struct.pack("<%dQ" % n_keys, *weights))
        f.write(b"".join(struct.pack("<%dI" % bm_words, *B.to_words(it[0], bm_words)) for it in items))
        f.write(b"".join(it[1] for it in items) + bytes(it[2] for it in items) + bytes(it[3] for it in items) + bytes(it[4] for it in items))
    p = subprocess.run([exes[variant], fin, fout], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "hostsim_bitmap_out ok: %d rows over %d keys" % (n, n_keys) in p.stdout, (variant, p.stdout[-1000:], p.stderr[-3000:])
    blob = open(fout, "rb").read()
    assert len(blob) == n * (128 + 1 + 64 + 128 + 8 + 1)
    at = [0, 128 * n, 129 * n, 193 * n, 321 * n, 329 * n, 330 * n]
    keys_a, st_a, hashes_b, keys_b, weight, st_w = [blob[a:b] for a, b in zip(at, at[1:])]
    return keys_a, st_a, hashes_b, keys_b, list(struct.unpack("<%dQ" % n, weight)), st_w


def build_items():
    """every row under every combination of sigma's decode status, the hash status and the pairing's verdict — the final status is the first
    non-zero of decode, rule 2 (filled in per bm_words), hash, verdict — then every row under a final status that owes nothing to the
    entry's own bytes (the settle must look at the final status alone)"""
    c = B.oracle()
    items = []
    for i, (name, bits) in enumerate(B.rows()):
        st, h, _ = c.hash_to_g1(D("bmo/hostsim", i))
        assert st == 0
        for decode_st in (0, 4, 6):
            for hash_st in (0, 1, 5):
                for verdict in (0, 9):
                    items.append((bits, h, hash_st, decode_st, verdict))
        for forced in (3, 2, 10):
            items.append((bits, h, 0, 0, -forced))
    return items


def resolve(items, bm_words, reg):
    out = []
    for bits, h, hash_st, decode_st, verdict in items:
        final = -verdict if verdict < 0 else (decode_st or B.rule2(bits, bm_words, reg) or hash_st or verdict)
        out.append((bits, h, hash_st, decode_st, final))
    return out


def check(programs, variant, pks, reg, weights, bm_words, tables):
    items = resolve(build_items(), bm_words, reg)
    keys_a, st_a, hashes_b, keys_b, weight, st_w = run(programs, variant, pks, reg, weights, items, bm_words, tables)
    kept = 0
    for i, (bits, h, hash_st, decode_st, final) in enumerate(items):
        label = (variant, bm_words, tables, i, bits[:6], hash_st, decode_st, final)
        want_st, want_key = B.aggregate_key(pks, bits, bm_words, reg)
        assert st_a[i] == want_st and keys_a[128 * i:128 * i + 128] == want_key, label
        keep = final in (0, 9)
        kept += keep
        assert hashes_b[64 * i:64 * i + 64] == (h if keep else bytes(64)), label
        assert keys_b[128 * i:128 * i + 128] == (want_key if keep else bytes(128)), label
        assert (st_w[i], weight[i]) == B.weight(weights, bits, bm_words, reg), label
    assert 0 < kept < len(items)


def test_case_set_is_what_the_issue_names(programs, derived):
    """the case set holds the rows and weights the issue names — and the host-compiled bodies give its headline rows their expected bytes"""
    sks, pks = B.keyset(derived["g2_not_in_subgroup"])
    named = dict(B.rows())
    items = resolve([(named[k], bytes(64), 0, 0, 0) for k in ("cancel", "doubling", "refused_before_oob", "oob_at_n_keys")], 2, B.REG_STATUS)
    keys_a, st_a, _, _, weight, st_w = run(programs, ("pair", "plain"), list(pks), B.REG_STATUS, B.weight_sets()["edge"][0], items, 2, True)
    assert st_a == bytes([0, 0, 6, 2]) == st_w and keys_a[:128] == bytes(128) and keys_a[128:256] == B.oracle().g2_add(pks[0], pks[0]) and weight[2:] == [0, 0]
    assert len(pks) == 46 and 46 % 8 and 46 % 32
    rows = dict(B.rows())
    assert [len(rows["pop%d" % p]) for p in (0, 1, 2, 8, 9)] == [0, 1, 2, 8, 9] and len(rows["all_good"]) == B.N_GOOD
    st = {name: B.aggregate_key(pks, bits, 3) for name, bits in rows.items()}
    assert st["cancel"] == (0, bytes(128)) and st["identity_only"] == (0, bytes(128)) and st["pop0"] == (0, bytes(128))
    assert st["doubling"] == (0, B.oracle().g2_add(pks[0], pks[0])) and st["doubling"][1] != bytes(128)
    assert {s for s, _ in st.values()} == {0, 2, 4, 6}
    assert st["refused_before_oob"][0] == 6 and st["oob_at_n_keys"][0] == 2 and st["oob_only"][0] == 2 and B.aggregate_key(pks, rows["oob_only"], 2)[0] == 0
    assert B.aggregate_key(pks, rows["first_key_of_word1"], 1) == (0, bytes(128))             # one word: the keys above 31 are absent
    ws = B.weight_sets()
    assert [ok for _, ok in ws.values()].count(False) == 1 and sum(ws["total_max"][0]) == 2 ** 64 - 1 and sum(ws["total_2_64"][0]) == 2 ** 64
    assert ws["edge"][0][:3] == [0, 1, 2 ** 63] and ws["edge"][0][B.K_IDENT] > 0
    assert B.weight(ws["edge"][0], rows["identity_only"], 2) == (0, ws["edge"][0][B.K_IDENT])
    assert B.weight(ws["total_max"][0], list(range(B.N_KEYS)), 2) == (4, 0)


@pytest.mark.parametrize("variant", VARIANTS, ids=["%s-%s" % v for v in VARIANTS])
def test_every_row_every_width_both_routes(programs, variant, derived):
    sks, pks = B.keyset(derived["g2_not_in_subgroup"])
    ws = B.weight_sets()
    # the plain builds walk every width on both routes and every weight set; the instrumented ones the exact width and a short one
    widths = B.BM_WORDS if variant[1] == "plain" else (2, 1)
    for bm_words in widths:
        for tables in (True, False):
            check(programs, variant, list(pks), B.REG_STATUS, ws["edge"][0], bm_words, tables)
    for name in (sorted(ws) if variant[1] == "plain" else ["total_max"]):
        weights, accepted = ws[name]
        if accepted:
            check(programs, variant, list(pks), B.REG_STATUS, weights, 3, True)


@pytest.mark.parametrize("variant", VARIANTS, ids=["%s-%s" % v for v in VARIANTS])
def test_total_of_2_64_minus_1_does_not_wrap(programs, variant, derived):
    """every key accepted (the refused ones replaced by good ones), every bit set: the full total, exactly 2^64 - 1"""
    sks, pks = B.keyset(derived["g2_not_in_subgroup"])
    good = [pks[j] if B.REG_STATUS[j] == 0 else pks[10 + j - B.N_GOOD] for j in range(B.N_KEYS)]
    weights = B.weight_sets()["total_max"][0]
    item = (list(range(B.N_KEYS)), bytes(64), 0, 0, 0)
    keys_a, st_a, _, _, weight, st_w = run(programs, variant, good, [0] * B.N_KEYS, weights, [item], 2, True)
    assert (st_w[0], weight[0], st_a[0]) == (0, 2 ** 64 - 1, 0)
    assert keys_a == B.aggregate_key(good, item[0], 2, [0] * B.N_KEYS)[1]


@pytest.mark.parametrize("variant", [("pair", "sanitizers"), ("one_lane", "plain")], ids=["pair-sanitizers", "one_lane-plain"])
def test_no_keys_and_no_rows(programs, variant):
    """an empty set: any set bit gives 2, every key and weight is zero; and a call of no rows"""
    items = resolve([([], bytes(64), 0, 0, 0), ([0], bytes(64), 0, 0, 0), ([40, 70], bytes(64), 0, 0, 0)], 3, [])
    for tables in (True, False):
        keys_a, st_a, hashes_b, keys_b, weight, st_w = run(programs, variant, [], [], [], items, 3, tables)
        assert st_a == bytes([0, 2, 2]) == st_w and keys_a == bytes(384) == keys_b and weight == [0, 0, 0]
    assert run(programs, variant, [], [], [], [], 2, True)[1] == b""
