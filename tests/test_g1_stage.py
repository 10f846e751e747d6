"""The staging and overlay bodies behind BN254_FLAG_G1_COMPRESSED and bn254_batch_g1_decompress_device (bn254_amd/csrc/bn254_g1stage.h),
compiled for the host as the stand-alone program tests/hostsim/hostsim_g1_stage.cpp — plain, under AddressSanitizer + UBSan, and with the
interval tracker (-DBN_TRACK_BOUNDS) — and run over tests/codec_cases.g1_cases() in the orders and cuts of codec_cases.orders, plus the
items of tests/compressed_keyed_cases.py.  Expectations are the oracle's: the stand-in BE32(q) || 0 and the item's own status where an
encoding does not decompress, the point where it does; the overlay replaces a 6, and only a 6, of such an item.  CPU only; nothing
sanitised is loaded into Python."""
import os
import subprocess

import pytest

from tests import codec_cases as cc
from tests import compressed_keyed_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "hostsim", "hostsim_g1_stage.cpp")
COMMON = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"]
BUILDS = {"plain": ["-O2"],
          "sanitizers": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"],
          "bounds": ["-O1", "-g", "-DBN_TRACK_BOUNDS"]}
CALL_STATUSES = (0, 6, 2, 9, 6, 1, 4, 6, 3, 5)               # what a call might have written: a 6 at every residue an item's index can have


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("hostsim_g1_stage")
    out = {}
    for name, flags in BUILDS.items():
        exe = str(d / ("hostsim_g1_stage_" + name))
        p = subprocess.run([os.environ.get("CXX", "g++")] + COMMON + flags + ["-o", exe, SRC], capture_output=True, text=True, timeout=900)
        assert p.returncode == 0, p.stderr[-3000:]
        out[name] = exe
    return out, d


def run(programs, build, encs, call_st):
    exes, d = programs
    n = len(encs)
    fin, fout = str(d / "in.bin"), str(d / "out.bin")
    with open(fin, "wb") as f:
        f.write(n.to_bytes(8, "little") + b"".join(encs) + bytes(call_st))
    p = subprocess.run([exes[build], fin, fout], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "hostsim_g1_stage ok: %d items" % n in p.stdout, (build, p.stdout[-1000:], p.stderr[-3000:])
    blob = open(fout, "rb").read()
    assert len(blob) == n * (64 + 1 + 1 + 64 + 1)
    at = [0, 64 * n, 65 * n, 66 * n, 130 * n, 131 * n]
    return [blob[a:b] for a, b in zip(at, at[1:])]


def check(programs, build, encs, want_st, want_pts, label):
    """want_st[i], want_pts[i]: the status and (where 0) the point the oracle owes encoding i"""
    n = len(encs)
    call_st = [CALL_STATUSES[(i + i // len(CALL_STATUSES)) % len(CALL_STATUSES)] for i in range(n)]
    staged, pre, after, plain, plain_st = run(programs, build, encs, call_st)
    assert pre == bytes(want_st) == plain_st, (label, build)
    for i in range(n):
        ok = want_st[i] == 0
        assert staged[64 * i:64 * i + 64] == (want_pts[i] if ok else K.STAND_IN), (label, build, i, encs[i].hex())
        assert plain[64 * i:64 * i + 64] == (want_pts[i] if ok else bytes(64)), (label, build, i, encs[i].hex())
    assert after == K.overlay(call_st, want_st), (label, build)
    changed = [i for i in range(n) if after[i] != call_st[i]]
    assert all(call_st[i] == 6 and want_st[i] == 3 for i in changed), (label, build)
    return changed


def test_oracle_and_restated_decoder_agree():
    """the oracle's g1_decompress (which the stand-ins come from) and the restated rules of codec_cases on every case"""
    for cs in cc.g1_cases():
        u, st = K.stand_in(cs.enc)
        assert st == cs.status and u == (cs.want if st == 0 else K.STAND_IN), cs.enc.hex()
    assert K.STAND_IN[:32] == cc.be(cc.Q) and cc.g1_expect(b"\x02" + K.STAND_IN[:32])[0] == cc.ST_MEMBER


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_codec_cases_every_order_and_cut(programs, build):
    cases = cc.g1_cases()
    assert {cs.status for cs in cases} == {0, 3, 6}
    replaced = 0
    for name, order in cc.orders(cases).items():
        # the plain build walks every cut; the instrumented ones the whole list and the cuts around one wave
        cuts = [len(order)] + list(cc.CUTS if build == "plain" else (1, 65))
        for cut in cuts:
            part = order[:cut]
            replaced += len(check(programs, build, [cs.enc for cs in part], [cs.status for cs in part], [cs.want for cs in part], (name, cut)))
    assert replaced > 0                                              # some status-3 item met a 6 and took its own status back
    check(programs, build, [], [], [], "empty")


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_keyed_case_set(programs, build, derived):
    items = K.items(130, derived["g2_not_in_subgroup"], tag="stage")
    assert {it.kind for it in items} == set(K.MUTATIONS)
    pairs = [K.stand_in(it.enc) for it in items]
    for it, (u, st) in zip(items, pairs):
        if it.kind in K.PINNED:
            assert it.want == K.PINNED[it.kind], it
        assert (st != 0) == (it.kind in ("prefix04", "noroot02", "noroot07", "x_plus_q", "zeros", "oob_bad", "refused_bad", "refused_noroot", "hash_bad")), it
    check(programs, build, [it.enc for it in items], [st for _, st in pairs], [u for u, _ in pairs], "keyed items")
