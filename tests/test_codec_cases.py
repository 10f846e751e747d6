"""The compressed decoders (bn254_amd/csrc/bn254_io.h: decompress_g1, bn254_codec_g2.h: decompress_g2, u512_divmod_q; bn254_field.h:
fp2_sqrt; the two fp2_u512_greater), compiled for the host in the classic and in the pair layout, on the case set of tests/codec_cases.py
— and that case set against the big-integer model.  CPU only; tests/test_gpu_codecs.py runs the same cases on the device."""
import collections
import os
import subprocess
import sys

import pytest

from oracle import bn254_model as m
from tests import codec_cases as cc
from tests import hostsim_binding as hs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = m.Q


@pytest.fixture(scope="module")
def g1():
    return cc.g1_cases()


@pytest.fixture(scope="module")
def g2(derived):
    return cc.g2_cases(derived["g2_not_in_subgroup"])


def _model(fn, to_bytes, enc):
    try:
        return m.OK, to_bytes(fn(enc))
    except m.Bn254Error as e:
        return e.code, None


def test_builder_imports_nothing_from_the_library():
    src = open(os.path.join(ROOT, "tests", "codec_cases.py")).read()
    assert "bn254_amd" not in src.replace("bn254_amd/csrc", "") and "hostsim" not in src
    p = subprocess.run([sys.executable, "-c", "import sys; from tests import codec_cases; "
                        "print([k for k in sys.modules if k.startswith('bn254_amd') or 'hostsim' in k])"],
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "[]", (p.stdout, p.stderr[-500:])


def test_restatement_and_model_agree_on_every_case(g1, g2):
    """the builder's statuses, outputs and pre-subgroup points are its own restatement (norm criterion, root from the norm equation, u512
    rule); the model's decoders (complex-method f2_sqrt) must say the same on every case.  The model's subgroup ladder on the cases
    with a root and a good sign byte is most of this test's time."""
    for cs in g1:
        assert _model(m.g1_from_compressed, m.g1_to_uncompressed, cs.enc) == (cs.status, cs.want), (cs.kind, cs.enc.hex())
    for cs in g2:
        assert _model(m.g2_from_compressed, m.g2_to_uncompressed, cs.enc) == (cs.status, cs.want), (cs.kind, cs.enc.hex())
        re, im = cc.g2_split(cs.enc)
        if cs.pre is not None:
            # the model's own root of the same right-hand side, chosen by the model's comparison
            y = m.f2_sqrt(cc.twist_rhs((re, im)))
            assert y is not None and m.f2_mul(y, y) == cc.twist_rhs((re, im))
            gt = m._u512(y) > m._u512(m.f2_neg(y))
            y = y if gt == (cs.enc[0] == 0x0B) else m.f2_neg(y)
            assert cs.pre == m.g2_to_uncompressed(((re, im), y))
            assert m.g2_on_curve(((re, im), y))
        elif im < Q:
            assert (m.f2_sqrt(cc.twist_rhs((re, im))) is None) == (not cc.f2_has_root(cc.twist_rhs((re, im))))
            assert cs.enc[0] not in (0x0A, 0x0B) or not cc.f2_has_root(cc.twist_rhs((re, im)))


def test_kind_census(g1, g2):
    k1 = collections.Counter(cs.kind for cs in g1)
    k2 = collections.Counter(cs.kind for cs in g2)
    assert set(k1) == set(cc.G1_KINDS) and set(k2) == set(cc.G2_KINDS), (k1, k2)
    assert k1["valid random"] >= 1024 and k2["valid random"] >= 512
    assert {cs.enc[0] for cs in g1 if cs.kind == "valid random"} == {2, 3}
    assert {cs.enc[0] for cs in g2 if cs.kind == "valid random"} == {0x0A, 0x0B}
    assert all(cs.status == 0 and cs.want for cs in g1 + g2 if cs.kind == "valid random")
    # G1 edges: every x under every prefix; all three statuses occur, and range / root come before the prefix
    edge = [cs for cs in g1 if cs.kind == "edge x"]
    xs = {int.from_bytes(cs.enc[1:], "big") for cs in edge}
    assert xs >= {0, 1, 2, 3, Q - 2, Q - 1, Q, Q + 1, 2 * Q - 1, 1 << 255, (1 << 256) - 1} | {(1 << 29 * k) + d for k in range(1, 9) for d in (-1, 1)}
    assert len(edge) == len(xs) * len(cc.G1_PREFIXES) and {cs.status for cs in edge} == {0, 3, 6}
    assert all(cs.status == 6 for cs in edge if int.from_bytes(cs.enc[1:], "big") >= Q)
    assert any(cs.status == 6 and cs.enc[0] not in (2, 3) and int.from_bytes(cs.enc[1:], "big") < Q for cs in edge)
    # G2 division edges: the coordinate grid, the whole values, three sign bytes each; the has-root quarters
    div = [cs for cs in g2 if cs.kind == "division edge"]
    vals = {int.from_bytes(cs.enc[1:], "big") for cs in div}
    assert vals >= {im * Q + re for re in cc.DIV_COORDS for im in cc.DIV_COORDS} | set(cc.DIV_WHOLE)
    assert vals >= {Q * Q - 1, Q * Q, Q * Q + 1, (1 << 512) - 1, 1 << 511, Q * Q + Q - 1, Q, Q - 1, Q + 1, (Q - 1) * Q, (1 << 256) * Q}
    assert len(div) == 3 * len(vals)
    bits = [cc._root_bit(v) for v in vals]
    n = sum(b is not None for b in bits)
    assert 4 * sum(b is True for b in bits) >= n and 4 * sum(b is False for b in bits) >= n, collections.Counter(bits)
    for cs in div:
        if cs.enc[0] == 0x0C:
            assert cs.status == (3 if cc._root_bit(int.from_bytes(cs.enc[1:], "big")) else 6)
    # a quotient of exactly q, and one beyond 2^256 whose low words are a field element: both reduce to an x WITH a root and owe 6
    for lo, hi in ((Q, Q + 1), (1 << 256, (1 << 256) + Q)):
        assert any(cs.status == 6 and cs.enc[0] == 0x0C and lo <= cc.g2_split(cs.enc)[1] < hi and
                   cc.f2_has_root(cc.twist_rhs((cc.g2_split(cs.enc)[0], cc.g2_split(cs.enc)[1] % (1 << 256) % Q))) for cs in div)
    # right-hand sides in Fq: at least four c of either class, three sign bytes each; y purely imaginary / y.im == 0
    for kind, part in (("rhs in Fq, non-residue", 1), ("rhs in Fq, residue", 0)):
        got = [cs for cs in g2 if cs.kind == kind]
        assert len(got) >= 12 and collections.Counter(cs.enc[0] for cs in got) == {0x0A: len(got) // 3, 0x0B: len(got) // 3, 0x0C: len(got) // 3}
        for cs in got:
            assert cc.twist_rhs(cc.g2_split(cs.enc))[1] == 0
            if cs.enc[0] != 0x0C:
                y = (int.from_bytes(cs.pre[64:96], "big"), int.from_bytes(cs.pre[96:], "big"))
                assert y[part] != 0 and y[1 - part] == 0 and cs.status == 6
    out = [cs for cs in g2 if cs.kind == "outside the subgroup"]
    assert sum(cs.status == 6 and cs.pre is not None for cs in out) >= 65 and sum(cs.status == 3 for cs in out) >= 65
    assert {cs.status for cs in g2 if cs.kind == "double fault"} == {3, 6} == {cs.status for cs in g2 if cs.kind == "triple fault"}
    assert [cs.enc for cs in g1 if cs.kind == "all zero"] == [bytes(33)] and [cs.enc for cs in g2 if cs.kind == "all zero"] == [bytes(65)]
    # the layouts the GPU tests run
    for cases in (g1, g2):
        o = cc.orders(cases)
        assert all(0 < f < min(cc.WAVE, len(o["mixed waves"]) - cc.WAVE * w) for w, f in enumerate(cc.wave_profile(o["mixed waves"])))
        prof = cc.wave_profile(o["failing waves"])
        assert prof[0] == cc.WAVE and prof[1] == cc.WAVE - 1


def test_g1_decoder_on_every_case(g1):
    for cs in g1:
        st, out = hs.g1_decompress(cs.enc)
        assert st == cs.status and out == (cs.want or bytes(64)), (cs.kind, cs.enc.hex())


def test_g2_decoders_on_every_case_in_both_layouts(g2):
    """status and, where it is 0, the bytes through the existing exports of both layouts; the decoder's own status and point before
    the subgroup test through the new ones — the y of every case with a root, where alone the two tie-breaks of the sign rule show"""
    seen_pre = 0
    for cs in g2:
        where = (cs.kind, cs.enc.hex())
        st, out = hs.g2_decompress(cs.enc)
        assert st == cs.status and out == (cs.want or bytes(128)), where
        st, out = hs.pair_g2_decompress(cs.enc)
        assert st == cs.status and out == (cs.want or bytes(128)), where
        for raw in (hs.g2_decompress_raw(cs.enc), hs.pair_g2_decompress(cs.enc, raw=True)):
            if cs.pre is not None:
                assert raw == (0, cs.pre), where
                seen_pre += 1
            else:
                assert raw[0] == cs.status != 0, where
    assert seen_pre >= 2 * 600


BOUNDS_DRIVER = r'''
import ctypes, json, sys
root = sys.argv[1]
sys.path.insert(0, root)
from tests import codec_cases as cc
d = json.load(open(root + "/tests/golden/derived_vectors.json"))
hs = ctypes.CDLL(root + "/tests/hostsim/libhostsim_bounds.so")
hp = ctypes.CDLL(root + "/tests/hostsim/libhostsim_pair_bounds.so")
n = 0
for cs in cc.g1_cases():
    if cs.kind != "valid random":
        o = ctypes.create_string_buffer(64); assert hs.hs_g1_decompress(cs.enc, o) == cs.status; n += 1
for cs in cc.g2_cases(d["g2_not_in_subgroup"]):
    if cs.kind in ("division edge", "rhs in Fq, non-residue", "rhs in Fq, residue", "all zero"):
        o = ctypes.create_string_buffer(128)
        want = 0 if cs.pre is not None else cs.status
        assert hs.hs_g2_decompress_raw(cs.enc, o) == want and (cs.pre is None or o.raw == cs.pre)
        assert hp.hp_g2_decompress_raw(cs.enc, o) == want and (cs.pre is None or o.raw == cs.pre)
        if cs.kind != "division edge":                     # ... and the subgroup ladder on the point the decoder hands it
            assert hs.hs_g2_decompress(cs.enc, o) == cs.status and hp.hp_g2_decompress(cs.enc, o) == cs.status
        n += 1
print("ok", n)
'''


def test_edge_cases_stay_inside_the_tracked_bounds(g1, g2):
    """the edge and Fq-rational cases once under the interval tracker (tests/test_bounds.py), in both layouts: zero, q - 1 and one-coordinate
    values are the inputs most likely to leave the intervals the square roots' operation sequence was proven on"""
    hs.build_all()
    p = subprocess.run([sys.executable, "-c", BOUNDS_DRIVER, ROOT], capture_output=True, text=True, timeout=1200)
    assert p.returncode == 0 and p.stdout.split()[:1] == ["ok"] and int(p.stdout.split()[1]) >= 400, (p.stdout[-500:], p.stderr[-2000:])
