"""bn254_batch_check_public_keys on the device against the case set of tests/cpk_cases.py: every expected status is the oracle's
(oracle/c_oracle.py: check_public_keys), none comes from the device, every comparison is byte-exact.  The call has a branch of its
own in six Miller kernels (k_miller_cpk; mode 1 of the lane-pair, trio, quad, eight-wave and lane-machine kernels), is the only
caller of the five final-exponentiation layouts with use_hash = 0, and decodes pk_g2 first with pk_g1 accumulated behind it: every
case runs on every one of these routes under all four flags values, at sizes that cross waves, workgroups, the octet final
exponentiation's 127 | 128 switch and every boundary of the routing table; behind a verify that left hash failures in the
workspace; with refused arguments; and through the Python and C++ mirrors.  The same cases run on the host build of the one-lane
kernel body in tests/test_cpk_cases.py.  Run with -m gpu."""
import ctypes
import functools
import os
import subprocess

import pytest

from tests import cpk_cases as ck
from tests.conftest import ws_default

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONET_DEFAULT = ws_default("NONET_MAX_BATCH_DEFAULT")
LM_DEFAULT = ws_default("LM_MAX_BATCH_DEFAULT")
TRIO_DEFAULT = ws_default("TRIO_MAX_BATCH_DEFAULT")
NONET_WIDE_MAX = ws_default("NONET_WIDE_MAX_BATCH")
ALL_ROUTES = {(0, 0), (0, 1), (1, 1), (1, 2), (2, 3), (0, 2)}
ON = 1 << 20
DEFAULTS = dict(pair=1, trio=TRIO_DEFAULT, roles=2, nonet=NONET_DEFAULT, wide=1, lm=LM_DEFAULT)
SHIFTS = (0, 17)
SIZES = (ck.length(), 1, 2, 7, 129, 1027)
OCTET_SIZES = SIZES + (127, 128)          # k_final_exp_trio: straight-line chains below 128 items, the accumulator machine from 128 on
# name -> (options that differ from the defaults, sizes, final-exponentiation layout the sizes up to 1 024 run on)
SETTINGS = {
    "one lane per item": (dict(pair=0), SIZES, "one lane"),                                      # k_miller_cpk + k_final_exp
    "lane pairs": (dict(trio=0), SIZES, "lane pairs"),
    "octets, eight wave roles": (dict(lm=0, nonet=0, trio=ON, roles=2), OCTET_SIZES, "octet"),
    "octets, four wave roles": (dict(lm=0, nonet=0, trio=ON, roles=1), OCTET_SIZES, "octet"),
    "octets, lane groups of one wave": (dict(lm=0, nonet=0, trio=ON, roles=0), OCTET_SIZES, "octet"),
    "nonet": (dict(lm=0, nonet=ON, trio=ON, wide=0), SIZES, "nonet"),
    "nonet wide": (dict(lm=0, nonet=ON, trio=ON, wide=1), SIZES, "nonet wide"),
    "lane machine, nonet wide": (dict(lm=ON, nonet=ON, trio=ON, wide=1), SIZES, "nonet wide"),
    "lane machine, nonet": (dict(lm=ON, nonet=ON, trio=ON, wide=0), SIZES, "nonet"),
    "lane machine, octets": (dict(lm=ON, nonet=0, trio=ON), OCTET_SIZES, "octet"),
}


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


def _set(eng, **kw):
    from bn254_amd import engine as E
    ids = dict(pair=E.OPT_PAIR_LANES, trio=E.OPT_TRIO_MAX_BATCH, roles=E.OPT_TRIO_WAVE_ROLES, nonet=E.OPT_NONET_MAX_BATCH, wide=E.OPT_NONET_WIDE,
               lm=E.OPT_LM_MAX_BATCH)
    for k, v in kw.items():
        eng.set_option(ids[k], v)


def _route(table, n):
    return next((miller, fe) for max_n, miller, fe in table if n <= max_n)


@functools.lru_cache(maxsize=None)
def _tiled(n, flags, shift):
    return ck.tiled(n, flags, shift)


def _check(eng, n, flags, shift, what):
    g2, g1, want = _tiled(n, flags, shift)
    got = eng.batch_check_public_keys(g2, g1, n, flags=flags)
    assert got == want, (what, "flags %d, shift %d" % (flags, shift), ck.first_difference(got, want, shift))


def _answers_the_case_set(eng):
    for flags in ck.FLAGS:
        _check(eng, ck.length(), flags, 0, "case set")


@pytest.mark.parametrize("name", list(SETTINGS))
def test_every_case_on_every_layout(eng, name):
    """a. sizes L, 1, 2, 7, 129 and 1 027 (127 and 128 too where the octet final exponentiation runs), tiled with two shifts, under
    flags 0 .. 3, on one route of the call per parameter"""
    opts, sizes, _ = SETTINGS[name]
    try:
        _set(eng, **opts)
        for n in sizes:
            for shift in SHIFTS:
                for flags in ck.FLAGS:
                    _check(eng, n, flags, shift, (name, n))
    finally:
        _set(eng, **DEFAULTS)


def test_the_settings_cover_every_route(eng):
    """the (miller, fe) rows that the sizes of test_every_case_on_every_layout select under its settings: every route of the table"""
    default = eng.route_table()
    taken = {}
    try:
        for name, (opts, sizes, fe_name) in SETTINGS.items():
            _set(eng, **opts)
            table = eng.route_table()
            taken[name] = {_route(table, n) for n in sizes}
            if opts.get("pair", 1):
                fe = {"lane pairs": 3, "octet": 2, "nonet": 1, "nonet wide": 0}[fe_name]
                assert {r[1] for r in (_route(table, n) for n in sizes if n <= NONET_WIDE_MAX)} == {fe}, (name, table)
            _set(eng, **DEFAULTS)
    finally:
        _set(eng, **DEFAULTS)
    assert set().union(*taken.values()) >= ALL_ROUTES | {(1, 0)}, taken
    assert eng.route_table() == default


def test_routing_table_boundaries_at_the_defaults(eng):
    """b. max_n - 1, max_n, max_n + 1 of every row of the default table but the last, under flags 0 and 1 | 2"""
    table = eng.route_table()
    assert table == [(NONET_WIDE_MAX, 0, 0), (LM_DEFAULT, 0, 1), (NONET_DEFAULT, 1, 1), (TRIO_DEFAULT, 1, 2), (2 ** 64 - 1, 2, 3)], table
    cuts = [n for max_n, _, _ in table[:-1] for n in (max_n - 1, max_n, max_n + 1)]
    assert max(cuts) == 16385 and {_route(table, n) for n in cuts} == {(r[1], r[2]) for r in table}
    for n in cuts:
        for flags, shift in ((0, n % ck.length()), (3, 0)):
            g2, g1, want = ck.tiled(n, flags, shift)
            got = eng.batch_check_public_keys(g2, g1, n, flags=flags)
            assert got == want, (n, flags, _route(table, n), ck.first_difference(got, want, shift))


STALE_N = 331                               # every layout below takes it (<= 1 024, >= 128); no multiple of L, of a wave or of a workgroup
STALE_LAYOUTS = ("one lane per item", "lane pairs", "octets, eight wave roles", "nonet", "nonet wide")


@pytest.fixture(scope="module")
def hash_starved_verify(eng):
    """a verify batch of STALE_N items of tests/datagen.make_verify_batch with identity and undecodable signatures and keys planted at
    items whose check_public_keys case (shift 0) is a MATCHING pair — a decode status left behind shows as a wrong 0"""
    from tests.datagen import make_verify_batch
    msgs, sigs, pks, _ = make_verify_batch(eng, STALE_N, corrupt_every=0)
    sigs, pks = bytearray(sigs), bytearray(pks)
    zeros = [i for i in range(STALE_N) if ck.expected(3)[i % ck.length()] == 0]
    assert len(zeros) >= 64
    planted = zeros[::4][:24]
    for j, i in enumerate(planted):
        kind = j % 4
        if kind == 0:
            sigs[64 * i:64 * i + 64] = bytes(64)                             # identity signature
        elif kind == 1:
            sigs[64 * i:64 * i + 32] = b"\xff" * 32                          # x >= q: 6
        elif kind == 2:
            pks[128 * i + 127] ^= 1                                          # off the twist: 4
        else:
            pks[128 * i:128 * i + 128] = bytes(128)                          # identity key
    return msgs, bytes(sigs), bytes(pks), planted


@pytest.mark.parametrize("name", STALE_LAYOUTS)
def test_behind_a_verify_that_left_hash_failures(eng, hash_starved_verify, name):
    """c. the verify's hash statuses (and decode statuses) stay in the workspace at the indices the next call uses: a final
    exponentiation that read BY_ST_HASH with use_hash = 0, or a first decode kernel that accumulated, would report them"""
    from bn254_amd.engine import OPT_HASH_MAX_TRIES
    msgs, sigs, pks, planted = hash_starved_verify
    opts, _, fe_name = SETTINGS[name]
    n = STALE_N
    try:
        _set(eng, **opts)
        if opts.get("pair", 1):
            assert _route(eng.route_table(), n)[1] == {"lane pairs": 3, "octet": 2, "nonet": 1, "nonet wide": 0}[fe_name]
        for flags in (0, 3):
            eng.set_option(OPT_HASH_MAX_TRIES, 1)
            try:
                st = eng.batch_verify(msgs, sigs, pks, flags=flags)
            finally:
                eng.set_option(OPT_HASH_MAX_TRIES, 0)
            assert st.count(1) * 100 >= 40 * n, (name, st.count(1), n)       # 52.7 % of the messages have no point at counter 0
            assert {4, 6} <= {st[i] for i in planted}
            g2, g1, want = _tiled(n, flags, 0)
            got = eng.batch_check_public_keys(g2, g1, n, flags=flags)
            assert 1 not in got, (name, flags, got.count(1))
            assert got == want, (name, flags, ck.first_difference(got, want))
    finally:
        _set(eng, **DEFAULTS)


def test_refused_arguments_leave_status_and_context_alone(eng):
    """d. n = 0 is a success that writes nothing; a NULL pointer with n > 0 is BN254_E_BAD_ARGUMENT; both decided on the host before
    any access"""
    fn, h = eng._lib.bn254_batch_check_public_keys, eng._h
    g2, g1, _ = _tiled(3, 0, 0)
    status = ctypes.create_string_buffer(b"\xee" * 8, 8)
    assert fn(h, g2, g1, 0, 0, status) == 0 and status.raw == b"\xee" * 8
    assert fn(h, None, None, 0, 0, None) == 0
    for args in ((None, g1, status), (g2, None, status), (g2, g1, None)):
        for flags in (0, 3):
            assert fn(h, args[0], args[1], 3, flags, args[2]) == -10001, args
    assert fn(None, g2, g1, 3, 0, status) == -10001
    assert status.raw == b"\xee" * 8
    _answers_the_case_set(eng)


def _one_case_per_code():
    """[(case, status under flags 0)]: a matching pair, the pair of identities, and the first case of each other code"""
    want, names, out = ck.expected(0), ck.names(), []
    for name in ("matching pair", "both identity"):
        assert want[names.index(name)] == 0
        out.append((ck.cases()[names.index(name)], 0))
    for code in (4, 6, 9):
        out.append((ck.cases()[want.index(code)], code))
    return out


def test_python_and_cpp_mirrors(tmp_path):
    """e. bn254_amd.api.check_public_keys and bn254::check_public_keys (bn254_amd/host/bn254.hpp) raise the ErrorKind of the status
    and return for a matching pair and for the pair of identities"""
    from bn254_amd.api import Error, ErrorKind, PublicKey, PublicKeyG1, check_public_keys
    picked = _one_case_per_code()
    assert [st for _, st in picked] == [0, 0, 4, 6, 9]
    for cs, st in picked:
        if st == 0:
            assert check_public_keys(PublicKey(cs.pk_g2), PublicKeyG1(cs.pk_g1)) is None, cs.name
        else:
            with pytest.raises(Error) as e:
                check_public_keys(PublicKey(cs.pk_g2), PublicKeyG1(cs.pk_g1))
            assert e.value.kind == ErrorKind(st), cs.name
    src = tmp_path / "cpk_mirror.cpp"
    src.write_text(CPP_MIRROR)
    exe = str(tmp_path / "cpk_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "bn254_amd", "host"), str(src), "-L" + os.path.join(ROOT, "bn254_amd"),
                           "-lbn254hip", "-Wl,-rpath," + os.path.join(ROOT, "bn254_amd"), "-o", exe])
    args = [a for cs, st in picked for a in (cs.pk_g2.hex(), cs.pk_g1.hex(), str(st))]
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "cpk mirror ok %d" % len(picked) in p.stdout, (p.stdout, p.stderr)


# arguments: triples of pk_g2 hex, pk_g1 hex, expected status
CPP_MIRROR = r"""
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "bn254.hpp"
template <size_t N> static bool unhex(const char* s, std::array<uint8_t, N>& out) {
  if (strlen(s) != 2 * N) return false;
  for (size_t i = 0; i < N; ++i) { unsigned v; if (sscanf(s + 2 * i, "%2x", &v) != 1) return false; out[i] = (uint8_t)v; }
  return true;
}
int main(int argc, char** argv) {
  try {
    if (argc < 4 || (argc - 1) % 3) return 2;
    int done = 0;
    for (int a = 1; a < argc; a += 3, ++done) {
      bn254::PublicKey pk2; bn254::PublicKeyG1 pk1;
      if (!unhex(argv[a], pk2.raw) || !unhex(argv[a + 1], pk1.raw)) return 3;
      const int want = atoi(argv[a + 2]);
      int got = 0;
      try { bn254::check_public_keys(pk2, pk1); }
      catch (const bn254::Error& e) { got = (int)e.kind; }
      if (got != want) { printf("case %d: got %d, want %d\n", done, got, want); return 4; }
    }
    printf("cpk mirror ok %d\n", done);
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
"""
