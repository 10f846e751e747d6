"""bn254_batch_pairing, _check and _device on the device against the case set of tests/pairing_cases.py: every expected status and Gt
is the oracle's (oracle/c_oracle.py: batch_pairing), none comes from another device route, every comparison is byte-exact.
pairing_device (bn254_amd/csrc/bn254_hip.hip) picks between three kernel families — the small-batch route (the lane machine in mode 2,
k_final_exp_nonet_product), lane pairs (k_miller_var_pair, k_final_exp_pair with item_stride = k) and one lane per pair (k_miller_var,
k_final_exp with k) — and each has a loop of its own for the product and for the lowest faulty pair of an item.  Every case runs on
every route under all four flags values with k = 1 .. 4, at sizes that cross waves and workgroups; on both sides of the route boundary
in pairs and in items; as items of up to 1 537 pairs; through the device form with and without Gt; behind a call that left decode
faults in the workspace; with refused arguments; and through the Python mirrors.  The Gt of an item that did not decode is the product
with the generator in place of every failed operand (include/bn254_hip.h) and is compared as well.  The same cases run on the host
builds of the kernel bodies in tests/test_pairing_cases.py.  Run with -m gpu."""
import ctypes
import functools

import pytest

from tests import pairing_cases as pc
from tests.conftest import ws_default

pytestmark = pytest.mark.gpu

LM_DEFAULT = ws_default("LM_MAX_BATCH_DEFAULT")
NONET_WIDE_MAX = ws_default("NONET_WIDE_MAX_BATCH")
DEFAULTS = dict(pair=1, wide=1, lm=LM_DEFAULT)
SMALL, PAIRS, ONE_LANE = "small batch", "lane pairs", "one lane"
LENGTHS = {k: len(pc.cases_of(k)) for k in pc.KS}
# name -> (options that differ from the defaults, the route every size of the setting takes, the sizes for items of k pairs)
SETTINGS = {
    "default": (dict(), SMALL, lambda k: (2 * LENGTHS[k] + 1,)),                 # two full cycles of the set plus one
    "lane machine off": (dict(lm=0), PAIRS, lambda k: (127, 128, 129)),         # a workgroup of k_final_exp_pair (128 items) less one, full, plus one
    "nonet wide off": (dict(wide=0), PAIRS, lambda k: (127, 128, 129)),         # lane pairs through the other condition
    "one lane per pair": (dict(pair=0), ONE_LANE, lambda k: (63, 64, 65)),      # a wave of k_final_exp less one, full, plus one
}
E_BAD_ARGUMENT, E_MISALIGNED = -10001, -10002


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def _set(eng, **kw):
    from bn254_amd import engine as E
    ids = dict(pair=E.OPT_PAIR_LANES, wide=E.OPT_NONET_WIDE, lm=E.OPT_LM_MAX_BATCH)
    for k, v in kw.items():
        eng.set_option(ids[k], v)


def _route(eng, opts, n, k):
    """the family pairing_device takes for n items of k pairs: the small-batch kernels need lane pairs, n k pairs within the lane
    machine's limit and the eighteen-lane-pair final exponentiation (fe 0) in the table's row for n ITEMS"""
    o = dict(DEFAULTS, **opts)
    fe = next(fe for max_n, _, fe in eng.route_table() if n <= max_n)
    if o["pair"] and o["lm"] > 0 and n * k <= o["lm"] and fe == 0:
        return SMALL
    return PAIRS if o["pair"] else ONE_LANE


def _compare(eng, k, n, flags, shift, what, check=True):
    g1, g2, want_st, want_gt, idx = pc.tiled(k, n, flags, shift)
    gt, st = eng.batch_pairing(g1, g2, n, k, flags=flags)
    assert st == want_st, (what, k, n, flags, pc.first_difference(k, idx, st, want_st))
    assert gt == want_gt, (what, k, n, flags, pc.first_difference(k, idx, gt, want_gt, 384))
    if check:
        st = eng.batch_pairing_check(g1, g2, n, k, flags=flags)
        assert st == want_st, (what, "check", k, n, flags, pc.first_difference(k, idx, st, want_st))


def _answers_the_case_set(eng, k=2):
    _compare(eng, k, LENGTHS[k], 3, 0, "case set")


@pytest.mark.parametrize("k", pc.KS)
@pytest.mark.parametrize("name", list(SETTINGS))
def test_every_case_on_every_route(eng, name, k):
    """the tiled set of k pairs per item under flags 0 .. 3 on one route per setting: statuses and Gt of bn254_batch_pairing on every
    item (a failed item's Gt included), statuses of bn254_batch_pairing_check; the shift moves every case to another slot per size"""
    opts, route, sizes = SETTINGS[name]
    try:
        _set(eng, **opts)
        for j, n in enumerate(sizes(k)):
            assert _route(eng, opts, n, k) == route, (name, n, k, eng.route_table())
            for flags in pc.FLAGS:
                _compare(eng, k, n, flags, 11 * j + flags, (name, route))
    finally:
        _set(eng, **DEFAULTS)


def test_the_settings_cover_the_three_routes(eng):
    default = eng.route_table()
    assert default[0] == (NONET_WIDE_MAX, 0, 0), default
    taken = {}
    try:
        for name, (opts, route, sizes) in SETTINGS.items():
            _set(eng, **opts)
            taken[name] = {_route(eng, opts, n, k) for k in pc.KS for n in sizes(k)}
            assert taken[name] == {route}, (name, taken[name], eng.route_table())
            _set(eng, **DEFAULTS)
    finally:
        _set(eng, **DEFAULTS)
    assert set().union(*taken.values()) == {SMALL, PAIRS, ONE_LANE}
    assert eng.route_table() == default
    # "nonet wide off" leaves the lane machine on and reaches lane pairs through the table; "lane machine off" leaves the table alone
    assert SETTINGS["nonet wide off"][0] == dict(wide=0) and SETTINGS["lane machine off"][0] == dict(lm=0)


def test_route_boundary_in_pairs_and_in_items_at_the_defaults(eng):
    """both sides of the small-batch route's two limits — n k <= LM_MAX_BATCH pairs and n items within the first row of the table —
    for k = 1, 2, 3, and the shape within the items limit but over the pairs limit.  The batches are the tiled set, so every status
    and every Gt has the oracle's value at no further cost: all items are compared, among them the first and the last 200 and every
    index = 0 mod 97 between.  No pairing is computed on the CPU beyond the set's own for k = 1 .. 3 under flags 0 and 3 (pc.expected:
    322 products of 732 pairings; pc.gt_of_failed: 224 products of 521), which the other tests share."""
    table = eng.route_table()
    items_max = table[0][0]
    assert (items_max, table[0][2]) == (NONET_WIDE_MAX, 0) and LM_DEFAULT % 6 == 0 and LM_DEFAULT >= items_max
    shapes = [(items_max, 1), (items_max + 1, 1)] + [(LM_DEFAULT // k + d, k) for k in (2, 3) for d in (0, 1)] + [(items_max, 2)]
    assert shapes == [(1024, 1), (1025, 1), (768, 2), (769, 2), (512, 3), (513, 3), (1024, 2)], shapes
    want = [SMALL, PAIRS, SMALL, PAIRS, SMALL, PAIRS, PAIRS]
    assert [_route(eng, {}, n, k) for n, k in shapes] == want
    for (n, k), route in zip(shapes, want):
        for flags in (0, 3):
            _compare(eng, k, n, flags, n % LENGTHS[k], (route, "boundary"), check=flags == 3)


LONG_SETTINGS = {SMALL: dict(), PAIRS: dict(lm=0), ONE_LANE: dict(pair=0)}


@functools.lru_cache(maxsize=None)
def _long_call(k, one):
    """three items of k pairs: the item under test between two neighbours with the OTHER verdict, so that a kernel that strides by
    anything but i k, or reads a pair too many or too few, meets a different product"""
    items = [pc.long_item(k, 2, not one), pc.long_item(k, 1, one), pc.long_item(k, 2, not one)]
    return b"".join(x[0] for x in items), b"".join(x[1] for x in items), bytes(x[2] for x in items), b"".join(x[3] for x in items)


@pytest.mark.parametrize("route", list(LONG_SETTINGS))
def test_long_items(eng, derived, route):
    """items far beyond the oracle's 16 pairs; each expectation is ONE oracle pairing by bilinearity (pc.long_item).  One item of
    LM_MAX_BATCH pairs is the longest the small-batch route takes, one more goes to lane pairs; three items of 500, 501 and 499 pairs
    per call need the stride i k.  Each once as a product that is one and once as one that is not."""
    opts = LONG_SETTINGS[route]
    one_item = LM_DEFAULT if route == SMALL else LM_DEFAULT + 1
    assert one_item == (1536 if route == SMALL else 1537)
    try:
        _set(eng, **opts)
        for one in (True, False):
            g1, g2, st, gt = pc.long_item(one_item, 1, one)
            assert _route(eng, opts, 1, one_item) == route
            assert eng.batch_pairing(g1, g2, 1, one_item, flags=3) == (gt, bytes([st])), (route, one_item, one)
            assert eng.batch_pairing_check(g1, g2, 1, one_item) == bytes([st]), (route, one_item, one)
            assert (st, gt.hex() == derived["gt_one"]) == ((0, True) if one else (9, False))
            for k in (500, 501, 499):
                g1, g2, want_st, want_gt = _long_call(k, one)
                assert _route(eng, opts, 3, k) == route and want_st == (bytes([9, 0, 9]) if one else bytes([0, 9, 0]))
                assert eng.batch_pairing(g1, g2, 3, k, flags=1) == (want_gt, want_st), (route, k, one)
                assert eng.batch_pairing_check(g1, g2, 3, k, flags=2) == want_st, (route, k, one)
    finally:
        _set(eng, **DEFAULTS)


@pytest.mark.parametrize("route", (SMALL, PAIRS))
def test_device_form_with_and_without_gt(eng, route):
    """bn254_batch_pairing_device on a caller's stream and on the context's own, with d_gt (program C_FE_EXACT) and with d_gt = NULL
    (the status-only program C_FE_CHECK): the statuses are the expected ones either way, the Gt where it is asked for, and the bytes
    behind both outputs keep their fill"""
    from tests.hip_ctypes import DevBuf, Stream
    k, fill = 2, 0xEE
    n = 2 * LENGTHS[k] + 1 if route == SMALL else 129
    opts = LONG_SETTINGS[route]
    stream, bufs = Stream(), []
    try:
        _set(eng, **opts)
        assert _route(eng, opts, n, k) == route
        for flags in (0, 3):
            g1, g2, want_st, want_gt, idx = pc.tiled(k, n, flags, 7)
            d_g1, d_g2 = DevBuf(len(g1), data=g1), DevBuf(len(g2), data=g2)
            bufs += [d_g1, d_g2]
            for own_stream in (False, True):
                for with_gt in (True, False):
                    d_gt, d_st = DevBuf(384 * n + 384, fill=fill), DevBuf(n + 64, fill=fill)
                    bufs += [d_gt, d_st]
                    eng.batch_pairing_device(d_g1.ptr, d_g2.ptr, n, k, d_gt.ptr if with_gt else None, d_st.ptr, flags=flags,
                                             stream=None if own_stream else stream.handle)
                    eng.synchronize() if own_stream else stream.synchronize()
                    what = (route, flags, own_stream, with_gt)
                    st, gt = d_st.download(), d_gt.download()
                    assert st[:n] == want_st, (what, pc.first_difference(k, idx, st[:n], want_st))
                    assert st[n:] == bytes([fill]) * 64 and gt[384 * n:] == bytes([fill]) * 384, what
                    if with_gt:
                        assert gt[:384 * n] == want_gt, (what, pc.first_difference(k, idx, gt[:384 * n], want_gt, 384))
                    else:
                        assert gt[:384 * n] == bytes([fill]) * (384 * n), what
    finally:
        _set(eng, **DEFAULTS)
        stream.destroy()
        for b in bufs:
            b.free()


@pytest.mark.parametrize("route", list(LONG_SETTINGS))
def test_behind_a_call_that_left_faults(eng, c, route):
    """260 items of two pairs whose every operand is out of range leave a decode status in each of the 520 workspace slots; the tiled set
    as 130 items of FOUR pairs then reuses those slots: a decode kernel that accumulated onto them, or a final exponentiation that read
    a slot of the old split, would report the 6 again"""
    opts = LONG_SETTINGS[route]
    n_bad, n = 260, 130
    bad1, bad2 = b"\xff" * (64 * 2 * n_bad), b"\xff" * (128 * 2 * n_bad)
    assert c.batch_pairing(bad1[:256], bad2[:512], 2, 2, 0)[1] == b"\x06\x06" and c.g2_validate(bad2[:128], 0) == 6
    try:
        _set(eng, **opts)
        assert _route(eng, opts, n_bad, 2) == _route(eng, opts, n, 4) == route
        for flags in (0, 3):
            assert eng.batch_pairing(bad1, bad2, n_bad, 2, flags=flags)[1] == b"\x06" * n_bad
            _compare(eng, 4, n, flags, 3, (route, "behind faults"), check=False)
            assert eng.batch_pairing_check(bad1, bad2, n_bad, 2, flags=flags) == b"\x06" * n_bad
            g1, g2, want_st, _, idx = pc.tiled(4, n, flags, 3)
            st = eng.batch_pairing_check(g1, g2, n, 4, flags=flags)
            assert st == want_st, (route, flags, pc.first_difference(4, idx, st, want_st))
    finally:
        _set(eng, **DEFAULTS)


def test_refused_arguments_leave_outputs_and_context_alone(eng):
    """k = 0, a NULL input with n > 0, a NULL gt for bn254_batch_pairing and a NULL status for _check are BN254_E_BAD_ARGUMENT, a
    misaligned device pointer is BN254_E_MISALIGNED, n = 0 is a success that writes nothing: all decided on the host before any access"""
    from tests.hip_ctypes import DevBuf
    L, h = eng._lib, eng._h
    g1, g2, _, _, _ = pc.tiled(2, 3, 0)
    pat = b"\xee" * (3 * 384)
    gt, status = ctypes.create_string_buffer(pat, len(pat)), ctypes.create_string_buffer(b"\xee" * 8, 8)
    assert L.bn254_batch_pairing(h, g1, g2, 0, 2, 0, gt, status) == 0
    assert L.bn254_batch_pairing(h, None, None, 0, 2, 0, None, None) == 0
    assert L.bn254_batch_pairing_check(h, g1, g2, 0, 2, 0, status) == 0 and L.bn254_batch_pairing_check(h, None, None, 0, 2, 0, None) == 0
    for flags in (0, 3):
        assert L.bn254_batch_pairing(h, g1, g2, 3, 0, flags, gt, status) == E_BAD_ARGUMENT             # k = 0
        assert L.bn254_batch_pairing_check(h, g1, g2, 3, 0, flags, status) == E_BAD_ARGUMENT
        assert L.bn254_batch_pairing(h, None, g2, 3, 2, flags, gt, status) == E_BAD_ARGUMENT
        assert L.bn254_batch_pairing(h, g1, None, 3, 2, flags, gt, status) == E_BAD_ARGUMENT
        assert L.bn254_batch_pairing(h, g1, g2, 3, 2, flags, None, status) == E_BAD_ARGUMENT
        assert L.bn254_batch_pairing_check(h, None, g2, 3, 2, flags, status) == E_BAD_ARGUMENT
        assert L.bn254_batch_pairing_check(h, g1, None, 3, 2, flags, status) == E_BAD_ARGUMENT
        assert L.bn254_batch_pairing_check(h, g1, g2, 3, 2, flags, None) == E_BAD_ARGUMENT
    assert L.bn254_batch_pairing(None, g1, g2, 3, 2, 0, gt, status) == E_BAD_ARGUMENT
    assert gt.raw == pat and status.raw == b"\xee" * 8
    bufs = []
    try:
        d_g1, d_g2, d_gt, d_st = DevBuf(len(g1) + 4, data=g1), DevBuf(len(g2) + 4, data=g2), DevBuf(3 * 384 + 4, fill=0xEE), DevBuf(8, fill=0xEE)
        bufs += [d_g1, d_g2, d_gt, d_st]
        dev = L.bn254_batch_pairing_device
        for off in (1, 2, 3):
            assert dev(h, d_g1.ptr + off, d_g2.ptr, 3, 2, 0, d_gt.ptr, d_st.ptr, None) == E_MISALIGNED
            assert dev(h, d_g1.ptr, d_g2.ptr + off, 3, 2, 0, d_gt.ptr, d_st.ptr, None) == E_MISALIGNED
            assert dev(h, d_g1.ptr, d_g2.ptr, 3, 2, 0, d_gt.ptr + off, d_st.ptr, None) == E_MISALIGNED
        assert dev(h, d_g1.ptr, d_g2.ptr, 3, 0, 0, d_gt.ptr, d_st.ptr, None) == E_BAD_ARGUMENT
        assert dev(h, None, d_g2.ptr, 3, 2, 0, d_gt.ptr, d_st.ptr, None) == E_BAD_ARGUMENT
        assert dev(h, d_g1.ptr, None, 3, 2, 0, d_gt.ptr, d_st.ptr, None) == E_BAD_ARGUMENT
        assert dev(h, d_g1.ptr, d_g2.ptr, 0, 2, 0, d_gt.ptr, d_st.ptr, None) == 0
        eng.synchronize()
        assert d_gt.download() == b"\xee" * (3 * 384 + 4) and d_st.download() == b"\xee" * 8
    finally:
        for b in bufs:
            b.free()
    _answers_the_case_set(eng)


def test_python_mirrors(eng, c, kats):
    """what bn254_amd/api.py has over these calls (bn254_amd/host/bn254.hpp has nothing over them): the two formatters of
    src/utils.rs:197-239, whose tuples fed back as ONE item of two pairs are a product that is one for a signature that verifies and
    one that is not for another message — statuses and Gt against the oracle's; and PublicKey.from_uncompressed, which decides through
    bn254_batch_pairing_check with the subgroup check"""
    import bn254_amd as bn
    H = bytes.fromhex
    v = kats["sign"][0]
    msg = H(v["message_hex"])
    sk = bn.PrivateKey.try_from(v["private_key"])
    sig, pk = bn.ECDSA.sign(msg, sk), bn.PublicKey.from_private_key(sk)
    be = lambda b: b"".join(b[i:i + 32][::-1] for i in range(0, len(b), 32))     # noqa: E731
    items = []
    for message in (msg, msg + b"!"):
        t = bn.format_pairing_check_values(message, sig.to_compressed(), pk.to_compressed())
        assert t == bn.format_pairing_check_uncompressed_values(message, sig.to_uncompressed(), pk.to_uncompressed())
        items.append((be(t[0][0]) + be(t[1][0]), be(t[0][1]) + be(t[1][1])))
    g1, g2 = b"".join(x[0] for x in items), b"".join(x[1] for x in items)
    want_gt, want_st = c.batch_pairing(g1, g2, 2, 2, 3)
    assert want_st == bytes([0, 9])
    assert eng.batch_pairing_check(g1, g2, 2, 2, flags=3) == want_st and eng.batch_pairing(g1, g2, 2, 2, flags=3) == (want_gt, want_st)
    cs = {x.name: x for x in pc.cases_of(1)}
    assert bn.PublicKey.from_uncompressed(cs["k=1: generic 0"].g2).raw == cs["k=1: generic 0"].g2
    for name, kind in (("k=1: G2 off the subgroup in pair 0", 4), ("k=1: G2 off the twist in pair 0", 4), ("k=1: G2 x.im >= q in pair 0", 6),
                       ("k=1: identity G2 in pair 0", 4)):
        with pytest.raises(bn.Error) as e:
            bn.PublicKey.from_uncompressed(cs[name].g2)
        assert e.value.kind == bn.ErrorKind(kind), name
