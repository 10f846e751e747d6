"""Hash-to-G1 on the device with the case set of tests/hash_cases.py: every message length 0 .. 200, every block edge of the padded stream
with chosen contents, messages up to 2^20 + 1 bytes, and messages whose first passing counter lies beyond every filter round — through
k_hash_direct at every width (whose survivors go on through k_hash_round and k_hash_finish with a multi-block state), the wide schedule at
both widths and three tail group sizes (the tail rebuilds the state per pass), the multi-round schedule, a cut counter budget, offset arrays
that start behind a junk prefix, the bounds check of a declared buffer at its last byte, and through the callers: sign, verify (host,
device, sliced), the keyed verify, aggregates over distinct messages, signer bitmaps, collect, merge and the multi-GPU layer.  Points,
statuses and try counts must be byte-equal to the C oracle's (tests/test_hash_cases.py checks that oracle against the big-integer model on
the same cases).  Run on the MI355X box: -m gpu."""
import ctypes

import pytest

from tests import collect_model, merge_model
from tests import hash_cases as hc
from tests.conftest import ws_default
from tests.datagen import sk_bytes
from tests.test_gpu_hash_schedule import DIRECT_MAX, WIDE_MAX, hash_device

pytestmark = pytest.mark.gpu

N_KEYS = 6
WIDTHS = (4, 8)


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


class Opts:
    def __init__(self, eng, **opts):
        self.eng, self.opts = eng, opts

    def __enter__(self):
        from bn254_amd import engine as E
        for k, v in self.opts.items():
            self.eng.set_option(getattr(E, "OPT_" + k), v)

    def __exit__(self, *exc):
        from bn254_amd import engine as E
        defaults = {"HASH_SCHEDULE": 0, "HASH_WIDE_WIDTH": 0, "HASH_TAIL_CHUNK": ws_default("HASH_TAIL_CHUNK_DEFAULT"), "HASH_MAX_TRIES": 0,
                    "HASH_DIRECT_WIDTH": ws_default("HASH_DIRECT_WIDTH_DEFAULT"), "MAX_CHUNK": 0}
        for k in self.opts:
            self.eng.set_option(getattr(E, "OPT_" + k), defaults[k])


def case_msgs():
    return [x.msg for x in hc.cases()]


@pytest.fixture(scope="module")
def mid_batch():
    """DIRECT_MAX + 1 messages: the case set, then filler — the smallest batch that takes a schedule of rounds"""
    msgs = case_msgs()
    assert len(msgs) < DIRECT_MAX // 4
    return msgs + hc.filler(DIRECT_MAX + 1 - len(msgs))


def hard_items(msgs):
    """(index, tries) of the hard9 / hard17 cases, which stand at the same indices in every batch that begins with the case set"""
    out = [(i, hc.claimed_tries(x)) for i, x in enumerate(hc.cases()) if x.kind in ("hard9", "hard17")]
    assert len(out) == len(hc.HARD9_LENGTHS) + len(hc.HARD17_LENGTHS) and all(msgs[i] == hc.cases()[i].msg for i, _ in out)
    return out


# ---- the direct route ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("width", [32, 16, 4, 1, 0])
def test_direct_route_whole_set_at_every_width(eng, width):
    """one call with every case, the 2^20 + 1 byte message included.  At widths of 16 and below the hard messages find no point in
    k_hash_direct and go through k_hash_round (round 1) and k_hash_finish; width 0 runs the rounds only"""
    msgs = case_msgs() + [hc.huge_case().msg]
    assert len(msgs) <= DIRECT_MAX
    if 0 < width <= 16:
        assert sum(t > width for _, t in hard_items(msgs)) >= (len(hc.HARD17_LENGTHS) if width == 16 else len(hard_items(msgs)))
    with Opts(eng, HASH_DIRECT_WIDTH=width):
        got = eng.batch_hash_to_g1(msgs)
    assert hc.first_difference(msgs, got) is None, width


@pytest.mark.parametrize("width", [32, 4])
def test_direct_route_single_item_calls_at_every_boundary_length(eng, width):
    singles = [x.msg for x in hc.caller_set() if len(x.msg) in hc.BOUNDARY]
    assert {len(m) for m in singles} == set(hc.BOUNDARY) and len(singles) >= 2 * len(hc.BOUNDARY) - 1
    with Opts(eng, HASH_DIRECT_WIDTH=width):
        for m in singles:
            pts, st, tries = eng.batch_hash_to_g1([m])
            assert (st[0], pts, tries[0]) == hc.expected(m), (width, len(m))


# ---- the wide schedule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [2, 4, 32])
@pytest.mark.parametrize("w0", WIDTHS)
def test_wide_schedule_every_item(eng, mid_batch, w0, chunk):
    """the hard messages survive the round (first passing counter >= its width) and are found by the tail, whose groups of 2 and 4 counters
    take several passes, each with the state rebuilt from a message of more than one block"""
    for i, tries in hard_items(mid_batch):
        assert tries - 1 >= w0, (i, tries)                       # counters 0 .. w0 - 1 belong to the round
    with Opts(eng, HASH_SCHEDULE=2, HASH_WIDE_WIDTH=w0, HASH_TAIL_CHUNK=chunk):
        got = eng.batch_hash_to_g1(mid_batch)
    assert hc.first_difference(mid_batch, got) is None, (w0, chunk)


# ---- the multi-round schedule --------------------------------------------------------------------------------------------------------------
def test_multi_round_schedule_every_item(eng, mid_batch):
    with Opts(eng, HASH_SCHEDULE=1):
        got = eng.batch_hash_to_g1(mid_batch)
    assert hc.first_difference(mid_batch, got) is None


def test_three_schedules_above_the_wide_bound(eng):
    """WIDE_MAX + 1 messages: by size (the multi-round schedule), forced multi-round, forced wide — equal, every case and every 97th filler
    message against the oracle"""
    cs = case_msgs()
    msgs = cs + hc.filler(WIDE_MAX + 1 - len(cs))
    got = {}
    for sched in (0, 1, 2):
        with Opts(eng, HASH_SCHEDULE=sched):
            got[sched] = eng.batch_hash_to_g1(msgs)
    assert got[0] == got[1] == got[2]
    only = list(range(len(cs))) + list(range(len(cs), len(msgs), 97))
    assert len(only) > len(cs) + 300
    assert hc.first_difference(msgs, got[0], only=only) is None


# ---- the counter budget --------------------------------------------------------------------------------------------------------------------
ROUTES = [("direct", {}), ("direct 4", {"HASH_DIRECT_WIDTH": 4}), ("rounds", {"HASH_DIRECT_WIDTH": 0}),
          ("wide", {"HASH_SCHEDULE": 2, "HASH_WIDE_WIDTH": 4, "HASH_TAIL_CHUNK": 2}), ("multi-round", {"HASH_SCHEDULE": 1})]


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_counter_budget_of_eight(eng, mid_batch, route):
    """BN254_OPT_HASH_MAX_TRIES = 8: every hard message reports HashToPointError, no point and 8 tries at its multi-block length; every other
    item is what it was (or fails the same way if it needs more than eight tries itself)"""
    name, opts = route
    msgs = case_msgs() if name.startswith(("direct", "rounds")) else mid_batch
    with Opts(eng, HASH_MAX_TRIES=8, **opts):
        pts, st, tries = got = eng.batch_hash_to_g1(msgs)
    for i, _ in hard_items(msgs):
        assert (st[i], pts[64 * i:64 * i + 64], tries[i]) == (1, bytes(64), 8), (name, i, len(msgs[i]))
    assert hc.first_difference(msgs, got, max_tries=8) is None, name
    unchanged = sum(hc.expected(m, 8) == hc.expected(m) for m in msgs)
    assert st.count(0) == unchanged >= len(msgs) - len(hard_items(msgs)) - len(msgs) // 50      # 0.5274^8 = 0.6 % of ordinary messages fail too


# ---- offsets -------------------------------------------------------------------------------------------------------------------------------
def host_hash_raw(eng, blob, offs):
    """bn254_batch_hash_to_g1 on the caller's own offsets array"""
    n = len(offs) - 1
    off = (ctypes.c_uint64 * (n + 1))(*offs)
    pts, st, tries = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n), ctypes.create_string_buffer(n)
    assert eng._lib.bn254_batch_hash_to_g1(eng._h, blob, off, n, pts, st, tries) == 0
    return pts.raw, st.raw, tries.raw


@pytest.mark.parametrize("route", ROUTES[:1] + ROUTES[2:], ids=[r[0] for r in ROUTES[:1] + ROUTES[2:]])
def test_offsets_that_start_behind_a_junk_prefix(eng, mid_batch, route):
    """msg_off[0] = 13 (include/bn254_hip.h): the host entry and the device entry give what the plain call gives"""
    name, opts = route
    msgs = case_msgs() if name in ("direct", "rounds") else mid_batch
    blob, offs = hc.pack(msgs)
    assert offs[0] == 13
    with Opts(eng, **opts):
        plain = eng.batch_hash_to_g1(msgs)
        assert host_hash_raw(eng, blob, offs) == plain, name
        assert hash_device(eng, blob, offs) == plain, name
        assert hash_device(eng, blob, offs, msgs_len=len(blob)) == plain, name
    assert hc.first_difference(msgs, plain) is None, name


@pytest.mark.parametrize("route", ROUTES[:1] + ROUTES[2:], ids=[r[0] for r in ROUTES[:1] + ROUTES[2:]])
def test_declared_buffer_size_at_the_last_byte(eng, mid_batch, route):
    """bn254_ctx_expect_msgs_len = the exact size, the last message ending at the buffer's last byte: everything hashes, a trailing empty
    message at hi == msgs_len included.  One byte less: the last message reports InvalidLength with zero tries and no point, and nothing
    else changes; a trailing empty message then lies past the declared size as well (offsets <= msgs_len is the header's rule)"""
    name, opts = route
    msgs = list(case_msgs() if name in ("direct", "rounds") else mid_batch)
    msgs += [b"", hc.message("hash-cases/last", 0, 119)]          # an empty message in FRONT of the last one: its span stays inside
    n = len(msgs)
    blob, offs = hc.pack(msgs)
    trailing = offs + [offs[-1]]
    with Opts(eng, **opts):
        exact = hash_device(eng, blob, offs, msgs_len=len(blob))
        exact_trailing = hash_device(eng, blob, trailing, msgs_len=len(blob))
        short = hash_device(eng, blob, offs, msgs_len=len(blob) - 1)
        short_trailing = hash_device(eng, blob, trailing, msgs_len=len(blob) - 1)
    assert hc.first_difference(msgs, exact) is None, name
    assert hc.first_difference(msgs + [b""], exact_trailing) is None and exact_trailing[1][n] == 0, name
    for got, ms, bad in ((short, msgs, {n - 1}), (short_trailing, msgs + [b""], {n - 1, n})):
        pts, st, tries = got
        assert {i for i in range(len(st)) if st[i] == 5} == bad, name
        for i in bad:
            assert (tries[i], pts[64 * i:64 * i + 64]) == (0, bytes(64)), (name, i)
        assert hc.first_difference(ms, got, only=range(n - 1)) is None, name


# ---- the callers ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def keys(c):
    sks = [sk_bytes(4200 + j) for j in range(N_KEYS)]
    return sks, [c.public_key_g2(sk) for sk in sks]


_SIG = {}


def sig_of(c, keys, msg, j):
    if (msg, j) not in _SIG:
        _SIG[msg, j] = c.sign(msg, keys[0][j % N_KEYS])
    return _SIG[msg, j]


def S():
    return [x.msg for x in hc.caller_set()]


@pytest.fixture(scope="module")
def verify_batch(c, keys):
    """(messages, signatures, key indices, expected statuses): S under key i % 6 with every eighth item carrying its neighbour's signature;
    then, for every boundary length, m with its own signature and m's signature under m || 0x00 and under m[:-1]"""
    msgs, sigs, idx, want = [], [], [], []
    s = S()
    for i, m in enumerate(s):
        bad = i % 8 == 7
        msgs.append(m); idx.append(i % N_KEYS); want.append(9 if bad else 0)
        sigs.append(sig_of(c, keys, s[i - 1], (i - 1) % N_KEYS) if bad else sig_of(c, keys, m, i))
    seen = set()
    for k, (m, other) in enumerate(hc.contents_pairs()):
        if m not in seen:
            seen.add(m)
            msgs.append(m); idx.append(k % N_KEYS); want.append(0); sigs.append(sig_of(c, keys, m, k))
        msgs.append(other); idx.append(k % N_KEYS); want.append(9); sigs.append(sig_of(c, keys, m, k))
    pks = b"".join(keys[1][j] for j in idx)
    oracle, _ = c.batch_verify(msgs, b"".join(sigs), pks, flags=0, nthreads=16)
    assert oracle == bytes(want) and 100 <= len(msgs) <= 140
    return msgs, b"".join(sigs), idx, bytes(want)


def test_batch_sign_vs_the_oracle(eng, c, keys):
    s = S()
    pairs = [(m, (i + d) % N_KEYS) for i, m in enumerate(s) for d in range(2)]
    sigs, st = eng.batch_sign([m for m, _ in pairs], b"".join(keys[0][j] for _, j in pairs))
    assert st == bytes(len(pairs))
    for k, (m, j) in enumerate(pairs):
        assert sigs[64 * k:64 * k + 64] == sig_of(c, keys, m, j), (k, len(m))


def test_batch_verify_host_device_single_and_sliced(eng, c, keys, verify_batch):
    from tests.test_gpu_key_dedup import verify_device
    msgs, sigs, idx, want = verify_batch
    pks = b"".join(keys[1][j] for j in idx)
    assert eng.batch_verify(msgs, sigs, pks) == want
    assert verify_device(eng, msgs, sigs, pks, 0) == want
    with Opts(eng, MAX_CHUNK=16):                                  # slices that start at non-zero, ragged offsets
        assert eng.batch_verify(msgs, sigs, pks) == want
    picked = [i for i, m in enumerate(msgs) if len(m) in (55, 64, 128, 65537)] + [7, len(msgs) - 1]
    assert {want[i] for i in picked} == {0, 9}
    for i in picked:
        assert eng.batch_verify([msgs[i]], sigs[64 * i:64 * i + 64], pks[128 * i:128 * i + 128]) == want[i:i + 1], (i, len(msgs[i]))


def test_keyed_verify_and_distinct_message_aggregates(eng, c, keys, verify_batch):
    msgs, sigs, idx, want = verify_batch
    n = len(msgs)
    assert eng.register_keys(b"".join(keys[1])) == bytes(N_KEYS)
    assert eng.batch_verify_keyed(msgs, sigs, idx) == want
    with Opts(eng, MAX_CHUNK=16):
        assert eng.batch_verify_keyed(msgs, sigs, idx) == want
    sizes = [4] * (n // 4) + ([n % 4] if n % 4 else [])
    seg = [0]
    for k in sizes:
        seg.append(seg[-1] + k)
    agg = []
    for i in range(len(sizes)):
        acc = bytes(64)
        for j in range(seg[i], seg[i + 1]):
            acc = c.g1_add(acc, sigs[64 * j:64 * j + 64])
        agg.append(acc)
    want_agg = bytes(9 if any(want[seg[i]:seg[i + 1]]) else 0 for i in range(len(sizes)))
    assert want_agg.count(0) >= 5 and want_agg.count(9) >= 10
    pks = b"".join(keys[1][j] for j in idx)
    assert eng.batch_aggregate_verify_distinct(msgs, pks, b"".join(agg), sizes) == want_agg


def _sum_g1(c, pts):
    acc = bytes(64)
    for p in pts:
        acc = c.g1_add(acc, p)
    return acc


def _sum_pk(c, keys, row):
    acc = None
    for j in row:
        acc = keys[1][j] if acc is None else c.g2_add(acc, keys[1][j])
    return acc


def test_signer_bitmaps(eng, c, keys):
    """one tuple per message of S, signed by keys i and i + 1; every eighth carries its neighbour's aggregate"""
    s = S()
    assert eng.register_keys(b"".join(keys[1])) == bytes(N_KEYS)
    rows = [[i % N_KEYS, (i + 1) % N_KEYS] for i in range(len(s))]
    good = [_sum_g1(c, [sig_of(c, keys, m, j) for j in rows[i]]) for i, m in enumerate(s)]
    sigs = [good[i - 1] if i % 8 == 7 else good[i] for i in range(len(s))]
    want, _ = c.batch_verify(s, b"".join(sigs), b"".join(_sum_pk(c, keys, r) for r in rows), flags=0, nthreads=16)
    assert want == bytes(9 if i % 8 == 7 else 0 for i in range(len(s)))
    bitmaps = [sum(1 << j for j in r) for r in rows]
    assert eng.batch_verify_keyed_bitmap(s, b"".join(sigs), bitmaps, 1) == want


def test_collect_and_merge(eng, c, keys):
    """one message of S per tuple, three shares / three partials each; in every fourth tuple the middle one belongs to the tuple before.  The
    share and partial statuses come from the oracle's verify, the rows, counts and taken flags from tests/collect_model.py and
    tests/merge_model.py, the aggregates from the oracle's additions"""
    s = S()
    n = len(s)
    assert eng.register_keys(b"".join(keys[1])) == bytes(N_KEYS)
    # collect
    share_keys = [(i + d) % N_KEYS for i in range(n) for d in range(3)]
    shares = [sig_of(c, keys, s[i - 1] if (i % 4 == 3 and d == 1) else s[i], i + d) for i in range(n) for d in range(3)]
    rep = [m for m in s for _ in range(3)]
    want, _ = c.batch_verify(rep, b"".join(shares), b"".join(keys[1][j] for j in share_keys), flags=0, nthreads=16)
    assert want == bytes(9 if (i % 4 == 3 and d == 1) else 0 for i in range(n) for d in range(3))
    rows, counts, chosen = collect_model.select(share_keys, want, [3] * n, bytes(n), 1)
    agg = b"".join(collect_model.aggregates(c, shares, chosen))
    for opts in ({}, {"MAX_CHUNK": 16}):
        with Opts(eng, **opts):
            got = eng.batch_collect_keyed_bitmap(s, b"".join(shares), share_keys, [3] * n, 1, want_counts=True)
        assert got == (want, bytes(n), agg, [w for r in rows for w in r], counts), opts
    assert eng.batch_verify_keyed_bitmap(s, agg, [r[0] for r in rows], 1) == bytes(n)
    # merge: partials signed by {i}, {i + 1, i + 2}, {i + 3}
    part_keys = [[[i % N_KEYS], [(i + 1) % N_KEYS, (i + 2) % N_KEYS], [(i + 3) % N_KEYS]] for i in range(n)]
    good = [[_sum_g1(c, [sig_of(c, keys, s[i], j) for j in r]) for r in part_keys[i]] for i in range(n)]
    parts = [good[i - 1][1] if (i % 4 == 3 and d == 1) else good[i][d] for i in range(n) for d in range(3)]
    flat_rows = [[sum(1 << j for j in r)] for t in part_keys for r in t]
    want, _ = c.batch_verify(rep, b"".join(parts), b"".join(_sum_pk(c, keys, r) for t in part_keys for r in t), flags=0, nthreads=16)
    assert want == bytes(9 if (i % 4 == 3 and d == 1) else 0 for i in range(n) for d in range(3))
    rows, counts, taken = merge_model.select(flat_rows, want, [3] * n, bytes(n), 1)
    agg = b"".join(merge_model.aggregates(c, parts, [3] * n, taken))
    got = eng.merge_keyed_bitmap(s, b"".join(parts), [w for r in flat_rows for w in r], [3] * n, 1, want_counts=True)
    assert got == (want, bytes(taken), bytes(n), agg, [w for r in rows for w in r], counts)
    assert eng.batch_verify_keyed_bitmap(s, agg, [r[0] for r in rows], 1) == bytes(n)


def test_multi_gpu_layer_four_contexts_on_one_gpu():
    """bn254_mgpu_batch_hash_to_g1: every shard's offsets start in the middle of the buffer"""
    import bn254_amd
    mg4 = bn254_amd.MultiEngine([0, 0, 0, 0])
    try:
        msgs = case_msgs()
        assert hc.first_difference(msgs, mg4.batch_hash_to_g1(msgs)) is None
    finally:
        mg4.close()
