"""Hash-to-G1 schedules of launch_hash_rounds (BN254_OPT_HASH_SCHEDULE): 1 = the multi-round filter schedule, 2 = one wide filter round, then
k_hash_finish_tail (the square roots of the decided messages and, in lane groups beside them, every remaining counter of the round's
survivors).  Points, statuses and try counts must be byte-equal under both and equal to the oracle's: at the sizes around every route bound,
for planted messages whose first passing counter lies beyond the wide round (found by a deterministic search with the oracle), with the tail's
group width cut to 2 and 4 so that its loop runs more than once, with the counter budget cut below / at / above the round's width, for offset
pairs that are reversed or run past the buffer, on a caller's stream, and through the verify-shaped entry points."""
import pytest

from tests.conftest import ws_default
from tests.datagen import D, sk_bytes

pytestmark = pytest.mark.gpu



def _size_default(name):
    """`#define <name> ((size_t)<integer>)` of bn254_ws.h"""
    import os
    import re
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bn254_amd", "csrc", "bn254_ws.h")).read()
    m = re.search(r"#define\s+%s\s+\(\(size_t\)(\d+)\)" % name, text)
    assert m, name
    return int(m.group(1))


DIRECT_MAX = _size_default("HASH_DIRECT_MAX_N")
WIDE_MAX = _size_default("HASH_WIDE_MAX_N")
SEARCH = 150000          # oracle calls of the search: 3.6e-5 of the messages need 17 tries or more -> about five of them
WIDTHS = (4, 8)          # forced widths of the wide round (BN254_OPT_HASH_WIDE_WIDTH); 0 = the width the library picks by size


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


_WANT = {}


def want_of(c, m):
    if m not in _WANT:
        _WANT[m] = c.hash_to_g1(m)
    return _WANT[m]


@pytest.fixture(scope="module")
def hard(c):
    """messages D(tag, i) by the number of tries the oracle needs: {tries: [messages]} for tries >= 5"""
    by_tries = {}
    for i in range(SEARCH):
        m = D("hash-sched/hard", i)
        w = c.hash_to_g1(m)
        if w[2] >= 5:
            _WANT[m] = w
            by_tries.setdefault(w[2], []).append(m)
    return by_tries


def at_least(hard, tries, cap=6):
    """up to `cap` messages per try count whose first passing counter is >= tries - 1"""
    return [m for t in sorted(hard) if t >= tries for m in hard[t][:cap]]


def test_the_search_finds_every_kind(hard):
    for w0 in WIDTHS:
        assert len(at_least(hard, w0 + 1)) >= 3 and len(at_least(hard, w0 + 3)) >= 3, w0     # first passing counter >= W0, >= W0 + 2
    assert len(at_least(hard, 17)) >= 3                                                        # ... >= 16


def filler(n):
    return [D("hash-sched", i)[: 1 + i % 32] for i in range(n)]


class Opts:
    def __init__(self, eng, **opts):
        self.eng, self.opts = eng, opts

    def __enter__(self):
        from bn254_amd import engine as E
        for k, v in self.opts.items():
            self.eng.set_option(getattr(E, "OPT_" + k), v)

    def __exit__(self, *exc):
        from bn254_amd import engine as E
        defaults = {"HASH_SCHEDULE": 0, "HASH_WIDE_WIDTH": 0, "HASH_TAIL_CHUNK": ws_default("HASH_TAIL_CHUNK_DEFAULT"), "HASH_MAX_TRIES": 0}
        for k in self.opts:
            self.eng.set_option(getattr(E, "OPT_" + k), defaults[k])


def hash_device(eng, blob, offs, stream=None, msgs_len=None):
    """bn254_batch_hash_to_g1_device on raw offsets -> (points, statuses, tries)"""
    import torch
    n = len(offs) - 1
    d_msgs = torch.frombuffer(bytearray(blob or b"\0"), dtype=torch.uint8).to("cuda:0")
    d_off = torch.tensor(offs, dtype=torch.int64, device="cuda:0")
    d_pts = torch.full((n * 64,), 0xEE, dtype=torch.uint8, device="cuda:0")
    d_st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda:0")
    d_tr = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    if msgs_len is not None:
        eng.expect_msgs_len(msgs_len)
    eng.batch_hash_to_g1_device(d_msgs.data_ptr(), d_off.data_ptr(), n, d_pts.data_ptr(), d_st.data_ptr(), d_tr.data_ptr(),
                                stream=None if stream is None else stream.cuda_stream)
    if stream is not None:
        stream.synchronize()
    eng.synchronize()
    return bytes(d_pts.cpu().numpy()), bytes(d_st.cpu().numpy()), bytes(d_tr.cpu().numpy())


def check(c, msgs, got, what, max_tries=255):
    pts, st, tries = got
    for i, m in enumerate(msgs):
        wst, wpt, wtries = want_of(c, m)
        if wtries > max_tries:
            wst, wpt, wtries = 1, bytes(64), max_tries          # hash.rs:62: HashToPointError
        assert (st[i], pts[64 * i:64 * i + 64], tries[i]) == (wst, wpt, wtries), (what, i)


@pytest.mark.parametrize("n", sorted({DIRECT_MAX + 1, 8192, 16385, 65536, WIDE_MAX, WIDE_MAX + 1}))
def test_schedules_agree_with_each_other_and_the_oracle(eng, c, hard, n):
    msgs = (at_least(hard, 9, cap=2) + filler(n))[:n]
    got = {}
    for sched in (0, 1, 2):
        with Opts(eng, HASH_SCHEDULE=sched):
            got[sched] = eng.batch_hash_to_g1(msgs)
    assert got[1] == got[2] == got[0], n
    check(c, msgs, got[2], n)


@pytest.mark.parametrize("chunk", [2, 4, 32])
@pytest.mark.parametrize("w0", WIDTHS + (0,))
def test_planted_hard_messages_and_the_tail_loop(eng, c, hard, w0, chunk):
    """the survivors of the wide round: first passing counter >= W0, >= W0 + 2 and >= 16 — with groups of 2 and 4 counters the latter need
    up to seven passes of the tail's loop"""
    n = 8192
    msgs = filler(n)
    planted = at_least(hard, 5)
    assert len(at_least(hard, 17)) >= 3
    for k, m in enumerate(planted):
        msgs[(k * 131) % n] = m
    with Opts(eng, HASH_SCHEDULE=2, HASH_WIDE_WIDTH=w0, HASH_TAIL_CHUNK=chunk):
        got = eng.batch_hash_to_g1(msgs)
    check(c, msgs, got, (w0, chunk))
    with Opts(eng, HASH_SCHEDULE=1):
        assert eng.batch_hash_to_g1(msgs) == got, (w0, chunk)


@pytest.mark.parametrize("w0", WIDTHS)
def test_counter_budget_around_the_round_width(eng, c, hard, w0):
    n = 8192
    msgs = filler(n)
    for k, m in enumerate(at_least(hard, 5)):
        msgs[(k * 131) % n] = m
    failed = 0
    for max_tries in (1, 2, w0 - 1, w0, w0 + 1, 40):
        for chunk in (4, 32):
            with Opts(eng, HASH_SCHEDULE=2, HASH_WIDE_WIDTH=w0, HASH_TAIL_CHUNK=chunk, HASH_MAX_TRIES=max_tries):
                got = eng.batch_hash_to_g1(msgs)
            check(c, msgs, got, (w0, max_tries, chunk), max_tries=max_tries)
            with Opts(eng, HASH_SCHEDULE=1, HASH_MAX_TRIES=max_tries):
                assert eng.batch_hash_to_g1(msgs) == got, (w0, max_tries, chunk)
        failed += got[1].count(1)
    assert failed > n // 2                 # a budget of one counter alone fails 52.7 % of the messages


@pytest.mark.parametrize("declared", [False, True])
@pytest.mark.parametrize("on_stream", [False, True])
def test_bad_offset_pairs_and_streams(eng, c, hard, declared, on_stream):
    """reversed pairs (always caught) and pairs past the declared buffer (caught with bn254_ctx_expect_msgs_len): InvalidLength, zero tries,
    no point, never dereferenced; the neighbours' results untouched.  On the context's stream and on a caller's."""
    import torch
    n = 8192
    msgs = filler(n)
    for k, m in enumerate(at_least(hard, 9, cap=2)):
        msgs[(k * 131) % n] = m
    blob = b"".join(msgs)
    offs = [0]
    for m in msgs:
        offs.append(offs[-1] + len(m))
    # item 100: reversed pair through its right neighbour's start; item 7000 .. the end: far past the buffer
    offs_bad = list(offs)
    offs_bad[101] = offs_bad[100] - 1 if offs_bad[100] else 0
    reversed_items = {100} if offs_bad[101] < offs_bad[100] else set()
    past = set()
    if declared:
        offs_bad[n] = len(blob) + (1 << 40)
        past = {n - 1}
    stream = torch.cuda.Stream(device="cuda:0") if on_stream else None
    results = {}
    for sched in (1, 2):
        for chunk in (4, 32):
            with Opts(eng, HASH_SCHEDULE=sched, HASH_WIDE_WIDTH=4, HASH_TAIL_CHUNK=chunk):
                results[sched, chunk] = hash_device(eng, blob, offs_bad, stream=stream, msgs_len=len(blob) if declared else None)
    assert len(set(results.values())) == 1
    pts, st, tries = results[2, 32]
    assert reversed_items
    for i in range(n):
        if i in reversed_items or i in past:
            assert (st[i], tries[i], pts[64 * i:64 * i + 64]) == (5, 0, bytes(64)), i
        elif i == 101:                                          # its own start moved one byte to the left: another (valid) message
            m = blob[offs_bad[101]:offs_bad[102]]
            assert (st[i], pts[64 * i:64 * i + 64], tries[i]) == c.hash_to_g1(m), i
        else:
            assert (st[i], pts[64 * i:64 * i + 64], tries[i]) == want_of(c, msgs[i]), i


def _signed_batch(eng, hard, n, pool):
    sks = [sk_bytes(7000 + j) for j in range(pool)]
    pk, st = eng.batch_g2_mul(None, b"".join(sks), pool, reduce_scalar=True)
    assert st == bytes(pool)
    msgs = filler(n)
    for k, m in enumerate(at_least(hard, 9, cap=2)):
        msgs[(k * 131) % n] = m
    sigs, st = eng.batch_sign(msgs, b"".join(sks[i % pool] for i in range(n)))
    assert st == bytes(n)
    sigs = bytearray(sigs)
    good = bytes(sigs)
    for i in range(63, n, 64):                                   # the 1/64 corrupted pattern: the neighbour's signature
        sigs[64 * i:64 * i + 64] = good[64 * (i - 1):64 * i]
    return msgs, bytes(sigs), pk, [i % pool for i in range(n)]


def test_verify_entry_points_under_both_schedules(eng, c, hard):
    """bn254_batch_verify_device (key dedup route), the keyed verify and the aggregate verify over distinct messages: schedule 2 == schedule 1
    == the oracle, hard messages among the items"""
    from tests.test_gpu_key_dedup import verify_device
    n, pool = 16385, 256
    msgs, sigs, pk, idx = _signed_batch(eng, hard, n, pool)
    pks = b"".join(pk[128 * j:128 * j + 128] for j in idx)
    want, _ = c.batch_verify(msgs, sigs, pks, flags=0, nthreads=16)
    assert want.count(9) == n // 64 and want.count(0) == n - n // 64
    assert eng.register_keys(pk) == bytes(pool)
    sizes = [4] * (n // 4) + ([n % 4] if n % 4 else [])
    seg = [0]
    for k in sizes:
        seg.append(seg[-1] + k)
    agg_sigs, st = eng.batch_g1_sum(sigs, seg)
    assert st == bytes(len(sizes))
    want_agg = bytes(9 if any(want[j] for j in range(seg[i], seg[i + 1])) else 0 for i in range(len(sizes)))
    got = {}
    for sched in (1, 2):
        with Opts(eng, HASH_SCHEDULE=sched, HASH_WIDE_WIDTH=4 if sched == 2 else 0):
            got[sched] = (verify_device(eng, msgs, sigs, pks, 0), eng.batch_verify_keyed(msgs, sigs, idx), eng.batch_aggregate_verify_distinct(msgs, pks, agg_sigs, sizes))
            assert verify_device.route["keyed_n"] == n
    assert got[1] == got[2]
    assert got[2][0] == want and got[2][1] == want
    assert got[2][2] == want_agg
