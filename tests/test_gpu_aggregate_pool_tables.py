"""The subset-sum tables of the aggregate verify's registered pools as they stand ON THE DEVICE, read back entry by entry through
bn254_debug_agg_tables and compared with the oracle's sums of the selected signers (tests/pooltab_cases.py: pools of 5, 8, 16, 17 and 43
signers over two messages; the 43-signer pool plants equal and opposite points, and sums equal to keys and to other sums, at every level
where two operands of a builder meet).  Every entry and every identity flag of every table — T8 keys, T2, T4, T8 signatures, T16 keys (by
chunk: 65 536 entries each) —, both builders of the 4-signer signature tables (BN254_OPT_AGG_T4_ROUTE), the aggregation kernel's walk over
every mask of a full and of a partial window with narrow and with widened tables against c_oracle.batch_aggregate_verify, and the hook's
refusals.  A context of its own; nothing runs at the workload's size.  Run on the MI355X box: -m gpu."""
import pytest

from bn254_amd import engine as E
from tests import pooltab_cases as pc
from tests.conftest import ws_default

pytestmark = pytest.mark.gpu

BAD_ARGUMENT = -10001
EXPECT = 1 << 20                       # tuples the registration is told to expect: every table's threshold is met


@pytest.fixture(scope="module")
def eng():
    e = E.Engine(0)
    e.set_option(E.OPT_AGG_SUBSET_MIN_TUPLES, 1)
    e.set_option(E.OPT_AGG_WIDE_MIN_TUPLES, 1)
    yield e
    e.close()


def register(eng, S, t4_route=0, wide=True):
    """-> the query form's answer after registering the pool of S signers"""
    P = pc.pool(S)
    eng.set_option(E.OPT_AGG_T4_ROUTE, t4_route)
    eng.set_option(E.OPT_AGG_WIDE_MIN_TUPLES, 1 if wide else 0)
    try:
        eng.register_pools(pc.MESSAGES, P.pk_pool, P.sig_pool, EXPECT)
    finally:
        eng.set_option(E.OPT_AGG_T4_ROUTE, 0)
        eng.set_option(E.OPT_AGG_WIDE_MIN_TUPLES, 1)
    info = eng.debug_agg_tables_info()
    assert info["n_groups"] == P.n_groups and info["groups4"] == P.groups4
    assert info["wide2"] == info["wide1"] == (1 if wide else 0) and info["t4_builder"] == (2 if t4_route else 1), info
    return info


def check_window(eng, S, table, w, m=0):
    which, W, g2 = pc.TABLES[table]
    want_pts, want_fl = pc.expected(S, table, w, m)
    got_pts, got_fl = eng.debug_agg_tables(which, pc.entry_base(S, table, w, m), 1 << W)
    assert got_fl == want_fl, (S, table, m, w)
    if got_pts != want_pts:
        size = 128 if g2 else 64
        bad = [i for i in range(1 << W) if got_pts[size * i:size * (i + 1)] != want_pts[size * i:size * (i + 1)]]
        raise AssertionError((S, table, m, w, len(bad), bad[:8]))


def check_tables(eng, S, tables):
    P = pc.pool(S)
    for table in tables:
        g2 = pc.TABLES[table][2]
        for m in range(1 if g2 else pc.M):
            for w in range(P.windows(table)):
                check_window(eng, S, table, w, m)


@pytest.mark.parametrize("S", pc.SIZES)
def test_every_entry_of_the_narrow_and_signature_tables(eng, S):
    """all five tables exist (the query form says so); the decoded pools, T8 keys, T2, T4 and T8 signatures, every entry and flag"""
    register(eng, S)
    P = pc.pool(S)
    fk, fs = P.decoded_flags()
    pts, fl = eng.debug_agg_tables(0, 0, S)
    assert fl == fk and all(pts[128 * j:128 * j + 128] == P.pks[j] for j in range(S) if fk[j] == 0)
    pts, fl = eng.debug_agg_tables(1, 0, pc.M * S)
    assert fl == fs and all(pts[64 * j:64 * j + 64] == P.sigs[j // S][j % S] for j in range(pc.M * S) if fs[j] == 0)
    check_tables(eng, S, ("T8k", "T2", "T4", "T8s"))
    # the last entry of every table is in range, the one behind it is not
    for table in pc.TABLES:
        which, W, g2 = pc.TABLES[table]
        total = ((1 if g2 else pc.M) * P.windows(table)) << W
        eng.debug_agg_tables(which, total - 1, 1)
        with pytest.raises(E.NativeError) as err:
            eng.debug_agg_tables(which, total - 1, 2)
        assert err.value.rc == BAD_ARGUMENT


T16_CHUNKS = [(S, k) for S in pc.SIZES for k in range((((S + 7) // 8) + 1) // 2)]


@pytest.mark.parametrize("S,chunk", T16_CHUNKS)
def test_every_entry_of_the_16_signer_key_table(eng, S, chunk):
    """T16, one chunk of 65 536 entries per case — every (hi, lo) pair, not the few a batch of tuples happens to read"""
    register(eng, S)
    check_window(eng, S, "T16", chunk)


@pytest.mark.parametrize("S", [17, 43])
def test_both_builders_of_the_4_signer_tables(eng, S):
    """BN254_OPT_AGG_T4_ROUTE = 1: T4 from k_pool_subsets_g1 (otherwise only the fallback when the pair table cannot be allocated) equals
    the default route's and the oracle's, and so does T8 built on top of it; the pair table is then not there to read"""
    P = pc.pool(S)
    n4, n8 = pc.M * P.groups4 * 16, pc.M * P.n_groups * 256
    register(eng, S, t4_route=0)
    quads = eng.debug_agg_tables(4, 0, n4), eng.debug_agg_tables(6, 0, n8)
    register(eng, S, t4_route=1)
    with pytest.raises(E.NativeError) as err:
        eng.debug_agg_tables(7, 0, 1)
    assert err.value.rc == BAD_ARGUMENT
    assert (eng.debug_agg_tables(4, 0, n4), eng.debug_agg_tables(6, 0, n8)) == quads
    check_tables(eng, S, ("T4", "T8s"))


@pytest.mark.parametrize("wide", [False, True])
def test_walk_over_every_mask_of_a_window(eng, wide):
    """through the aggregation kernel: 256 tuples that enumerate every mask of window 0 (the duplicated signers 0, 1, the cancelling 2, 3, the
    planted sums) and 256 for the partial last window (bits that name no signer: IndexOutOfBounds), on the narrow tables and on the
    widened ones, against the oracle's statuses"""
    from oracle import c_oracle as c
    S = 43
    P = pc.pool(S)
    register(eng, S, wide=wide)
    tuple_msg, lists = [], []
    for window in (0, P.n_groups - 1):
        tm, ls = pc.walk_tuples(S, window)
        tuple_msg += tm
        lists += ls
    off, flat = [0], []
    for lst in lists:
        flat += lst
        off.append(len(flat))
    want = c.batch_aggregate_verify(pc.MESSAGES, P.pk_pool, P.sig_pool, tuple_msg, off, flat, flags=0, nthreads=8)
    got = eng.batch_aggregate_verify_registered(tuple_msg, lists)
    assert got == want, [(i, got[i], want[i]) for i in range(len(want)) if got[i] != want[i]][:10]
    assert want.count(0) >= 200 and 2 in want                               # the cases are not all failures


def test_the_hook_refuses_what_it_cannot_serve():
    e = E.Engine(0)
    try:
        def refused(which, first, count):
            with pytest.raises(E.NativeError) as err:
                e.debug_agg_tables(which, first, count)
            assert err.value.rc == BAD_ARGUMENT
        P = pc.pool(8)
        with pytest.raises(E.NativeError) as err:                           # before any registration
            e.debug_agg_tables_info()
        assert err.value.rc == BAD_ARGUMENT
        refused(0, 0, 1)
        e.register_pools(pc.MESSAGES, P.pk_pool, P.sig_pool, 1)             # one tuple expected: the pools only, no table
        assert e.debug_agg_tables_info() == dict(n_groups=0, groups4=0, wide2=0, wide1=0, t4_builder=0)
        assert e.debug_agg_tables(0, 0, 8)[0] == P.pk_pool and len(e.debug_agg_tables(2, 0, pc.M)[0]) == 64 * pc.M
        for which in (3, 4, 5, 6, 7):
            refused(which, 0, 1)
        refused(0, 8, 1)
        refused(0, 0, 9)
        import ctypes
        one = ctypes.create_string_buffer(64)                               # first + count wraps: refused before anything is read or written
        assert e._lib.bn254_debug_agg_tables(e._h, 1, 2 ** 63, 2 ** 63, one, one) == BAD_ARGUMENT
        assert e._lib.bn254_debug_agg_tables(e._h, 1, 1, 2 ** 64 - 1, one, one) == BAD_ARGUMENT
        refused(8, 0, 1)
        # a call with raw pools overwrites the context's pool buffers: the registration, and with it the hook's answer, is gone
        st = e.batch_aggregate_verify(pc.MESSAGES, P.pk_pool, P.sig_pool, [0], [[0, 1]])
        assert st == bytes(1)
        refused(0, 0, 1)
        with pytest.raises(E.NativeError):
            e.debug_agg_tables_info()
        assert ws_default("AGG_SUBSET_MIN_TUPLES_DEFAULT") > 1              # why the registration above built no table
    finally:
        e.close()
