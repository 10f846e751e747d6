"""Compressed G1 signatures on the registered-key calls (include/bn254_hip.h: BN254_FLAG_G1_COMPRESSED) and
bn254_batch_g1_decompress_device, on the GPU.  Every call is held to the header's defining identity: with the flag it returns, byte for
byte, what the same call without the flag returns on the stand-ins S(c) — computed by the ORACLE (tests/compressed_keyed_cases.py:
stand_in), never by the device — except that an item that did not decompress reports its own status where that run read 6.  The keyed
verify is also held to the oracle directly (c_oracle.verify plus the rule order).  Run on the MI355X box: -m gpu."""
import os
import subprocess

import pytest

from bn254_amd import engine as E
from tests import codec_cases as cc
from tests import compressed_keyed_cases as K
from tests import threshold_cases as TC
from tests.conftest import ws_default
from tests.hip_ctypes import DevBuf, Stream

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAG = E.FLAG_G1_COMPRESSED
BAD_ARGUMENT = -10001
SEED = bytes(range(32))
SIZES = (1, 2, 63, 64, 65, 200)
COLLECT_SIZES = (0, 1, 2, 63, 64, 65, 130)
u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


@pytest.fixture(scope="module")
def keyset(eng, derived):
    pks, key_st = K.keys(derived["g2_not_in_subgroup"])
    assert list(eng.register_keys(b"".join(pks))) == key_st
    return pks, key_st


def register(eng, keyset):
    assert list(eng.register_keys(b"".join(keyset[0]))) == keyset[1]


@pytest.fixture(scope="module")
def items(derived):
    """256 items, every kind of the case set among them; longer batches tile them"""
    out = K.items(256, derived["g2_not_in_subgroup"], tag="gpu")
    assert {it.kind for it in out} == set(K.MUTATIONS)
    for it in out:
        assert it.kind not in K.PINNED or it.want == K.PINNED[it.kind], it
    assert {it.want for it in out} >= {0, 1, 2, 3, 4, 6, 9}
    return out


def tiled(items, n):
    return [items[i % len(items)] for i in range(n)]


def with_options(eng, opts, fn):
    """opts: {option: (value, value to restore)}"""
    try:
        for k, (v, _) in opts.items():
            eng.set_option(k, v)
        return fn()
    finally:
        for k, (_, back) in opts.items():
            eng.set_option(k, back)


HASH_TRIES = {E.OPT_HASH_MAX_TRIES: (K.HASH_MAX_TRIES, 0)}


def identity(run, encs, label):
    """run(item bytes, flags) -> a tuple of outputs, the item statuses first.  The defining identity; returns the outputs under the flag."""
    pairs = [K.stand_in(e) for e in encs]
    plain = run(b"".join(u for u, _ in pairs), 0)
    want = (K.overlay(plain[0], [st for _, st in pairs]),) + tuple(plain[1:])
    got = run(b"".join(encs), FLAG)
    assert got[0] == want[0], (label, [(i, a, b) for i, (a, b) in enumerate(zip(got[0], want[0])) if a != b][:8])
    assert tuple(got) == want, (label, [k for k in range(len(want)) if got[k] != want[k]])
    return got


# ---- bn254_batch_g1_decompress_device -----------------------------------------------------------------------------------------------------------
def test_g1_decompress_device(eng):
    """the host form's bytes on every codec case, from an input pointer at base + 1 and on a caller's stream; n == 0 touches nothing"""
    cases = cc.g1_cases()
    n = len(cases)
    enc = b"".join(cs.enc for cs in cases)
    want_out, want_st = eng.batch_g1_decompress(enc, n)
    assert list(want_st) == [cs.status for cs in cases]
    assert all(want_out[64 * i:64 * i + 64] == (cs.want or bytes(64)) for i, cs in enumerate(cases))
    stream = Stream()
    d_in, d_out, d_st = DevBuf(33 * n + 1, data=b"\xEE" + enc), DevBuf(64 * n, fill=0xEE), DevBuf(n, fill=0xEE)
    try:
        eng.batch_g1_decompress_device(d_in.ptr + 1, n, d_out.ptr, d_st.ptr, stream=stream.handle)
        stream.synchronize()
        assert d_st.download(n) == want_st and d_out.download(64 * n) == want_out
        d_st.upload(b"\xEE" * n)
        eng.batch_g1_decompress_device(d_in.ptr + 1, 0, d_out.ptr, d_st.ptr, stream=stream.handle)
        eng.batch_g1_decompress_device(None, 0, None, None)
        stream.synchronize()
        assert d_st.download(n) == b"\xEE" * n
        with pytest.raises(E.NativeError) as e:
            eng.batch_g1_decompress_device(d_in.ptr + 1, n, d_out.ptr + 1, d_st.ptr, stream=stream.handle)
        assert e.value.rc == -10002                                  # BN254_E_MISALIGNED: the 64-byte outputs are written as words
    finally:
        for b in (d_in, d_out, d_st):
            b.free()
        stream.destroy()


# ---- verify_keyed -------------------------------------------------------------------------------------------------------------------------------
def keyed_run(eng, batch, seed=None):
    msgs, keys = [it.msg for it in batch], [it.key for it in batch]
    if seed is None:
        return lambda data, flags: (eng.batch_verify_keyed(msgs, data, keys, flags=flags),)
    return lambda data, flags: (eng.batch_verify_keyed_randomized(msgs, data, keys, seed, flags=flags),)


def check_keyed(eng, batch, label, seed=None):
    got = identity(keyed_run(eng, batch, seed), [it.enc for it in batch], label)
    assert list(got[0]) == [it.want for it in batch], (label, [(i, it.kind, g, it.want) for i, (it, g) in enumerate(zip(batch, got[0])) if g != it.want][:8])


def test_verify_keyed_sizes_and_routes(eng, keyset, items):
    """n in {1, 2, 63, 64, 65, 200} and one n on every row of the routing table: the identity, and the oracle's statuses directly"""
    register(eng, keyset)
    rows = eng.route_table()
    on_rows = [min(r[0], rows[i - 1][0] + 1 if i else 1) if r[0] >= 1 << 40 else r[0] for i, r in enumerate(rows)]
    assert len(set(on_rows)) == len(rows)

    def run():
        for n in sorted(set(SIZES) | set(on_rows)):
            check_keyed(eng, tiled(items, n), n)
    with_options(eng, HASH_TRIES, run)


def test_verify_keyed_sliced_and_stale_workspace(eng, keyset, items):
    """BN254_OPT_MAX_CHUNK at the smallest value that cuts 200 items into at least 3 slices with a ragged last one (the staging runs once, in
    front of the slicing); and a compressed call behind a larger uncompressed one, whose workspace and statuses it must not inherit"""
    register(eng, keyset)
    n = 200
    chunk = min(k for k in range(1, n) if n % k and -(-n // k) >= 3)
    batch = tiled(items, n)
    with_options(eng, {**HASH_TRIES, E.OPT_MAX_CHUNK: (chunk, 0)}, lambda: check_keyed(eng, batch, ("chunk", chunk)))
    big = tiled(items[::-1], 300)
    plain = b"".join(K.stand_in(it.enc)[0] for it in big)

    def stale():
        eng.batch_verify_keyed([it.msg for it in big], plain, [it.key for it in big])
        check_keyed(eng, batch[:65], "stale")
    with_options(eng, HASH_TRIES, stale)


def test_verify_keyed_randomized(eng, keyset, items):
    """the grouped route (minimum batch lowered to 1) with failing groups: every failing item is found exactly"""
    register(eng, keyset)
    batch = tiled(items, 200)
    assert sum(1 for it in batch if it.want == 9) >= 8
    with_options(eng, {**HASH_TRIES, E.OPT_RAND_MIN_BATCH: (1, ws_default("RAND_MIN_BATCH_DEFAULT"))}, lambda: check_keyed(eng, batch, "randomized", SEED))


def test_verify_keyed_device_form(eng, keyset, items):
    """the _device form on a caller's stream with the signatures at base + 1"""
    register(eng, keyset)
    batch = tiled(items, 130)
    n = len(batch)
    blob, off = E.pack_messages([it.msg for it in batch])
    enc = b"".join(it.enc for it in batch)
    stream = Stream()
    bufs = [DevBuf(len(bytes(blob)), data=bytes(blob)), DevBuf(8 * (n + 1), data=u64(off)), DevBuf(33 * n + 1, data=b"\x02" + enc),
            DevBuf(4 * n, data=u32(it.key for it in batch)), DevBuf(n, fill=0xEE)]
    try:
        def run():
            eng.batch_verify_keyed_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr + 1, bufs[3].ptr, n, bufs[4].ptr, flags=FLAG, stream=stream.handle)
            stream.synchronize()
            return bufs[4].download(n)
        assert list(with_options(eng, HASH_TRIES, run)) == [it.want for it in batch]
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


# ---- verify_keyed_bitmap ------------------------------------------------------------------------------------------------------------------------
def bitmap_items(c, n, tag):
    """n aggregates over 1 to 3 good keys as (msg, enc, row, pinned status or None): the sum of the signers' signatures, compressed, then
    mutated as the keyed items are; a refused key's bit (4) and a bit beyond the set (2) with a good and with a faulty encoding"""
    kinds = ("unchanged", "flipped", "prefix04", "noroot07", "x_plus_q", "zeros", "refused_good", "refused_bad", "beyond_good", "beyond_bad", "wrong_row")
    pinned = {"unchanged": 0, "flipped": 9, "prefix04": 3, "noroot07": 6, "x_plus_q": 6, "refused_good": 4, "refused_bad": 3, "beyond_good": 2,
              "beyond_bad": 3, "wrong_row": 9}
    out = []
    for i in range(n):
        kind = kinds[i] if i < len(kinds) else kinds[(i // 2) % len(kinds)] if i % 2 == 0 else "unchanged"
        msg = K.message(tag, i)
        signers = sorted({i % K.N_GOOD, (3 * i + 1) % K.N_GOOD, (5 * i + 2) % K.N_GOOD})[:1 + i % 3]
        secret = sum(int.from_bytes(K.sk(j), "big") for j in signers) % K.R
        enc = c.g1_compress(c.sign(msg, secret.to_bytes(32, "big")))
        row = sum(1 << j for j in signers)
        if kind == "flipped":
            enc = bytes([5 - enc[0]]) + enc[1:]
        elif kind in ("prefix04", "refused_bad", "beyond_bad"):
            enc = b"\x04" + enc[1:]
        elif kind == "noroot07":
            enc = b"\x07" + K.no_root_x("%s/%d" % (tag, i))
        elif kind == "x_plus_q":
            enc = enc[:1] + cc.be(int.from_bytes(enc[1:], "big") + K.Q)
        elif kind == "zeros":
            enc = bytes(33)
        if kind.startswith("refused"):
            row |= 1 << K.K_OFF_SUB
        elif kind.startswith("beyond"):
            row |= 1 << (K.N_KEYS + 3)
        elif kind == "wrong_row":
            row ^= 1 << ((signers[0] + 1) % K.N_GOOD) if len(signers) == 1 else 1 << signers[0]
        out.append((msg, enc, row, pinned.get(kind)))
    return out


def check_bitmap(eng, batch, label, seed=None):
    msgs, rows = [b[0] for b in batch], [b[2] for b in batch]
    if seed is None:
        run = lambda data, flags: (eng.batch_verify_keyed_bitmap(msgs, data, rows, K.BM, flags=flags),)                      # noqa: E731
    else:
        run = lambda data, flags: (eng.batch_verify_keyed_bitmap_randomized(msgs, data, rows, K.BM, seed, flags=flags),)      # noqa: E731
    got = identity(run, [b[1] for b in batch], label)
    assert all(p is None or g == p for g, (_, _, _, p) in zip(got[0], batch)), (label, [(i, g, b[3]) for i, (g, b) in enumerate(zip(got[0], batch)) if b[3] not in (None, g)][:8])
    return got[0]


@pytest.fixture(scope="module")
def bm_items(c):
    return bitmap_items(c, 200, "bitmap")


def test_verify_keyed_bitmap_sizes_and_routes(eng, keyset, bm_items):
    register(eng, keyset)
    rows = eng.route_table()
    on_rows = [min(r[0], rows[i - 1][0] + 1 if i else 1) if r[0] >= 1 << 40 else r[0] for i, r in enumerate(rows)]
    for n in sorted(set(SIZES) | set(on_rows)):
        st = check_bitmap(eng, tiled(bm_items, n), n)
        if n >= 64:
            assert {0, 2, 3, 4, 6, 9} <= set(st)


def test_verify_keyed_bitmap_sliced_stale_randomized(eng, keyset, bm_items):
    register(eng, keyset)
    n = 200
    chunk = min(k for k in range(1, n) if n % k and -(-n // k) >= 3)
    with_options(eng, {E.OPT_MAX_CHUNK: (chunk, 0)}, lambda: check_bitmap(eng, bm_items, ("chunk", chunk)))
    big = tiled(bm_items[::-1], 300)
    eng.batch_verify_keyed_bitmap([b[0] for b in big], b"".join(K.stand_in(b[1])[0] for b in big), [b[2] for b in big], K.BM)
    check_bitmap(eng, bm_items[:65], "stale")

    def rand():
        st = check_bitmap(eng, bm_items, "randomized", SEED)
        last = eng.debug_bitmap_rand_last()
        assert last["ran"] == 1 and last["failed_groups"] >= 1 and last["rechecked"] >= 1, last
        return st
    assert 9 in with_options(eng, {E.OPT_BITMAP_RAND_MIN_TUPLES: (1, ws_default("BITMAP_RAND_MIN_TUPLES_DEFAULT"))}, rand)


# ---- collect ------------------------------------------------------------------------------------------------------------------------------------
def collect_tuples(c, sizes, tag, faults=True, planted=None):
    """tuples (msg, [(enc, key)]): share t of tuple i by good key (7 i + 3 t) % 7, every fifth share of the tuples of 63 to 65 shares mutated
    by the keyed kinds where faults; planted: {(tuple, share): kind} on top"""
    planted = planted or {}
    kinds = ("flipped", "prefix04", "noroot02", "noroot07", "x_plus_q", "other_key", "zeros", "oob_good", "oob_bad", "refused_good", "refused_bad")
    out, k = [], 0
    for i, size in enumerate(sizes):
        msg = K.message(tag, i)
        shares = []
        for t in range(size):
            key = (7 * i + 3 * t) % K.N_GOOD
            enc = c.g1_compress(c.sign(msg, K.sk(key)))
            if (i, t) in planted or (faults and 5 < size < 130 and t % 5 == 3):
                kind = planted.get((i, t)) or kinds[k % len(kinds)]
                k += (i, t) not in planted
                if kind == "flipped":
                    enc = bytes([5 - enc[0]]) + enc[1:]
                elif kind in ("prefix04", "oob_bad", "refused_bad"):
                    enc = b"\x04" + enc[1:]
                elif kind in ("noroot02", "noroot07"):
                    enc = bytes([int(kind[-2:])]) + K.no_root_x("%s/%d/%d" % (tag, i, t))
                elif kind == "x_plus_q":
                    enc = enc[:1] + cc.be(int.from_bytes(enc[1:], "big") + K.Q)
                elif kind == "other_key":
                    enc = c.g1_compress(c.sign(msg, K.sk((key + 1) % K.N_GOOD)))
                elif kind == "zeros":
                    enc = bytes(33)
                if kind.startswith("oob"):
                    key = K.N_KEYS + 2
                elif kind.startswith("refused"):
                    key = K.K_OFF_SUB
            shares.append((enc, key))
        out.append((msg, shares))
    return out


def flat(tuples):
    return ([t[0] for t in tuples], [e for t in tuples for e, _ in t[1]], [k for t in tuples for _, k in t[1]], [len(t[1]) for t in tuples])


def collect_run(eng, tuples, route):
    msgs, _, keys, sizes = flat(tuples)
    if route == "exact":
        return lambda data, flags: eng.batch_collect_keyed_bitmap(msgs, data, keys, sizes, K.BM, flags=flags, want_counts=True)
    if route == "randomized":
        return lambda data, flags: eng.batch_collect_keyed_bitmap_randomized(msgs, data, keys, sizes, K.BM, SEED, flags=flags, want_counts=True)
    return lambda data, flags: eng.batch_collect_keyed_bitmap_optimistic(msgs, data, keys, sizes, K.BM, flags=flags, want_counts=True)


COLLECT_ROUTES = {
    "exact": {E.OPT_COLLECT_WAVE_MIN_SHARES: (64, 16)},
    "randomized": {E.OPT_COLLECT_WAVE_MIN_SHARES: (64, 16), E.OPT_COLLECT_RAND_MIN_SHARES: (1, E.COLLECT_RAND_MIN_SHARES_DEFAULT),
                   E.OPT_COLLECT_RAND_MIN_PER_KEY: (0, E.COLLECT_RAND_MIN_PER_KEY_DEFAULT)},
    "optimistic": {E.OPT_COLLECT_WAVE_MIN_SHARES: (64, 16), E.OPT_COLLECT_OPT_MIN_SHARES: (1, E.COLLECT_OPT_MIN_SHARES_DEFAULT)},
}


@pytest.fixture(scope="module")
def col_tuples(c):
    """the seven sizes, then two tuples of five shares by five distinct keys: in one a share is -sigma (decodes, so the tuple's optimistic
    check runs and fails: the exact way), in the other a share has a bad prefix (never a candidate: the check of the other four passes)"""
    n = len(COLLECT_SIZES)
    return collect_tuples(c, COLLECT_SIZES + (5, 5), "collect", planted={(n, 2): "flipped", (n + 1, 1): "prefix04"})


@pytest.mark.parametrize("route", sorted(COLLECT_ROUTES))
def test_collect_every_route(eng, keyset, col_tuples, route):
    """tuples of 0, 1, 2, 63, 64, 65 and 130 compressed shares, both sum kernels (wave from 64 shares on), faults that fail some tuples'
    optimistic check and leave others passing; the route asserted through its debug hook; on the exact route the share statuses are the
    keyed verify's on the message repeated (from the oracle), and the outputs close the loop into the bitmap verify (defining identity 2)"""
    register(eng, keyset)
    pks, key_st = keyset
    msgs, encs, keys, sizes = flat(col_tuples)

    def run():
        got = identity(collect_run(eng, col_tuples, route), encs, route)
        if route == "randomized":
            last = eng.debug_collect_rand_last()
            assert last["slices"] >= 1 and last["groups"] >= 1 and last["failed_groups"] >= 1, last
        elif route == "optimistic":
            last = eng.debug_collect_opt_last()
            # the tuples of 1, 2 and 5 shares are checked (a tuple that names a key twice goes the exact way unchecked): -sigma fails its tuple
            assert last["checked"] == 4 and last["passed"] == 3 and last["exact_tuples"] >= 1 + 4 and last["exact_shares"] >= 5, last
        else:
            assert eng.debug_collect_rand_last()["slices"] == 0 and eng.debug_collect_opt_last()["checked"] == 0
        return got
    share_st, tuple_st, agg, bits, counts = with_options(eng, COLLECT_ROUTES[route], run)
    rep = [m for m, k in zip(msgs, sizes) for _ in range(k)]
    direct = [K.direct_status(pks, key_st, m, e, k) for m, e, k in zip(rep, encs, keys)]
    if route != "optimistic":                                        # the optimistic call does not verify what it does not need (its documented deviation)
        assert list(share_st) == direct
    assert {0, 2, 3, 4, 6, 9} <= set(direct) and tuple_st == bytes(len(col_tuples))
    assert all(s != 0 for s, e in zip(share_st, encs) if K.stand_in(e)[1])          # what does not decompress is never taken
    assert counts[0] == 0 and agg[:64] == bytes(64) and counts[COLLECT_SIZES.index(130)] == K.N_GOOD and counts[-2:] == [4, 4]
    assert eng.batch_verify_keyed_bitmap(msgs, agg, bits, K.BM) == bytes(len(col_tuples))


def test_collect_device_form_reversed_range(eng, keyset, c):
    """the _device form on a caller's stream, shares at base + 1: the host form's bytes; and with one reversed share range whose shares are
    status-3 encodings: the tuple reads 2 and so do its shares — the fill comes before the decode — while the other tuples are untouched"""
    register(eng, keyset)
    tuples = collect_tuples(c, (3, 4, 5, 2), "collect-dev", faults=False)
    tuples[1] = (tuples[1][0], [(b"\x04" + e[1:], k) for e, k in tuples[1][1]])
    msgs, encs, keys, sizes = flat(tuples)
    n, n_shares = len(tuples), len(keys)
    host = eng.batch_collect_keyed_bitmap(msgs, b"".join(encs), keys, sizes, K.BM, flags=FLAG, want_counts=True)
    assert list(host[0][3:7]) == [3] * 4 and host[4] == [3, 0, 5, 2]
    blob, off = E.pack_messages(msgs)
    soff = [sum(sizes[:i]) for i in range(n + 1)]
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        bufs.append(DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE))
        return bufs[-1]
    try:
        d_msgs, d_moff, d_shares, d_keys = dev(bytes(blob)), dev(u64(off)), dev(b"\x03" + b"".join(encs)), dev(u32(keys))
        d_sst, d_tst, d_agg, d_bits, d_cnt = dev(nbytes=n_shares), dev(nbytes=n), dev(nbytes=64 * n), dev(nbytes=4 * K.BM * n), dev(nbytes=4 * n)

        def run(share_off):
            d_soff = dev(u64(share_off))
            eng.batch_collect_keyed_bitmap_device(d_msgs.ptr, d_moff.ptr, d_shares.ptr + 1, d_keys.ptr, d_soff.ptr, n_shares, n, K.BM, d_sst.ptr, d_tst.ptr,
                                                  d_agg.ptr, d_bits.ptr, d_cnt.ptr, flags=FLAG, stream=stream.handle)
            stream.synchronize()
            words, cnt = d_bits.download(4 * K.BM * n), d_cnt.download(4 * n)
            return (d_sst.download(n_shares), d_tst.download(n), d_agg.download(64 * n),
                    [int.from_bytes(words[4 * k:4 * k + 4], "little") for k in range(K.BM * n)], [int.from_bytes(cnt[4 * k:4 * k + 4], "little") for k in range(n)])
        assert run(soff) == host
        rev = soff[:]
        rev[2] = soff[1] - 1                         # tuple 1 reversed; tuple 2 then starts before the earlier offset soff[1]: refused too
        g = run(rev)
        assert list(g[1]) == [0, 2, 2, 0] and list(g[0]) == list(host[0][:3]) + [2] * 9 + list(host[0][12:])
        assert g[4] == [3, 0, 0, 2] and g[2][:64] == host[2][:64] and g[2][192:] == host[2][192:] and g[2][64:192] == bytes(128)
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


# ---- merge --------------------------------------------------------------------------------------------------------------------------------------
def merge_tuples(c):
    """4 tuples of up to 5 compressed partials over the good keys: disjoint partials, an overlap (the later partial is not taken), a wrong sum,
    encodings that do not decompress, a partial over the refused key, and one clean tuple"""
    plan = [[([0, 1], "ok"), ([2], "ok"), ([1, 3], "ok"), ([4], "prefix04"), ([5, 6], "ok")],
            [([0], "flipped"), ([1, 2], "ok"), ([3], "noroot07"), ([4], "ok")],
            [([6], "ok"), ([5, K.K_OFF_SUB], "ok"), ([0, 1, 2], "x_plus_q")],
            [([0, 1, 2], "ok"), ([3, 4], "ok"), ([5], "ok"), ([6], "ok")]]
    out = []
    for i, t in enumerate(plan):
        msg = K.message("merge", i)
        parts = []
        for p, (signers, kind) in enumerate(t):
            secret = sum(int.from_bytes(K.sk(j), "big") for j in signers if j < K.N_GOOD) % K.R
            enc = c.g1_compress(c.sign(msg, secret.to_bytes(32, "big")))
            if kind == "flipped":
                enc = bytes([5 - enc[0]]) + enc[1:]
            elif kind == "prefix04":
                enc = b"\x04" + enc[1:]
            elif kind == "noroot07":
                enc = b"\x07" + K.no_root_x("merge/%d/%d" % (i, p))
            elif kind == "x_plus_q":
                enc = enc[:1] + cc.be(int.from_bytes(enc[1:], "big") + K.Q)
            parts.append((enc, sum(1 << j for j in signers)))
        out.append((msg, parts))
    return out


@pytest.mark.parametrize("optimistic", [False, True])
def test_merge(eng, keyset, c, optimistic):
    register(eng, keyset)
    tuples = merge_tuples(c)
    msgs, encs, rows, sizes = flat(tuples)
    run = lambda data, flags: eng.merge_keyed_bitmap(msgs, data, rows, sizes, K.BM, flags=flags, want_counts=True, optimistic=optimistic)   # noqa: E731

    def go():
        got = identity(run, encs, ("merge", optimistic))
        last = eng.debug_merge_opt_last()
        assert (last["checked"] >= 1 and last["passed"] >= 1 and last["exact_tuples"] >= 1) if optimistic else last["checked"] == 0, last
        return got
    part_st, taken, tuple_st, agg, bits, counts = with_options(eng, {E.OPT_MERGE_OPT_MIN_PARTS: (1, E.MERGE_OPT_MIN_PARTS_DEFAULT)}, go)
    assert list(part_st) == [0, 0, 0, 3, 0, 9, 0, 6, 0, 0, 4, 6, 0, 0, 0, 0]
    assert list(taken) == [1, 1, 0, 0, 1, 0, 1, 0, 1, 1, 0, 0, 1, 1, 1, 1]              # partial 2 overlaps partial 0 in key 1: first fit, as without the flag
    assert tuple_st == bytes(4) and counts == [5, 3, 1, 7] and bits == [0b1100111, 0b0010110, 0b1000000, 0b1111111]
    assert eng.batch_verify_keyed_bitmap(msgs, agg, bits, K.BM) == bytes(4)


# ---- threshold ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_keys,t", [(7, 5), (20, 14)])
def test_threshold(eng, keyset, c, n_keys, t):
    """a dealt key set (tests/threshold_cases.py: secrets_of), exact and optimistic under the group key: enough valid shares; too few valid
    shares ONLY because of compressed faults — tuple status 9 and the row of the keys that were there —; more than enough with faults"""
    name = "compressed%d_t%d" % (n_keys, t)
    secrets, f0 = TC.secrets_of(name, n_keys, t, None)
    sks = [s.to_bytes(32, "big") for s in secrets]
    bm = (n_keys + 31) // 32
    faults = ("prefix04", "noroot07", "x_plus_q")
    shapes = [[(j, None) for j in range(t)], [(j, faults[j % 3] if j in (1, t - 1) else None) for j in range(t)],
              [(j, faults[j % 3] if j % 4 == 2 else None) for j in range(n_keys)], [(j, None) for j in range(n_keys - 1, n_keys - t - 1, -1)]]
    tuples = []
    for i, shape in enumerate(shapes):
        msg = K.message(name, i)
        shares = []
        for j, kind in shape:
            enc = c.g1_compress(c.sign(msg, sks[j]))
            if kind == "prefix04":
                enc = b"\x04" + enc[1:]
            elif kind == "noroot07":
                enc = b"\x07" + K.no_root_x("%s/%d/%d" % (name, i, j))
            elif kind == "x_plus_q":
                enc = enc[:1] + cc.be(int.from_bytes(enc[1:], "big") + K.Q)
            shares.append((enc, j))
        tuples.append((msg, shares))
    msgs, encs, keys, sizes = flat(tuples)
    group_pk = c.public_key_g2(f0.to_bytes(32, "big"))
    try:
        assert eng.register_keys(b"".join(c.public_key_g2(s) for s in sks)) == bytes(n_keys)
        assert eng.set_group_key(group_pk) == 0
        exact = identity(lambda data, flags: eng.batch_threshold_combine_keyed(msgs, data, keys, sizes, bm, t, flags=flags), encs, name)
        assert eng.debug_threshold_opt_last()["checked"] == 0

        def opt():
            got = identity(lambda data, flags: eng.batch_threshold_combine_keyed_optimistic(msgs, data, keys, sizes, bm, t, flags=flags), encs, name + "/optimistic")
            last = eng.debug_threshold_opt_last()
            assert last["checked"] >= 1 and last["passed"] >= 1, last
            return got
        optimistic = with_options(eng, {E.OPT_THRESHOLD_OPT_MIN_SHARES: (1, E.THRESHOLD_OPT_MIN_SHARES_DEFAULT)}, opt)
        for share_st, tuple_st, group, bits, counts in (exact, optimistic):
            assert list(tuple_st) == [0, 9, 0, 0]
            row1 = [j for j in range(32 * bm) if (bits[bm + j // 32] >> (j % 32)) & 1]
            assert row1 == [j for j in range(t) if j not in (1, t - 1)] and counts[1] == t - 2 and group[64:128] == bytes(64)
            pre = [K.stand_in(e)[1] for e in encs]
            assert all(s == p for s, p in zip(share_st, pre) if p) and {3, 6} <= set(share_st)
            want = c.sign(msgs[0], f0.to_bytes(32, "big"))               # the group signature is the signature under f(0), whichever t keys gave it
            assert [group[:64], group[128:192], group[192:256]] == [want, c.sign(msgs[2], f0.to_bytes(32, "big")), c.sign(msgs[3], f0.to_bytes(32, "big"))]
        assert exact[2] == optimistic[2] and exact[1] == optimistic[1]
    finally:
        register(eng, keyset)


# ---- argument handling --------------------------------------------------------------------------------------------------------------------------
def test_flag_refused_where_it_is_not_taken(eng, keyset, c):
    """every other entry point that reads 64-byte G1 points under a flags argument returns BN254_E_BAD_ARGUMENT when the bit is set"""
    register(eng, keyset)
    msg = K.message("refused", 0)
    sig, pk, g1 = c.sign(msg, K.sk(0)), keyset[0][0], c.g1_generator()
    calls = [lambda: eng.batch_verify([msg], sig, pk, flags=FLAG),
             lambda: eng.batch_verify_randomized([msg], sig, pk, SEED, flags=FLAG),
             lambda: eng.batch_pairing_check(g1, pk, 1, 1, flags=FLAG),
             lambda: eng.batch_pairing(g1, pk, 1, 1, flags=FLAG),
             lambda: eng.batch_check_public_keys(pk, g1, 1, flags=FLAG),
             lambda: eng.batch_aggregate_verify([msg], pk, sig, [0], [[0]], flags=FLAG),
             lambda: eng.register_pools([msg], pk, sig, 1, flags=FLAG),
             lambda: eng.batch_aggregate_verify_distinct([msg], pk, sig, [1], flags=FLAG),
             lambda: eng.batch_aggregate_verify_distinct_keyed([msg], [0], sig, [1], flags=FLAG),
             lambda: eng.batch_aggregate_verify_distinct_keyed_randomized([msg], [0], sig, [1], SEED, flags=FLAG),
             lambda: eng.batch_pop_verify(pk, sig, flags=FLAG)]
    for k, call in enumerate(calls):
        with pytest.raises(E.NativeError) as e:
            call()
        assert e.value.rc == BAD_ARGUMENT, k
    import ctypes
    st = ctypes.create_string_buffer(1)
    assert eng._lib.bn254_ctx_register_keys_pop(eng._h, pk, sig, 1, FLAG, st) == BAD_ARGUMENT
    d = DevBuf(256, fill=0)
    try:
        for name, args in (("bn254_batch_verify_device", (d.ptr, d.ptr, d.ptr, d.ptr, 1, FLAG, d.ptr, None)),
                           ("bn254_batch_pairing_device", (d.ptr, d.ptr, 1, 1, FLAG, d.ptr, d.ptr, None)),
                           ("bn254_batch_pop_verify_device", (d.ptr, d.ptr, 1, FLAG, d.ptr, None))):
            assert getattr(eng._lib, name)(eng._h, *args) == BAD_ARGUMENT, name
    finally:
        d.free()
    # the set registered before the refused registration still stands, and the flag works where it is taken
    assert eng.batch_verify_keyed([msg], c.g1_compress(sig), [0], flags=FLAG) == b"\0"


# ---- the mirrors --------------------------------------------------------------------------------------------------------------------------------
def test_python_mirrors(eng, keyset):
    """bn254_amd.api: compressed=True on the keyed verify, the signers verify, the aggregate, merge and threshold families — 33-byte bytes in,
    the Error Signature.from_compressed would raise as the status, any other length Error(InvalidEncoding) before any device work"""
    from bn254_amd.api import ECDSA, Error, ErrorKind, PublicKey, Signature, threshold_deal
    sk = threshold_deal(0x1234567, 3, 4, "compressed/api")
    pk = [PublicKey.from_private_key(s) for s in sk]
    group_pk = PublicKey.from_private_key(type(sk[0])(0x1234567))
    E3, E6, E9 = Error(ErrorKind.InvalidEncoding), Error(ErrorKind.NotMemberError), Error(ErrorKind.VerificationFailed)
    try:
        assert ECDSA.register_keys(pk, engine=eng) == [None] * 4
        msg = b"round 12"
        sigs = [ECDSA.sign(msg, s) for s in sk]
        wire = [s.to_compressed() for s in sigs]
        bad, big = b"\x04" + wire[1][1:], wire[3][:1] + b"\xff" * 32
        assert all(isinstance(w, bytes) and len(w) == 33 for w in wire)
        three = ([msg] * 3, [wire[0], bad, wire[2]], [0, 1, 3])
        assert ECDSA.batch_verify_keyed(*three, engine=eng, compressed=True) == [None, E3, E9]
        assert ECDSA.batch_verify_keyed_randomized(*three, seed=SEED, engine=eng, compressed=True) == [None, E3, E9]
        for call in (lambda s: ECDSA.batch_verify_keyed([msg], [s], [0], engine=eng, compressed=True),
                     lambda s: ECDSA.verify_keyed_signers(msg, s, [0], engine=eng, compressed=True),
                     lambda s: ECDSA.aggregate_keyed_signers(msg, [s], [0], engine=eng, compressed=True),
                     lambda s: ECDSA.merge_keyed_signers(msg, [(s, [0])], engine=eng, compressed=True),
                     lambda s: ECDSA.threshold_combine_keyed(msg, [s], [0], 3, engine=eng, compressed=True)):
            for wrong in (wire[0][:32], wire[0] + b"\0", sigs[0].raw):
                with pytest.raises(Error) as e:
                    call(wrong)
                assert e.value == E3
        plain = ECDSA.aggregate_keyed_signers(msg, [sigs[2], sigs[0], sigs[3]], [2, 0, 3], engine=eng)
        shares = ([wire[2], wire[0], bad, wire[3], big], [2, 0, 1, 3, 1])
        for agg in (ECDSA.aggregate_keyed_signers, ECDSA.aggregate_keyed_signers_optimistic,
                    lambda *a, **k: ECDSA.aggregate_keyed_signers_randomized(*a, seed=SEED, **k)):
            sigma, signers, statuses = agg(msg, *shares, engine=eng, compressed=True)
            assert isinstance(sigma, Signature) and sigma.raw == plain[0].raw and signers == [0, 2, 3] and statuses == [None, None, E3, None, E6]
        packed = sigma.to_compressed()
        assert ECDSA.verify_keyed_signers(msg, packed, signers, engine=eng, compressed=True) is None
        items = [(msg, packed, signers), (msg, bad, [1]), (msg, packed, [0, 1, 2, 3])]
        assert ECDSA.batch_verify_keyed_signers(items, engine=eng, compressed=True) == [None, E3, E9]
        assert ECDSA.batch_verify_keyed_signers_randomized(items, seed=SEED, engine=eng, compressed=True) == [None, E3, E9]
        left = ECDSA.aggregate_keyed_signers(msg, wire[:2], [0, 1], engine=eng, compressed=True)
        parts = [(left[0].to_compressed(), left[1]), (wire[2], [2]), (bad, [3]), (wire[1], [1])]
        for merge in (ECDSA.merge_keyed_signers, ECDSA.merge_keyed_signers_optimistic):
            merged, union, statuses, taken = merge(msg, parts, engine=eng, compressed=True)
            assert union == [0, 1, 2] and statuses == [None, None, E3, None] and taken == [True, True, False, False]
            assert ECDSA.verify_keyed_signers(msg, merged, union, engine=eng) is None
        ECDSA.register_group_key(group_pk, engine=eng)
        for combine in (ECDSA.threshold_combine_keyed, ECDSA.threshold_combine_keyed_optimistic):
            group, used, statuses = combine(msg, [wire[3], bad, wire[0], wire[2]], [3, 1, 0, 2], 3, engine=eng, compressed=True)
            assert used == [0, 2, 3] and statuses == [None, E3, None, None] and ECDSA.verify(msg, group, group_pk) is None
            with pytest.raises(Error) as e:
                combine(msg, [wire[3], bad, big], [3, 1, 0], 3, engine=eng, compressed=True)
            assert e.value == E9 and e.value.signers == [3] and e.value.statuses == [None, E3, E6]
    finally:
        register(eng, keyset)


def test_cpp_mirror_and_example(tmp_path):
    """host/compressed_example.cpp — collect, then bitmap verify, from compressed shares through bn254.hpp — builds with -Wall -Werror against
    the library and prints success"""
    from bn254_amd import _native
    host = os.path.join(ROOT, "bn254_amd", "host")
    exe = str(tmp_path / "compressed_example")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", os.path.join(host, "compressed_example.cpp"), "-o", exe, _native.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "compressed shares: ok" in p.stdout, (p.stdout, p.stderr)
