"""bn254_batch_collect_keyed_bitmap[_randomized][_device] with MORE THAN 65 536 TUPLES, on the GPU: k_cl_sum_wave's grid-stride loop (one
block takes tuples i and i + 65 536 and reuses part[] and cnt[]), the carry loop of k_aggd_scan_totals (more than 256 block totals), the
deepest binary search of cl_tuple_of, and the _device form's range rule across scan blocks.
65 900 tuples over the 46-key set of tests/test_gpu_collect_keyed_bitmap.py: one share each, every seventh tuple empty, nine tuples of 20, 64
or 70 shares on both sides of 65 536 (5 and 5 + 65 536, 255 and 255 + 65 536 are long in the same block), every eleventh share sigma + G1.
Nothing expected comes from the device: the statuses are planted, the aggregate of a one-share tuple is the share or zeros, the long tuples
go through the oracle's g1_add, rows and counts are tests/collect_model.py's, the range rule is the restatement of
tests/test_collect_keyed_bitmap.py.  Run on the MI355X box: -m gpu."""
import struct

import pytest

from bn254_amd import engine as E
from tests import collect_model
from tests.datagen import D
from tests.test_collect_keyed_bitmap import range_rule
from tests.test_gpu_collect_keyed_bitmap import BM, N_GOOD, c, collect, eng, keyset, reg_set, sign, with_options   # noqa: F401
from tests.test_gpu_collect_keyed_bitmap_randomized import SEEDS, rand_collect

pytestmark = pytest.mark.gpu

WAVE_BLOCKS = 65536                                              # CL_WAVE_MAX_BLOCKS of bn254_collect.hip
N = WAVE_BLOCKS + 364
LONG = dict(zip([0, 5, 255, 256, WAVE_BLOCKS - 1, WAVE_BLOCKS, WAVE_BLOCKS + 5, WAVE_BLOCKS + 255, N - 1], [20, 64, 70] * 3))
N_MSGS = 32


def size_of(i):
    return LONG.get(i, 0 if i % 7 == 0 else 1)


def differing(got, want, width):
    """the first tuples (or shares) at which two outputs differ"""
    if got == want:
        return []
    assert len(got) == len(want)
    return [i for i in range(len(want) // width) if got[width * i:width * i + width] != want[width * i:width * i + width]][:8]


def same(got, want, what):
    """the five outputs, compared without printing 4 MB on a failure"""
    for k, (name, width) in enumerate((("share_status", 1), ("tuple_status", 1), ("agg", 64), ("bits", BM), ("counts", 1))):
        assert not differing(got[k], want[k], width), (what, name, differing(got[k], want[k], width))


@pytest.fixture(scope="module")
def many(eng, c, keyset):
    """-> dict(tuples, msgs, shares, keys, sizes, soff, good, origin, want = the five outputs)"""
    sks, _ = keyset
    reg_set(eng, keyset)
    pool = [D("collect/many-tuples", j) for j in range(N_MSGS)]
    sigs = sign(eng, [(m, sks[k]) for m in pool for k in range(N_GOOD)])
    g1 = c.g1_generator()
    wrong = {}
    msgs, shares, keys, sizes, good, origin = [], [], [], [], [], []
    for i in range(N):
        msgs.append(pool[i % N_MSGS])
        sizes.append(size_of(i))
        for t in range(sizes[-1]):
            key = (3 * i + t) % N_GOOD
            at = (i % N_MSGS) * N_GOOD + key
            ok = len(shares) % 11 != 10
            if not ok and at not in wrong:
                wrong[at] = c.g1_add(sigs[at], g1)
            shares.append(sigs[at] if ok else wrong[at])
            keys.append(key)
            good.append(ok)
            origin.append(i)
    assert sizes.count(0) > N // 8 and max(sizes) == 70 and all(sizes[i] >= 20 and sizes[i + WAVE_BLOCKS] >= 20 for i in (0, 5, 255))
    assert (N + 255) // 256 > 256                                 # the scans' block totals need the carry loop
    soff = [0]
    for k in sizes:
        soff.append(soff[-1] + k)
    status = bytes(0 if g else 9 for g in good)
    rows, counts, chosen = collect_model.select(keys, status, sizes, bytes(N), BM)
    agg = [shares[p[0]] if len(p) == 1 else bytes(64) if not p else collect_model.aggregates(c, shares, [p])[0] for p in chosen]
    assert max(counts) > 32 and sum(1 for p in chosen if len(p) > 1) == len(LONG)
    tuples = [(msgs[i], list(zip(shares[soff[i]:soff[i + 1]], keys[soff[i]:soff[i + 1]]))) for i in range(N)]
    return dict(tuples=tuples, msgs=msgs, shares=shares, keys=keys, sizes=sizes, soff=soff, good=good, origin=origin,
                want=(status, bytes(N), b"".join(agg), [w for r in rows for w in r], counts))


@pytest.mark.parametrize("wave_min", [16, 1, 1 << 30], ids=["default", "all_waves", "all_lanes"])
def test_host_form(eng, keyset, many, wave_min):
    """BN254_OPT_COLLECT_WAVE_MIN_SHARES at its default, at 1 (every non-empty tuple goes through the grid-stride loop) and at 1 << 30"""
    reg_set(eng, keyset)
    got = with_options(eng, {E.OPT_COLLECT_WAVE_MIN_SHARES: wave_min}, lambda: collect(eng, many["tuples"]))
    same(got, many["want"], wave_min)


def test_randomized_form(eng, keyset, many):
    reg_set(eng, keyset)
    got, hook = rand_collect(eng, many["tuples"], SEEDS[0])
    assert hook["slices"] >= 1 and hook["groups"] >= sum(many["sizes"]) // 64, hook
    same(got, many["want"], "randomised")


def expect_for(c, many, off):
    """the five outputs for the share offsets `off`, from the range rule's restatement: a refused tuple reads 2 and is empty, its shares and
    every orphan read 2; an accepted tuple whose range is the valid run's is the valid run's; one whose range changed (it swallowed a
    neighbour) is worked out anew: a share signed for another message reads 9.  -> (outputs, refused tuples, tuples worked out anew)"""
    soff, shares, keys, good, origin = (many[k] for k in ("soff", "shares", "keys", "good", "origin"))
    n_shares = len(keys)
    ok, tuple_of = range_rule(off, n_shares)
    st, tst, agg, bits, counts = bytearray(many["want"][0]), bytearray(N), bytearray(many["want"][2]), list(many["want"][3]), list(many["want"][4])
    refused, anew = set(), set()
    for s in range(n_shares):
        if tuple_of[s] == N:
            st[s] = 2
    for i in range(N):
        if ok[i] and (off[i], off[i + 1]) == (soff[i], soff[i + 1]):
            continue
        if ok[i]:
            idx = list(range(off[i], off[i + 1]))
            sub = [0 if good[s] and origin[s] % N_MSGS == i % N_MSGS else 9 for s in idx]
            for s, v in zip(idx, sub):
                st[s] = v
            rows, cnts, chosen = collect_model.select([keys[s] for s in idx], sub, [len(idx)], [0], BM)
            agg[64 * i:64 * i + 64] = collect_model.aggregates(c, [shares[s] for s in idx], chosen)[0]
            bits[BM * i:BM * i + BM], counts[i] = rows[0], cnts[0]
            anew.add(i)
        else:
            tst[i] = 2
            agg[64 * i:64 * i + 64], bits[BM * i:BM * i + BM], counts[i] = bytes(64), [0] * BM, 0
            refused.add(i)
    return (bytes(st), bytes(tst), bytes(agg), bits, counts), refused, anew


def test_device_form_ranges(eng, c, keyset, many):
    """the _device form on a caller's stream: the valid offsets give the expected bytes and a bitmap verify behind them on the same stream
    reads 0 everywhere; then, one call each, a reversed range at tuple 255 (refuses 256 too: the first tuple of the next scan block), one at
    65 535 (refuses 65 536), a range that swallows its neighbour at 65 540 and a last tuple that runs past n_shares"""
    from tests.hip_ctypes import DevBuf, Stream
    from bn254_amd.engine import pack_messages
    reg_set(eng, keyset)
    soff, keys = many["soff"], many["keys"]
    n_shares = len(keys)
    blob, off = pack_messages(many["msgs"])
    u64 = lambda v: struct.pack("<%dQ" % len(v), *v)   # noqa: E731
    u32 = lambda v: struct.pack("<%dI" % len(v), *v)   # noqa: E731
    sizes_out = (n_shares, N, 64 * N, 4 * BM * N, 4 * N)
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_msgs, d_moff, d_shares, d_keys = dev(bytes(blob)), dev(u64(list(off))), dev(b"".join(many["shares"])), dev(u32(keys) + bytes(4))
        outs = [dev(nbytes=k) for k in sizes_out]
        d_vst = dev(nbytes=N)
        d_soff = dev(nbytes=8 * (N + 1))

        def run(share_off, verify=False):
            for b, k in zip(outs, sizes_out):
                b.upload(b"\xEE" * k)
            d_soff.upload(u64(share_off))
            eng.batch_collect_keyed_bitmap_device(d_msgs.ptr, d_moff.ptr, d_shares.ptr, d_keys.ptr, d_soff.ptr, n_shares, N, BM,
                                                  *(b.ptr for b in outs), stream=stream.handle)
            if verify:
                eng.batch_verify_keyed_bitmap_device(d_msgs.ptr, d_moff.ptr, outs[2].ptr, outs[3].ptr, BM, N, d_vst.ptr, stream=stream.handle)
            stream.synchronize()
            raw = [b.download(k) for b, k in zip(outs, sizes_out)]
            return raw[0], raw[1], raw[2], list(struct.unpack("<%dI" % (BM * N), raw[3])), list(struct.unpack("<%dI" % N, raw[4]))

        same(run(soff, verify=True), many["want"], "valid offsets")
        assert d_vst.download(N) == bytes(N)
        i = 255
        rev = soff[:]
        rev[i + 1] = soff[i] - 1                     # tuple 255 reversed; tuple 256 then starts before the earlier offset soff[255]
        want, refused, anew = expect_for(c, many, rev)
        assert refused == {255, 256} and not anew and want[0].count(2) == many["sizes"][255] + many["sizes"][256]
        same(run(rev), want, "reversed at 255")
        i = WAVE_BLOCKS - 1
        rev = soff[:]
        rev[i + 1] = soff[i] - 1
        want, refused, anew = expect_for(c, many, rev)
        assert refused == {WAVE_BLOCKS - 1, WAVE_BLOCKS} and not anew and want[0].count(2) == 64 + 70
        same(run(rev), want, "reversed at 65 535")
        i = WAVE_BLOCKS + 4
        lap = soff[:]
        lap[i + 1] = soff[i + 2]                     # tuple 65 540 swallows the 20 shares of 65 541, which is left a reversed range;
        lap[i + 2] = soff[i + 1]                     # ... and 65 542 then starts before the earlier offset soff[65 542]
        want, refused, anew = expect_for(c, many, lap)
        assert refused == {i + 1, i + 2} and anew == {i} and want[0].count(2) == many["sizes"][i + 2] == 1
        assert want[0][soff[i + 1]:soff[i + 2]] == bytes([9]) * 20 and want[4][i] == many["want"][4][i]
        same(run(lap), want, "swallowed at 65 540")
        past = soff[:]
        past[N] = n_shares + 1                       # the last tuple runs past n_shares
        want, refused, anew = expect_for(c, many, past)
        assert refused == {N - 1} and not anew and want[0].count(2) == 70
        same(run(past), want, "past n_shares")
        same(run(soff), many["want"], "valid offsets again")
    finally:
        for b in bufs:
            b.free()
        stream.destroy()
