"""The compressed decoders and the verify from compressed encodings on the device, against the case set of tests/codec_cases.py: every
expected status and byte comes from that builder (its restated arithmetic, the C oracle's points, the big-integer model's subgroup
verdict) — none from the device.  The same cases run on the host builds of the decoders in tests/test_codec_cases.py, so a failure here
alone points at a kernel (the wave vote, dead lanes, the launch code), a failure in both at the shared source.  Run with -m gpu."""

import pytest

from tests import codec_cases as cc
from tests.conftest import ws_default

pytestmark = pytest.mark.gpu

NONET_DEFAULT = ws_default("NONET_MAX_BATCH_DEFAULT")
LM_DEFAULT = ws_default("LM_MAX_BATCH_DEFAULT")
TRIO_DEFAULT = ws_default("TRIO_MAX_BATCH_DEFAULT")
SETTINGS = ((LM_DEFAULT, NONET_DEFAULT, 1, TRIO_DEFAULT), (0, NONET_DEFAULT, 1, TRIO_DEFAULT), (2048, 1500, 0, 4096), (700, 5000, 1, 5000))
PAIR_WG_ITEMS = 128                      # k_decompress_g2_pair: 256 lanes, two per item
ODD_CUTS = (1, 2, 7, 63, 65, 127, 129, 1025, 1535, 1665, 4097, 16385)
ALL_ROUTES = {(0, 0), (0, 1), (1, 1), (1, 2), (2, 3), (0, 2)}


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


def _set_thresholds(eng, lm, nonet, wide, trio):
    from bn254_amd.engine import OPT_LM_MAX_BATCH, OPT_NONET_MAX_BATCH, OPT_NONET_WIDE, OPT_TRIO_MAX_BATCH
    eng.set_option(OPT_LM_MAX_BATCH, lm); eng.set_option(OPT_NONET_MAX_BATCH, nonet)
    eng.set_option(OPT_NONET_WIDE, wide); eng.set_option(OPT_TRIO_MAX_BATCH, trio)


def _route(table, n):
    return next((miller, fe) for max_n, miller, fe in table if n <= max_n)


def _boundary_cuts(eng):
    """{setting: (route table, [n - 1, n, n + 1 for every row])} for the default thresholds and the three other settings of the routing-table test"""
    out = {}
    try:
        for st in SETTINGS:
            _set_thresholds(eng, *st)
            table = eng.route_table()
            out[st] = (table, [n for max_n, _, _ in table[:-1] for n in (max_n - 1, max_n, max_n + 1) if n >= 1])
    finally:
        _set_thresholds(eng, *SETTINGS[0])
    return out


def _round_robin(cases, kinds):
    by = [[cs for cs in cases if cs.kind == k and cs.status != 0] for k in kinds]
    out = []
    for j in range(max(len(b) for b in by)):
        out += [b[j] for b in by if j < len(b)]
    return out


class Batch:
    """n tuples of tests/datagen.make_verify_batch, compressed by the builder's byte logic, with case-set faults planted in signatures (every
    third plant), keys (every third) and both (every third): at item 0, the last item, the last item of every cut in `cuts`, the first and last
    item of workgroups, and every 23rd item between.  expected = the model's G1 status, else its G2 status, else make_verify_batch's own byte."""

    def __init__(self, eng, derived, n, cuts, corrupt_every):
        from tests.datagen import make_verify_batch
        self.n = n
        self.msgs, sigs, pks, base = make_verify_batch(eng, n, corrupt_every=corrupt_every)
        key_cache = {}
        s33, p65 = [], []
        for i in range(n):
            s33.append(cc.g1_compress(sigs[64 * i:64 * i + 64]))
            k = pks[128 * i:128 * i + 128]
            if k not in key_cache:
                key_cache[k] = cc.g2_compress(k)
            p65.append(key_cache[k])
        self.clean = (b"".join(s33), b"".join(p65), base)
        g1_bad = _round_robin(cc.g1_cases(), cc.G1_KINDS)
        g2_bad = _round_robin(cc.g2_cases(derived["g2_not_in_subgroup"]), cc.G2_KINDS)
        wg = [w * PAIR_WG_ITEMS + d for w in (1, 2, n // PAIR_WG_ITEMS - 1, n // PAIR_WG_ITEMS) for d in (-1, 0)]
        pos = sorted({p for p in [0, n - 1] + [k - 1 for k in cuts] + wg + list(range(20, n, 23)) if 0 <= p < n})
        expected = bytearray(base)
        self.plants = {}
        for j, p in enumerate(pos):
            g1 = g1_bad[(j // 3 * 2 + (j % 3 == 2)) % len(g1_bad)] if j % 3 != 1 else None
            g2 = g2_bad[(j // 3 * 2 + (j % 3 == 2)) % len(g2_bad)] if j % 3 != 0 else None
            if g1:
                s33[p] = g1.enc
            if g2:
                p65[p] = g2.enc
            expected[p] = g1.status if g1 else g2.status
            self.plants[p] = (g1, g2)
        self.s33, self.p65, self.expected = b"".join(s33), b"".join(p65), bytes(expected)
        both = [p for p, (a, b) in self.plants.items() if a and b]
        assert both and {a.status for a, b in self.plants.values() if a} == {3, 6} == {b.status for a, b in self.plants.values() if b}
        assert any(self.plants[p][0].status != self.plants[p][1].status for p in both)      # signature before key shows
        assert {b.kind for a, b in self.plants.values() if b} == set(cc.G2_KINDS) - {"valid random"}
        assert 0 in self.plants and n - 1 in self.plants and {0, 9} <= set(expected)

    def cut(self, n, planted=True):
        s, p, e = (self.s33, self.p65, self.expected) if planted else self.clean
        return self.msgs[:n], s[:33 * n], p[:65 * n], e[:n]


@pytest.fixture(scope="module")
def big(eng, derived):
    cuts = sorted({n for _, ns in _boundary_cuts(eng).values() for n in ns} | set(ODD_CUTS))
    return Batch(eng, derived, TRIO_DEFAULT + 2, cuts, corrupt_every=13)


# ---- the decoders ----------------------------------------------------------------------------------------------------------------------
def _check_decoder(run, cases, size, where):
    out, st = run(b"".join(cs.enc for cs in cases), len(cases))
    bad = [(i, cs.kind, cs.enc.hex(), st[i], cs.status) for i, cs in enumerate(cases) if st[i] != cs.status]
    assert not bad, (where, len(bad), bad[:5])
    # a failed item's output is all-zero bytes: what k_g1_decompress / k_g2_decompress write today (p.inf -> the identity's encoding)
    bad = [(i, cs.kind, cs.enc.hex()) for i, cs in enumerate(cases) if out[size * i:size * i + size] != (cs.want or bytes(size))]
    assert not bad, (where, len(bad), bad[:5])


@pytest.mark.parametrize("group", ["g1", "g2"])
def test_decoders_on_the_whole_case_set_in_three_orders_and_ragged_cuts(eng, derived, group):
    """batch_g1_decompress / batch_g2_decompress: every case, as built, with every wave mixing valid and failing items, and with waves of
    failing items only (one of them with a single valid item among 63 failures); whole, and cut to sizes around the wave"""
    cases = cc.g1_cases() if group == "g1" else cc.g2_cases(derived["g2_not_in_subgroup"])
    run, size = (eng.batch_g1_decompress, 64) if group == "g1" else (eng.batch_g2_decompress, 128)
    for name, order in cc.orders(cases).items():
        _check_decoder(run, order, size, (name, "whole"))
        for k in cc.CUTS:
            _check_decoder(run, order[:k], size, (name, k, 0))
            _check_decoder(run, order[cc.WAVE:cc.WAVE + k], size, (name, k, cc.WAVE))       # "failing waves": the wave with the single valid item first
    prof = cc.wave_profile(cc.orders(cases)["failing waves"])
    assert prof[0] == cc.WAVE and prof[1] == cc.WAVE - 1


# ---- verify from compressed encodings on every decoder -----------------------------------------------------------------------------------
def _decoder(eng_state, n):
    lm, pair = eng_state
    return "lane machine" if pair and lm > 0 and n <= lm else ("pair lanes" if pair else "one lane")


def _verify_cut(eng, big, n, where):
    msgs, s33, p65, want = big.cut(n)
    got = eng.batch_verify_compressed(msgs, s33, p65)
    bad = [(i, got[i], want[i], tuple(cs and cs.kind for cs in big.plants.get(i, ()))) for i in range(n) if got[i] != want[i]]
    assert not bad, (where, n, len(bad), bad[:6])


def test_verify_compressed_on_every_route_and_every_decoder(eng, big):
    """bn254_batch_verify_compressed with planted faults at n - 1, n, n + 1 of every row of the routing table, under the default thresholds and
    three other settings, at odd sizes (dead lanes in the last workgroup of the lane-pair decoder), and with the lane machine / the lane
    pairs switched off: all six (miller, fe) routes and all three G2 decoders (k_decompress_g2_pair + bn254_lm_g2_subgroup, k_decompress_g2_pair
    with its own ladder, k_decompress_g2_ws) see malformed input"""
    from bn254_amd.engine import OPT_LM_MAX_BATCH, OPT_PAIR_LANES
    default = eng.route_table()
    assert default == [(1024, 0, 0), (LM_DEFAULT, 0, 1), (NONET_DEFAULT, 1, 1), (TRIO_DEFAULT, 1, 2), (2 ** 64 - 1, 2, 3)], default
    assert big.n >= TRIO_DEFAULT + 2
    routes, decoders = set(), set()
    boundary = _boundary_cuts(eng)
    try:
        for st in SETTINGS:
            _set_thresholds(eng, *st)
            table, ns = boundary[st]
            assert eng.route_table() == table
            for n in ns + (list(ODD_CUTS) if st == SETTINGS[0] else []):
                _verify_cut(eng, big, n, st)
                routes.add(_route(table, n)); decoders.add(_decoder((st[0], 1), n))
        _set_thresholds(eng, *SETTINGS[0])
        eng.set_option(OPT_LM_MAX_BATCH, 0)                       # the lane-pair decoder with its own ladder at the small sizes too
        for n in list(ODD_CUTS) + boundary[SETTINGS[1]][1]:
            _verify_cut(eng, big, n, "OPT_LM_MAX_BATCH = 0")
            decoders.add(_decoder((0, 1), n))
        eng.set_option(OPT_LM_MAX_BATCH, LM_DEFAULT)
        eng.set_option(OPT_PAIR_LANES, 0)                         # one lane per item: k_decompress_g2_ws
        for n in (1, 63, 64, 65, 129, 1537, 4097):
            _verify_cut(eng, big, n, "OPT_PAIR_LANES = 0")
            decoders.add(_decoder((LM_DEFAULT, 0), n))
    finally:
        eng.set_option(OPT_PAIR_LANES, 1)
        _set_thresholds(eng, *SETTINGS[0])
    assert routes >= ALL_ROUTES, routes
    assert decoders == {"lane machine", "pair lanes", "one lane"}, decoders
    assert eng.route_table() == default


def test_verify_compressed_65536_tuples_on_the_default_route(eng, derived):
    n = 65536
    b = Batch(eng, derived, n, (n,), corrupt_every=64)
    assert _route(eng.route_table(), n) == (2, 3)
    _verify_cut(eng, b, n, "65536")
    assert sum(1 for x in b.expected if x not in (0, 9)) >= n // 23 and len(b.plants) >= n // 23


def test_compressed_expectations_of_the_parity_file_hold_against_the_model(eng, big):
    """the unplanted batch verifies as make_verify_batch says (no decoder answer is taken from the device)"""
    msgs, s33, p65, want = big.cut(2000, planted=False)
    assert eng.batch_verify_compressed(msgs, s33, p65) == want and set(want) == {0, 9}


# ---- the device entry point --------------------------------------------------------------------------------------------------------------
def _dev_bytes(torch, dev, data, lead=0):
    """a device tensor holding `lead` filler bytes and then data; returns (tensor, pointer to the data)"""
    t = torch.frombuffer(bytearray(b"\xa5" * lead + bytes(data)), dtype=torch.uint8).to(dev)
    return t, t.data_ptr() + lead


def test_device_entry_point_streams_slices_and_unaligned_buffers(big):
    """Engine.batch_verify_compressed_device (bn254_batch_verify_compressed_device called directly) against the host call and the model-derived
    expectation: on the context's stream, on a caller's stream, sliced on the device (BN254_OPT_MAX_CHUNK 1000 and n - 1: the compressed
    slicing lambda with its 33 * lo / 65 * lo strides), and with both encodings starting one byte into their allocations (strides of 33 and 65
    bytes: byte loads, no alignment rule)"""
    import bn254_amd
    import torch
    from bn254_amd.engine import OPT_MAX_CHUNK
    dev = torch.device("cuda", 0)
    n = 2500
    msgs, s33, p65, want = big.cut(n)
    assert {0, 3, 6, 9} <= set(want)
    offs = [0]
    for msg in msgs:
        offs.append(offs[-1] + len(msg))
    d_msgs, p_msgs = _dev_bytes(torch, dev, b"".join(msgs))
    d_off = torch.tensor(offs, dtype=torch.int64, device=dev)
    fresh = bn254_amd.Engine(0)
    try:
        assert fresh.batch_verify_compressed(msgs, s33, p65) == want
        caller = torch.cuda.Stream(device=dev)
        for name, chunk, lead, stream in (("context stream", 0, 0, None), ("caller stream", 0, 0, caller), ("chunk 1000", 1000, 0, None),
                                          ("chunk n - 1", n - 1, 0, caller), ("one byte in", 0, 1, None), ("one byte in, sliced", 333, 1, caller)):
            fresh.set_option(OPT_MAX_CHUNK, chunk)
            d_s, p_s = _dev_bytes(torch, dev, s33, lead)
            d_p, p_p = _dev_bytes(torch, dev, p65, lead)
            assert (p_s & 3) == lead and (p_p & 3) == lead
            d_st = torch.full((n + 16,), 0xEE, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            if stream is None:
                fresh.batch_verify_compressed_device(p_msgs, d_off.data_ptr(), p_s, p_p, n, d_st.data_ptr() + 8)
                fresh.synchronize()
            else:
                with torch.cuda.stream(stream):
                    fresh.batch_verify_compressed_device(p_msgs, d_off.data_ptr(), p_s, p_p, n, d_st.data_ptr() + 8, stream=stream.cuda_stream)
                stream.synchronize()
            got = bytes(d_st.cpu().numpy())
            assert got[:8] == b"\xee" * 8 == got[8 + n:], name         # nothing outside the n status bytes
            got = got[8:8 + n]
            bad = [(i, got[i], want[i]) for i in range(n) if got[i] != want[i]]
            assert not bad, (name, len(bad), bad[:6])
            del d_s, d_p
    finally:
        fresh.close()


def test_device_entry_point_argument_checks(eng):
    """a d_msg_off that is not 8-byte aligned is BN254_E_MISALIGNED, null arguments are BN254_E_BAD_ARGUMENT (both refused before any access:
    pointer VALUES only), n = 0 returns 0 and writes nothing"""
    import torch
    L, h = eng._lib, eng._h
    f = L.bn254_batch_verify_compressed_device
    p, off = 0x7F0000001000, 0x7F0000100000
    assert f(h, p, off + 4, p + 4096, p + 8192, 2, p + 12288, None) == -10002
    assert f(h, p, off + 1, p + 4096, p + 8192, 2, p + 12288, None) == -10002
    for hole in range(5):
        args = [p, off, p + 4096, p + 8192, p + 12288]
        args[hole] = None
        assert f(h, args[0], args[1], args[2], args[3], 2, args[4], None) == -10001, hole
    assert f(None, p, off, p + 4096, p + 8192, 0, p + 12288, None) == -10001
    d_st = torch.full((8,), 0xEE, dtype=torch.uint8, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert f(h, None, None, None, None, 0, d_st.data_ptr(), None) == 0
    eng.batch_verify_compressed_device(None, None, None, None, 0, d_st.data_ptr())
    eng.synchronize()
    assert d_st.cpu().tolist() == [0xEE] * 8


def test_device_entry_point_bound_checks_message_offsets(eng, big):
    """as test_device_entry_points_bound_check_message_offsets does for the uncompressed call: a reversed span, or — once
    bn254_ctx_expect_msgs_len has declared the buffer — a span past it, reports 5 and is never read; every other item its expected byte"""
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    for n in (70, 5000):
        msgs, s33, p65, want = big.cut(n, planted=False)
        assert all(len(x) == 32 for x in msgs) and want[3] == 0 and want[n - 2] == 0 and want[n - 1] == 0
        blob = b"".join(msgs)
        off = [32 * i for i in range(n + 1)]
        d_msgs, p_msgs = _dev_bytes(torch, dev, blob)
        d_s, p_s = _dev_bytes(torch, dev, s33)
        d_p, p_p = _dev_bytes(torch, dev, p65)
        for declare in (True, False):
            bad = list(off)
            bad[4] = off[3] - 1            # item 3 reversed -> 5; item 4 = [off[3] - 1, off[5]) is another message: not compared
            exp = bytearray(want)
            exp[3] = 5
            if declare:
                bad[n - 1] = len(blob) + (1 << 40)        # item n-2 runs past the buffer, item n-1 = [huge, off[n]) is reversed
                exp[n - 2] = exp[n - 1] = 5
                eng.expect_msgs_len(len(blob))
            else:
                bad[n] = off[n - 1] - 1                   # undeclared size: only reversed pairs can be seen — item n-1
                exp[n - 1] = 5
            d_off = torch.tensor(bad, dtype=torch.int64, device=dev)
            d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
            torch.cuda.synchronize()
            eng.batch_verify_compressed_device(p_msgs, d_off.data_ptr(), p_s, p_p, n, d_st.data_ptr(), stream=stream.cuda_stream)
            stream.synchronize()
            got = d_st.cpu().numpy().tobytes()
            diff = [(i, got[i], exp[i]) for i in range(n) if i != 4 and got[i] != exp[i]]
            assert not diff, (n, declare, diff[:10])
            assert got[4] in (5, 9)
