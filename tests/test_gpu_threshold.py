"""Threshold signatures over the registered keys (include/bn254_hip.h: bn254_batch_threshold_combine_keyed[_device]) on the GPU: every key
set and tuple shape of tests/threshold_cases.py through the host form, the dealt 5-of-9 set through the _device form as well.
Identity 1: the share statuses are bn254_batch_verify_keyed's on the tuple's message repeated.  The rows, the counts and the tuple statuses
against tests/threshold_model.py; the group signatures against BOTH expectations — sum lambda_j sigma_j in Python integers and the model's
group operations (any key set), and for dealt keys the model's signature under f(0).  The closed loop: bn254_batch_verify under the group
key that ECDSA.threshold_group_key interpolates.  Both layouts of the sum, a slice length that splits tuples, a stale workspace, no keys
registered, a key with a failed proof of possession, refused arguments, and the Python and C++ mirrors.  Run on the MI355X box: -m gpu."""
import ctypes
import os
import subprocess

import pytest

from bn254_amd import engine as E
from tests import threshold_cases as TC
from tests import threshold_model as TM
from tests.datagen import D

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = TC.R


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def derive(eng, sks):
    """share keys sk * G2; the secret 0 is the identity key (128 zero bytes)"""
    out, st = eng.batch_g2_mul(None, b"".join((s or 1).to_bytes(32, "big") for s in sks), len(sks), reduce_scalar=True)
    assert st == bytes(len(sks))
    return [out[128 * j:128 * j + 128] if s else bytes(128) for j, s in enumerate(sks)]


def plant(eng, c, name, secrets, shapes, n_keys):
    """the tuple shapes as tuples (message, [(share, key)]): valid shares signed on the device, the faulty ones made from them"""
    msgs = [D("threshold/" + name, i) for i in range(len(shapes))]
    plan = [(i, key, kind) for i, (_, shape) in enumerate(shapes) for key, kind in shape]
    sigs, st = eng.batch_sign([msgs[i] for i, _, _ in plan], b"".join((secrets[key] or 1).to_bytes(32, "big") for _, key, _ in plan)) if plan else (b"", b"")
    assert st == bytes(len(plan))
    g1 = c.g1_generator()
    tuples = [(m, []) for m in msgs]
    for s, (i, key, kind) in enumerate(plan):
        sg = sigs[64 * s:64 * s + 64] if secrets[key] else bytes(64)
        if kind == "again":
            sg, key = tuples[i][1][-1]
        elif kind == "wrong":
            sg = c.g1_add(sg, g1)
        elif kind == "curve":
            sg = bytearray(sg); sg[40] ^= 4; sg = bytes(sg)
        elif kind == "big":
            sg = b"\xff" + sg[1:]
        elif kind == "oob":
            key = n_keys + 3
        tuples[i][1].append((sg, key))
    return tuples


def flat(tuples):
    return ([t[0] for t in tuples], [s for t in tuples for s, _ in t[1]], [k for t in tuples for _, k in t[1]], [len(t[1]) for t in tuples])


def combine(eng, tuples, bm_words, t, flags=0):
    msgs, shares, keys, sizes = flat(tuples)
    return eng.batch_threshold_combine_keyed(msgs, b"".join(shares), keys, sizes, bm_words, t, flags=flags)


def keyed(eng, tuples, flags=0):
    msgs, shares, keys, sizes = flat(tuples)
    rep = [m for m, k in zip(msgs, sizes) for _ in range(k)]
    return eng.batch_verify_keyed(rep, b"".join(shares), keys, flags=flags) if rep else b""


def expected(tuples, share_st, bm_words, t, f0):
    """-> (tuple statuses, rows, counts, group signatures by expectation 1, by expectation 2 or None)"""
    msgs, shares, keys, sizes = flat(tuples)
    sel = TM.select(keys, share_st, sizes, [0] * len(tuples), bm_words, t)
    e1 = [TM.group_signature(shares, chosen) if st == 0 else bytes(64) for st, _, _, chosen in sel]
    e2 = None if f0 is None else [TM.signature_under(m, f0) if st == 0 else bytes(64) for m, (st, _, _, _) in zip(msgs, sel)]
    return bytes(st for st, _, _, _ in sel), [w for _, _, row, _ in sel for w in row], [count for _, count, _, _ in sel], b"".join(e1), e2


class KeySet:
    def __init__(self, eng, c, spec):
        self.name, self.n_keys, dealt_t, secret = spec
        self.t = TC.threshold_of(self.name, dealt_t)
        self.secrets, self.f0 = TC.secrets_of(self.name, self.n_keys, dealt_t, secret)
        self.pks = derive(eng, self.secrets)
        self.bm_words = (self.n_keys + 31) // 32
        self.shapes = TC.shapes_for(self.name, self.n_keys, self.t)
        self.register(eng)
        self.tuples = plant(eng, c, self.name, self.secrets, self.shapes, self.n_keys)
        self.share_st = keyed(eng, self.tuples)
        self.want = expected(self.tuples, self.share_st, self.bm_words, self.t, self.f0)

    def register(self, eng):
        assert eng.register_keys(b"".join(self.pks)) == bytes(self.n_keys)


@pytest.fixture(scope="module")
def sets(eng, c):
    """every key set of the case set with its tuples, the keyed verify's statuses and both expectations, computed once"""
    return {spec[0]: KeySet(eng, c, spec) for spec in TC.KEY_SETS}


def check(ks, got, label):
    share_st, tuple_st, group, bits, counts = got
    w_tuple, w_bits, w_counts, e1, e2 = ks.want
    assert share_st == ks.share_st, (label, [(i, a, b) for i, (a, b) in enumerate(zip(share_st, ks.share_st)) if a != b][:8])
    assert tuple_st == w_tuple, (label, list(tuple_st), list(w_tuple))
    assert bits == w_bits and counts == w_counts, label
    names = [s[0] for s in ks.shapes]
    assert group == e1, (label, [names[i] for i in range(len(names)) if group[64 * i:64 * i + 64] != e1[64 * i:64 * i + 64]])
    if e2 is not None:
        assert group == b"".join(e2), (label, [names[i] for i in range(len(names)) if group[64 * i:64 * i + 64] != e2[i]])


@pytest.mark.parametrize("name", [spec[0] for spec in TC.KEY_SETS])
def test_every_case_host_form(eng, sets, name):
    ks = sets[name]
    ks.register(eng)
    # the kinds earn the statuses the case set names (identity 1 is what check() holds the call to)
    kinds = [kind for _, shape in ks.shapes for _, kind in shape]
    at = 0
    for kind in kinds:
        if kind != "again":
            assert ks.share_st[at] == TC.KIND_STATUS[kind], (kind, at)
        at += 1
    got = combine(eng, ks.tuples, ks.bm_words, ks.t)
    check(ks, got, name)
    by = {s[0]: i for i, s in enumerate(ks.shapes)}
    tuple_st, group, bits, counts = got[1], got[2], got[3], got[4]
    G = lambda i: group[64 * i:64 * i + 64]      # noqa: E731
    if "t_minus_1" in by:
        i = by["t_minus_1"]
        assert tuple_st[i] == 9 and G(i) == bytes(64) and counts[i] == ks.t - 1
        assert sum(bin(w).count("1") for w in bits[i * ks.bm_words:(i + 1) * ks.bm_words]) == ks.t - 1           # the row is V: who is there
    for i in range(len(ks.shapes)):
        if tuple_st[i] == 0:
            assert sum(bin(w).count("1") for w in bits[i * ks.bm_words:(i + 1) * ks.bm_words]) == ks.t and counts[i] >= ks.t
    if name == "dealt9_t5":
        assert tuple_st[by["empty"]] == 9 and tuple_st[by["all_bad"]] == 9 and counts[by["all_bad"]] == 0
        assert bits[by["more_than_t"]] == 0x1F and bits[by["upper_keys"]] == 0x1F0 and bits[by["low_big"]] == 0x3D and bits[by["low_oob_short"]] == 0x1D
    if name == "zero9_t5":
        assert tuple_st[by["exactly_t"]] == 0 and G(by["exactly_t"]) == bytes(64)                                    # f(0) = 0: the identity
    if name == "ident9":
        assert (bits[by["exactly_t"]] >> TC.IDENT_KEY) & 1 and ks.pks[TC.IDENT_KEY] == bytes(128)
    if name.startswith("dealt70"):
        i = by["everybody"]
        row = bits[i * 3:i * 3 + 3]
        assert row == [(1 << min(32, max(0, ks.t - 32 * w))) - 1 for w in range(3)] and counts[i] == 70


def test_subsets_of_one_message(eng, sets):
    """one message, three subsets as three tuples: keys of one polynomial give the same point whatever subset signed — the model's
    signature under f(0) —, independent keys give three different points, each the model's weighted sum"""
    subsets = [[0, 1, 2, 3, 4], [8, 2, 4, 6, 7], [4, 5, 6, 7, 8]]
    msg = D("threshold/one message", 0)
    for name in ("dealt9_t5", "random9"):
        ks = sets[name]
        ks.register(eng)
        plan = [j for sub in subsets for j in sub]
        sigs, st = eng.batch_sign([msg] * len(plan), b"".join(ks.secrets[j].to_bytes(32, "big") for j in plan))
        assert st == bytes(len(plan))
        shares = [sigs[64 * s:64 * s + 64] for s in range(len(plan))]
        share_st, tuple_st, group, bits, counts = eng.batch_threshold_combine_keyed([msg] * 3, sigs, plan, [5, 5, 5], 1, 5)
        assert share_st == bytes(15) and tuple_st == bytes(3) and counts == [5, 5, 5]
        assert bits == [sum(1 << j for j in sub) for sub in subsets]
        got = [group[64 * i:64 * i + 64] for i in range(3)]
        want = [TM.group_signature(shares, [(j, 5 * i + k) for k, j in sorted(enumerate(sub), key=lambda kj: kj[1])]) for i, sub in enumerate(subsets)]
        assert got == want, name
        if ks.f0 is not None:
            assert got[0] == got[1] == got[2] == TM.signature_under(msg, ks.f0)
        else:
            assert len(set(got)) == 3


def test_closed_loop_under_the_group_key(eng, sets):
    """dealt keys: the group key interpolated from t share keys (two different subsets: the same key) is f(0) * G2, and bn254_batch_verify
    accepts every group signature of a tuple with status 0 under it"""
    from bn254_amd.api import ECDSA, PublicKey
    for name in ("dealt9_t5", "dealt9_t2", "dealt70_t64"):
        ks = sets[name]
        ks.register(eng)
        _, tuple_st, group, _, _ = combine(eng, ks.tuples, ks.bm_words, ks.t)
        low = list(range(ks.t))
        high = list(range(ks.n_keys - 1, ks.n_keys - 1 - ks.t, -1))
        gk = ECDSA.threshold_group_key(low, [PublicKey(ks.pks[j]) for j in low], engine=eng)
        assert gk.raw == ECDSA.threshold_group_key(high, [PublicKey(ks.pks[j]) for j in high], engine=eng).raw == derive(eng, [ks.f0])[0]
        ok = [i for i in range(len(ks.tuples)) if tuple_st[i] == 0]
        assert len(ok) >= 2
        st = eng.batch_verify([ks.tuples[i][0] for i in ok], b"".join(group[64 * i:64 * i + 64] for i in ok), gk.raw * len(ok), flags=0)
        assert st == bytes(len(ok)), (name, list(st))
        # ... and a failed tuple's zero signature does not verify under it
        bad = [i for i in range(len(ks.tuples)) if tuple_st[i] == 9][:1]
        assert bad and eng.batch_verify([ks.tuples[bad[0]][0]], bytes(64), gk.raw, flags=0) == b"\x09"


DEFAULTS = {E.OPT_PAIR_LANES: 1, E.OPT_MAX_CHUNK: 0, E.OPT_COLLECT_WAVE_MIN_SHARES: 16}
ROUTES = [("pair_lanes_off", {E.OPT_PAIR_LANES: 0}), ("sliced", {E.OPT_MAX_CHUNK: 3}), ("all_waves", {E.OPT_COLLECT_WAVE_MIN_SHARES: 1}),
          ("all_lanes", {E.OPT_COLLECT_WAVE_MIN_SHARES: 1 << 30})]


def with_options(eng, opts, fn):
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            eng.set_option(k, DEFAULTS[k])


@pytest.mark.parametrize("route", [r[0] for r in ROUTES])
def test_routes_give_the_same_bytes(eng, sets, route):
    """lane and wave layouts of both sums forced, a slice length that splits every tuple's shares, one lane per verify: the default call's bytes"""
    opts = dict(ROUTES)[route]
    for name in ("dealt9_t5", "dealt70_t65"):
        ks = sets[name]
        ks.register(eng)
        check(ks, with_options(eng, opts, lambda: combine(eng, ks.tuples, ks.bm_words, ks.t)), (name, route))


def test_stage_intervals(eng, sets):
    """bn254_ctx_last_kernel_ms after a profiled threshold call (the collect's events, the interpolation inside its last interval): four
    non-negative intervals, and the shares' Miller loop among them"""
    ks = sets["dealt9_t5"]
    ks.register(eng)
    try:
        eng.set_profiling(True)
        got = combine(eng, ks.tuples, ks.bm_words, ks.t)
        ms = eng.last_kernel_ms()
    finally:
        eng.set_profiling(False)
    print("threshold ms", ms)
    check(ks, got, "profiled")
    assert len(ms) == 4 and all(v >= 0 for v in ms.values()) and ms["miller_loop"] > 0


def test_flags_and_wider_bitmap(eng, sets):
    """BN254_FLAG_REJECT_IDENTITY: the identity key's all-zero share reads 4 and the key drops out; a bitmap wider than the key set"""
    ks = sets["ident9"]
    ks.register(eng)
    want_st = keyed(eng, ks.tuples, flags=2)
    assert want_st != ks.share_st and 4 in want_st
    got = combine(eng, ks.tuples, ks.bm_words, ks.t, flags=2)
    w_tuple, w_bits, w_counts, e1, _ = expected(ks.tuples, want_st, ks.bm_words, ks.t, None)
    assert got == (want_st, w_tuple, e1, w_bits, w_counts)
    ks9 = sets["dealt9_t5"]
    ks9.register(eng)
    wide = combine(eng, ks9.tuples, 3, ks9.t)
    base = combine(eng, ks9.tuples, 1, ks9.t)
    assert wide[:3] == base[:3] and wide[4] == base[4] and wide[3] == [w for b in base[3] for w in (b, 0, 0)]


def test_stale_workspace_and_threshold_above_the_set(eng, sets):
    """a larger call first, then a small one: nothing of the first shows; then thresholds the set cannot meet"""
    big, small = sets["dealt70_t64"], sets["dealt9_t2"]
    big.register(eng)
    check(big, combine(eng, big.tuples, big.bm_words, big.t), "big first")
    small.register(eng)
    check(small, combine(eng, small.tuples, small.bm_words, small.t), "small after big")
    for t in (10, 1000, (1 << 32) - 1):
        share_st, tuple_st, group, bits, counts = combine(eng, small.tuples, small.bm_words, t)
        assert share_st == small.share_st and tuple_st == bytes([9]) * len(small.tuples) and group == bytes(64 * len(small.tuples))
        sel = TM.select(flat(small.tuples)[2], share_st, flat(small.tuples)[3], [0] * len(small.tuples), 1, t)
        assert bits == [w for _, _, row, _ in sel for w in row] and counts == [n for _, n, _, _ in sel] and max(counts) == 9


def test_no_keys_registered(eng, c, sets):
    """an empty key set: every decodable share reads 2, every tuple 9 with an empty row; then the set again (no stale state)"""
    ks = sets["dealt9_t5"]
    try:
        eng.register_keys(b"")
        share_st, tuple_st, group, bits, counts = combine(eng, ks.tuples, 0, ks.t)
        shares = flat(ks.tuples)[1]
        assert list(share_st) == [c.g1_validate(s, 0) or 2 for s in shares]
        assert tuple_st == bytes([9]) * len(ks.tuples) and group == bytes(64 * len(ks.tuples)) and counts == [0] * len(ks.tuples) and bits == []
    finally:
        ks.register(eng)
    check(ks, combine(eng, ks.tuples, ks.bm_words, ks.t), "registered again")


def test_key_with_a_failed_proof_of_possession(eng, sets):
    """the dealt set registered with its proofs, key 1 presenting key 0's: every share of key 1 reads 9, the key is in no row, and the
    four other lowest keys with key 5 still interpolate to the group signature"""
    ks = sets["dealt9_t5"]
    try:
        pks, pops, st = eng.batch_pop_prove(b"".join(s.to_bytes(32, "big") for s in ks.secrets))
        assert st == bytes(9) and pks == b"".join(ks.pks)
        proofs = pops[:64] + pops[:64] + pops[128:]
        assert eng.register_keys_pop(pks, proofs) == bytes([0, 9, 0, 0, 0, 0, 0, 0, 0])
        i = [s[0] for s in ks.shapes].index("more_than_t")
        share_st, tuple_st, group, bits, counts = combine(eng, [ks.tuples[i]], 1, ks.t)
        assert list(share_st) == [0, 9, 0, 0, 0, 0, 0, 0, 0] == list(keyed(eng, [ks.tuples[i]]))
        assert tuple_st == b"\0" and bits == [0x3D] and counts == [8] and group == ks.want[4][i]
    finally:
        ks.register(eng)


def test_refused_arguments(eng, sets):
    ks = sets["dealt9_t5"]
    ks.register(eng)
    msgs, shares, keys, sizes = flat(ks.tuples)
    n, n_shares = len(msgs), len(keys)
    blob, off = E.pack_messages(msgs)
    soff = [sum(sizes[:i]) for i in range(n + 1)]
    sst, tst, sig, bits = (ctypes.create_string_buffer(k) for k in (n_shares + 8, n + 8, 64 * n, 4 * n))
    k32 = (ctypes.c_uint32 * n_shares)(*keys)

    def call(threshold=5, bm_words=1, share_off=soff, n_sh=n_shares):
        return eng._lib.bn254_batch_threshold_combine_keyed(eng._h, bytes(blob), off, b"".join(shares), k32, (ctypes.c_uint64 * (n + 1))(*share_off), n_sh, n,
                                                            bm_words, threshold, 0, sst, tst, sig, bits, None)
    assert call() == 0 and tst.raw[:n] == ks.want[0]                   # n_valid may be NULL
    assert call(threshold=0) == -10001
    assert call(bm_words=0) == -10001                                   # cannot hold key 8
    for bad in ([1] + soff[1:], soff[:2] + [soff[1] - 1] + soff[3:], soff[:n] + [n_shares - 1], soff[:n] + [n_shares + 1]):
        assert call(share_off=bad) == -10001, bad
    assert eng._lib.bn254_batch_threshold_combine_keyed(eng._h, None, None, None, None, None, 0, 0, 1, 0, 0, None, None, None, None, None) == -10001
    assert eng._lib.bn254_batch_threshold_combine_keyed(eng._h, None, None, None, None, None, 0, 0, 1, 1, 0, None, None, None, None, None) == 0


@pytest.mark.parametrize("name", [spec[0] for spec in TC.KEY_SETS])
def test_every_case_device_form(eng, sets, name):
    """every key set and tuple shape through the _device form on a caller's stream — rows of bm_words words each, n_valid written — held
    to the same expectations as the host form; then again with a slice length that splits the tuples, and without the n_valid array"""
    from tests.hip_ctypes import DevBuf, Stream
    ks = sets[name]
    ks.register(eng)
    msgs, shares, keys, sizes = flat(ks.tuples)
    n, n_shares, bm = len(msgs), len(keys), ks.bm_words
    blob, off = E.pack_messages(msgs)
    soff = [sum(sizes[:i]) for i in range(n + 1)]
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    words = lambda raw, k: [int.from_bytes(raw[4 * j:4 * j + 4], "little") for j in range(k)]   # noqa: E731
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_msgs, d_moff, d_shares, d_keys, d_soff = dev(bytes(blob)), dev(u64(off)), dev(b"".join(shares)), dev(u32(keys) + bytes(4)), dev(u64(soff))
        d_sst, d_tst, d_sig, d_bits, d_cnt = dev(nbytes=n_shares + 4), dev(nbytes=n), dev(nbytes=64 * n), dev(nbytes=4 * bm * n), dev(nbytes=4 * n)

        def run(with_counts=True):
            for b in (d_sst, d_tst, d_sig, d_bits, d_cnt):
                b.upload(b"\xEE" * b.nbytes)
            eng.batch_threshold_combine_keyed_device(d_msgs.ptr, d_moff.ptr, d_shares.ptr, d_keys.ptr, d_soff.ptr, n_shares, n, bm, ks.t, d_sst.ptr, d_tst.ptr,
                                                     d_sig.ptr, d_bits.ptr, d_cnt.ptr if with_counts else None, stream=stream.handle)
            stream.synchronize()
            return (d_sst.download(n_shares), d_tst.download(n), d_sig.download(64 * n), words(d_bits.download(4 * bm * n), bm * n),
                    words(d_cnt.download(4 * n), n))
        got = run()
        check(ks, got, (name, "device"))
        assert got == combine(eng, ks.tuples, bm, ks.t)
        check(ks, with_options(eng, {E.OPT_MAX_CHUNK: 3}, run), (name, "device, sliced"))
        bare = run(with_counts=False)
        assert bare[:4] == got[:4] and bare[4] == [0xEEEEEEEE] * n      # a NULL n_valid: nothing written there, the rest the same
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


def test_device_form(eng, sets):
    """the _device form on a caller's stream: the host form's bytes, a verify under the group key behind it on the same stream with no
    synchronisation in between; a refused share range reads 2 and a reversed message offset 5, both with an empty row and the identity;
    bn254_ctx_expect_msgs_len is honoured; misaligned share keys, a zero threshold and a short bitmap are refused"""
    from tests.hip_ctypes import DevBuf, Stream
    ks = sets["dealt9_t5"]
    ks.register(eng)
    msgs, shares, keys, sizes = flat(ks.tuples)
    n, n_shares, t = len(msgs), len(keys), ks.t
    assert ks.bm_words == 1                            # this set's rows are one word each (wider rows: test_every_case_device_form)
    blob, off = E.pack_messages(msgs)
    off = list(off)
    soff = [sum(sizes[:i]) for i in range(n + 1)]
    gk = derive(eng, [ks.f0])[0]
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_msgs, d_shares, d_keys, d_gk = dev(bytes(blob)), dev(b"".join(shares)), dev(u32(keys) + bytes(4)), dev(gk * n)
        d_sst, d_tst, d_sig, d_bits, d_cnt, d_vst = dev(nbytes=n_shares), dev(nbytes=n), dev(nbytes=64 * n), dev(nbytes=4 * n), dev(nbytes=4 * n), dev(nbytes=n)

        def run(moff, share_off, msgs_len=None, keys_ptr=None, bm_words=1, threshold=t):
            d_moff, d_soff = dev(u64(moff)), dev(u64(share_off))
            if msgs_len is not None:
                eng.expect_msgs_len(msgs_len)
            eng.batch_threshold_combine_keyed_device(d_msgs.ptr, d_moff.ptr, d_shares.ptr, keys_ptr or d_keys.ptr, d_soff.ptr, n_shares, n, bm_words, threshold,
                                                     d_sst.ptr, d_tst.ptr, d_sig.ptr, d_bits.ptr, d_cnt.ptr, stream=stream.handle)
            eng.batch_verify_device(d_msgs.ptr, d_moff.ptr, d_sig.ptr, d_gk.ptr, n, d_vst.ptr, stream=stream.handle)
            stream.synchronize()
            words, cnt = d_bits.download(4 * n), d_cnt.download(4 * n)
            return (d_sst.download(n_shares), d_tst.download(n), d_sig.download(64 * n), [int.from_bytes(words[4 * k:4 * k + 4], "little") for k in range(n)],
                    [int.from_bytes(cnt[4 * k:4 * k + 4], "little") for k in range(n)], d_vst.download(n))
        host = combine(eng, ks.tuples, 1, t)
        check(ks, host, "host")
        got = run(off, soff)
        assert got[:5] == host
        assert all(got[5][i] == (0 if host[1][i] == 0 else 9) for i in range(n))            # the closed loop, enqueued behind the call
        assert with_options(eng, {E.OPT_MAX_CHUNK: 4}, lambda: run(off, soff))[:5] == host
        # tuple i's share range reversed: it and the next one (which then starts before an earlier offset) read 2, their shares are orphans
        i = 2
        assert sizes[i] and sizes[i + 1]
        rev = soff[:]
        rev[i + 1] = soff[i] - 1
        g = run(off, rev)
        for k in range(n):
            if k in (i, i + 1):
                assert g[1][k] == 2 and g[2][64 * k:64 * k + 64] == bytes(64) and g[3][k] == 0 and g[4][k] == 0, k
            else:
                assert (g[1][k], g[2][64 * k:64 * k + 64], g[3][k], g[4][k]) == (host[1][k], host[2][64 * k:64 * k + 64], host[3][k], host[4][k]), k
        assert all(g[0][s] == (2 if soff[i] <= s < soff[i + 2] else host[0][s]) for s in range(n_shares))
        # a reversed message offset: 5 for the tuple and for its shares that got as far as the hash status
        k = 1
        mrev = off[:]
        mrev[k + 1] = off[k] - 1
        g = run(mrev, soff)
        assert g[1][k] == 5 and g[2][64 * k:64 * k + 64] == bytes(64) and g[3][k] == 0 and g[4][k] == 0
        assert all(g[0][s] == (5 if host[0][s] in (0, 9) else host[0][s]) for s in range(soff[k], soff[k + 1])) and g[0][:soff[k]] == host[0][:soff[k]]
        g = run(off, soff, msgs_len=off[n] - 1)
        assert g[1][n - 1] == 5 and g[1][:n - 1] == host[1][:n - 1]
        assert run(off, soff)[:5] == host              # the declaration was consumed
        for kwargs, rc in (({"keys_ptr": d_keys.ptr + 1}, -10002), ({"threshold": 0}, -10001), ({"bm_words": 0}, -10001)):
            with pytest.raises(E.NativeError) as e:
                run(off, soff, **kwargs)
            assert e.value.rc == rc, kwargs
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


def test_python_and_cpp_mirrors(eng, sets, tmp_path):
    """ECDSA.threshold_combine_keyed on keys dealt by threshold_deal verifies under ECDSA.threshold_group_key's key and under f(0) * G2;
    ECDSA.g1_msm is the weighted sum; host/threshold_example.cpp builds with -Wall -Werror against the library and prints success"""
    from bn254_amd import _native
    from bn254_amd.api import ECDSA, Error, ErrorKind, PrivateKey, PublicKey, threshold_deal, _lagrange_at_zero
    secret = PrivateKey(0x5EDA << 200)
    sks = threshold_deal(secret.value, 3, 5, seed=2026)
    pks = [PublicKey(raw) for raw in derive(eng, [k.value for k in sks])]
    try:
        assert ECDSA.register_keys(pks, engine=eng) == [None] * 5
        msg = b"height 1000"
        sig_raw, st = eng.batch_sign([msg] * 5, b"".join(k.to_bytes() for k in sks))
        from bn254_amd.api import Signature
        shares = [Signature(sig_raw[64 * j:64 * j + 64]) for j in range(5)]
        sigma, used, statuses = ECDSA.threshold_combine_keyed(msg, [shares[4], shares[1], shares[0], shares[3]], [4, 1, 2, 3], 3, engine=eng)
        assert used == [1, 3, 4] and statuses == [None, None, Error(ErrorKind.VerificationFailed), None]
        gk = ECDSA.threshold_group_key([0, 2, 4], [pks[0], pks[2], pks[4]], engine=eng)
        assert gk.raw == derive(eng, [secret.value])[0]
        assert eng.batch_verify([msg], sigma.raw, gk.raw, flags=0) == b"\0"
        assert sigma.raw == TM.signature_under(msg, secret.value)
        lam = _lagrange_at_zero([2, 4, 5])
        assert ECDSA.g1_msm([shares[1], shares[3], shares[4]], lam, engine=eng).raw == sigma.raw
        with pytest.raises(Error) as e:
            ECDSA.threshold_combine_keyed(msg, [shares[4], shares[1], shares[0]], [4, 1, 2], 3, engine=eng)
        assert e.value.kind == ErrorKind.VerificationFailed and e.value.signers == [1, 4] and e.value.statuses[2] == Error(ErrorKind.VerificationFailed)
        res = ECDSA.batch_threshold_combine_keyed([(msg, shares, range(5)), (b"other", [], [])], 3, engine=eng)
        assert res[0][0].raw == sigma.raw and res[0][1] == [0, 1, 2] and res[1].kind == ErrorKind.VerificationFailed and res[1].signers == []
    finally:
        sets["dealt9_t5"].register(eng)
    host = os.path.join(ROOT, "bn254_amd", "host")
    exe = str(tmp_path / "threshold_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", host,
                           os.path.join(host, "threshold_example.cpp"), "-o", exe, _native.LIB_PATH, "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "threshold signatures: ok" in out.stdout
