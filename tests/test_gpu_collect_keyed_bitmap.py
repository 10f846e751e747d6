"""Building signer-bitmap aggregates from individual signatures (include/bn254_hip.h: bn254_batch_collect_keyed_bitmap[_device]) on the GPU.
Identity 1: the share statuses are those of bn254_batch_verify_keyed on the tuple's message repeated.  The rows, counts and aggregate bytes
are compared with tests/collect_model.py plus the oracle's g1_add, on every route (default, pair lanes off, sliced, both sum layouts forced).
Identity 2: the outputs fed to bn254_batch_verify_keyed_bitmap give 0 for every accepted tuple.  Run on the MI355X box: -m gpu."""
import os
import subprocess

import pytest

from bn254_amd import engine as E
from tests import collect_model
from tests.datagen import D, sk_bytes

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
N_GOOD = 40
K_OFF_TWIST, K_OFF_SUB, K_BIG, K_IDENT, K_DUP0, K_NEG1 = range(N_GOOD, N_GOOD + 6)
N_KEYS = N_GOOD + 6
BM = 2
SIZES = [0, 1, 2, 15, 16, 17, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def derive(eng, sks):
    out, st = eng.batch_g2_mul(None, b"".join(s.to_bytes(32, "big") for s in sks), len(sks), reduce_scalar=True)
    assert st == bytes(len(sks))
    return [out[128 * j:128 * j + 128] for j in range(len(sks))]


@pytest.fixture(scope="module")
def keyset(eng, derived):
    """40 good keys, then: off the twist (4), outside the subgroup (4), a coordinate >= q (6), the identity, key 0 AGAIN and the NEGATION of
    key 1.  Returns (secret keys as integers — 0 for keys nobody can sign for —, encodings)."""
    sks = [int.from_bytes(sk_bytes(700 + j), "big") % R for j in range(N_GOOD)]
    pks = derive(eng, sks)
    off_twist = bytearray(pks[3]); off_twist[100] ^= 2
    big = bytearray(pks[5]); big[0] = 0xFF
    neg1 = derive(eng, [R - sks[1]])[0]
    pks += [bytes(off_twist), bytes.fromhex(derived["g2_not_in_subgroup"]), bytes(big), bytes(128), pks[0], neg1]
    sks += [0, 0, 0, 0, sks[0], R - sks[1]]
    reg = eng.register_keys(b"".join(pks))
    assert list(reg) == [0] * N_GOOD + [4, 4, 6, 0, 0, 0], reg[N_GOOD:]
    return sks, pks


def reg_set(eng, keyset):
    return eng.register_keys(b"".join(keyset[1]))


def sign(eng, pairs):
    """pairs of (message, secret key as an integer != 0) -> signatures"""
    sigs, st = eng.batch_sign([m for m, _ in pairs], b"".join(s.to_bytes(32, "big") for _, s in pairs))
    assert st == bytes(len(pairs))
    return [sigs[64 * i:64 * i + 64] for i in range(len(pairs))]


def build(eng, c, keyset, tag, sizes=SIZES, extras=True):
    """tuples (message, [(share, key)]): valid shares, a wrong sigma, one off the curve, the identity, shares naming a refused key, n_keys and
    n_keys + 20, the identity share of the identity key (valid), duplicates of a valid share, a valid and an invalid share of one key in
    both orders, keys 1 and K_NEG1, keys 0 and K_DUP0, and a tuple with no valid share"""
    sks, pks = keyset
    g1 = c.g1_generator()
    plan = []                                                      # (tuple, key, kind)
    for i, k in enumerate(sizes):
        for t in range(k):
            key = (7 * i + 3 * t) % N_GOOD
            kind = "ok"
            if k > 2 and t % 9 == 5:
                kind = "wrong"
            elif k > 2 and t % 9 == 6:
                kind = ["curve", "ident", "refused", "nkeys", "nkeys20", "identkey", "neg1", "dup0", "big"][(t // 9 + i) % 9]
            elif k > 2 and t % 9 == 8:
                kind = "again"
            plan.append((i, key, kind))
    n = len(sizes)
    if extras:
        special = [[(3, "wrong"), (4, "curve"), (K_OFF_SUB, "refused")], [(1, "ok"), (K_NEG1, "neg1")], [(0, "ok"), (K_DUP0, "dup0")],
                   [(9, "ok"), (9, "again"), (9, "again")], [(5, "ok"), (5, "wrong")], [(6, "wrong"), (6, "ok")], [(K_IDENT, "identkey")]]
        for j, sp in enumerate(special):
            plan += [(n + j, key, kind) for key, kind in sp]
        n += len(special)
    msgs = [D("collect/%s" % tag, i) for i in range(n)]
    secret = {"neg1": sks[K_NEG1], "dup0": sks[K_DUP0]}
    valid = sign(eng, [(msgs[i], secret.get(kind, sks[key] or 1)) for i, key, kind in plan])
    tuples = [(m, []) for m in msgs]
    for (i, key, kind), sg in zip(plan, valid):
        if kind == "wrong":
            sg = c.g1_add(sg, g1)
        elif kind == "curve":
            sg = bytearray(sg); sg[40] ^= 4; sg = bytes(sg)
        elif kind == "ident":
            sg = bytes(64)
        elif kind == "refused":
            key = K_OFF_TWIST + key % 2
        elif kind == "big":
            key = K_BIG
        elif kind == "nkeys":
            key = N_KEYS
        elif kind == "nkeys20":
            key = N_KEYS + 20
        elif kind == "identkey":
            key, sg = K_IDENT, bytes(64)
        elif kind == "neg1":
            key = K_NEG1
        elif kind == "dup0":
            key = K_DUP0
        elif kind == "again" and tuples[i][1]:
            sg, key = tuples[i][1][-1]
        tuples[i][1].append((sg, key))
    return tuples


def flat(tuples):
    return ([t[0] for t in tuples], [s for t in tuples for s, _ in t[1]], [k for t in tuples for _, k in t[1]], [len(t[1]) for t in tuples])


def collect(eng, tuples, flags=0, bm_words=BM):
    msgs, shares, keys, sizes = flat(tuples)
    return eng.batch_collect_keyed_bitmap(msgs, b"".join(shares), keys, sizes, bm_words, flags=flags, want_counts=True)


def keyed(eng, tuples, flags=0):
    msgs, shares, keys, sizes = flat(tuples)
    rep = [m for m, k in zip(msgs, sizes) for _ in range(k)]
    return eng.batch_verify_keyed(rep, b"".join(shares), keys, flags=flags)


DEFAULTS = {E.OPT_PAIR_LANES: 1, E.OPT_MAX_CHUNK: 0, E.OPT_COLLECT_WAVE_MIN_SHARES: 16}
ROUTES = [("default", {}), ("pair_lanes_off", {E.OPT_PAIR_LANES: 0}), ("sliced", {E.OPT_MAX_CHUNK: 37}),
          ("all_waves", {E.OPT_COLLECT_WAVE_MIN_SHARES: 1}), ("all_lanes", {E.OPT_COLLECT_WAVE_MIN_SHARES: 1 << 30})]


def with_options(eng, opts, fn):
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            eng.set_option(k, DEFAULTS[k])


@pytest.fixture(scope="module")
def cases(eng, c, keyset):
    return build(eng, c, keyset, "cases")


def expected(c, tuples, share_st, tuple_st, bm_words=BM):
    _, shares, keys, sizes = flat(tuples)
    rows, counts, chosen = collect_model.select(keys, share_st, sizes, tuple_st, bm_words)
    return [w for r in rows for w in r], counts, b"".join(collect_model.aggregates(c, shares, chosen))


def test_identities_and_outputs_every_route(eng, c, keyset, cases):
    """identity 1 (flags 0 and 2), the outputs against the model and the oracle's additions, and identity 2, on every route; the two sum
    layouts give the same bytes"""
    reg_set(eng, keyset)
    msgs = [t[0] for t in cases]
    for f in (0, 2):
        want = keyed(eng, cases, f)
        if f == 0:
            assert {0, 2, 4, 6, 9} <= set(want) and want.count(0) > len(want) // 2, set(want)
        bits, counts, agg = expected(c, cases, want, bytes(len(cases)))
        seen = {}
        for name, opts in ROUTES:
            share_st, tuple_st, got_agg, got_bits, got_counts = with_options(eng, opts, lambda: collect(eng, cases, f))
            assert share_st == want, (name, f, [(i, a, b) for i, (a, b) in enumerate(zip(share_st, want)) if a != b][:8])
            assert tuple_st == bytes(len(cases)), (name, f)
            assert got_bits == bits and got_counts == counts, (name, f)
            assert got_agg == agg, (name, f, [i for i in range(len(cases)) if got_agg[64 * i:64 * i + 64] != agg[64 * i:64 * i + 64]])
            seen[name] = got_agg
        assert seen["all_waves"] == seen["all_lanes"]
        if f == 0:                                              # identity 2: the closed loop
            assert eng.batch_verify_keyed_bitmap(msgs, agg, bits, BM) == bytes(len(cases))
            n0 = len(SIZES)
            assert counts[n0] == 0 and agg[64 * n0:64 * n0 + 64] == bytes(64)                    # no valid share
            assert counts[n0 + 1] == 2 and agg[64 * (n0 + 1):64 * (n0 + 2)] == bytes(64)         # key 1 and its negation: the identity
            assert counts[n0 + 2] == 2 and counts[n0 + 3] == 1 and counts[n0 + 4] == 1 and counts[n0 + 5] == 1 and counts[n0 + 6] == 1
            assert counts[SIZES.index(130)] <= N_KEYS < 130


def test_oracle_anchor(eng, c, keyset):
    """a dozen shares whose status comes from hash_to_g1 + pairing_check alone, three aggregates from g1_add alone"""
    sks, pks = keyset
    reg_set(eng, keyset)
    neg_g2 = c.g2_mul(c.g2_generator(), (R - 1).to_bytes(32, "big"))
    tuples = build(eng, c, keyset, "anchor", sizes=[4, 5, 3], extras=False)
    tuples[1][1][2] = (c.g1_add(tuples[1][1][2][0], c.g1_generator()), tuples[1][1][2][1])
    tuples[2][1][0] = (tuples[2][1][0][0], (tuples[2][1][0][1] + 1) % N_GOOD)
    want, agg = [], []
    for m, shares in tuples:
        st, h, _ = c.hash_to_g1(m)
        assert st == 0
        acc, seen = bytes(64), set()
        for sg, key in shares:
            want.append(c.pairing_check(h + sg, pks[key] + neg_g2, 2))
            if want[-1] == 0 and key not in seen:
                seen.add(key)
                acc = c.g1_add(acc, sg)
        agg.append(acc)
    assert len(want) == 12 and want.count(9) == 2 and want.count(0) == 10
    for name, opts in ROUTES:
        share_st, tuple_st, got_agg, _, _ = with_options(eng, opts, lambda: collect(eng, tuples))
        assert list(share_st) == want and got_agg == b"".join(agg), name


def test_both_sides_of_every_routing_row(eng, c, keyset):
    """n_shares on both sides of every row of the routing table, as tuples of 1 to 3 shares with every fifth share wrong"""
    sks, pks = keyset
    reg_set(eng, keyset)
    rows = eng.route_table()
    sizes = sorted({n for r in rows[:-1] for n in (r[0], r[0] + 1)} | {1, 2, 63, 64, 65})
    top = sizes[-1]
    g1 = c.g1_generator()
    lens, total = [], 0
    while total < top:
        lens.append(min(1 + len(lens) % 3, top - total))
        total += lens[-1]
    msgs = [D("collect/many", i) for i in range(len(lens))]
    plan = [(i, (5 * i + t) % N_GOOD) for i, k in enumerate(lens) for t in range(k)]
    sigs = sign(eng, [(msgs[i], sks[key]) for i, key in plan])
    sigs = [c.g1_add(sg, g1) if s % 5 == 4 else sg for s, sg in enumerate(sigs)]
    for n_shares in sizes:
        tuples, at = [], 0
        for i, k in enumerate(lens):
            k = min(k, n_shares - at)
            if k <= 0:
                break
            tuples.append((msgs[i], [(sigs[s], plan[s][1]) for s in range(at, at + k)]))
            at += k
        want = keyed(eng, tuples)
        share_st, tuple_st, agg, bits, counts = collect(eng, tuples)
        assert share_st == want and tuple_st == bytes(len(tuples)), n_shares
        assert (bits, counts, agg) == expected(c, tuples, want, tuple_st), n_shares


def test_hash_once(eng, c, keyset, derived):
    """a message whose hash needs several tries under 70 shares; and the front end of one tuple of 4 096 shares is faster than the hash stage
    of the keyed verify on the 4 096 repeated messages"""
    sks, pks = keyset
    reg_set(eng, keyset)
    vec = max(derived["hash_to_g1"], key=lambda v: v["tries"])
    assert vec["tries"] >= 3
    m = bytes.fromhex(vec["message_hex"])
    sigs = sign(eng, [(m, sks[t % N_GOOD]) for t in range(70)])
    sigs[13] = c.g1_add(sigs[13], c.g1_generator())
    tuples = [(m, [(sg, t % N_GOOD) for t, sg in enumerate(sigs)])]
    share_st, tuple_st, agg, bits, counts = collect(eng, tuples)
    assert list(share_st) == [9 if t == 13 else 0 for t in range(70)] == list(keyed(eng, tuples)) and tuple_st == b"\0"
    assert (bits, counts, agg) == expected(c, tuples, share_st, tuple_st) and counts == [N_GOOD]
    big = [(m, [(sigs[t % 70], t % N_GOOD) for t in range(4096)])]
    try:
        eng.set_profiling(True)
        st_a = collect(eng, big)[0]
        ms_collect = eng.last_kernel_ms()
        st_b = keyed(eng, big)
        ms_keyed = eng.last_kernel_ms()
    finally:
        eng.set_profiling(False)
    assert st_a == st_b
    print("collect ms", ms_collect, "keyed ms", ms_keyed)
    assert ms_collect["decode"] < ms_keyed["hash_to_g1"], (ms_collect, ms_keyed)


def test_no_keys_registered(eng, c, keyset, cases):
    """an empty key set: every decodable share gets 2, the rows are empty, the aggregates the identity; then the set again (no stale state)"""
    try:
        eng.register_keys(b"")
        share_st, tuple_st, agg, bits, counts = collect(eng, cases, bm_words=0)
        _, shares, _, _ = flat(cases)
        assert list(share_st) == [c.g1_validate(s, 0) or 2 for s in shares] == list(keyed(eng, cases))
        assert tuple_st == bytes(len(cases)) and agg == bytes(64 * len(cases)) and counts == [0] * len(cases) and bits == []
    finally:
        reg_set(eng, keyset)
    want = keyed(eng, cases)
    share_st, tuple_st, agg, bits, counts = collect(eng, cases)
    assert share_st == want and (bits, counts, agg) == expected(c, cases, want, tuple_st)


def test_device_form(eng, c, keyset, cases):
    """the _device form on a caller's stream: the host form's bytes; refused share ranges (reversed, overlapping, past n_shares) give tuple
    status 2, empty outputs and orphans that read 2; reversed message offsets give 5; bn254_ctx_expect_msgs_len is honoured; misaligned
    share keys and a bitmap one word short are refused; a bitmap verify follows on the same stream with no synchronisation in between"""
    from tests.hip_ctypes import DevBuf, Stream
    from bn254_amd.engine import pack_messages
    reg_set(eng, keyset)
    tuples = [t for t in cases if 0 < len(t[1]) <= 17][:9]
    msgs, shares, keys, sizes = flat(tuples)
    n, n_shares = len(tuples), len(keys)
    blob, off = pack_messages(msgs)
    off = list(off)
    soff = [sum(sizes[:i]) for i in range(n + 1)]
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    stream = Stream()
    bufs = []

    def dev(data=None, nbytes=None):
        b = DevBuf(len(data), data=data) if data is not None else DevBuf(nbytes, fill=0xEE)
        bufs.append(b)
        return b
    try:
        d_msgs, d_shares, d_keys = dev(bytes(blob)), dev(b"".join(shares)), dev(u32(keys) + bytes(4))
        d_sst, d_tst, d_agg, d_bits, d_cnt, d_vst = dev(nbytes=n_shares), dev(nbytes=n), dev(nbytes=64 * n), dev(nbytes=4 * BM * n), dev(nbytes=4 * n), dev(nbytes=n)

        def run(moff, share_off, msgs_len=None, keys_ptr=None, bm_words=BM):
            d_moff, d_soff = dev(u64(moff)), dev(u64(share_off))
            if msgs_len is not None:
                eng.expect_msgs_len(msgs_len)
            eng.batch_collect_keyed_bitmap_device(d_msgs.ptr, d_moff.ptr, d_shares.ptr, keys_ptr or d_keys.ptr, d_soff.ptr, n_shares, n, bm_words,
                                                  d_sst.ptr, d_tst.ptr, d_agg.ptr, d_bits.ptr, d_cnt.ptr, stream=stream.handle)
            eng.batch_verify_keyed_bitmap_device(d_msgs.ptr, d_moff.ptr, d_agg.ptr, d_bits.ptr, BM, n, d_vst.ptr, stream=stream.handle)
            stream.synchronize()
            words = d_bits.download(4 * BM * n)
            return (d_sst.download(n_shares), d_tst.download(n), d_agg.download(64 * n),
                    [int.from_bytes(words[4 * k:4 * k + 4], "little") for k in range(BM * n)],
                    [int.from_bytes(d_cnt.download(4 * n)[4 * k:4 * k + 4], "little") for k in range(n)], d_vst.download(n))

        host = collect(eng, tuples)
        got = run(off, soff)
        assert got[:5] == host and got[5] == bytes(n)
        assert with_options(eng, {E.OPT_MAX_CHUNK: 5}, lambda: run(off, soff))[:5] == host

        def refused(share_off, bad, orphans):
            g = run(off, share_off)
            for i in range(n):
                if i in bad:
                    assert g[1][i] == 2 and g[2][64 * i:64 * i + 64] == bytes(64) and g[3][BM * i:BM * i + BM] == [0] * BM and g[4][i] == 0, i
                else:
                    assert g[1][i] == 0 and g[2][64 * i:64 * i + 64] == host[2][64 * i:64 * i + 64] and g[4][i] == host[4][i], i
            for s in range(n_shares):
                assert g[0][s] == (2 if s in orphans else host[0][s]), s
            assert all(g[5][i] == 0 for i in range(n) if i not in bad)
        i = 3
        rev = soff[:]
        rev[i + 1] = soff[i] - 1                     # tuple i reversed; tuple i + 1 then starts before the earlier offset soff[i]: refused too
        refused(rev, {i, i + 1}, set(range(soff[i], soff[i + 2])))
        past = soff[:]
        past[n] = n_shares + 1                       # the last tuple runs past n_shares
        refused(past, {n - 1}, set(range(soff[n - 1], n_shares)))
        lap = soff[:]
        lap[i + 1] = soff[i + 2]                     # tuple i swallows tuple i + 1, whose range [soff[i+2], soff[i+2]) is empty but accepted;
        lap[i + 2] = soff[i + 1]                     # ... and tuple i + 2 then starts before the earlier offset soff[i + 2]: overlap
        g = run(off, lap)
        assert g[1][i + 1] == 2 and g[1][i + 2] == 2 and g[1][i] == 0 and g[4][i + 1] == 0 and g[4][i + 2] == 0
        assert all(g[0][s] == 2 for s in range(soff[i + 2], soff[i + 3]))
        # message offsets: reversed -> 5 for the tuple and its shares; a declared length one byte short -> 5 for the last tuple
        k = next(j for j in range(1, n - 1) if off[j + 1] > off[j])
        mrev = off[:]
        mrev[k + 1] = off[k] - 1
        g = run(mrev, soff)
        assert g[1][k] == 5 and g[4][k] == 0 and all(g[0][s] == (5 if host[0][s] in (0, 9) else host[0][s]) for s in range(soff[k], soff[k + 1]))
        assert g[0][:soff[k]] == host[0][:soff[k]]
        g = run(off, soff, msgs_len=off[n] - 1)
        assert g[1][n - 1] == 5 and g[1][:n - 1] == bytes(n - 1)
        assert run(off, soff)[:5] == host              # the declaration was consumed
        with pytest.raises(E.NativeError) as e:
            run(off, soff, keys_ptr=d_keys.ptr + 1)
        assert e.value.rc == -10002                    # BN254_E_MISALIGNED
        with pytest.raises(E.NativeError) as e:
            run(off, soff, bm_words=BM - 1)            # cannot hold key 45
        assert e.value.rc == -10001                    # BN254_E_BAD_ARGUMENT
        with pytest.raises(E.NativeError) as e:
            collect(eng, tuples, bm_words=BM - 1)
        assert e.value.rc == -10001
        # host form: share_off must start at 0, never decrease, and end at n_shares
        import ctypes
        sst, tst, agg, bits = (ctypes.create_string_buffer(k) for k in (n_shares + 8, n + 8, 64 * n, 4 * BM * n))
        k32 = (ctypes.c_uint32 * n_shares)(*keys)
        for bad in ([1] + soff[1:], soff[:2] + [soff[1] - 1] + soff[3:], soff[:n] + [n_shares - 1], soff[:n] + [n_shares + 1]):
            rc = eng._lib.bn254_batch_collect_keyed_bitmap(eng._h, bytes(blob), (ctypes.c_uint64 * (n + 1))(*off), b"".join(shares), k32,
                                                           (ctypes.c_uint64 * (n + 1))(*bad), n_shares, n, BM, 0, sst, tst, agg, bits, None)
            assert rc == -10001, bad
    finally:
        for b in bufs:
            b.free()
        stream.destroy()


def test_python_and_cpp_mirrors(eng, keyset, tmp_path):
    """ECDSA.aggregate_keyed_signers round-trips into ECDSA.verify_keyed_signers; so does the compiled C++ mirror"""
    from bn254_amd.api import ECDSA, Error, ErrorKind, PrivateKey, PublicKey
    sk = [PrivateKey(int.from_bytes(sk_bytes(j), "big")) for j in range(4)]
    pk = [PublicKey.from_private_key(s) for s in sk]
    try:
        assert ECDSA.register_keys(pk, engine=eng) == [None] * 4
        msg = b"round 10"
        sigs = [ECDSA.sign(msg, s) for s in sk]
        sigma, signers, statuses = ECDSA.aggregate_keyed_signers(msg, [sigs[2], sigs[0], sigs[1], sigs[2], sigs[3]], [2, 0, 3, 2, 9], engine=eng)
        assert signers == [0, 2] and statuses == [None, None, Error(ErrorKind.VerificationFailed), None, Error(ErrorKind.IndexOutOfBounds)]
        assert ECDSA.verify_keyed_signers(msg, sigma, signers, engine=eng) is None
        res = ECDSA.batch_aggregate_keyed_signers([(msg, sigs, [0, 1, 2, 3]), (b"other", [], [])], engine=eng)
        assert res[0][1] == [0, 1, 2, 3] and res[1][1] == [] and res[1][0].raw == bytes(64)
        assert ECDSA.batch_verify_keyed_signers([(msg, res[0][0], res[0][1]), (b"other", res[1][0], [])], engine=eng) == [None, None]
    finally:
        reg_set(eng, keyset)
    src = tmp_path / "collect_mirror.cpp"
    src.write_text(CPP_MIRROR)
    exe = str(tmp_path / "collect_mirror")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "bn254_amd", "host"), str(src), "-L" + os.path.join(ROOT, "bn254_amd"),
                           "-lbn254hip", "-Wl,-rpath," + os.path.join(ROOT, "bn254_amd"), "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "collect mirror ok" in p.stdout, (p.stdout, p.stderr)


CPP_MIRROR = r"""
#include <cstdio>
#include "bn254.hpp"
int main() {
  try {
    bn254::PrivateKey k[3];
    for (int j = 0; j < 3; ++j) { k[j].bytes = {}; k[j].bytes[31] = (uint8_t)(7 + j); k[j].bytes[5] = 0x11; }
    std::vector<bn254::PublicKey> pk;
    for (int j = 0; j < 3; ++j) pk.push_back(bn254::PublicKey::from_private_key(k[j]));
    if (bn254::ECDSA::register_keys(pk) != std::vector<uint8_t>{0, 0, 0}) return 2;
    std::vector<uint8_t> msg = {'c', 'o', 'l', 'l', 'e', 'c', 't'};
    auto s0 = bn254::ECDSA::sign(msg, k[0]), s1 = bn254::ECDSA::sign(msg, k[1]), s2 = bn254::ECDSA::sign(msg, k[2]);
    auto r = bn254::ECDSA::aggregate_keyed_signers(msg, {s2, s0, s1, s2}, {2, 0, 2, 5}, 3);
    if (r.signer_indices != std::vector<uint32_t>{0, 2} || r.statuses != std::vector<uint8_t>{0, 0, 9, 2}) return 3;
    bn254::ECDSA::verify_keyed_signers(msg, r.signature, r.signer_indices, 3);
    try { bn254::ECDSA::verify_keyed_signers(msg, r.signature, {0, 1, 2}, 3); return 4; }
    catch (const bn254::Error& e) { if (e.kind != bn254::ErrorKind::VerificationFailed) return 5; }
    printf("collect mirror ok\n");
    return 0;
  } catch (const std::exception& e) { printf("failed: %s\n", e.what()); return 1; }
}
"""
