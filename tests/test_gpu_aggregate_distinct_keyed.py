"""Aggregates over distinct messages against REGISTERED keys (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct_keyed[_device]) on
the GPU.  The defining identity: the statuses equal those of bn254_batch_aggregate_verify_distinct(flags | BN254_FLAG_G2_SUBGROUP_CHECK) on
the expanded keys, with rule 2 taken from the registration (2 for an index outside the set).  Every route is compared: the slot kernel at
width 1 and 2, the expanded keys, pair lanes off and the lane-machine sizes.  Run on the MI355X box: -m gpu."""
import ctypes
import os
import subprocess

import pytest

from bn254_amd import engine as E
from tests.conftest import ws_default
from tests.datagen import D, sk_bytes
from tests.test_gpu_aggregate_distinct import expected, g1_sum, sign_all

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SLOTS_W = 2 * ws_default("AGGD_WG_ELEMS")   # table pairs one workgroup of the width-2 slot kernel takes
N_GOOD = 64


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
    """64 good keys, then four that registration refuses or marks: off the twist (4), outside the subgroup (4), a coordinate >= q (6) and
    the identity.  Returns (sks, pks, registration statuses with flags 0)."""
    sks = [sk_bytes(j) for j in range(N_GOOD)]
    out, st = eng.batch_g2_mul(None, b"".join(sks), N_GOOD, reduce_scalar=True)
    assert st == bytes(N_GOOD)
    pks = [out[128 * j:128 * j + 128] for j in range(N_GOOD)]
    off_twist = bytearray(pks[3]); off_twist[100] ^= 2
    big = bytearray(pks[5]); big[0] = 0xFF
    pks += [bytes(off_twist), bytes.fromhex(derived["g2_not_in_subgroup"]), bytes(big), bytes(128)]
    sks += [sks[3], sks[0], sks[5], bytes(31) + b"\x01"]      # placeholders: these keys never reach a pairing
    reg = eng.register_keys(b"".join(pks))
    assert list(reg[:N_GOOD]) == [0] * N_GOOD and list(reg[N_GOOD:]) == [4, 4, 6, 0], reg[N_GOOD:]
    return sks, pks, reg


def reg_set(eng, keyset, flags=0):
    sks, pks, _ = keyset
    return eng.register_keys(b"".join(pks), flags=flags)


KIDX_OFF_TWIST, KIDX_OFF_SUB, KIDX_BIG, KIDX_IDENT = N_GOOD, N_GOOD + 1, N_GOOD + 2, N_GOOD + 3


def build(eng, c, keyset, sizes, tag, n_variants=8):
    """aggregates of the given sizes, each in n_variants forms: valid; sigma wrong; two messages swapped; a key index swapped; a refused
    key (4 / 6); an index n_keys or 0xFFFFFFFF; the identity key (its pair contributes one: the aggregate stays valid).
    Returns a list of (messages, sigma, key indices)."""
    sks, pks, reg = keyset
    n_keys = len(pks)
    g1 = c.g1_generator()
    aggs, t = [], 0
    for si, k in enumerate(sizes):
        for v in range(n_variants):
            msgs = [D("aggdk/%s/%d/%d" % (tag, si, v), j) for j in range(k)]
            kidx = [(t + 7 * j) % N_GOOD for j in range(k)]
            t += k + 3
            sigma = g1_sum(eng, sign_all(eng, msgs, [sks[x] for x in kidx])) if k else bytes(64)
            if v == 1:
                sigma = c.g1_add(sigma, g1) if sigma != bytes(64) else g1
            elif v == 2 and k >= 2:
                msgs[0], msgs[k - 1] = msgs[k - 1], msgs[0]
            elif v == 3 and k:
                kidx[k // 2] = (kidx[k // 2] + 1) % N_GOOD
            elif v == 4 and k:
                kidx[k - 1] = [KIDX_OFF_TWIST, KIDX_OFF_SUB, KIDX_BIG][si % 3]
            elif v == 5 and k:
                kidx[k // 3] = [n_keys, 0xFFFFFFFF][si % 2]
            elif v == 6 and k:
                msgs.append(D("aggdk/ident/%s/%d" % (tag, si), 0))
                kidx.append(KIDX_IDENT)                            # the identity key: e(H(m), O) = 1
            elif v == 7 and k >= 2:
                kidx[0], kidx[1] = kidx[1], kidx[0]                # two key indices swapped
            aggs.append((msgs, sigma, kidx))
    return aggs


def flat(aggs):
    return [m for a in aggs for m in a[0]], [x for a in aggs for x in a[2]], b"".join(a[1] for a in aggs), [len(a[0]) for a in aggs]


def keyed(eng, aggs, flags=0):
    msgs, idx, sigs, sizes = flat(aggs)
    return eng.batch_aggregate_verify_distinct_keyed(msgs, idx, sigs, sizes, flags=flags)


def unkeyed_rule(eng, c, keyset, aggs, flags=0, reg=None):
    """the defining identity: the unkeyed call with the subgroup check on the expanded keys, rule 2 from the registration (2 outside the
    set; an out-of-range index expands to key 0, whose pair rule 2 overrides)"""
    sks, pks, reg0 = keyset
    reg = reg0 if reg is None else reg
    msgs, idx, sigs, sizes = flat(aggs)
    kp = b"".join(pks[x] if x < len(pks) else pks[0] for x in idx)
    base = eng.batch_aggregate_verify_distinct(msgs, kp, sigs, sizes, flags=flags | 1)
    out = []
    for i, (m, sigma, kidx) in enumerate(aggs):
        st = c.g1_validate(sigma, flags)
        if not st:
            for x in kidx:
                st = 2 if x >= len(pks) else reg[x]
                if st:
                    break
        out.append(st or base[i])
        if not any(x >= len(pks) for x in kidx):
            assert out[-1] == base[i], (i, out[-1], base[i])
    return bytes(out)


@pytest.fixture(scope="module")
def ragged(eng, c, keyset):
    sizes = [0, 1, 2, 3, 4, 5, 127, 128, 129, SLOTS_W - 2, SLOTS_W - 1, SLOTS_W, SLOTS_W + 1, 2 * SLOTS_W + 1]
    return build(eng, c, keyset, sizes, "ragged")


ROUTES = [("auto", {}), ("width1", {E.OPT_AGGD_KEYED_ROUTE: 1}), ("width2", {E.OPT_AGGD_KEYED_ROUTE: 2}), ("expand", {E.OPT_AGGD_KEYED_ROUTE: 3}),
          ("expand_lane_machine", {E.OPT_AGGD_KEYED_ROUTE: 3, E.OPT_LM_MAX_BATCH: 1 << 20}), ("pair_lanes_off", {E.OPT_PAIR_LANES: 0}),
          ("slots_lane_machine_helpers", {E.OPT_LM_MAX_BATCH: 1 << 20})]


def with_options(eng, opts, fn):
    defaults = {E.OPT_AGGD_KEYED_ROUTE: 0, E.OPT_PAIR_LANES: 1, E.OPT_LM_MAX_BATCH: ws_default("LM_MAX_BATCH_DEFAULT")}
    try:
        for k, v in opts.items():
            eng.set_option(k, v)
        return fn()
    finally:
        for k in opts:
            eng.set_option(k, defaults[k])


def test_ragged_every_route_against_the_rule_and_the_oracle(eng, c, keyset, ragged):
    """sizes 0..5, the slot workgroup boundaries -2..+1, straddling workgroups; every corruption; every route gives the same bytes"""
    reg_set(eng, keyset)
    want = {f: unkeyed_rule(eng, c, keyset, ragged, f) for f in (0, 1)}
    assert want[0].count(0) >= 20 and want[0].count(9) >= 20 and {2, 4, 6} <= set(want[0])
    for name, opts in ROUTES:
        for f in (0, 1):
            got = with_options(eng, opts, lambda: keyed(eng, ragged, f))
            assert got == want[f], (name, f, [(i, g, w, len(ragged[i][0])) for i, (g, w) in enumerate(zip(got, want[f])) if g != w][:8])
    # the oracle on the small aggregates that name only good keys (the header's rule composed from g1 / g2 validation, hashing, pairing)
    sks, pks, _ = keyset
    for i, (msgs, sigma, kidx) in enumerate(ragged):
        if len(msgs) <= 5 and all(x < N_GOOD for x in kidx):
            assert want[0][i] == expected(c, msgs, [pks[x] for x in kidx], [sks[x] for x in kidx], sigma, 1), i


def test_small_sizes_lane_machine_rows(eng, c, keyset, ragged):
    """latency-bound sizes (m within the lane machine's row): the default route (the slot kernel) and the expanded keys (the lane machine)
    against the rule"""
    reg_set(eng, keyset)
    small = ragged[:6 * 8]                                             # sizes 0..5, all variants
    assert len(flat(small)[0]) <= ws_default("LM_MAX_BATCH_DEFAULT")
    want = unkeyed_rule(eng, c, keyset, small, 1)
    assert keyed(eng, small, 1) == want
    assert with_options(eng, {E.OPT_AGGD_KEYED_ROUTE: 3}, lambda: keyed(eng, small, 1)) == want


def test_reject_identity_from_registration(eng, c, keyset, ragged):
    """REJECT_IDENTITY: the registration's flag counts for the keys (the identity key -> 4 in j order), the call's flag for sigma"""
    sks, pks, _ = keyset
    try:
        reg = reg_set(eng, keyset, flags=2)
        assert reg[KIDX_IDENT] == 4
        for f in (2, 3):
            assert keyed(eng, ragged, f) == unkeyed_rule(eng, c, keyset, ragged, f, reg=reg), f
        assert 4 in keyed(eng, [a for a in ragged if KIDX_IDENT in a[2]], 2)
    finally:
        reg_set(eng, keyset)


def test_no_keys_registered(eng, c, keyset, ragged):
    """an empty key set: every non-empty aggregate whose sigma decodes gets 2; empty aggregates check e(sigma, -G2) == 1"""
    try:
        eng.register_keys(b"")
        got = keyed(eng, ragged, 0)
        for i, (msgs, sigma, _) in enumerate(ragged):
            st = c.g1_validate(sigma, 0)
            want = st if st else (2 if msgs else (0 if sigma == bytes(64) else 9))
            assert got[i] == want, i
    finally:
        reg_set(eng, keyset)


def test_multi_level_reduction(eng, c, keyset):
    """one aggregate of 2^16 + 3 pairs (width 2: level 0 and two further levels) between two small ones: valid -> 0; a key index changed
    near the end -> 9; a message of the small neighbour swapped -> only that one fails"""
    reg_set(eng, keyset)
    sks, pks, _ = keyset
    k = (1 << 16) + 3
    msgs = [D("aggdk/big", j) for j in range(k)]
    kidx = [(5 * j) % N_GOOD for j in range(k)]
    sigs, st = eng.batch_sign(msgs, b"".join(sks[x] for x in kidx))
    assert st == bytes(k)
    sigma, st = eng.batch_g1_sum(sigs, (ctypes.c_uint64 * 2)(0, k))
    assert st == b"\x00"
    sm = [D("aggdk/big/side", j) for j in range(3)]
    ss = g1_sum(eng, sign_all(eng, sm, sks[:3]))
    batch = [(sm, ss, [0, 1, 2]), (msgs, sigma, kidx), (sm, ss, [0, 1, 2])]
    for route in (0, 2):
        got = with_options(eng, {E.OPT_AGGD_KEYED_ROUTE: route}, lambda: keyed(eng, batch))
        assert got == bytes(3), route
    bad = kidx[:]
    bad[k - 5] = (bad[k - 5] + 1) % N_GOOD
    assert keyed(eng, [(sm, ss, [0, 1, 2]), (msgs, sigma, bad), ([sm[1], sm[0], sm[2]], ss, [0, 1, 2])]) == bytes([0, 9, 9])


def test_device_form(eng, keyset):
    """the _device form on a caller's stream: a reversed or overlapping agg_off gives 2; a new key set registered between two calls takes
    effect"""
    from tests.hip_ctypes import DevBuf, Stream
    from bn254_amd.engine import pack_messages
    reg_set(eng, keyset)
    sks, pks, _ = keyset
    sizes = [2, 3, 1, 4]
    m = sum(sizes)
    msgs = [D("aggdk/dev", j) for j in range(m)]
    sigs = sign_all(eng, msgs, [sks[j] for j in range(m)])
    sigmas, pos = [], 0
    for k in sizes:
        sigmas.append(g1_sum(eng, sigs[pos:pos + k]))
        pos += k
    blob, off = pack_messages(msgs)
    u64 = lambda v: b"".join(int(x).to_bytes(8, "little") for x in v)   # noqa: E731
    u32 = lambda v: b"".join(int(x).to_bytes(4, "little") for x in v)   # noqa: E731
    st_dev = Stream()
    bufs = []
    try:
        def dev(data):
            b = DevBuf(len(data), data=data)
            bufs.append(b)
            return b

        d_msgs, d_off, d_sigs = dev(blob), dev(u64(off)), dev(b"".join(sigmas))
        d_idx = dev(u32(range(m)))
        d_status = DevBuf(8, fill=0xEE)
        bufs.append(d_status)

        def run(agg):
            d_agg = dev(u64(agg))
            eng.batch_aggregate_verify_distinct_keyed_device(d_msgs.ptr, d_off.ptr, d_idx.ptr, m, d_sigs.ptr, d_agg.ptr, len(sizes), d_status.ptr,
                                                             stream=st_dev.handle)
            st_dev.synchronize()
            return list(d_status.download(len(sizes)))

        assert run([0, 2, 5, 6, 10]) == [0, 0, 0, 0]
        assert run([0, 2, 1, 6, 10]) == [0, 2, 2, 0]                   # aggregate 1 reversed, aggregate 2 starts before 2
        assert run([0, 3, 5, 6, 10]) == [9, 9, 0, 0]                   # ranges shifted: sigma 0 and 1 miss or gain a pair
        # a new key set between two calls: keys 0..9 rotated by one -> every aggregate fails its pairing check
        eng.register_keys(b"".join(pks[1:10] + pks[:1] + pks[10:]))
        assert run([0, 2, 5, 6, 10]) == [9, 9, 9, 9]
        eng.register_keys(b"".join(pks[:4]))                            # 4 keys: indices 4.. are out of range
        assert run([0, 2, 5, 6, 10]) == [0, 2, 2, 2]
    finally:
        for b in bufs:
            b.free()
        st_dev.destroy()
        reg_set(eng, keyset)


def shared_inputs(eng, n_keys, tag):
    """65 536 messages, message j signed by key j % n_keys of an n_keys-key set (GPU key derivation)"""
    sks = [sk_bytes(10000 + j) for j in range(n_keys)]
    out, st = eng.batch_g2_mul(None, b"".join(sks), n_keys, reduce_scalar=True)
    assert st == bytes(n_keys)
    pks = [out[128 * j:128 * j + 128] for j in range(n_keys)]
    m = 1 << 16
    msgs = [D("aggdk/full/%s" % tag, j) for j in range(m)]
    kidx = [j % n_keys for j in range(m)]
    sigs, st = eng.batch_sign(msgs, b"".join(sks[x] for x in kidx))
    assert st == bytes(m)
    return sks, pks, msgs, kidx, sigs


def test_k1_equals_batch_verify_keyed(eng):
    """k = 1 everywhere at 65 536 tuples, every 8th mutated: byte for byte the statuses of bn254_batch_verify_keyed"""
    sks, pks, msgs, kidx, sigs = shared_inputs(eng, 256, "k1")
    n = len(msgs)
    pks = pks + [bytes(128)]
    eng.register_keys(b"".join(pks))
    kidx = kidx[:]
    S = [sigs[64 * i:64 * i + 64] for i in range(n)]
    for i in range(0, n, 8):
        r = (i // 8) % 5
        if r == 0:
            S[i] = S[i + 1]                                             # wrong signature
        elif r == 1:
            kidx[i] = (kidx[i] + 3) % 256                               # wrong key
        elif r == 2:
            kidx[i] = 256 + 1 + (i % 3)                                 # out of range
        elif r == 3:
            s = bytearray(S[i]); s[40] ^= 4; S[i] = bytes(s)             # sigma off the curve
        else:
            kidx[i] = 256                                               # the identity key
    sig = b"".join(S)
    want = eng.batch_verify_keyed(msgs, sig, kidx, flags=0)
    assert len(set(want)) >= 3
    for route in (0, 1, 2, 3):
        got = with_options(eng, {E.OPT_AGGD_KEYED_ROUTE: route},
                           lambda: eng.batch_aggregate_verify_distinct_keyed(msgs, kidx, sig, [1] * n))
        assert got == want, (route, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8])


@pytest.mark.parametrize("n_keys", [256, 1024])
def test_full_size_shapes_against_unkeyed(eng, c, n_keys):
    """65 536 x 1, 4 096 x 16 and 1 x 65 536 over an n_keys set, with corruptions, against the unkeyed call on the expanded keys"""
    sks, pks, msgs, kidx, sigs = shared_inputs(eng, n_keys, "n%d" % n_keys)
    eng.register_keys(b"".join(pks))
    m = len(msgs)
    g1 = c.g1_generator()
    for k in (1, 16, m):
        n = m // k
        off = (ctypes.c_uint64 * (n + 1))(*[i * k for i in range(n + 1)])
        sig_sum, st = eng.batch_g1_sum(sigs, off)
        assert st == bytes(n)
        sigma = [sig_sum[64 * i:64 * i + 64] for i in range(n)]
        ki = kidx[:]
        ms = msgs[:]
        step = max(1, n // 64)
        for a in range(0, n, step):
            r = (a // step) % 3
            if r == 0:
                sigma[a] = c.g1_add(sigma[a], g1)
            elif r == 1:
                ki[a * k + k - 1] = (ki[a * k + k - 1] + 1) % n_keys
            elif k >= 2:
                ms[a * k], ms[a * k + 1] = ms[a * k + 1], ms[a * k]
        S = b"".join(sigma)
        got = eng.batch_aggregate_verify_distinct_keyed(ms, ki, S, [k] * n)
        want = eng.batch_aggregate_verify_distinct(ms, b"".join(pks[x] for x in ki), S, [k] * n, flags=1)
        assert got == want, (k, [(i, g, w) for i, (g, w) in enumerate(zip(got, want)) if g != w][:8])
        assert want.count(9) >= min(n, 2) and (n < 3 or want.count(0) > 0), k


def test_python_api(eng, keyset):
    """ECDSA.aggregate_verify_keyed / batch_aggregate_verify_distinct_keyed: None for a valid aggregate, VerificationFailed for swapped
    indices, IndexOutOfBounds outside the set"""
    from bn254_amd.api import ECDSA, Error, ErrorKind, PrivateKey, PublicKey
    sk = [PrivateKey(int.from_bytes(sk_bytes(j), "big")) for j in range(3)]
    pk = [PublicKey.from_private_key(s) for s in sk]
    assert ECDSA.register_keys(pk, engine=eng) == [None, None, None]
    msgs = [b"round 9 validator 0", b"round 9 validator 1", b"round 9 validator 2"]
    sigs = [ECDSA.sign(m, s) for m, s in zip(msgs, sk)]
    sigma = sigs[0] + sigs[1] + sigs[2]
    try:
        assert ECDSA.aggregate_verify_keyed(msgs, sigma, [0, 1, 2], engine=eng) is None
        with pytest.raises(Error) as e:
            ECDSA.aggregate_verify_keyed(msgs, sigma, [1, 0, 2], engine=eng)
        assert e.value.kind == ErrorKind.VerificationFailed
        res = ECDSA.batch_aggregate_verify_distinct_keyed([(msgs, sigma, [0, 1, 2]), (msgs[:2], sigs[0] + sigs[1], [0, 1]),
                                                           (msgs[:2], sigma, [0, 3])], engine=eng)
        assert res == [None, None, Error(ErrorKind.IndexOutOfBounds)]
    finally:
        reg_set(eng, keyset)


def test_cpp_example(tmp_path):
    """host/aggregate_distinct_keyed_example.cpp builds with -Wall -Werror against the library and prints success"""
    from bn254_amd import _native
    exe = str(tmp_path / "aggregate_distinct_keyed_example")
    host = os.path.join(ROOT, "bn254_amd", "host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", host,
                           os.path.join(host, "aggregate_distinct_keyed_example.cpp"), "-o", exe, _native.LIB_PATH,
                           "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "keyed aggregate over distinct messages: ok" in out.stdout
