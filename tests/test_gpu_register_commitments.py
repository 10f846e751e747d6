"""Registering the share keys of a vector of Feldman commitments (include/bn254_hip.h: bn254_ctx_register_keys_commitments) on the GPU.
For the committees (n, t) = (1, 1), (5, 3), (33, 17), (97, 65) and (256, 171): the defining identity — the context is what
bn254_ctx_register_keys leaves on the outputs of bn254_batch_g2_poly_eval at x = 1 .. n (key statuses, the statuses of a keyed verify over
signatures made with the dealt secrets, the rows of the line tables) —, the evaluated keys against Python integers and the C oracle, the
dealing check (passes at t with C_0 as the group key, fails at t - 1), and the closed loop into the optimistic threshold combine.  A
commitment fault; commitments outside the order-r subgroup; the previous key set and group key dropped; refused arguments.
Run on the MI355X box: -m gpu."""
import ctypes
import os
import random
import re

import pytest

from bn254_amd import engine as E
from tests import dealing_cases as DC
from tests import polyeval_model as PM

pytestmark = pytest.mark.gpu
R = PM.R
BAD_ARGUMENT = -10001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (5, 3), (33, 17), (97, 65), (256, 171)]
SEED = DC.SEEDS[1]


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def coefficients_of(secret, t, seed):
    """the polynomial threshold_deal and threshold_commitments draw: f(0) = secret, the rest from random.Random(seed)"""
    rnd = random.Random(seed)
    return [secret % R] + [rnd.randrange(R) for _ in range(t - 1)]


def split_default():
    text = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    return int(re.search(r"#define POLY_EVAL_WAVE_MIN_COEFFS_DEFAULT (\d+)", text).group(1))


def table_rows(eng, n):
    words, _, st, inf = eng.debug_key_tables(1, 0, n)
    return words, st, inf


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dof%d" % (s[1], s[0]))
def test_committee(eng, c, shape):
    from bn254_amd.api import ECDSA, PublicKey, Signature, threshold_commitments, threshold_deal
    n, t = shape
    secret = (0xFE1D << 200) + 1000 * n + t
    sks = threshold_deal(secret, t, n, seed=n)
    cs = threshold_commitments(secret, t, seed=n)
    a = coefficients_of(secret, t, n)
    assert cs[0].raw == PM.key_of(c, a[0]) and cs[-1].raw == PM.key_of(c, a[-1]) and [k.value for k in sks] == [PM.eval_scalar(a, j + 1) for j in range(n)]
    raw = b"".join(p.raw for p in cs)
    msgs = [b"round %d" % (j % 3) for j in range(n)]
    sigs, st = eng.batch_sign(msgs, b"".join(k.to_bytes() for k in sks))
    assert st == bytes(n)
    # the evaluated keys are f(j + 1) * G2: Python integers and the oracle's key derivation
    keys, st = eng.batch_g2_poly_eval(raw, [0, t], [0] * n, list(range(1, n + 1)))
    assert st == bytes(n) and keys == b"".join(PM.share_keys(c, a, n))
    # the plain registration of those bytes ...
    assert eng.register_keys(keys) == bytes(n)
    plain = table_rows(eng, n), eng.batch_verify_keyed(msgs, sigs, list(range(n)))
    assert plain[1] == bytes(n)
    assert eng.register_keys(b"") == b""
    # ... and the registration from the commitments: the same context
    key_st, call_st = eng.register_keys_commitments(raw, n)
    assert (key_st, call_st) == (bytes(n), 0) and eng.n_registered_keys == n and not eng.group_key_set
    assert (table_rows(eng, n), eng.batch_verify_keyed(msgs, sigs, list(range(n)))) == plain
    wrong = list(range(1, n)) + [0]
    assert eng.batch_verify_keyed(msgs, sigs, wrong) == (bytes(n) if n == 1 else bytes([9]) * n)
    assert eng.batch_verify_keyed(msgs[:1], sigs[:64], [n]) == b"\x02"                       # exactly n keys are registered
    # a dealing by construction, its group key C_0; one coefficient too many for threshold t - 1
    assert eng.check_dealing(t, SEED) == (cs[0].raw, 0, 0xFFFFFFFF)
    if n > t and t > 1:
        assert eng.check_dealing(t - 1, SEED) == (bytes(128), 9, 0xFFFFFFFF)
    # the closed loop: name C_0, combine t shares optimistically, and the signature verifies under C_0
    ECDSA.register_group_key(cs[0], engine=eng)
    msg = b"height 7"
    share_sigs, st = eng.batch_sign([msg] * n, b"".join(k.to_bytes() for k in sks))
    assert st == bytes(n)
    try:
        eng.set_option(E.OPT_THRESHOLD_OPT_MIN_SHARES, 0)
        res = ECDSA.threshold_combine_keyed_optimistic(msg, [Signature(share_sigs[64 * j:64 * j + 64]) for j in range(n)], range(n), t, engine=eng, n_keys=n)
        hook = eng.debug_threshold_opt_last()
    finally:
        eng.set_option(E.OPT_THRESHOLD_OPT_MIN_SHARES, E.THRESHOLD_OPT_MIN_SHARES_DEFAULT)
    assert hook == dict(checked=1, passed=1, exact_tuples=0, exact_shares=0)
    assert eng.batch_verify([msg], res[0].raw, cs[0].raw, flags=0) == bytes(1)
    # the API form gives the same registration and, asked to, names the group key
    assert ECDSA.register_keys_from_commitments(cs, n, register_group_key=True, engine=eng) == [None] * n
    assert eng.group_key_set and table_rows(eng, n) == plain[0]
    assert ECDSA.register_keys_from_commitments(cs, n, engine=eng) == [None] * n and not eng.group_key_set


@pytest.mark.parametrize("split", [1, 1 << 30])
def test_both_layouts_register_the_same_keys(eng, split):
    from bn254_amd.api import threshold_commitments
    raw = b"".join(p.raw for p in threshold_commitments(12345, 17, seed=3))
    try:
        assert eng.register_keys_commitments(raw, 33) == (bytes(33), 0)
        want = table_rows(eng, 33)
        eng.set_option(E.OPT_POLY_EVAL_WAVE_MIN_COEFFS, split)
        assert eng.register_keys_commitments(raw, 33) == (bytes(33), 0) and table_rows(eng, 33) == want
    finally:
        eng.set_option(E.OPT_POLY_EVAL_WAVE_MIN_COEFFS, split_default())


def test_commitment_fault_leaves_no_keys(eng):
    """a commitment off the curve behind one with a coordinate >= q: the lowest index wins, key_status is untouched, no keys and no group key
    are left — the previous set is gone too"""
    from bn254_amd.api import ECDSA, Error, ErrorKind, PublicKey, threshold_commitments
    cs = threshold_commitments(777, 5, seed=9)
    raw = [p.raw for p in cs]
    assert eng.register_keys_commitments(b"".join(raw), 7) == (bytes(7), 0)
    assert eng.set_group_key(raw[0]) == 0 and eng.group_key_set
    bad = list(raw)
    bad[1], bad[3] = DC.plant(raw[1], "big"), DC.plant(raw[3], "curve")
    lib, h = eng._lib, eng._h
    key_st, st = ctypes.create_string_buffer(b"\xee" * 7, 7), ctypes.create_string_buffer(b"\xee", 1)
    assert lib.bn254_ctx_register_keys_commitments(h, b"".join(bad), 5, 7, 0, key_st, st) == 0
    assert st.raw == bytes([DC.FAULT_STATUS["big"]]) and key_st.raw == b"\xee" * 7
    msg = [b"m"]
    sig, _ = eng.batch_sign(msg, (1).to_bytes(32, "big"))
    assert eng.batch_verify_keyed(msg, sig, [0]) == b"\x02"                                    # no key 0: nothing is registered
    pk, dst, bad_key = ctypes.create_string_buffer(128), ctypes.create_string_buffer(1), ctypes.c_uint32(0)
    assert lib.bn254_ctx_check_dealing(h, 1, DC.SEEDS[0], 0, pk, dst, ctypes.byref(bad_key)) == BAD_ARGUMENT      # ... so nothing to check
    assert eng.register_keys_commitments(b"".join(bad), 7) == (None, DC.FAULT_STATUS["big"]) and eng.n_registered_keys == 0 and not eng.group_key_set
    with pytest.raises(Error) as e:
        ECDSA.register_keys_from_commitments([PublicKey(b) for b in bad], 7, register_group_key=True, engine=eng)
    assert e.value.kind == ErrorKind.NotMemberError and not eng.group_key_set
    # key_status may be NULL
    assert lib.bn254_ctx_register_keys_commitments(h, b"".join(raw), 5, 7, 0, None, st) == 0 and st.raw == b"\0"
    assert eng.batch_verify_keyed(msg, sig, [0]) == b"\x09"


def test_commitments_outside_the_subgroup(eng):
    """commitments on the curve and outside the order-r subgroup decode (flags 0) and evaluate; registration's own subgroup check then refuses
    every key, as bn254_ctx_register_keys refuses the evaluated bytes"""
    off = PM.off_subgroup_point(31)
    gen_multiple = PM.M.g2_to_uncompressed(PM.M.g2_mul(PM.M.G2_GEN, 5))
    raw = gen_multiple + off
    keys, st = eng.batch_g2_poly_eval(raw, [0, 2], [0] * 3, [1, 2, 3])
    assert st == bytes(3) and keys == b"".join(PM.eval_by_group([gen_multiple, off], x) for x in (1, 2, 3))
    want = eng.register_keys(keys)
    assert want == bytes([4]) * 3
    assert eng.register_keys_commitments(raw, 3) == (want, 0)
    assert eng.check_dealing(2, SEED)[1:] == (4, 0)


def test_refused_arguments(eng):
    from bn254_amd.api import threshold_commitments
    raw = b"".join(p.raw for p in threshold_commitments(1, 2, seed=1))
    lib, h = eng._lib, eng._h
    call = lib.bn254_ctx_register_keys_commitments
    key_st, st = ctypes.create_string_buffer(b"\xee" * 4, 4), ctypes.create_string_buffer(b"\xee", 1)
    assert call(None, raw, 2, 4, 0, key_st, st) == BAD_ARGUMENT
    assert call(h, None, 2, 4, 0, key_st, st) == BAD_ARGUMENT
    assert call(h, raw, 0, 4, 0, key_st, st) == BAD_ARGUMENT
    assert call(h, raw, 2, 0, 0, key_st, st) == BAD_ARGUMENT
    assert call(h, raw, 2, 1 << 32, 0, key_st, st) == BAD_ARGUMENT
    assert call(h, raw, 2, 4, 0, key_st, None) == BAD_ARGUMENT
    assert key_st.raw == b"\xee" * 4 and st.raw == b"\xee"
    # the identity as a commitment vector: every key is the identity; BN254_FLAG_REJECT_IDENTITY refuses them as a registration does
    assert eng.register_keys_commitments(bytes(256), 4) == (eng.register_keys(bytes(512)), 0)
    assert eng.register_keys_commitments(bytes(256), 4, flags=E.FLAG_REJECT_IDENTITY) == (eng.register_keys(bytes(512), flags=E.FLAG_REJECT_IDENTITY), 0)
