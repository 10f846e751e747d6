"""The reshare of a threshold key (include/bn254_hip.h: bn254_ctx_reshare_commitments) on the GPU.  The committees of tests/reshare_cases.py —
(1, 1) -> (1, 1), (3, 2) -> (4, 3), (5, 3) -> (3, 2), (7, 5) -> (7, 5), (70, 47) -> (70, 47) — with every disqualification (an index past
the key set, a refused key, a failed proof of possession, a decode fault in commitment 0, a middle one and the last, D_0 another key, the
negated key, the identity; two faults in one dealer; a registered identity key that qualifies), too few qualified dealers, a threshold above
the key set and above the dealers: against tests/reshare_model.py (Python integers, a textbook Lagrange formula, the C oracle); DEFINING
IDENTITY 1 against bn254_batch_g2_vector_combine with the coefficients of bn254_debug_lagrange_at_zero, under both layouts of the sums;
DEFINING IDENTITY 2, the closed loop: C'_0 is the old group key, the new committee registered from the commitments passes the dealing check
with it, and signatures of the new members' shares combine to one that verifies under the OLD group key, the same for two dealer subsets.
Once (256, 171) -> (256, 171).  Refused arguments; the context unchanged; the Python and C++ mirrors.  Run on the MI355X box: -m gpu."""
import ctypes
import os
import subprocess

import pytest

from bn254_amd import engine as E
from tests import dealing_cases as DC
from tests import reshare_cases as RC
from tests import reshare_model as RM

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = RM.R
BAD_ARGUMENT = -10001
NO_KEY = 0xFFFFFFFF
SEED = DC.SEEDS[1]


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


@pytest.fixture(scope="module")
def c():
    from oracle import c_oracle
    return c_oracle


def be(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def chunks(raw, size=128):
    return [raw[i:i + size] for i in range(0, len(raw), size)]


def derive(eng, scalars):
    """a * G2::one() by the fixed-base route of bn254_batch_g2_mul, a call this feature does not touch: INPUTS only"""
    out, st = eng.batch_g2_mul(None, be(s % R for s in scalars), len(scalars))
    assert st == bytes(len(scalars))
    return chunks(out)


def register(eng, c, cs):
    """the old committee of a case, its faults planted; a failed proof of possession through bn254_ctx_register_keys_pop with another key's
    proof.  The registration statuses are what the model assumes"""
    n = len(cs["secrets"])
    keys = derive(eng, cs["secrets"])
    assert keys[n - 1] == RM.key_of(c, cs["secrets"][n - 1])
    want = []
    for j in range(n):
        kind = cs["key_faults"].get(j)
        if kind:
            keys[j] = DC.plant(keys[j], kind)
        want.append(DC.FAULT_STATUS[kind] if kind else 9 if j in cs["pop_fail"] else 0)
    if cs["pop_fail"]:
        pks, pops, st = eng.batch_pop_prove(be(cs["secrets"]))
        assert st == bytes(n) and pks == b"".join(keys)
        pops = chunks(pops, 64)
        for j in cs["pop_fail"]:
            pops[j] = pops[(j + 1) % n]
        got = eng.register_keys_pop(b"".join(keys), b"".join(pops))
    else:
        got = eng.register_keys(b"".join(keys))
    assert list(got) == want
    return keys


def vectors_of(eng, cs):
    flat = derive(eng, [v for _, vec in cs["dealers"] for v in vec])
    t_new = cs["t_new"]
    rows = [flat[i * t_new:(i + 1) * t_new] for i in range(len(cs["dealers"]))]
    for (i, k), kind in cs["faults"].items():
        rows[i][k] = DC.plant(rows[i][k], kind)
    return rows


def check_case(eng, c, cs, extra_words=0):
    """one call against the model, and DEFINING IDENTITY 1 on its result; returns (commitments, used keys)"""
    n = len(cs["secrets"])
    bm_words = (n + 31) // 32 + extra_words
    rows = vectors_of(eng, cs)
    keys = [k for k, _ in cs["dealers"]]
    out, st, dealer_st, row = eng.reshare_commitments(b"".join(p for r in rows for p in r), keys, cs["t_new"], cs["threshold"], bm_words=bm_words)
    status, want_st, used, taken, lam, scalars = RM.reshare_expected(cs)
    assert (st, list(dealer_st), row) == (status, want_st, RM.bits_of(used, bm_words)), cs["name"]
    if status != 0:
        assert out == bytes(128 * cs["t_new"]), cs["name"]
        return None, used
    assert chunks(out) == [RM.key_of(c, v) for v in scalars], cs["name"]
    coeff = eng.debug_lagrange_at_zero([k + 1 for k in used], [0, len(used)])
    assert coeff == be(lam), cs["name"]
    for split in (1, 1 << 30):
        try:
            eng.set_option(E.OPT_COLLECT_WAVE_MIN_SHARES, split)
            assert eng.batch_g2_vector_combine(b"".join(p for i in taken for p in rows[i]), coeff, len(taken), cs["t_new"]) == (out, bytes(cs["t_new"])), cs["name"]
            again = eng.reshare_commitments(b"".join(p for r in rows for p in r), keys, cs["t_new"], cs["threshold"], bm_words=bm_words)
            assert again == (out, st, dealer_st, row), cs["name"]
        finally:
            eng.set_option(E.OPT_COLLECT_WAVE_MIN_SHARES, 16)
    return out, used


@pytest.mark.parametrize("committee", RC.COMMITTEES, ids=lambda cm: "%dof%d_to_%dof%d" % (cm[0][1], cm[0][0], cm[1][1], cm[1][0]))
def test_case_set(eng, c, committee):
    old, new = committee
    cases = RC.rs_cases_for(old, new)
    assert len(cases) >= (5 if old[0] == old[1] else 18)
    last = None
    for cs in cases:
        now = (tuple(cs["secrets"]), tuple(sorted(cs["key_faults"].items())), tuple(sorted(cs["pop_fail"])))
        if now != last:
            register(eng, c, cs)
            last = now
        check_case(eng, c, cs, extra_words=2 if cs["name"] == "honest_all" else 0)
    # the context is as the call found it: a keyed verify over the registered (old) keys still passes
    cs = cases[0]
    register(eng, c, cs)
    check_case(eng, c, cs)
    n = old[0]
    msgs = [b"still here %d" % (j % 3) for j in range(n)]
    sigs, st = eng.batch_sign(msgs, be(cs["secrets"]))
    assert st == bytes(n) and eng.batch_verify_keyed(msgs, sigs, list(range(n))) == bytes(n)


@pytest.mark.parametrize("committee", RC.COMMITTEES[:4], ids=lambda cm: "%dof%d_to_%dof%d" % (cm[0][1], cm[0][0], cm[1][1], cm[1][0]))
def test_closed_loop(eng, c, committee):
    """DEFINING IDENTITY 2: the group key stays, the new committee is a dealing of it, and its signatures verify under the OLD group key —
    the same for two dealer subsets S"""
    from bn254_amd.api import ECDSA, PrivateKey, Signature, threshold_combine_subshares
    (n, t), (n_new, t_new) = committee
    f, secrets = RC.old_committee(n, t)
    group = RM.key_of(c, f[0])
    msg = b"epoch 12"
    seen = []
    for name in ("honest_all", "honest_exactly_t_high"):
        cs = next(x for x in RC.rs_cases_for(*committee) if x["name"] == name)
        register(eng, c, cs)
        assert eng.check_dealing(t, SEED) == (group, 0, NO_KEY)
        out, used = check_case(eng, c, cs)
        assert out[:128] == group
        seen.append(tuple(used))
        # the new members' shares: each combines the sub-shares it received from the dealers of S
        vec = dict(cs["dealers"])
        shares = [threshold_combine_subshares(used, [PrivateKey(RM.evaluate(vec[k], j + 1)) for k in used]) for j in range(n_new)]
        assert eng.register_keys_commitments(out, n_new) == (bytes(n_new), 0)
        assert eng.check_dealing(t_new, SEED) == (group, 0, NO_KEY)
        sigs, st = eng.batch_sign([msg] * n_new, b"".join(k.to_bytes() for k in shares))
        assert st == bytes(n_new)
        res = ECDSA.threshold_combine_keyed(msg, [Signature(s) for s in chunks(sigs, 64)], range(n_new), t_new, engine=eng, n_keys=n_new)
        assert res[1] == list(range(t_new)) and eng.batch_verify([msg], res[0].raw, group, flags=0) == bytes(1)
        seen.append(res[0].raw)
    assert seen[1] == seen[3] and (seen[0] != seen[2] or n == t)


def test_large_committee_once(eng, c):
    """(256, 171) -> (256, 171): the scalar model, C'_0 and the dealing check"""
    old, new = RC.DEVICE_ONLY_COMMITTEE
    f, secrets = RC.old_committee(*old)
    cs = RC.rs_case("honest_all", secrets, RC.honest_dealers(secrets, new[1], list(range(old[0]))), old[1], new[1])
    keys = derive(eng, secrets)
    assert eng.register_keys(b"".join(keys)) == bytes(old[0])
    rows = vectors_of(eng, cs)
    out, st, dealer_st, row = eng.reshare_commitments(b"".join(p for r in rows for p in r), list(range(old[0])), new[1], old[1], bm_words=8)
    status, want_st, used, taken, lam, scalars = RM.reshare_expected(cs)
    assert (st, dealer_st, row) == (0, bytes(old[0]), RM.bits_of(range(old[1]), 8))
    assert chunks(out) == [RM.key_of(c, v) for v in scalars] and out[:128] == RM.key_of(c, f[0])
    assert eng.check_dealing(old[1], SEED) == (out[:128], 0, NO_KEY)
    assert eng.register_keys_commitments(out, new[0]) == (bytes(new[0]), 0)
    assert eng.check_dealing(new[1], SEED) == (out[:128], 0, NO_KEY)


def test_refused_arguments(eng, c):
    cs = next(x for x in RC.rs_cases_for((5, 3), (3, 2)) if x["name"] == "honest_all")
    register(eng, c, cs)
    rows = vectors_of(eng, cs)
    vectors = b"".join(p for r in rows for p in r)
    lib, h = eng._lib, eng._h
    call = lib.bn254_ctx_reshare_commitments
    keys = (ctypes.c_uint32 * 5)(0, 1, 2, 3, 4)
    dst, row = ctypes.create_string_buffer(b"\xee" * 5, 5), (ctypes.c_uint32 * 2)(0xEEEEEEEE, 0xEEEEEEEE)
    out, st = ctypes.create_string_buffer(b"\xee" * 256, 256), ctypes.create_string_buffer(b"\xee", 1)
    good = [h, vectors, keys, 5, 2, 3, 0, dst, row, 1, out, st]
    for at in (0, 1, 2, 7, 8, 10, 11):                                                             # a NULL argument
        args = list(good)
        args[at] = None
        assert call(*args) == BAD_ARGUMENT, at
    for at, value in ((3, 0), (4, 0), (5, 0), (6, 1), (9, 0), (3, 1 << 32), (3, 1 << 31)):         # d, t_new, threshold, flags, bm_words, d * t_new
        args = list(good)
        args[at] = value
        assert call(*args) == BAD_ARGUMENT, (at, value)
    for order in ((0, 1, 1, 3, 4), (0, 2, 1, 3, 4), (4, 3, 2, 1, 0)):                              # not strictly increasing
        args = list(good)
        args[2] = (ctypes.c_uint32 * 5)(*order)
        assert call(*args) == BAD_ARGUMENT, order
    assert dst.raw == b"\xee" * 5 and list(row) == [0xEEEEEEEE] * 2 and out.raw == b"\xee" * 256 and st.raw == b"\xee"
    # the good call itself, and the context afterwards
    assert call(*good) == 0 and st.raw == b"\0" and dst.raw == bytes(5) and list(row) == [0b111, 0xEEEEEEEE]
    assert out.raw == b"".join(RM.key_of(c, v) for v in RM.reshare_expected(cs)[5])
    msgs = [b"m%d" % j for j in range(5)]
    sigs, sst = eng.batch_sign(msgs, be(cs["secrets"]))
    assert sst == bytes(5) and eng.batch_verify_keyed(msgs, sigs, list(range(5))) == bytes(5)
    # no registered keys
    assert eng.register_keys(b"") == b""
    assert call(*good) == BAD_ARGUMENT


def test_python_mirror(eng, c):
    """the API's own helpers end to end: deal (5, 3), reshare to (7, 4), register the new committee, sign"""
    from bn254_amd.api import (ECDSA, Error, ErrorKind, PublicKey, Signature, threshold_combine_subshares, threshold_commitments, threshold_deal)
    secret = (0xABCD << 180) + 99
    sks = threshold_deal(secret, 3, 5, seed=5)
    old = threshold_commitments(secret, 3, seed=5)
    assert ECDSA.register_keys_from_commitments(old, 5, engine=eng) == [None] * 5
    dealers = [(i, threshold_commitments(sks[i].value, 4, seed=100 + i)) for i in (4, 1, 3, 0)]
    assert dealers[0][1][0].raw == RM.key_of(c, sks[4].value)
    new, used, statuses = ECDSA.reshare_commitments(dealers, 3, engine=eng)
    assert used == [0, 1, 3] and statuses == [None] * 4 and len(new) == 4 and new[0].raw == old[0].raw == RM.key_of(c, secret)
    shares = [threshold_combine_subshares(used, [threshold_deal(sks[i].value, 4, 7, seed=100 + i)[j] for i in used]) for j in range(7)]
    assert ECDSA.register_keys_from_commitments(new, 7, register_group_key=True, engine=eng) == [None] * 7
    assert ECDSA.check_dealing(4, SEED, engine=eng).raw == old[0].raw
    msg = b"after the rotation"
    sigs, st = eng.batch_sign([msg] * 7, b"".join(k.to_bytes() for k in shares))
    res = ECDSA.threshold_combine_keyed(msg, [Signature(s) for s in chunks(sigs, 64)][2:6], range(2, 6), 4, engine=eng, n_keys=7)
    assert eng.batch_verify([msg], res[0].raw, old[0].raw, flags=0) == bytes(1)
    # dealer 1 publishes a vector whose first commitment is not its key; dealer 3's does not decode: too few are left
    assert ECDSA.register_keys_from_commitments(old, 5, engine=eng) == [None] * 5
    bad = [(k, list(v)) for k, v in dealers]
    bad[1][1][0] = old[0]
    new2, used2, statuses2 = ECDSA.reshare_commitments(bad, 3, engine=eng)
    assert used2 == [0, 3, 4] and statuses2 == [None, Error(ErrorKind.VerificationFailed), None, None] and new2[0].raw == old[0].raw
    bad[2][1][2] = PublicKey(DC.plant(bad[2][1][2].raw, "curve"))
    with pytest.raises(Error) as e:
        ECDSA.reshare_commitments(bad, 3, engine=eng)
    assert e.value.kind == ErrorKind.VerificationFailed and e.value.qualified == [0, 4]
    assert e.value.statuses == [None, Error(ErrorKind.VerificationFailed), Error(ErrorKind.InvalidGroupPoint), None]
    with pytest.raises(ValueError):
        ECDSA.reshare_commitments(dealers + [dealers[0]], 3, engine=eng)
    with pytest.raises(ValueError):
        threshold_combine_subshares([0, 0], shares[:2])


def test_cpp_mirror(eng, tmp_path):
    """host/reshare_example.cpp (both new calls through bn254.hpp) built with -Wall -Werror"""
    from bn254_amd import _native
    host = os.path.join(ROOT, "bn254_amd", "host")
    exe = str(tmp_path / "reshare_example")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", host,
                           os.path.join(host, "reshare_example.cpp"), "-o", exe, _native.LIB_PATH, "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "reshare: ok" in out.stdout
