"""One case set for compressed G1 signatures on the registered-key calls (include/bn254_hip.h: BN254_FLAG_G1_COMPRESSED), shared by the CPU
test of the staging and overlay bodies (tests/test_g1_stage.py) and the GPU tests (tests/test_gpu_compressed_keyed.py).  Built on
tests/codec_cases.py and oracle/c_oracle.py (sign, g1_compress, g1_decompress, verify); nothing here imports the library under test.

The key set: 9 registered keys — 7 good ones, one outside the order-r subgroup (registration status 4) and the identity (128 zero bytes).

An item is Item(kind, msg, enc, key, want): a 33-byte encoding said to be by registered key `key` on `msg`, and the status
bn254_batch_verify_keyed owes it, taken DIRECTLY from the oracle plus the rule order (decompression first — range 6, root 6, prefix 3 —,
then 2 for a key index out of range, the key's registration status, 1 for a message that does not hash within HASH_MAX_TRIES counters, and
only then the pairing check of c_oracle.verify).  The second expectation, the defining identity, needs the stand-ins: stand_in(enc) = the
64 bytes S(c) and the item's own status, by the oracle's g1_decompress and never by the device."""
import collections
import functools
import hashlib
import random

from oracle import bn254_model as m
from oracle import c_oracle as c
from tests import codec_cases as cc

Q, R = m.Q, m.R
N_KEYS, N_GOOD = 9, 7
K_OFF_SUB, K_IDENT = 7, 8
BM = 1
HASH_MAX_TRIES = 3                      # BN254_OPT_HASH_MAX_TRIES of the runs that include the "hash fails" items
STAND_IN = cc.be(Q) + bytes(32)         # BE32(q) || 0..0: decode status 6 under every flags value
Item = collections.namedtuple("Item", "kind msg enc key want")


def D(tag, i):
    return hashlib.sha256(tag.encode() + i.to_bytes(8, "little")).digest()


def sk(j):
    return (int.from_bytes(D("compressed/sk", j), "big") % (R - 1) + 1).to_bytes(32, "big")


def keys(not_in_subgroup_hex):
    """the 9 encodings (not_in_subgroup_hex: derived["g2_not_in_subgroup"] of tests/golden/derived_vectors.json) and what registration says"""
    pks = [c.public_key_g2(sk(j)) for j in range(N_GOOD)] + [bytes.fromhex(not_in_subgroup_hex), bytes(128)]
    return pks, [0] * N_GOOD + [4, 0]


@functools.lru_cache(maxsize=None)
def stand_in(enc):
    """(S(c), st): the oracle's decompression, or the stand-in and the status it was refused with"""
    try:
        return c.g1_decompress(enc), 0
    except c.OracleError as e:
        return STAND_IN, e.code


@functools.lru_cache(maxsize=None)
def _tries(msg):
    st, _, tries = c.hash_to_g1(msg)
    assert st == 0
    return tries


def message(tag, i, hashes=True):
    """a 32-byte message that hashes within HASH_MAX_TRIES counters (hashes) or needs more"""
    k = 0
    while (_tries(D("compressed/%s/%d" % (tag, i), k)) <= HASH_MAX_TRIES) != hashes:
        k += 1
    return D("compressed/%s/%d" % (tag, i), k)


def hash_fails(msg, max_tries):
    return bool(max_tries) and _tries(msg) > max_tries


def direct_status(pks, key_st, msg, enc, key, max_tries=0):
    """what bn254_batch_verify_keyed owes the item, from the oracle and the rule order alone"""
    u, st = stand_in(enc)
    if st:
        return st
    if key >= len(pks):
        return 2
    if key_st[key]:
        return key_st[key]
    if hash_fails(msg, max_tries):
        return 1
    return c.verify(msg, u, pks[key])


def _no_root_x(rnd):
    while True:
        x = rnd.randrange(Q)
        if cc.legendre(x * x * x + m.B1) < 0:
            return x


def no_root_x(tag):
    """BE32 of an x below q with no point on the curve, one per tag"""
    return cc.be(_no_root_x(random.Random("compressed/no-root/" + tag)))


MUTATIONS = ("unchanged", "flipped", "prefix04", "noroot02", "noroot07", "x_plus_q", "other_key", "zeros", "oob_good", "oob_bad", "far_oob_good",
             "refused_good", "refused_bad", "refused_noroot", "ident_key", "hash_good", "hash_bad")


def mutate(kind, i, pks, tag, rnd):
    """-> (msg, enc, key) of item i of the given kind"""
    key = i % N_GOOD
    msg = message(tag, i, hashes=not kind.startswith("hash_"))
    sig = c.sign(msg, sk(key))
    enc = c.g1_compress(sig)
    assert enc == cc.g1_compress(sig)
    if kind == "flipped":                                    # the other root: -sigma
        enc = bytes([5 - enc[0]]) + enc[1:]
    elif kind in ("prefix04", "oob_bad", "refused_bad", "hash_bad"):
        enc = b"\x04" + enc[1:]
    elif kind == "noroot02":
        enc = b"\x02" + cc.be(_no_root_x(rnd))
    elif kind in ("noroot07", "refused_noroot"):             # two faults: the root comes before the prefix
        enc = b"\x07" + cc.be(_no_root_x(rnd))
    elif kind == "x_plus_q":
        enc = enc[:1] + cc.be(int.from_bytes(enc[1:], "big") + Q)
    elif kind == "other_key":
        enc = c.g1_compress(c.sign(msg, sk((key + 1) % N_GOOD)))
    elif kind == "zeros":
        enc = bytes(33)
    if kind in ("oob_good", "oob_bad"):
        key = N_KEYS
    elif kind == "far_oob_good":
        key = N_KEYS + 20
    elif kind.startswith("refused_"):
        key = K_OFF_SUB
    elif kind == "ident_key":
        key = K_IDENT
    return msg, enc, key


def items(n, not_in_subgroup_hex, tag="items", max_tries=HASH_MAX_TRIES, kinds=MUTATIONS, valid_every=2):
    """n items: every `valid_every`-th position after the first round of kinds is an unchanged signature, the others walk the kinds in order, so
    that every wave of 64 mixes valid and failing items and any n >= len(kinds) holds every kind"""
    pks, key_st = keys(not_in_subgroup_hex)
    rnd = random.Random("compressed/" + tag)
    out, k = [], 0
    for i in range(n):
        if i >= len(kinds) and i % valid_every:
            kind = "unchanged"
        else:
            kind = kinds[k % len(kinds)]
            k += 1
        msg, enc, key = mutate(kind, i, pks, tag, rnd)
        out.append(Item(kind, msg, enc, key, direct_status(pks, key_st, msg, enc, key, max_tries)))
    return out


# what the issue pins for the kinds whose status does not depend on the oracle's arithmetic (zeros: the oracle decides)
PINNED = {"unchanged": 0, "flipped": 9, "prefix04": 3, "noroot02": 6, "noroot07": 6, "x_plus_q": 6, "other_key": 9, "oob_good": 2, "oob_bad": 3,
          "far_oob_good": 2, "refused_good": 4, "refused_bad": 3, "refused_noroot": 6, "hash_good": 1, "hash_bad": 3}


def overlay(statuses, pre):
    """the one change of the defining identity: an item that did not decompress reports its own status where the run on S(c) read 6"""
    return bytes(p if p and s == 6 else s for s, p in zip(statuses, pre))
