"""One set of planted faults for the proof-of-possession calls (include/bn254_hip.h: bn254_batch_pop_verify, bn254_ctx_register_keys_pop),
shared by tests/test_gpu_pop.py and tests/test_gpu_register_keys_pop.py.  Nothing here imports the library under test: the caller hands in
keys and proofs it made (on the device, with batch_pop_prove) and signatures on the UNTAGGED key bytes (batch_sign), every fault is made
here on the bytes, and the expected status of a case is what a verify of the host-composed message TAG || pk reports — the library's own
batch_verify for the bulk, oracle.c_oracle.verify for the anchors.

A case is Case(name, pk, pop): 128 and 64 uncompressed bytes, all-zero = the identity of the batch ABI."""
import collections

from oracle import bn254_model as m

Q = m.Q
TAG = b"BN254G2_POP_V01:"
Case = collections.namedtuple("Case", "name pk pop")
O1, O2 = bytes(64), bytes(128)
# the status of every planted case under flags 0 / BN254_FLAG_REJECT_IDENTITY (the subgroup check is always on), as the scheme fixes them:
# a wrong proof is 9, a proof or key that does not decode reports its decode status (the proof's first), the identity is a point unless refused
EXPECT = {
    "good": (0, 0),
    "another key's proof": (9, 9),
    "untagged signature": (9, 9),
    "proof off the curve": (4, 4),
    "proof x >= q": (6, 6),
    "proof y >= q": (6, 6),
    "identity proof": (9, 4),
    "key off the twist": (4, 4),
    "key outside the subgroup": (4, 4),
    "key x.re >= q": (6, 6),
    "key y.im >= q": (6, 6),
    "identity key, identity proof": (0, 4),
    "identity key, good proof of another key": (9, 4),
    "proof off the curve, key off the twist": (4, 4),
    "proof x >= q, key off the twist": (6, 6),
}


def message(pk):
    return TAG + bytes(pk)


def _words(b):
    return [int.from_bytes(b[i:i + 32], "big") for i in range(0, len(b), 32)]


def coord(b, idx, value):
    w = _words(b)
    w[idx] = value
    return b"".join(int(v).to_bytes(32, "big") for v in w)


def off_curve(b):
    """the last coordinate + 1: the same x, no point of the curve / the twist"""
    w = _words(b)
    return coord(b, len(w) - 1, (w[-1] + 1) % Q)


def neg(b):
    w = _words(b)
    half = len(w) // 2
    return b"".join(int(v).to_bytes(32, "big") for v in w[:half] + [(-v) % Q for v in w[half:]])


def planted(pks, pops, untagged, off_subgroup_key):
    """The faults over the good pairs (pks[j], pops[j]), j < 8 at least: untagged[j] = sk_j * H(pk_j), the signature on the key bytes WITHOUT
    the tag; off_subgroup_key = a point of the twist outside the order-r subgroup."""
    assert len(pks) >= 8 and len(pops) == len(pks) and len(untagged) >= 1
    w1, w2 = _words(pops[3]), _words(pks[5])
    return [
        Case("good", pks[0], pops[0]),
        Case("another key's proof", pks[0], pops[1]),
        Case("untagged signature", pks[0], untagged[0]),
        Case("proof off the curve", pks[2], off_curve(pops[2])),
        Case("proof x >= q", pks[3], coord(pops[3], 0, w1[0] + Q)),            # reduced mod q it would be the good proof
        Case("proof y >= q", pks[3], coord(pops[3], 1, w1[1] + Q)),
        Case("identity proof", pks[4], O1),
        Case("key off the twist", off_curve(pks[4]), pops[4]),
        Case("key outside the subgroup", off_subgroup_key, pops[4]),
        Case("key x.re >= q", coord(pks[5], 0, w2[0] + Q), pops[5]),             # reduced mod q it would be the proven key
        Case("key y.im >= q", coord(pks[5], 3, w2[3] + Q), pops[5]),
        Case("identity key, identity proof", O2, O1),
        Case("identity key, good proof of another key", O2, pops[6]),
        Case("proof off the curve, key off the twist", off_curve(pks[7]), off_curve(pops[7])),   # the proof's status comes first
        Case("proof x >= q, key off the twist", off_curve(pks[7]), coord(pops[7], 0, _words(pops[7])[0] + Q)),
    ]


def expected(cases, flags):
    return bytes(EXPECT[cs.name][1 if flags & 2 else 0] for cs in cases)


def tile(cases, pks, pops, every=5):
    """the good pairs with case k % len(cases) planted at every `every`-th item: (pk list, pop list, {item: case})"""
    pks, pops, at = list(pks), list(pops), {}
    for k, i in enumerate(range(every - 1, len(pks), every)):
        cs = cases[k % len(cases)]
        pks[i], pops[i], at[i] = cs.pk, cs.pop, cs
    return pks, pops, at
