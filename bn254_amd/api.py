"""Host-side mirror of the reference's public API (/root/reference/src/lib.rs:60-63) on top of the
C ABI: same names, argument meaning and error behaviour, plus the batch entry point of the
north star.  Rust is not available in this image, so this mirror is Python (tests/bench) and
bn254_amd/host/bn254.hpp (C++); INTEGRATION.md holds the Rust shim a maintainer would add.

    ECDSA.sign(message, private_key) -> Signature               src/ecdsa.rs:26-35
    ECDSA.verify(message, signature, public_key) -> None/raise   src/ecdsa.rs:49-64
    ECDSA.batch_verify(messages, signatures, public_keys) -> [None | Error, ...]      (new)
    ECDSA.batch_verify_randomized(messages, signatures, public_keys, seed) -> same    (new, opt-in, probabilistic)
    ECDSA.aggregate_verify(messages, signature, public_keys) -> None/raise              (new: distinct messages, one sum)
    ECDSA.batch_aggregate_verify_distinct([(messages, signature, public_keys), ...]) -> [None | Error, ...]   (new)
    PrivateKey.prove_possession() / PublicKey.verify_possession(proof) / ECDSA.batch_verify_possession / ECDSA.register_keys_proven
                                                                 (new: proofs of possession, the remedy of src/lib.rs:34-38)
    check_public_keys(public_key_g2, public_key_g1)              src/ecdsa.rs:78-93
    PrivateKey / PublicKey / PublicKeyG1 / Signature             src/types.rs:13,81,151,222

All group arithmetic runs on the GPU through libbn254hip.so (no CPU fallback).  Points are
held as the reference's uncompressed byte encodings (identity = all-zero bytes).
"""
import enum

from . import engine as _engine

_Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
_R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


class ErrorKind(enum.IntEnum):
    """1 + index of the variant in /root/reference/src/error.rs:6-29 (0 = Ok)."""
    HashToPointError = 1
    IndexOutOfBounds = 2
    InvalidEncoding = 3
    InvalidGroupPoint = 4
    InvalidLength = 5
    NotMemberError = 6
    ToAffineConversion = 7
    PointInJacobian = 8
    VerificationFailed = 9
    SerializationError = 10
    HexDecodeFailed = 11


class Error(Exception):
    def __init__(self, kind):
        self.kind = ErrorKind(kind)
        super().__init__(self.kind.name)

    def __eq__(self, other):
        return isinstance(other, Error) and other.kind == self.kind

    def __hash__(self):
        return hash(self.kind)


def _raise(status):
    if status:
        raise Error(status)


def _eng():
    return _engine.default_engine()


def _lagrange_at_zero(xs):
    """the Lagrange coefficients at zero of the distinct points xs, mod r: prod x_k / prod (x_k - x_j) over k != j"""
    out = []
    for j, xj in enumerate(xs):
        num = den = 1
        for k, xk in enumerate(xs):
            if k != j:
                num, den = num * xk % _R, den * (xk - xj) % _R
        out.append(num * pow(den, -1, _R) % _R)
    return out


def threshold_deal(secret, t, n, seed):
    """Shamir-share `secret` (an integer, taken mod r) among n key indices with threshold t: a polynomial f of degree t - 1 with f(0) = secret
    and the other coefficients drawn from random.Random(seed); returns the n share secrets [PrivateKey(f(1)), .., PrivateKey(f(n))] — key
    index j holds f(j + 1), the numbering of ECDSA.threshold_combine_keyed.  For tests and examples: pure Python integers, NOT constant-time,
    and a seeded generator is no source of key material; a deployment deals with a DKG or a trusted dealer of its own."""
    import random
    if not 1 <= int(t) <= int(n):
        raise ValueError("need 1 <= t <= n")
    rnd = random.Random(seed)
    coeffs = [int(secret) % _R] + [rnd.randrange(_R) for _ in range(int(t) - 1)]
    return [PrivateKey(sum(c * pow(x, e, _R) for e, c in enumerate(coeffs)) % _R) for x in range(1, int(n) + 1)]


def threshold_commitments(secret, t, seed):
    """The Feldman commitments C_k = a_k * G2::one(), k < t, of the polynomial threshold_deal(secret, t, n, seed) shares — the same
    coefficients from the same generator — as t PublicKeys, C_0 = the group key.  What a dealer publishes beside the shares:
    ECDSA.register_keys_from_commitments derives the n share keys from them, ECDSA.batch_verify_dealt_shares checks a share against them.
    Under the warning of threshold_deal: pure Python integers and the C ABI, for tests and examples."""
    import random
    if int(t) < 1:
        raise ValueError("need 1 <= t")
    rnd = random.Random(seed)
    coeffs = [int(secret) % _R] + [rnd.randrange(_R) for _ in range(int(t) - 1)]
    out, st = _eng().batch_g2_mul(None, b"".join(c.to_bytes(32, "big") for c in coeffs), len(coeffs), reduce_scalar=True)
    for b in st:
        _raise(b)
    return [PublicKey(out[128 * k:128 * k + 128]) for k in range(len(coeffs))]


def threshold_combine_subshares(used_indices, subshares):
    """What a member of the NEXT committee keeps after a reshare: sum lambda_i(S) * sub_i mod r as a PrivateKey, over the sub-shares it
    received from the old members S = used_indices (key indices, x = index + 1; the set ECDSA.reshare_commitments reports), sub_i a
    PrivateKey — old member i's sub-dealing at this member's point.  Under the warning of threshold_deal: pure Python integers, for tests
    and examples."""
    keys, subs = [int(k) for k in used_indices], list(subshares)
    if len(keys) != len(subs) or len(set(keys)) != len(keys) or not keys:
        raise ValueError("need one sub-share per distinct used index")
    lam = _lagrange_at_zero([k + 1 for k in keys])
    return PrivateKey(sum(l * s.value for l, s in zip(lam, subs)) % _R)


def _neg_fq_bytes(b):
    v = int.from_bytes(b, "big")
    return (0 if v == 0 else _Q - v).to_bytes(32, "big")


class PrivateKey:
    """PrivateKey(Fr), /root/reference/src/types.rs:13-77."""

    def __init__(self, value):
        self.value = value % _R

    @classmethod
    def try_from(cls, data):
        if isinstance(data, str):
            try:
                data = bytes.fromhex(data)
            except ValueError:
                raise Error(ErrorKind.HexDecodeFailed)
        if len(data) != 32:                          # Fr::from_slice -> InvalidLength (types_test.rs:29-46)
            raise Error(ErrorKind.InvalidLength)
        return cls(int.from_bytes(data, "big"))      # values >= r are reduced (examples/bn254.rs:7-12)

    @classmethod
    def random(cls, rng):
        """rng: object with .randbytes(n) (e.g. random.Random) — Fr::random."""
        return cls(int.from_bytes(rng.randbytes(64), "big"))

    def to_bytes(self):
        return self.value.to_bytes(32, "big")

    def to_hex(self):
        return self.to_bytes().hex()

    def prove_possession(self):
        """The proof of possession of this key's PublicKey: the signature on POP_TAG + pk, pk the key's 128 uncompressed bytes
        (include/bn254_hip.h: bn254_batch_pop_prove).  A signer must refuse application messages that begin with POP_TAG."""
        _, pops, st = _eng().batch_pop_prove(self.to_bytes())
        _raise(st[0])
        return Signature(pops)

    def __eq__(self, other):
        return isinstance(other, PrivateKey) and other.value == self.value


class _G1Point:
    SIZE = 64

    def __init__(self, raw):
        assert len(raw) == 64
        self.raw = bytes(raw)

    @classmethod
    def from_uncompressed(cls, data):
        """utils.rs:119-127: length, coordinates < q, on curve."""
        data = bytes(data)
        if len(data) != 64:
            raise Error(ErrorKind.InvalidLength)
        _, st = _eng().batch_g1_add(data, bytes(64), 1)     # decode + (P + O) on the device
        _raise(st[0] if data != bytes(64) else ErrorKind.InvalidGroupPoint)
        return cls(data)

    @classmethod
    def from_compressed(cls, data):
        """bn::G1::from_compressed (types.rs:233-237): 0x02/0x03 || x."""
        data = bytes(data)
        if len(data) != 33:
            raise Error(ErrorKind.InvalidEncoding)
        out, st = _eng().batch_g1_decompress(data, 1)
        _raise(st[0])
        return cls(out)

    def to_uncompressed(self):
        if self.raw == bytes(64):
            raise Error(ErrorKind.PointInJacobian)          # utils.rs:184
        return self.raw

    def to_compressed(self):
        """utils.rs:84-104: 0x02 (y even) / 0x03 (y odd) || x."""
        if self.raw == bytes(64):
            raise Error(ErrorKind.PointInJacobian)
        return bytes([3 if self.raw[63] & 1 else 2]) + self.raw[:32]

    def __add__(self, other):
        out, st = _eng().batch_g1_add(self.raw, other.raw, 1)
        _raise(st[0])
        return type(self)(out)

    def __neg__(self):
        if self.raw == bytes(64):
            return type(self)(self.raw)
        return type(self)(self.raw[:32] + _neg_fq_bytes(self.raw[32:]))

    def __sub__(self, other):
        return self + (-other)


class Signature(_G1Point):
    """Signature(G1), /root/reference/src/types.rs:222-286 (no PartialEq in the reference)."""


class PublicKeyG1(_G1Point):
    """PublicKeyG1(G1), /root/reference/src/types.rs:151-218."""

    @classmethod
    def from_private_key(cls, private_key):
        out, st = _eng().batch_g1_mul(None, private_key.to_bytes(), 1, reduce_scalar=True)      # None = G1::one(): the fixed-base table
        _raise(st[0])
        return cls(out)


class PublicKey:
    """PublicKey(G2), /root/reference/src/types.rs:81-148."""
    SIZE = 128

    def __init__(self, raw):
        assert len(raw) == 128
        self.raw = bytes(raw)

    @classmethod
    def from_private_key(cls, private_key):
        out, st = _eng().batch_g2_mul(None, private_key.to_bytes(), 1, reduce_scalar=True)
        _raise(st[0])
        return cls(out)

    @classmethod
    def from_uncompressed(cls, data):
        """utils.rs:107-116: length, coordinates < q, on curve and in the order-r subgroup."""
        data = bytes(data)
        if len(data) != 128:
            raise Error(ErrorKind.InvalidLength)
        if data == bytes(128):
            raise Error(ErrorKind.InvalidGroupPoint)
        # decode with the subgroup check on the device: e(G1, pk) pairing-check path validates it
        st = _eng().batch_pairing_check((1).to_bytes(32, "big") + (2).to_bytes(32, "big"), data, 1, 1,
                                        flags=_engine.FLAG_G2_SUBGROUP_CHECK)
        if st[0] not in (0, ErrorKind.VerificationFailed):
            raise Error(st[0])
        return cls(data)

    @classmethod
    def from_compressed(cls, data):
        """bn::G2::from_compressed (types.rs:91-93): 0x0a/0x0b || BE64(x.im*q + x.re); subgroup-checked."""
        data = bytes(data)
        if len(data) != 65:
            raise Error(ErrorKind.InvalidEncoding)
        out, st = _eng().batch_g2_decompress(data, 1)
        _raise(st[0])
        return cls(out)

    def verify_possession(self, proof):
        """None iff `proof` (a Signature) is this key's proof of possession — ECDSA.verify of POP_TAG + the key's bytes with the key
        validated as from_uncompressed does (subgroup check, identity refused); raises the Error otherwise.  The proof is bound to
        the key's encoding bytes (include/bn254_hip.h: bn254_batch_pop_verify)."""
        _raise(ECDSA._possession_status([self], [proof], None)[0])

    def to_uncompressed(self):
        if self.raw == bytes(128):
            raise Error(ErrorKind.PointInJacobian)          # utils.rs:163
        return self.raw

    def to_compressed(self):
        """utils.rs:130-158: sign || BE64(x.im*q + x.re), sign 0x0b iff u512(y) > u512(-y)."""
        if self.raw == bytes(128):
            raise Error(ErrorKind.PointInJacobian)
        w = [int.from_bytes(self.raw[i:i + 32], "big") for i in range(0, 128, 32)]
        y = w[3] * _Q + w[2]
        yn = ((-w[3]) % _Q) * _Q + ((-w[2]) % _Q)
        return bytes([0x0B if y > yn else 0x0A]) + (w[1] * _Q + w[0]).to_bytes(64, "big")

    def __add__(self, other):
        out, st = _eng().batch_g2_add(self.raw, other.raw, 1)
        _raise(st[0])
        return PublicKey(out)

    def __neg__(self):
        if self.raw == bytes(128):
            return PublicKey(self.raw)
        return PublicKey(self.raw[:64] + _neg_fq_bytes(self.raw[64:96]) + _neg_fq_bytes(self.raw[96:]))

    def __sub__(self, other):
        return self + (-other)

    def __eq__(self, other):
        return isinstance(other, PublicKey) and other.raw == self.raw

    def __hash__(self):
        return hash(self.raw)


class ECDSA:
    """BLS-style aggregate signatures on BN254 (the reference calls the struct ECDSA, src/ecdsa.rs:12-13)."""

    @staticmethod
    def sign(message, private_key):
        sigs, st = _eng().batch_sign([bytes(message)], private_key.to_bytes())
        _raise(st[0])
        return Signature(sigs)

    @staticmethod
    def verify(message, signature, public_key):
        """Returns None on success, raises Error(VerificationFailed / HashToPointError) otherwise."""
        st = _eng().batch_verify([bytes(message)], signature.raw, public_key.raw)
        _raise(st[0])

    @staticmethod
    def batch_verify(messages, signatures, public_keys, engine=None):
        """result[i] is None iff ECDSA.verify(messages[i], signatures[i], public_keys[i]) succeeds,
        else the Error it would raise."""
        n = len(messages)
        if not (len(signatures) == n and len(public_keys) == n):
            raise Error(ErrorKind.InvalidLength)
        eng = engine or _eng()
        st = eng.batch_verify([bytes(m) for m in messages], b"".join(s.raw for s in signatures), b"".join(p.raw for p in public_keys))
        return [None if s == 0 else Error(s) for s in st]


    @staticmethod
    def register_keys(public_keys, engine=None):
        """Register a validator set with the engine for `batch_verify_keyed` (replaces the previous set): result[j] is None,
        or the Error PublicKey.from_uncompressed would raise for key j (types.rs:96-99; the subgroup check always runs)."""
        eng = engine or _eng()
        st = eng.register_keys(b"".join(p.raw for p in public_keys))
        return [None if s == 0 else Error(s) for s in st]

    @staticmethod
    def _possession_status(public_keys, proofs, engine):
        if len(public_keys) != len(proofs):
            raise Error(ErrorKind.InvalidLength)
        eng = engine or _eng()
        return eng.batch_pop_verify(b"".join(p.raw for p in public_keys), b"".join(s.raw for s in proofs), flags=_engine.FLAG_REJECT_IDENTITY)

    @staticmethod
    def batch_verify_possession(public_keys, proofs, engine=None):
        """result[j] is None iff public_keys[j].verify_possession(proofs[j]) succeeds, else the Error it would raise."""
        return [None if s == 0 else Error(s) for s in ECDSA._possession_status(public_keys, proofs, engine)]

    @staticmethod
    def register_keys_proven(public_keys, proofs, engine=None):
        """register_keys with every key's proof of possession checked on the device (include/bn254_hip.h: bn254_ctx_register_keys_pop):
        result[j] is None, the Error register_keys gives for key j, or the Error verify_possession raises — and that result is the key's
        registration status: every keyed call (batch_verify_keyed, the keyed-signers calls, the keyed aggregates) refuses a key whose
        proof failed with Error(VerificationFailed).  The identity is refused, as a key and as a proof."""
        if len(public_keys) != len(proofs):
            raise Error(ErrorKind.InvalidLength)
        eng = engine or _eng()
        st = eng.register_keys_pop(b"".join(p.raw for p in public_keys), b"".join(s.raw for s in proofs), flags=_engine.FLAG_REJECT_IDENTITY)
        return [None if s == 0 else Error(s) for s in st]

    @staticmethod
    def _g1_input(signatures, compressed):
        """-> (the list of a call's G1 input points as bytes, the engine flag).  compressed=True: the signatures are the 33-byte wire
        encodings as `bytes` (Signature.to_compressed) — any other length raises Error(InvalidEncoding), as Signature.from_compressed
        does — and are decompressed on the device, inside the call (include/bn254_hip.h: BN254_FLAG_G1_COMPRESSED): an encoding that
        does not decompress gets the Error from_compressed would raise as its status and is never verified, taken or counted.  Else:
        Signature objects, a raw encoding of the wrong length raises Error(InvalidLength)."""
        if compressed:
            raw = [bytes(s) for s in signatures]
            if any(len(b) != _engine.G1_COMPRESSED_BYTES for b in raw):
                raise Error(ErrorKind.InvalidEncoding)
            return raw, _engine.FLAG_G1_COMPRESSED
        raw = [s.raw for s in signatures]
        if any(len(b) != _engine.G1_BYTES for b in raw):
            raise Error(ErrorKind.InvalidLength)
        return raw, 0

    @staticmethod
    def _flag_kw(flag):
        """the keyword a call of the engine takes beyond its arguments without the flag: none for decoded signatures"""
        return {"flags": flag} if flag else {}

    @staticmethod
    def batch_verify_keyed(messages, signatures, key_indices, engine=None, compressed=False):
        """batch_verify with public_keys[i] named by its index in the registered set: result[i] is None iff
        ECDSA.verify(messages[i], signatures[i], registered[key_indices[i]]) succeeds, Error(IndexOutOfBounds) for an index
        outside the set, else the Error verify would raise.  compressed=True: signatures[i] is the 33-byte wire encoding (bytes); the
        Error Signature.from_compressed would raise comes first (ECDSA._g1_input)."""
        n = len(messages)
        if not (len(signatures) == n and len(key_indices) == n):
            raise Error(ErrorKind.InvalidLength)
        raw, flag = ECDSA._g1_input(signatures, compressed)
        eng = engine or _eng()
        st = eng.batch_verify_keyed([bytes(m) for m in messages], b"".join(raw), [int(k) for k in key_indices], **ECDSA._flag_kw(flag))
        return [None if s == 0 else Error(s) for s in st]

    @staticmethod
    def verify_keyed_signers(message, signature, signer_indices, engine=None, compressed=False):
        """One message, one already aggregated signature, and the indices (in the registered set, ECDSA.register_keys) of the keys that
        signed: None iff e(H(message), sum of those keys) * e(signature, -G2) == 1; raises Error(IndexOutOfBounds) for an index outside
        the set, a refused key's registration Error, else what verify raises (include/bn254_hip.h: bn254_batch_verify_keyed_bitmap).
        Assumes a proof of possession of every registered key (ECDSA.register_keys_proven registers a set with its proofs checked).
        compressed=True: signature is the 33-byte wire encoding (ECDSA._g1_input)."""
        _raise(ECDSA._keyed_signers_status([(message, signature, signer_indices)], engine, compressed=compressed)[0])

    @staticmethod
    def _signer_rows(items, compressed):
        """(message, signature, signer_indices) triples -> (message bytes, signature bytes, indices as integers)"""
        rows = []
        for item in items:
            if len(item) != 3:
                raise Error(ErrorKind.InvalidLength)
            message, signature, signer_indices = item
            raw, flag = ECDSA._g1_input([signature], compressed)
            rows.append((bytes(message), raw[0], ECDSA._signer_indices(signer_indices)))
        return rows

    @staticmethod
    def _signer_indices(signer_indices):
        idx = [int(j) for j in signer_indices]
        if any(j < 0 for j in idx):
            raise Error(ErrorKind.IndexOutOfBounds)
        return idx

    @staticmethod
    def _signer_bitmaps(eng, idx_lists):
        """-> (bitmap words, bm_words): as wide as the registered set plus ONE bit, on which every index outside the set lands (rule 2 reports
        the lowest bad bit, and every such index lies above the set); an engine that does not know its set: as wide as the largest index"""
        n_keys = getattr(eng, "n_registered_keys", None)
        top = n_keys if n_keys is not None else max([j for idx in idx_lists for j in idx], default=-1)
        bm_words = top // 32 + 1
        bits = [0] * (len(idx_lists) * bm_words)
        for i, idx in enumerate(idx_lists):
            for j in idx:
                j = min(j, top)
                bits[i * bm_words + j // 32] |= 1 << (j % 32)
        return bits, bm_words

    @staticmethod
    def _keyed_signers_status(items, engine, seed=None, flags=0, compressed=False):
        rows = ECDSA._signer_rows(items, compressed)
        flags |= _engine.FLAG_G1_COMPRESSED if compressed else 0
        eng = engine or _eng()
        bits, bm_words = ECDSA._signer_bitmaps(eng, [r[2] for r in rows])
        if seed is not None:
            return eng.batch_verify_keyed_bitmap_randomized([r[0] for r in rows], b"".join(r[1] for r in rows), bits, bm_words, seed, flags)
        return eng.batch_verify_keyed_bitmap([r[0] for r in rows], b"".join(r[1] for r in rows), bits, bm_words, **ECDSA._flag_kw(flags))

    @staticmethod
    def batch_aggregate_public_keys_signers(signer_lists, engine=None):
        """result[i]: the PublicKey that is the sum of the registered keys signer_lists[i] names (the identity for an empty list or a sum
        that cancels), or Error(IndexOutOfBounds) for an index outside the set / a refused key's registration Error — summed on the
        device from the set's subset tables (include/bn254_hip.h: bn254_batch_aggregate_keys_bitmap)"""
        eng = engine or _eng()
        lists = [ECDSA._signer_indices(idx) for idx in signer_lists]
        bits, bm_words = ECDSA._signer_bitmaps(eng, lists)
        keys, st = eng.batch_aggregate_keys_bitmap(bits, bm_words, len(lists))
        return [PublicKey(keys[128 * i:128 * i + 128]) if s == 0 else Error(s) for i, s in enumerate(st)]

    @staticmethod
    def aggregate_public_key_signers(signer_indices, engine=None):
        """the sum of the registered keys signer_indices names; raises the Error batch_aggregate_public_keys_signers would return"""
        res = ECDSA.batch_aggregate_public_keys_signers([signer_indices], engine)[0]
        if isinstance(res, Error):
            raise res
        return res

    @staticmethod
    def batch_verify_keyed_signers_export(items, engine=None, compressed=False):
        """batch_verify_keyed_signers that also returns what the device computed: result[i] = (None or the Error, H(message) as 64 bytes,
        the signers' aggregate PublicKey).  The two outputs are zero bytes / the identity key unless the item passed every check before the
        pairing (Error None or VerificationFailed) — include/bn254_hip.h: bn254_batch_verify_keyed_bitmap_export"""
        rows = ECDSA._signer_rows(items, compressed)
        flags = _engine.FLAG_G1_COMPRESSED if compressed else 0
        eng = engine or _eng()
        bits, bm_words = ECDSA._signer_bitmaps(eng, [r[2] for r in rows])
        st, hashes, keys = eng.batch_verify_keyed_bitmap_export([r[0] for r in rows], b"".join(r[1] for r in rows), bits, bm_words, **ECDSA._flag_kw(flags))
        return [(None if s == 0 else Error(s), hashes[64 * i:64 * i + 64], PublicKey(keys[128 * i:128 * i + 128])) for i, s in enumerate(st)]

    @staticmethod
    def verify_keyed_signers_export(message, signature, signer_indices, engine=None, compressed=False):
        """one item of batch_verify_keyed_signers_export: (None or the Error, H(message) bytes, aggregate PublicKey) — nothing is raised"""
        return ECDSA.batch_verify_keyed_signers_export([(message, signature, signer_indices)], engine, compressed)[0]

    @staticmethod
    def register_key_weights(weights, engine=None):
        """voting weights of the registered keys, one non-negative integer below 2^64 per key (None forgets them); a total of 2^64 or more
        or a count other than the registered one is refused.  Every registration forgets the weights."""
        (engine or _eng()).set_key_weights(None if weights is None else [int(w) for w in weights])

    @staticmethod
    def batch_signers_weight(signer_lists, engine=None):
        """result[i]: the sum of the weights of the registered keys signer_lists[i] names, or the Error of the first bad index (as
        batch_aggregate_public_keys_signers).  A registered identity key counts its weight."""
        eng = engine or _eng()
        lists = [ECDSA._signer_indices(idx) for idx in signer_lists]
        bits, bm_words = ECDSA._signer_bitmaps(eng, lists)
        weight, st = eng.batch_bitmap_weights(bits, bm_words, len(lists))
        return [w if s == 0 else Error(s) for w, s in zip(weight, st)]

    @staticmethod
    def signers_weight(signer_indices, engine=None):
        res = ECDSA.batch_signers_weight([signer_indices], engine)[0]
        if isinstance(res, Error):
            raise res
        return res

    @staticmethod
    def batch_verify_keyed_signers(items, engine=None, compressed=False):
        """items: a list of (message, signature, signer_indices); result[i] is None iff ECDSA.verify_keyed_signers on item i succeeds, else
        the Error it would raise.  An item that is not such a triple raises Error(InvalidLength) before any device work.
        compressed=True: every signature is its 33-byte wire encoding (ECDSA._g1_input)."""
        return [None if s == 0 else Error(s) for s in ECDSA._keyed_signers_status(items, engine, compressed=compressed)]

    @staticmethod
    def aggregate_keyed_signers(message, signatures, key_indices, engine=None, n_keys=None, compressed=False):
        """One message and the individual signatures of some registered keys (signatures[k] said to be by key key_indices[k] of the set,
        ECDSA.register_keys): every signature is verified against its key, those that pass are added — one per key, however many valid
        ones a key sent — and the result is (aggregate Signature, sorted indices of the keys that signed, statuses), statuses[k] None or
        the Error ECDSA.batch_verify_keyed would give signature k.  The pair feeds ECDSA.verify_keyed_signers.  Raises the message's
        Error(HashToPointError) (include/bn254_hip.h: bn254_batch_collect_keyed_bitmap).  compressed=True: the signatures are their 33-byte
        wire encodings (ECDSA._g1_input); the aggregate comes back as a Signature."""
        r = ECDSA.batch_aggregate_keyed_signers([(message, signatures, key_indices)], engine, n_keys, compressed)[0]
        if isinstance(r, Error):
            raise r
        return r

    @staticmethod
    def batch_aggregate_keyed_signers(items, engine=None, n_keys=None, compressed=False):
        """items: a list of (message, signatures, key_indices); result[i] is what ECDSA.aggregate_keyed_signers returns for item i, or the
        Error it would raise.  A malformed item (not such a triple, lengths that differ, an index that is negative or >= 2^32) raises
        before any device work.  n_keys: the size of the registered set, for an engine that did not register it itself."""
        return ECDSA._aggregate_keyed_signers(items, engine, n_keys, compressed=compressed)

    @staticmethod
    def _aggregate_keyed_signers(items, engine, n_keys, seed=None, flags=0, optimistic=False, compressed=False):
        rows = []
        for item in items:
            if len(item) != 3:
                raise Error(ErrorKind.InvalidLength)
            message, signatures, key_indices = item
            sigs, idx = list(signatures), [int(j) for j in key_indices]
            if len(sigs) != len(idx):
                raise Error(ErrorKind.InvalidLength)
            sigs, flag = ECDSA._g1_input(sigs, compressed)
            if any(j < 0 or j >= 1 << 32 for j in idx):
                raise Error(ErrorKind.IndexOutOfBounds)
            rows.append((bytes(message), sigs, idx))
        flags |= _engine.FLAG_G1_COMPRESSED if compressed else 0
        eng = engine or _eng()
        if n_keys is None:
            n_keys = getattr(eng, "n_registered_keys", None)
        if n_keys is None:             # the bitmaps are as wide as the registered set, which the items cannot tell
            raise ValueError("the engine does not know its registered key count: pass n_keys")
        bm_words = max((int(n_keys) + 31) // 32, 1)
        args = ([r[0] for r in rows], b"".join(s for r in rows for s in r[1]), [j for r in rows for j in r[2]], [len(r[2]) for r in rows], bm_words)
        if optimistic:
            share_st, tuple_st, agg, bits = eng.batch_collect_keyed_bitmap_optimistic(*args, **ECDSA._flag_kw(flags))
        elif seed is not None:
            share_st, tuple_st, agg, bits = eng.batch_collect_keyed_bitmap_randomized(*args, seed, flags)
        else:
            share_st, tuple_st, agg, bits = eng.batch_collect_keyed_bitmap(*args, **ECDSA._flag_kw(flags))
        out, at = [], 0
        for i, (_, _, idx) in enumerate(rows):
            st = share_st[at:at + len(idx)]
            at += len(idx)
            if tuple_st[i]:
                out.append(Error(tuple_st[i]))
                continue
            row = bits[i * bm_words:(i + 1) * bm_words]
            signers = [j for j in range(32 * bm_words) if (row[j // 32] >> (j % 32)) & 1]
            out.append((Signature(agg[64 * i:64 * i + 64]), signers, [None if b == 0 else Error(b) for b in st]))
        return out

    @staticmethod
    def threshold_combine_keyed(message, signatures, key_indices, threshold, engine=None, n_keys=None, compressed=False):
        """t-of-n threshold BLS over the registered keys (ECDSA.register_keys; key j is the share key f(j + 1) * G2 of a dealing, so index 0
        is a legal signer): every share signatures[k], said to be by key key_indices[k], is verified against its key; if at least
        `threshold` keys have a valid share, the shares of the `threshold` LOWEST such keys are interpolated at zero.  Returns (the group
        Signature — which ECDSA.verify accepts under the group key, ECDSA.threshold_group_key —, the sorted indices used, statuses) with
        statuses[k] None or the Error ECDSA.batch_verify_keyed would give share k.  Raises Error(VerificationFailed) with fewer valid
        keys — the error's .signers lists who was there, .statuses the shares' — and the message's Error(HashToPointError).  This call
        checks every share against its registered key; that the registered keys lie on one polynomial of degree threshold - 1 is
        ECDSA.check_dealing's to check, once per key set (include/bn254_hip.h: bn254_batch_threshold_combine_keyed)."""
        r = ECDSA.batch_threshold_combine_keyed([(message, signatures, key_indices)], threshold, engine, n_keys, compressed)[0]
        if isinstance(r, Error):
            raise r
        return r

    @staticmethod
    def batch_threshold_combine_keyed(items, threshold, engine=None, n_keys=None, compressed=False):
        """items: a list of (message, signatures, key_indices), one threshold for all; result[i] is what ECDSA.threshold_combine_keyed returns
        for item i, or the Error it would raise.  A malformed item raises Error(InvalidLength) / Error(IndexOutOfBounds), a threshold below
        1 ValueError, before any device work.  compressed=True: the shares are their 33-byte wire encodings (ECDSA._g1_input)."""
        return ECDSA._threshold_batch(items, threshold, engine, n_keys, False, compressed)

    @staticmethod
    def register_group_key(public_key, engine=None):
        """Name the group key f(0) * G2 of the registered dealing (ECDSA.threshold_group_key computes it from share keys) for
        threshold_combine_keyed_optimistic; None forgets it.  Raises the Error PublicKey.from_uncompressed would raise for the key, and
        then no group key is set.  ECDSA.register_keys / register_keys_proven forget the group key: a new key set is a new dealing.  This
        call does not check that the registered keys interpolate to this key (ECDSA.check_dealing computes the key they do interpolate
        to) — a key that does not belong to the set only makes the optimistic call as slow as the exact one (include/bn254_hip.h:
        bn254_ctx_set_group_key)."""
        eng = engine or _eng()
        _raise(eng.set_group_key(None if public_key is None else public_key.raw))

    @staticmethod
    def threshold_combine_keyed_optimistic(message, signatures, key_indices, threshold, engine=None, n_keys=None, compressed=False):
        """threshold_combine_keyed by interpolating the `threshold` lowest keys with a well-formed share first and verifying the RESULT once
        under the group key (ECDSA.register_group_key) — the check the signature's consumer will make.  A result that passes is the group
        signature; then the shares outside the keys used were not verified (their status is None if they are well-formed and name a
        registered key) and shares whose errors cancel under the coefficients read None.  A result that fails sends the tuple through
        the exact call: the same return value or Error.  Take threshold_combine_keyed when the per-share verdicts matter
        (include/bn254_hip.h: bn254_batch_threshold_combine_keyed_optimistic)."""
        r = ECDSA.batch_threshold_combine_keyed_optimistic([(message, signatures, key_indices)], threshold, engine, n_keys, compressed)[0]
        if isinstance(r, Error):
            raise r
        return r

    @staticmethod
    def batch_threshold_combine_keyed_optimistic(items, threshold, engine=None, n_keys=None, compressed=False):
        """batch_threshold_combine_keyed, every item as threshold_combine_keyed_optimistic treats it.  A malformed item and a threshold below
        1 raise as there, an engine without a group key ValueError, all before any device work."""
        return ECDSA._threshold_batch(items, threshold, engine, n_keys, True, compressed)

    @staticmethod
    def _threshold_batch(items, threshold, engine, n_keys, optimistic, compressed=False):
        if int(threshold) < 1 or int(threshold) >= 1 << 32:
            raise ValueError("threshold must be between 1 and 2^32 - 1")
        rows = []
        for item in items:
            if len(item) != 3:
                raise Error(ErrorKind.InvalidLength)
            message, signatures, key_indices = item
            sigs, idx = list(signatures), [int(j) for j in key_indices]
            if len(sigs) != len(idx):
                raise Error(ErrorKind.InvalidLength)
            sigs, _ = ECDSA._g1_input(sigs, compressed)
            if any(j < 0 or j >= 1 << 32 for j in idx):
                raise Error(ErrorKind.IndexOutOfBounds)
            rows.append((bytes(message), sigs, idx))
        eng = engine or _eng()
        if n_keys is None:
            n_keys = getattr(eng, "n_registered_keys", None)
        if n_keys is None:
            raise ValueError("the engine does not know its registered key count: pass n_keys")
        bm_words = max((int(n_keys) + 31) // 32, 1)
        if optimistic and not getattr(eng, "group_key_set", False):
            raise ValueError("the engine has no group key: ECDSA.register_group_key first")
        call = eng.batch_threshold_combine_keyed_optimistic if optimistic else eng.batch_threshold_combine_keyed
        share_st, tuple_st, group, bits, _ = call(
            [r[0] for r in rows], b"".join(s for r in rows for s in r[1]), [j for r in rows for j in r[2]], [len(r[2]) for r in rows], bm_words,
            int(threshold), **ECDSA._flag_kw(_engine.FLAG_G1_COMPRESSED if compressed else 0))
        out, at = [], 0
        for i, (_, _, idx) in enumerate(rows):
            st = [None if b == 0 else Error(b) for b in share_st[at:at + len(idx)]]
            at += len(idx)
            row = bits[i * bm_words:(i + 1) * bm_words]
            signers = [j for j in range(32 * bm_words) if (row[j // 32] >> (j % 32)) & 1]
            if tuple_st[i]:
                err = Error(tuple_st[i])
                err.signers, err.statuses = signers, st
                out.append(err)
            else:
                out.append((Signature(group[64 * i:64 * i + 64]), signers, st))
        return out

    @staticmethod
    def threshold_group_key(indices, public_keys, engine=None):
        """The group key f(0) * G2 interpolated from the share keys of `indices` (distinct key indices; public_keys[k] is the key of
        indices[k] = f(indices[k] + 1) * G2): sum lambda_k pk_k, the coefficients from Python integers, the points through
        bn254_batch_g2_mul and bn254_batch_g2_sum.  Any `threshold` keys of one dealing give the same key."""
        idx, pks = [int(j) for j in indices], list(public_keys)
        if len(idx) != len(pks) or not idx or len(set(idx)) != len(idx):
            raise Error(ErrorKind.InvalidLength)
        if any(j < 0 or j >= 1 << 32 for j in idx):
            raise Error(ErrorKind.IndexOutOfBounds)
        lam = _lagrange_at_zero([j + 1 for j in idx])
        eng = engine or _eng()
        prod, st = eng.batch_g2_mul(b"".join(p.raw for p in pks), b"".join(k.to_bytes(32, "big") for k in lam), len(idx))
        for b in st:
            _raise(b)
        out, st = eng.batch_g2_sum(prod, [0, len(idx)])
        _raise(st[0])
        return PublicKey(out)

    @staticmethod
    def check_dealing(threshold, seed=None, engine=None, register=False):
        """Are the registered keys (ECDSA.register_keys / register_keys_proven; key j standing for x_j = j + 1) a `threshold`-of-n dealing —
        do they lie on one polynomial of degree below `threshold`?  Returns the group PublicKey they interpolate to; with register=True
        it is then named as the group key (ECDSA.register_group_key).  Raises Error(VerificationFailed) for a key set that is no dealing
        (or has fewer keys than the threshold), and, for a key whose registration status is non-zero, that key's Error with the index
        in .key.  The check is randomised over `seed` (32 bytes; None draws them from os.urandom): a refusal is always right, an
        acceptance wrong with probability at most 2^-128 if the seed is fresh — drawn after the keys were fixed — and the keys were
        registered with the subgroup check, which ECDSA.register_keys always runs (include/bn254_hip.h: bn254_ctx_check_dealing)."""
        import os
        if int(threshold) < 1 or int(threshold) >= 1 << 32:
            raise ValueError("threshold must be between 1 and 2^32 - 1")
        seed = os.urandom(32) if seed is None else bytes(seed)
        if len(seed) != 32:
            raise Error(ErrorKind.InvalidLength)
        eng = engine or _eng()
        pk, st, bad = eng.check_dealing(int(threshold), seed)
        if st:
            err = Error(st)
            err.key = None if bad == 0xFFFFFFFF else bad
            raise err
        key = PublicKey(pk)
        if register:
            ECDSA.register_group_key(key, eng)
        return key

    @staticmethod
    def commitments_eval(commitments, xs, engine=None):
        """The polynomial with the G2 coefficients `commitments` (PublicKeys, lowest degree first: a dealer's Feldman commitments) at the
        integer points xs (each 0 <= x < 2^32): [sum x^k C_k as a PublicKey, ..] (include/bn254_hip.h: bn254_batch_g2_poly_eval).  The share
        key of key index j is the value at x = j + 1.  Raises the first commitment's decode Error."""
        cs, xs = list(commitments), [int(x) for x in xs]
        if any(len(c.raw) != _engine.G2_BYTES for c in cs):
            raise Error(ErrorKind.InvalidLength)
        if any(x < 0 or x >= 1 << 32 for x in xs):
            raise Error(ErrorKind.IndexOutOfBounds)
        out, st = (engine or _eng()).batch_g2_poly_eval(b"".join(c.raw for c in cs), [0, len(cs)], [0] * len(xs), xs)
        for b in st:
            _raise(b)
        return [PublicKey(out[128 * e:128 * e + 128]) for e in range(len(xs))]

    @staticmethod
    def register_keys_from_commitments(commitments, n, register_group_key=False, engine=None):
        """Register the n share keys pk_j = f(j + 1) * G2 of the dealing whose Feldman commitments these are, derived on the device
        (include/bn254_hip.h: bn254_ctx_register_keys_commitments) — ECDSA.register_keys on commitments_eval(commitments, 1 .. n) without the
        keys crossing to the host and back.  result[j] is None or the Error register_keys would give key j.  A commitment that does not
        decode raises its Error, and then NO keys are registered.  With register_group_key=True commitments[0] is then named as the group
        key (ECDSA.register_group_key, whose checks apply).  ECDSA.check_dealing(len(commitments)) passes on such a set by construction."""
        cs = list(commitments)
        if not cs or int(n) < 1 or int(n) >= 1 << 32 or any(len(c.raw) != _engine.G2_BYTES for c in cs):
            raise Error(ErrorKind.InvalidLength)
        eng = engine or _eng()
        key_st, st = eng.register_keys_commitments(b"".join(c.raw for c in cs), int(n))
        _raise(st)
        if register_group_key:
            ECDSA.register_group_key(cs[0], eng)
        return [None if s == 0 else Error(s) for s in key_st]

    @staticmethod
    def combine_commitments(vectors, engine=None):
        """The commitments of the SUM of the qualified dealers' polynomials (a DKG's last step): the element-wise sum of their commitment
        vectors, all of one length, through bn254_batch_g2_sum — [sum_d vectors[d][k] for k].  Raises the first decode Error."""
        vs = [list(v) for v in vectors]
        if not vs or not vs[0] or any(len(v) != len(vs[0]) for v in vs):
            raise Error(ErrorKind.InvalidLength)
        t, d = len(vs[0]), len(vs)
        out, st = (engine or _eng()).batch_g2_sum(b"".join(vs[i][k].raw for k in range(t) for i in range(d)), [k * d for k in range(t + 1)])
        for b in st:
            _raise(b)
        return [PublicKey(out[128 * k:128 * k + 128]) for k in range(t)]

    @staticmethod
    def batch_verify_dealt_shares(vectors, index, secrets, engine=None):
        """What the holder of key `index` checks in a DKG round: dealer d's share secrets[d] (a PrivateKey) is good iff secrets[d] * G2::one()
        equals dealer d's commitment vector vectors[d] evaluated at index + 1.  The left sides by the fixed-base key derivation, the right
        sides by ONE bn254_batch_g2_poly_eval over all the vectors.  Returns one verdict per dealer: None, Error(VerificationFailed), or the
        decode Error of that dealer's first faulty commitment."""
        vs, sks = [list(v) for v in vectors], list(secrets)
        if len(vs) != len(sks) or int(index) < 0 or int(index) + 1 >= 1 << 32:
            raise Error(ErrorKind.InvalidLength)
        if not vs:
            return []
        eng = engine or _eng()
        left, st = eng.batch_g2_mul(None, b"".join(k.to_bytes() for k in sks), len(sks), reduce_scalar=True)
        for b in st:
            _raise(b)
        off = [0]
        for v in vs:
            off.append(off[-1] + len(v))
        right, rst = eng.batch_g2_poly_eval(b"".join(c.raw for v in vs for c in v), off, list(range(len(vs))), [int(index) + 1] * len(vs))
        return [Error(rst[d]) if rst[d] else None if left[128 * d:128 * d + 128] == right[128 * d:128 * d + 128] else Error(ErrorKind.VerificationFailed)
                for d in range(len(vs))]

    @staticmethod
    def g2_msm(points, scalars, engine=None):
        """sum scalars[k] * points[k] in G2 (points: PublicKey, scalars: integers, taken mod r) as a PublicKey (include/bn254_hip.h:
        bn254_batch_g2_msm); raises the first point's decode Error"""
        pts, ks = list(points), [int(k) % _R for k in scalars]
        if len(pts) != len(ks) or any(len(p.raw) != _engine.G2_BYTES for p in pts):
            raise Error(ErrorKind.InvalidLength)
        out, st = (engine or _eng()).batch_g2_msm(b"".join(p.raw for p in pts), b"".join(k.to_bytes(32, "big") for k in ks), [0, len(pts)])
        _raise(st[0])
        return PublicKey(out)

    @staticmethod
    def g2_vector_combine(vectors, scalars, engine=None):
        """[sum_i scalars[i] * vectors[i][k] for k]: vectors of PublicKeys, all of one length, one integer (taken mod r) per vector
        (include/bn254_hip.h: bn254_batch_g2_vector_combine) — a linear combination of commitment vectors.  Raises the first decode Error."""
        vs, ks = [list(v) for v in vectors], [int(k) % _R for k in scalars]
        if not vs or not vs[0] or len(vs) != len(ks) or any(len(v) != len(vs[0]) for v in vs) or any(len(p.raw) != _engine.G2_BYTES for v in vs for p in v):
            raise Error(ErrorKind.InvalidLength)
        out, st = (engine or _eng()).batch_g2_vector_combine(b"".join(p.raw for v in vs for p in v), b"".join(k.to_bytes(32, "big") for k in ks),
                                                             len(vs), len(vs[0]))
        for b in st:
            _raise(b)
        return [PublicKey(out[128 * k:128 * k + 128]) for k in range(len(vs[0]))]

    @staticmethod
    def reshare_commitments(dealers, threshold, engine=None):
        """Hand the registered (OLD) committee's group key on to the next committee: dealers is an iterable of (key_index, [PublicKey ..]) —
        old member key_index's commitments to its sub-dealing, threshold_commitments(share.value, t_new, seed), all of one length t_new; it
        is sorted by index, and a repeated index raises ValueError.  A dealer qualifies if its key is registered and not refused, its
        commitments decode and the first one IS its registered key; the `threshold` lowest qualified indices S are combined under their
        Lagrange coefficients (include/bn254_hip.h: bn254_ctx_reshare_commitments).  Returns (the t_new commitments of the new polynomial as
        PublicKeys — [0] is the unchanged group key; ECDSA.register_keys_from_commitments registers the new committee from them —, the
        sorted indices used, statuses) with statuses[i] None or the Error of the i-th dealer in index order.  With fewer qualified dealers
        it raises Error(VerificationFailed) carrying .statuses and .qualified (their indices).  Not checked: that the registered keys are a
        dealing (ECDSA.check_dealing), that the private sub-shares match the vectors (each recipient's ECDSA.batch_verify_dealt_shares)."""
        ds = sorted(((int(k), list(v)) for k, v in dealers), key=lambda kv: kv[0])
        if any(a[0] == b[0] for a, b in zip(ds, ds[1:])):
            raise ValueError("a dealer index is repeated")
        if int(threshold) < 1 or int(threshold) >= 1 << 32:
            raise ValueError("threshold must be between 1 and 2^32 - 1")
        if not ds or not ds[0][1] or any(len(v) != len(ds[0][1]) for _, v in ds) or any(len(p.raw) != _engine.G2_BYTES for _, v in ds for p in v):
            raise Error(ErrorKind.InvalidLength)
        if any(k < 0 or k >= 1 << 32 for k, _ in ds):
            raise Error(ErrorKind.IndexOutOfBounds)
        t_new = len(ds[0][1])
        out, st, dealer_st, row = (engine or _eng()).reshare_commitments(b"".join(p.raw for _, v in ds for p in v), [k for k, _ in ds], t_new, int(threshold))
        statuses = [None if s == 0 else Error(s) for s in dealer_st]
        used = [32 * w + b for w, word in enumerate(row) for b in range(32) if (word >> b) & 1]
        if st != 0:
            err = Error(st)
            err.statuses, err.qualified = statuses, used
            raise err
        return [PublicKey(out[128 * k:128 * k + 128]) for k in range(t_new)], used, statuses

    @staticmethod
    def g1_msm(points, scalars, engine=None):
        """sum scalars[k] * points[k] in G1 (points: Signature / PublicKeyG1, scalars: integers, taken mod r) as a Signature
        (include/bn254_hip.h: bn254_batch_g1_msm); raises the first point's decode Error"""
        pts, ks = list(points), [int(k) % _R for k in scalars]
        if len(pts) != len(ks) or any(len(p.raw) != _engine.G1_BYTES for p in pts):
            raise Error(ErrorKind.InvalidLength)
        out, st = (engine or _eng()).batch_g1_msm(b"".join(p.raw for p in pts), b"".join(k.to_bytes(32, "big") for k in ks), [0, len(pts)])
        _raise(st[0])
        return Signature(out)

    @staticmethod
    def merge_keyed_signers(message, parts, engine=None, n_keys=None, compressed=False):
        """One message and some PARTIAL aggregates of it — parts[k] = (Signature, signer_indices), the sum of the signatures of those keys of
        the registered set, as a child of an aggregation tree sends it: every partial is verified as ECDSA.verify_keyed_signers verifies it,
        and, in the order given, the valid ones whose indices do not overlap what was taken before are added (first fit: sort by
        descending number of signers for the largest cover).  Returns (aggregate Signature, sorted indices of the union, statuses, taken):
        statuses[k] is None or the Error verify_keyed_signers would raise for partial k, taken[k] a bool.  The first two feed
        ECDSA.verify_keyed_signers.  Raises the message's Error(HashToPointError) (include/bn254_hip.h: bn254_batch_merge_keyed_bitmap).
        Assumes a proof of possession of every registered key (ECDSA.register_keys_proven registers a set with its proofs checked)."""
        r = ECDSA.batch_merge_keyed_signers([(message, parts)], engine, n_keys, compressed=compressed)[0]
        if isinstance(r, Error):
            raise r
        return r

    @staticmethod
    def batch_merge_keyed_signers(items, engine=None, n_keys=None, optimistic=False, compressed=False):
        """items: a list of (message, parts); result[i] is what ECDSA.merge_keyed_signers returns for item i, or the Error it would raise.
        A malformed item (not such a pair, a part that is not a pair, a signature of the wrong length, an index that is negative or >= 2^32)
        raises before any device work.  n_keys: the size of the registered set, for an engine that did not register it itself (without
        either the bitmaps are as wide as the largest index).  optimistic: see batch_merge_keyed_signers_optimistic.  compressed=True: every
        part's signature is its 33-byte wire encoding (ECDSA._g1_input); the merged aggregate comes back as a Signature."""
        rows = []
        for item in items:
            if not isinstance(item, (tuple, list)) or len(item) != 2:
                raise Error(ErrorKind.InvalidLength)
            message, parts = item
            sigs, sets = [], []
            for part in parts:
                if not isinstance(part, (tuple, list)) or len(part) != 2:
                    raise Error(ErrorKind.InvalidLength)
                raw, _ = ECDSA._g1_input([part[0]], compressed)
                idx = [int(j) for j in part[1]]
                if any(j < 0 or j >= 1 << 32 for j in idx):
                    raise Error(ErrorKind.IndexOutOfBounds)
                sigs.append(raw[0])
                sets.append(idx)
            rows.append((bytes(message), sigs, sets))
        eng = engine or _eng()
        # the bitmaps as ECDSA.verify_keyed_signers builds them: as wide as the registered set plus ONE bit, on which every index outside
        # the set lands (such a partial reads IndexOutOfBounds and is never taken, so the bit never reaches the union)
        if n_keys is None:
            n_keys = getattr(eng, "n_registered_keys", None)
        top = int(n_keys) if n_keys is not None else max([j for _, _, sets in rows for idx in sets for j in idx], default=-1)
        bm_words = top // 32 + 1
        bits = []
        for _, _, sets in rows:
            for idx in sets:
                row = [0] * bm_words
                for j in idx:
                    j = min(j, top)
                    row[j // 32] |= 1 << (j % 32)
                bits += row
        merge = eng.merge_keyed_bitmap_optimistic if optimistic else eng.merge_keyed_bitmap
        part_st, taken, tuple_st, agg, union = merge([r[0] for r in rows], b"".join(s for r in rows for s in r[1]), bits, [len(r[1]) for r in rows], bm_words,
                                                     **ECDSA._flag_kw(_engine.FLAG_G1_COMPRESSED if compressed else 0))
        out, at = [], 0
        for i, (_, sigs, _) in enumerate(rows):
            st, tk = part_st[at:at + len(sigs)], taken[at:at + len(sigs)]
            at += len(sigs)
            if tuple_st[i]:
                out.append(Error(tuple_st[i]))
                continue
            row = union[i * bm_words:(i + 1) * bm_words]
            signers = [j for j in range(32 * bm_words) if (row[j // 32] >> (j % 32)) & 1]
            out.append((Signature(agg[64 * i:64 * i + 64]), signers, [None if b == 0 else Error(b) for b in st], [bool(b) for b in tk]))
        return out

    @staticmethod
    def batch_merge_keyed_signers_optimistic(items, engine=None, n_keys=None, compressed=False):
        """batch_merge_keyed_signers with one verify per item — the sum of its partials that pass every check short of the pairing, against
        the keys of the union of their indices — and the partials verified one by one only in an item whose sum fails or in which two such
        partials overlap (include/bn254_hip.h: bn254_batch_merge_keyed_bitmap_optimistic).  The same result list and the same refusals
        before any device work.  The aggregate and the indices are always a pair ECDSA.verify_keyed_signers accepts.  ONE deviation:
        partials whose errors cancel within an item that passes (sigma_a + D and sigma_b - D, also with no indices at all) read None and
        are taken — a None there means "taken into a sum that verifies", not "individually valid".  Who needs per-partial verdicts takes
        batch_merge_keyed_signers."""
        return ECDSA.batch_merge_keyed_signers(items, engine, n_keys, optimistic=True, compressed=compressed)

    @staticmethod
    def merge_keyed_signers_optimistic(message, parts, engine=None, n_keys=None, compressed=False):
        """merge_keyed_signers through batch_merge_keyed_signers_optimistic: the same quadruple, the same Errors raised, the same one
        deviation (partials whose errors cancel within a sum that verifies read None and are taken)."""
        r = ECDSA.batch_merge_keyed_signers_optimistic([(message, parts)], engine, n_keys, compressed)[0]
        if isinstance(r, Error):
            raise r
        return r

    @staticmethod
    def batch_aggregate_keyed_signers_optimistic(items, engine=None, n_keys=None, compressed=False):
        """batch_aggregate_keyed_signers with one verify per item — the sum of its signatures that pass every check short of the pairing,
        against the sum of their keys — and the signatures verified one by one only in an item whose sum fails, that names a key twice, or
        that is too short (include/bn254_hip.h: bn254_batch_collect_keyed_bitmap_optimistic).  The same result list and the same refusals
        before any device work; no seed.  The aggregate and the indices are always a pair ECDSA.verify_keyed_signers accepts.  ONE
        deviation: signatures whose errors cancel within an item that passes (sigma_a + D and sigma_b - D) read None and are counted — a
        None there means "counted in a sum that verifies", not "individually valid".  Who needs per-signature verdicts takes
        batch_aggregate_keyed_signers."""
        return ECDSA._aggregate_keyed_signers(items, engine, n_keys, optimistic=True, compressed=compressed)

    @staticmethod
    def aggregate_keyed_signers_optimistic(message, signatures, key_indices, engine=None, n_keys=None, compressed=False):
        """aggregate_keyed_signers through batch_aggregate_keyed_signers_optimistic: the same triple, the same Errors raised."""
        r = ECDSA.batch_aggregate_keyed_signers_optimistic([(message, signatures, key_indices)], engine, n_keys, compressed)[0]
        if isinstance(r, Error):
            raise r
        return r

    @staticmethod
    def batch_aggregate_keyed_signers_randomized(items, seed=None, engine=None, n_keys=None, rand64=False, compressed=False):
        """batch_aggregate_keyed_signers with the pairing checks of the signatures combined, 64 signatures of one key at a time across the
        items of the call (include/bn254_hip.h: bn254_batch_collect_keyed_bitmap_randomized): the same result list and the same refusals
        before any device work.  An Error among the statuses is always the exact one; a None is wrong with probability <= 2^-128 per group
        (2^-64 with rand64) for a fresh SECRET seed (32 bytes; default os.urandom): who knows the seed can make two bad signatures of one
        key pass together."""
        import os
        if seed is None:
            seed = os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed must be 32 bytes")
        return ECDSA._aggregate_keyed_signers(items, engine, n_keys, bytes(seed), _engine.FLAG_RAND64 if rand64 else 0, compressed=compressed)

    @staticmethod
    def aggregate_keyed_signers_randomized(message, signatures, key_indices, seed=None, engine=None, n_keys=None, rand64=False, compressed=False):
        """aggregate_keyed_signers through batch_aggregate_keyed_signers_randomized: the same triple, the same Errors raised."""
        r = ECDSA.batch_aggregate_keyed_signers_randomized([(message, signatures, key_indices)], seed, engine, n_keys, rand64, compressed)[0]
        if isinstance(r, Error):
            raise r
        return r

    @staticmethod
    def batch_verify_keyed_signers_randomized(items, seed=None, engine=None, rand64=False, compressed=False):
        """batch_verify_keyed_signers with the pairing checks of whole groups of items combined (include/bn254_hip.h:
        bn254_batch_verify_keyed_bitmap_randomized): the same result list; an Error is always the exact one, a None is wrong with probability
        <= 2^-128 per group (2^-64 with rand64) for a secret seed (32 bytes; default os.urandom)."""
        import os
        if seed is None:
            seed = os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed must be 32 bytes")
        flags = _engine.FLAG_RAND64 if rand64 else 0
        return [None if s == 0 else Error(s) for s in ECDSA._keyed_signers_status(items, engine, bytes(seed), flags, compressed)]

    @staticmethod
    def batch_verify_keyed_randomized(messages, signatures, key_indices, seed=None, engine=None, rand64=False, compressed=False):
        """batch_verify_keyed through the combined check of items that share a key (64 per pairing product; include/bn254_hip.h:
        bn254_batch_verify_keyed_randomized).  Errors are exact; a None is wrong with probability <= 2^-128 per group."""
        import os
        n = len(messages)
        if not (len(signatures) == n and len(key_indices) == n):
            raise Error(ErrorKind.InvalidLength)
        raw, flag = ECDSA._g1_input(signatures, compressed)
        eng = engine or _eng()
        st = eng.batch_verify_keyed_randomized([bytes(m) for m in messages], b"".join(raw), [int(k) for k in key_indices],
                                               seed if seed is not None else os.urandom(32), flags=(_engine.FLAG_RAND64 if rand64 else 0) | flag)
        return [None if s == 0 else Error(s) for s in st]

    @staticmethod
    def batch_verify_compressed(messages, signatures33, public_keys65, engine=None):
        """batch_verify straight from the compressed wire encodings (33-byte signatures, 65-byte public keys):
        result[i] is None, or the Error that Signature/PublicKey.from_compressed or verify would raise."""
        n = len(messages)
        if not (len(signatures33) == n and len(public_keys65) == n):
            raise Error(ErrorKind.InvalidLength)
        if any(len(s) != 33 for s in signatures33) or any(len(p) != 65 for p in public_keys65):
            raise Error(ErrorKind.InvalidEncoding)
        eng = engine or _eng()
        st = eng.batch_verify_compressed([bytes(m) for m in messages], b"".join(bytes(s) for s in signatures33),
                                         b"".join(bytes(p) for p in public_keys65))
        return [None if s == 0 else Error(s) for s in st]

    @staticmethod
    def batch_verify_randomized(messages, signatures, public_keys, seed=None, engine=None, rand64=False):
        """Same result shape as batch_verify through the randomised combined check (64 items per pairing
        product, include/bn254_hip.h: bn254_batch_verify_randomized).  Errors are always exact; a None is wrong
        with probability <= 2^-128 per group for a fresh secret `seed` (32 bytes; default os.urandom)."""
        import os
        n = len(messages)
        if not (len(signatures) == n and len(public_keys) == n):
            raise Error(ErrorKind.InvalidLength)
        eng = engine or _eng()
        st, _ = eng.batch_verify_randomized([bytes(m) for m in messages], b"".join(s.raw for s in signatures),
                                            b"".join(p.raw for p in public_keys), seed if seed is not None else os.urandom(32),
                                            flags=_engine.FLAG_RAND64 if rand64 else 0)
        return [None if s == 0 else Error(s) for s in st]

    @staticmethod
    def aggregate_verify(messages, signature, public_keys, engine=None):
        """Aggregate signature over DISTINCT messages (the IRTF BLS draft's AggregateVerify): signature = the sum of the signatures of
        public_keys[j] on messages[j] (`Add for Signature`, src/types.rs:264-270).  Returns None, or raises the Error of the first failing
        check: signature, keys, messages, then VerificationFailed (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct).
        Assumes a proof of possession of every key (PublicKey.verify_possession, ECDSA.batch_verify_possession; for registered keys
        ECDSA.register_keys_proven); distinct messages are NOT enforced here."""
        if len(messages) != len(public_keys):
            raise Error(ErrorKind.InvalidLength)
        _raise(ECDSA._distinct_status([(messages, signature, public_keys)], engine)[0])

    @staticmethod
    def _distinct_status(aggregates, engine):
        msgs, pks, sigs, sizes = [], [], [], []
        for messages, signature, public_keys in aggregates:
            if len(messages) != len(public_keys):
                raise Error(ErrorKind.InvalidLength)
            msgs.extend(bytes(m) for m in messages)
            pks.extend(p.raw for p in public_keys)
            sigs.append(signature.raw)
            sizes.append(len(messages))
        eng = engine or _eng()
        return eng.batch_aggregate_verify_distinct(msgs, b"".join(pks), b"".join(sigs), sizes)

    @staticmethod
    def batch_aggregate_verify_distinct(aggregates, engine=None):
        """aggregates: a list of (messages, signature, public_keys); result[i] is None iff ECDSA.aggregate_verify on item i succeeds,
        else the Error it would raise.  A length mismatch in any item raises Error(InvalidLength) before any device work."""
        return [None if s == 0 else Error(s) for s in ECDSA._distinct_status(aggregates, engine)]

    @staticmethod
    def aggregate_verify_keyed(messages, signature, key_indices, engine=None):
        """aggregate_verify with public_keys[j] named by its index in the registered set (ECDSA.register_keys): Error(IndexOutOfBounds)
        for an index outside the set, a refused key's registration Error, else what aggregate_verify raises
        (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct_keyed)."""
        if len(messages) != len(key_indices):
            raise Error(ErrorKind.InvalidLength)
        _raise(ECDSA._distinct_keyed_status([(messages, signature, key_indices)], engine)[0])

    @staticmethod
    def _distinct_keyed_status(aggregates, engine, seed=None, flags=0):
        msgs, idx, sigs, sizes = [], [], [], []
        for messages, signature, key_indices in aggregates:
            if len(messages) != len(key_indices):
                raise Error(ErrorKind.InvalidLength)
            msgs.extend(bytes(m) for m in messages)
            idx.extend(int(k) for k in key_indices)
            sigs.append(signature.raw)
            sizes.append(len(messages))
        eng = engine or _eng()
        if seed is not None:
            return eng.batch_aggregate_verify_distinct_keyed_randomized(msgs, idx, b"".join(sigs), sizes, seed, flags)
        return eng.batch_aggregate_verify_distinct_keyed(msgs, idx, b"".join(sigs), sizes)

    @staticmethod
    def batch_aggregate_verify_distinct_keyed(aggregates, engine=None):
        """aggregates: a list of (messages, signature, key_indices); result[i] is None iff ECDSA.aggregate_verify_keyed on item i succeeds,
        else the Error it would raise.  A length mismatch in any item raises Error(InvalidLength) before any device work."""
        return [None if s == 0 else Error(s) for s in ECDSA._distinct_keyed_status(aggregates, engine)]

    @staticmethod
    def batch_aggregate_verify_distinct_keyed_randomized(aggregates, seed=None, engine=None, rand64=False):
        """batch_aggregate_verify_distinct_keyed with the pairing checks of whole groups of aggregates combined under random weights
        (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct_keyed_randomized): the same result shape and InvalidLength checks; an
        Error is always the exact one, a None is wrong with probability <= 2^-128 per group (2^-64 with rand64) for a secret seed
        (32 bytes, default os.urandom(32))."""
        import os
        if seed is None:
            seed = os.urandom(32)
        if len(seed) != 32:
            raise ValueError("seed must be 32 bytes")
        flags = _engine.FLAG_RAND64 if rand64 else 0
        return [None if s == 0 else Error(s) for s in ECDSA._distinct_keyed_status(aggregates, engine, bytes(seed), flags)]


def check_public_keys(public_key_g2, public_key_g1):
    """/root/reference/src/ecdsa.rs:78-93."""
    st = _eng().batch_check_public_keys(public_key_g2.raw, public_key_g1.raw, 1)
    _raise(st[0])


def _le_chunks(data):
    """each 32-byte big-endian chunk byte-reversed: zeropool-bn's Borsh (little-endian) affine coordinates"""
    return b"".join(data[i:i + 32][::-1] for i in range(0, len(data), 32))


_NEG_G2_ONE = None


def _neg_g2_one():
    global _NEG_G2_ONE
    if _NEG_G2_ONE is None:
        g2 = PublicKey.from_private_key(PrivateKey(1))
        _NEG_G2_ONE = (-g2).raw
    return _NEG_G2_ONE


def format_pairing_check_uncompressed_values(message, signature, public_key):
    """/root/reference/src/utils.rs:216-239: the two (G1, G2) tuples of the verification equation
    e(H(m), pk) * e(sig, -G2::one()) as 64-/128-byte little-endian buffers for an on-chain alt_bn128
    pairing precompile.  `signature` (64 B) and `public_key` (128 B) are the uncompressed big-endian
    encodings; like the reference this does NOT validate them (it only re-orders bytes) and raises
    IndexError-like InvalidLength on short input where the reference would panic."""
    signature, public_key = bytes(signature), bytes(public_key)
    if len(signature) < 64 or len(public_key) < 128:
        raise Error(ErrorKind.InvalidLength)
    pts, st, _ = _eng().batch_hash_to_g1([bytes(message)])
    _raise(st[0])
    return [(_le_chunks(pts), _le_chunks(public_key[:128])), (_le_chunks(signature[:64]), _le_chunks(_neg_g2_one()))]


def format_pairing_check_values(message, signature, public_key):
    """/root/reference/src/utils.rs:197-214: the same from COMPRESSED signature (33 B) and public key (65 B);
    both are decoded (and thereby validated) first."""
    sig = Signature.from_compressed(signature)
    pk = PublicKey.from_compressed(public_key)
    return format_pairing_check_uncompressed_values(message, sig.raw, pk.raw)


def format_pairing_check_keyed_signers(message, signature, signer_indices, engine=None, compressed=False):
    """format_pairing_check_uncompressed_values(message, signature, apk) for apk = the sum of the registered keys signer_indices names
    (the reference's layout, src/utils.rs:216-239), from ONE device call: the bitmap verify that returns H(message) and apk
    (ECDSA.verify_keyed_signers_export).  Raises the item's Error for any failure — VerificationFailed included: a failing aggregate is
    never formatted — and Error(PointInJacobian) for an identity aggregate key, as PublicKey.to_uncompressed does.  compressed=True:
    signature is the 33-byte wire encoding; the formatted signature is its decompressed form."""
    err, h, apk = ECDSA.verify_keyed_signers_export(message, signature, signer_indices, engine, compressed)
    if err is not None:
        raise err
    sig = Signature.from_compressed(signature).raw if compressed else bytes(signature.raw)
    return [(_le_chunks(h), _le_chunks(apk.to_uncompressed())), (_le_chunks(sig[:64]), _le_chunks(_neg_g2_one()))]
