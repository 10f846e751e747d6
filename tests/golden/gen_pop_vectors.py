"""Writes tests/golden/pop_vectors.json: (sk, pk, pop) triples of the proof-of-possession scheme (include/bn254_hip.h: BN254_POP_TAG) from
oracle.bn254_model alone — pk = public_key(sk), pop = sign(TAG || pk, sk).  Run from the repository root: python tests/golden/gen_pop_vectors.py"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import bn254_model as M  # noqa: E402

TAG = b"BN254G2_POP_V01:"
SKS = [1, M.R - 1, 2 ** 256 - 1, M.R + 7, int.from_bytes(hashlib.sha256(b"pop vector 4").digest(), "big") % M.R, 0x1234567890ABCDEF]

out = []
for sk in SKS:
    skb = sk.to_bytes(32, "big")
    k = M.private_key_from_bytes(skb)
    pk = M.g2_to_uncompressed(M.public_key(k))
    out.append({"sk": skb.hex(), "pk": pk.hex(), "pop": M.g1_to_uncompressed(M.sign(TAG + pk, k)).hex()})
with open(os.path.join(ROOT, "tests", "golden", "pop_vectors.json"), "w") as f:
    json.dump({"tag": TAG.decode(), "vectors": out}, f, indent=1)
