#!/usr/bin/env python3
"""Compressed G1 signatures on the registered-key calls (BN254_FLAG_G1_COMPRESSED) against the two routes beside the flag, whole HOST-POINTER
calls under a host clock (time.perf_counter around the call: staging, kernels, copies home and the wait), 256 registered keys, two thirds of
them signing every tuple, every share valid.  Per shape three routes, alternating, `--reps` runs each after two warm-up runs — the median
with the min and max beside it:
  (A) the call with the flag on the 33-byte encodings;
  (B) the route that exists without the flag: bn254_batch_g1_decompress (host memory to host memory), the host-side filter — a share that
      does not decompress comes back as 64 zero bytes, which is the identity and decodes, so it has to be replaced by something no decoder
      accepts and its status remembered —, the uncompressed call, and the two status arrays merged by hand.  Its interval contains its host
      work: that is the route;
  (C) the uncompressed call on points that are already uncompressed: the floor.  A - C = the square roots plus the staging kernel, minus
      the 31 bytes per share that no longer cross PCIe.
Shapes: the exact and the optimistic collect at n tuples x k shares (default 256 x 171 and 2048 x 171), bn254_batch_verify_keyed at
`--keyed` items (default 65 536).  Every line says whether A's outputs are B's and C's bytes.
--uncompressed-only measures route C alone and records a digest of its outputs: run once per build (BN254_LIB names another build of the
library) to compare a build with its parent — same digests, times within each other's spread.
    python tools/compressed_throughput.py [out.jsonl] [--reps R] [--keys K] [--keyed N] [--note TEXT] [--uncompressed-only] [shape ...]   shape = n:k"""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: one HIP runtime per process)
import bn254_amd  # noqa: E402
from bn254_amd import _native  # noqa: E402
from tests.datagen import sk_bytes  # noqa: E402

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
Q = 0x30644E72E131A029B85045B68181585D97816A916871CA8D3C208C16D87CFD47
SHAPES = [(256, 171), (2048, 171)]
MSG_LEN = 32
FLAG = 4                                                  # BN254_FLAG_G1_COMPRESSED
STAND_IN = np.frombuffer(Q.to_bytes(32, "big") + bytes(32), dtype=np.uint8)


def _check(rc):
    if rc != 0:
        raise RuntimeError("library call failed: %d" % rc)


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return {"ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def compress(points):
    """n * 64 bytes -> n * 33 (the byte rule of the reference's src/utils.rs:84-104)"""
    p = np.frombuffer(points, dtype=np.uint8).reshape(-1, 64)
    out = np.empty((len(p), 33), dtype=np.uint8)
    out[:, 0] = 2 + (p[:, 63] & 1)
    out[:, 1:] = p[:, :32]
    return out.tobytes()


def buf(n):
    return ctypes.create_string_buffer(max(n, 1))


def decompress_and_filter(lib, h, enc, m, points, pre):
    """route B's first two steps: points = what the uncompressed call may read, pre = the statuses to merge in afterwards"""
    _check(lib.bn254_batch_g1_decompress(h, enc, m, points, pre))
    st = np.frombuffer(pre, dtype=np.uint8, count=m)
    bad = np.flatnonzero(st)
    if len(bad):
        np.frombuffer(points, dtype=np.uint8, count=64 * m).reshape(m, 64)[bad] = STAND_IN
    return st, bad


def merge_statuses(status, m, st, bad):
    if len(bad):
        out = np.frombuffer(status, dtype=np.uint8, count=m)
        hit = bad[out[bad] == 6]
        out[hit] = st[hit]


def measure(routes, reps, only=None):
    names = [r for r in routes if only is None or r in only]
    for _ in range(2):
        for r in names:
            routes[r]()
    ms = {r: [] for r in names}
    for _ in range(reps):
        for r in names:
            ms[r].append(wall(routes[r]))
    return {r: spread(v) for r, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--keys", type=int, default=256)
    ap.add_argument("--keyed", type=int, default=65536)
    ap.add_argument("--note", default=None, help="recorded with every line, e.g. which build ran")
    ap.add_argument("--uncompressed-only", action="store_true")
    a = ap.parse_intermixed_args()
    out = open(a.out, "a") if a.out else sys.stdout
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes] or SHAPES
    only = ("C",) if a.uncompressed_only else None
    n_keys = a.keys
    eng = bn254_amd.Engine(0)
    lib, h = eng._lib, eng._h
    box = {"device": torch.cuda.get_device_name(0), "lib_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16],
           "n_keys": n_keys, "reps": a.reps, "clock": "host, whole host-pointer calls"}
    if a.note:
        box["note"] = a.note
    rng = np.random.default_rng(20261021)
    sks = [int.from_bytes(sk_bytes(11000 + j), "big") % R for j in range(n_keys)]
    pool, st = eng.batch_g2_mul(None, b"".join(s.to_bytes(32, "big") for s in sks), n_keys, reduce_scalar=True)
    assert st == bytes(n_keys) and eng.register_keys(pool) == bytes(n_keys)
    bm_words = (n_keys + 31) // 32
    for n, k in shapes:
        k = min(k, n_keys)
        m = n * k
        keys = np.concatenate([rng.permutation(n_keys)[:k] for _ in range(n)]).astype(np.uint32)
        msgs = [hashlib.sha256(b"compressed/tp/%d/%d/%d" % (n, k, i)).digest() for i in range(n)]
        shares, st = eng.batch_sign([msgs[s // k] for s in range(m)], b"".join(sks[j].to_bytes(32, "big") for j in keys))
        assert st == bytes(m)
        enc = compress(shares)
        blob = b"".join(msgs)
        moff = (ctypes.c_uint64 * (n + 1))(*[MSG_LEN * i for i in range(n + 1)])
        soff = (ctypes.c_uint64 * (n + 1))(*[k * i for i in range(n + 1)])
        c_keys = (ctypes.c_uint32 * m)(*keys.tolist())
        for name in ("bn254_batch_collect_keyed_bitmap", "bn254_batch_collect_keyed_bitmap_optimistic"):
            fn = getattr(lib, name)
            o = {r: (buf(m), buf(n), buf(64 * n), (ctypes.c_uint32 * (n * bm_words))(), (ctypes.c_uint32 * n)()) for r in "ABC"}
            points, pre = buf(64 * m), buf(m)

            def call(items, flags, r):
                _check(fn(h, blob, moff, items, c_keys, soff, m, n, bm_words, flags, *o[r]))

            def route_b():
                st_b, bad = decompress_and_filter(lib, h, enc, m, points, pre)
                call(points, 0, "B")
                merge_statuses(o["B"][0], m, st_b, bad)
            routes = {"A": lambda: call(enc, FLAG, "A"), "B": route_b, "C": lambda: call(shares, 0, "C")}
            res = measure(routes, a.reps, only)
            digest = hashlib.sha256(b"".join(bytes(x) for x in o["C"])).hexdigest()[:16]
            row = {"kind": "compressed", "call": name, "shape": "%dx%d" % (n, k), "n": n, "shares_per_tuple": k, "n_shares": m, **res,
                   "outputs_C_sha256": digest, **box}
            if only is None:
                row["A_is_B"] = all(bytes(x) == bytes(y) for x, y in zip(o["A"], o["B"]))
                row["A_is_C"] = all(bytes(x) == bytes(y) for x, y in zip(o["A"], o["C"]))
                row["all_valid"] = bytes(o["A"][0]) == bytes(m) and bytes(o["A"][1]) == bytes(n)
                row["A_minus_C_ms"] = round(res["A"]["ms"] - res["C"]["ms"], 3)
                row["B_minus_A_ms"] = round(res["B"]["ms"] - res["A"]["ms"], 3)
            print(json.dumps(row), file=out, flush=True)
    if a.keyed:
        m = a.keyed
        keys = rng.integers(0, n_keys, m).astype(np.uint32)
        msgs = [hashlib.sha256(b"compressed/keyed/%d" % i).digest() for i in range(m)]
        sigs, st = eng.batch_sign(msgs, b"".join(sks[j].to_bytes(32, "big") for j in keys))
        assert st == bytes(m)
        enc = compress(sigs)
        blob = b"".join(msgs)
        moff = (ctypes.c_uint64 * (m + 1))(*[MSG_LEN * i for i in range(m + 1)])
        c_keys = (ctypes.c_uint32 * m)(*keys.tolist())
        o = {r: buf(m) for r in "ABC"}
        points, pre = buf(64 * m), buf(m)

        def keyed(items, flags, r):
            _check(lib.bn254_batch_verify_keyed(h, blob, moff, items, c_keys, m, flags, o[r]))

        def keyed_b():
            st_b, bad = decompress_and_filter(lib, h, enc, m, points, pre)
            keyed(points, 0, "B")
            merge_statuses(o["B"], m, st_b, bad)
        res = measure({"A": lambda: keyed(enc, FLAG, "A"), "B": keyed_b, "C": lambda: keyed(sigs, 0, "C")}, a.reps, only)
        row = {"kind": "compressed", "call": "bn254_batch_verify_keyed", "n": m, **res, "outputs_C_sha256": hashlib.sha256(bytes(o["C"])).hexdigest()[:16], **box}
        if only is None:
            row["A_is_B"], row["A_is_C"], row["all_valid"] = bytes(o["A"]) == bytes(o["B"]), bytes(o["A"]) == bytes(o["C"]), bytes(o["A"]) == bytes(m)
            row["A_minus_C_ms"] = round(res["A"]["ms"] - res["C"]["ms"], 3)
            row["B_minus_A_ms"] = round(res["B"]["ms"] - res["A"]["ms"], 3)
        print(json.dumps(row), file=out, flush=True)


if __name__ == "__main__":
    main()
