#!/usr/bin/env python3
"""What the signer-bitmap calls return besides a status byte (bn254_batch_verify_keyed_bitmap_export, bn254_batch_aggregate_keys_bitmap,
bn254_batch_bitmap_weights) against the routes that existed, per shape (tuples:keys) that many registered keys, two thirds of them
signing every tuple, every aggregate valid.  Whole HOST-POINTER calls under a host clock (time.perf_counter around the call: staging, kernels, copies home and the
wait) and the `_device` forms under events on the caller's stream.  Per shape the routes alternate, `--reps` runs each after two warm-up
runs — the median with the min and max beside it:
  export  (A) bn254_batch_verify_keyed_bitmap_export: statuses, H(m) and the aggregate keys from one call;
          (B) the route that exists: bn254_batch_verify_keyed_bitmap, plus bn254_batch_hash_to_g1, plus the host gather of the set keys'
              128-byte encodings per tuple, plus bn254_batch_g2_sum over them.  Its interval contains its host work: that is the route;
          (C) the plain bn254_batch_verify_keyed_bitmap: the floor.  A - C = two small kernels and 192 B per tuple coming home.
  keys    (A) bn254_batch_aggregate_keys_bitmap; (B) the host gather plus bn254_batch_g2_sum.
  weights (A) bn254_batch_bitmap_weights; (B) the host bit walk in numpy (unpacked bits times the weight vector, in uint64).
Every line says whether A's outputs are B's bytes, and carries a digest of A's outputs taken on each of the four routes of the sum (subset
tables or key by key, lane pairs on and off): they must be equal.  The bitmaps of a shape are drawn from 64 distinct rows (tuple i takes
row i % 64), so that the signers' secret keys are summed 64 times, not n times; the calls do the same work per tuple either way.
--verify-only measures the plain bitmap verify alone and records a digest of its statuses: run once per build (BN254_LIB names another
build of the library), alternating, to compare a build with its parent — same digests, times within each other's spread.
    python tools/bitmap_out_throughput.py [out.jsonl] [--reps R] [--note TEXT] [--verify-only] [shape ...]   shape = tuples:keys"""
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
from bn254_amd import engine as E  # noqa: E402
from tests.datagen import D, sk_bytes  # noqa: E402

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SHAPES = [(65536, 256), (256, 256), (256, 4096)]
PATTERNS = 64
ROUTES = {"tables_pair": {E.OPT_BITMAP_ROUTE: 1, E.OPT_PAIR_LANES: 1}, "keys_pair": {E.OPT_BITMAP_ROUTE: 2, E.OPT_PAIR_LANES: 1},
          "tables_lane": {E.OPT_BITMAP_ROUTE: 1, E.OPT_PAIR_LANES: 0}, "keys_lane": {E.OPT_BITMAP_ROUTE: 2, E.OPT_PAIR_LANES: 0}}


def _check(rc):
    if rc != 0:
        raise RuntimeError("library call failed: %d" % rc)


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return {"ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def measure(routes, reps, clock=wall):
    """routes: name -> callable; two warm-up runs each, then `reps` rounds in which the routes alternate"""
    times = {k: [] for k in routes}
    for _ in range(2):
        for fn in routes.values():
            fn()
    for _ in range(reps):
        for k, fn in routes.items():
            times[k].append(clock(fn))
    return {k: spread(v) for k, v in times.items()}


def event_ms(fn):
    """one _device call between two events on the current stream"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def build_shape(eng, n, n_keys, seed):
    """keys registered; n messages, their valid aggregates and bitmaps (two thirds of the keys set)"""
    rng = np.random.default_rng(seed)
    sks = [int.from_bytes(sk_bytes(7000 + j), "big") % R for j in range(n_keys)]
    pks, st = eng.batch_g2_mul(None, b"".join(s.to_bytes(32, "big") for s in sks), n_keys, reduce_scalar=True)
    assert st == bytes(n_keys) and eng.register_keys(pks) == bytes(n_keys)
    bm_words = (n_keys + 31) // 32
    pat_bits = rng.random((PATTERNS, bm_words * 32)) < 2 / 3
    pat_bits[:, n_keys:] = False
    pat_sk = [sum(sks[j] for j in np.nonzero(row)[0]) % R or 1 for row in pat_bits]
    pat_words = np.packbits(pat_bits, axis=1, bitorder="little").view("<u4")
    which = np.arange(n) % PATTERNS
    bits = np.ascontiguousarray(pat_words[which])
    msgs = [D("bitmap_out/%d" % seed, i) for i in range(n)]
    sigs, st = eng.batch_sign(msgs, b"".join(pat_sk[w].to_bytes(32, "big") for w in which))
    assert st == bytes(n)
    blob, off = E.pack_messages(msgs)
    weights = rng.integers(1, 1 << 40, size=n_keys, dtype=np.uint64)
    return {"pks": np.frombuffer(pks, dtype=np.uint8).reshape(n_keys, 128), "bits": bits, "bm_words": bm_words,
            "msgs": np.frombuffer(blob, dtype=np.uint8).copy(), "off": np.frombuffer(bytes(off), dtype=np.uint64).copy(),
            "sigs": np.frombuffer(sigs, dtype=np.uint8).copy(), "weights": weights, "signers": float(pat_bits.sum(axis=1).mean())}


def gather(S, n_keys):
    """the host's route to an aggregate key: per tuple the encodings of its set keys, in ascending order, and the segment offsets"""
    unpacked = np.unpackbits(S["bits"].view(np.uint8), axis=1, bitorder="little")[:, :n_keys]
    rows, cols = np.nonzero(unpacked)
    seg = np.zeros(len(unpacked) + 1, dtype=np.uint64)
    np.cumsum(unpacked.sum(axis=1, dtype=np.uint64), out=seg[1:])
    return np.ascontiguousarray(S["pks"][cols]), seg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default="profiles/bitmap_out.jsonl")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--note", default="")
    ap.add_argument("--verify-only", action="store_true")
    ap.add_argument("shapes", nargs="*")
    args = ap.parse_intermixed_args()
    shapes = [tuple(int(x) for x in s.split(":")) for s in args.shapes] or SHAPES
    eng = bn254_amd.Engine(0)
    lib, h = eng._lib, eng._h
    base = {"device": torch.cuda.get_device_name(0), "lib_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16],
            "reps": args.reps, "signing": "two thirds"}
    if args.note:
        base["note"] = args.note
    caller = torch.cuda.Stream()                          # the _device forms run here, and so do the events around them
    stream = ctypes.c_void_p(caller.cuda_stream)
    with open(args.out, "a") as out:
        for n, n_keys in shapes:
            S = build_shape(eng, n, n_keys, seed=n_keys + n)
            bmw = S["bm_words"]
            status, status_b = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            hashes, hashes_b = np.zeros(n * 64, np.uint8), np.zeros(n * 64, np.uint8)
            keys, keys_b = np.zeros(n * 128, np.uint8), np.zeros(n * 128, np.uint8)
            hash_st, sum_st = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
            line = dict(base, shape="%dx%d" % (n, n_keys), n=n, n_keys=n_keys, signers_per_tuple=round(S["signers"], 1))

            def verify(st):
                _check(lib.bn254_batch_verify_keyed_bitmap(h, ptr(S["msgs"]), ptr(S["off"]), ptr(S["sigs"]), ptr(S["bits"]), bmw, n, 0, ptr(st)))

            if args.verify_only:
                t = measure({"C": lambda: verify(status)}, args.reps)
                assert not status.any()
                out.write(json.dumps(dict(line, kind="bitmap_verify_only", call="bn254_batch_verify_keyed_bitmap", clock="host, whole host-pointer calls",
                                          statuses_sha256=digest(status), **t)) + "\n")
                out.flush()
                continue

            def export():
                _check(lib.bn254_batch_verify_keyed_bitmap_export(h, ptr(S["msgs"]), ptr(S["off"]), ptr(S["sigs"]), ptr(S["bits"]), bmw, n, 0, ptr(status),
                                                                  ptr(hashes), ptr(keys)))

            def sum_by_gather(dst):
                pts, seg = gather(S, n_keys)
                _check(lib.bn254_batch_g2_sum(h, ptr(pts), ptr(seg), n, ptr(dst), ptr(sum_st)))

            def export_b():
                verify(status_b)
                _check(lib.bn254_batch_hash_to_g1(h, ptr(S["msgs"]), ptr(S["off"]), n, ptr(hashes_b), ptr(hash_st), None))
                sum_by_gather(keys_b)

            # the export call: A, B, C under the host clock
            t = measure({"A": export, "B": export_b, "C": lambda: verify(status_b)}, args.reps)
            same = bool((status == status_b).all() and (hashes == hashes_b).all() and (keys == keys_b).all())
            assert not status.any() and not hash_st.any() and not sum_st.any()
            per_route = {}
            for name, opts in ROUTES.items():
                for k, v in opts.items():
                    eng.set_option(k, v)
                export()
                per_route[name] = digest(status, hashes, keys)
            eng.set_option(E.OPT_BITMAP_ROUTE, 0)
            eng.set_option(E.OPT_PAIR_LANES, 1)
            export()
            out.write(json.dumps(dict(line, kind="bitmap_export", call="bn254_batch_verify_keyed_bitmap_export", clock="host, whole host-pointer calls",
                                      A_is_B=same, outputs_sha256=digest(status, hashes, keys), outputs_sha256_by_route=per_route,
                                      digests_equal_across_routes=len(set(per_route.values())) == 1 and per_route["tables_pair"] == digest(status, hashes, keys),
                                      A_minus_C_ms=round(t["A"]["ms"] - t["C"]["ms"], 3), B_minus_A_ms=round(t["B"]["ms"] - t["A"]["ms"], 3), **t)) + "\n")
            # the keys alone
            keys_a = np.zeros(n * 128, np.uint8)

            def keys_call():
                _check(lib.bn254_batch_aggregate_keys_bitmap(h, ptr(S["bits"]), bmw, n, 0, ptr(keys_a), ptr(status)))
            t = measure({"A": keys_call, "B": lambda: sum_by_gather(keys_b)}, args.reps)
            out.write(json.dumps(dict(line, kind="bitmap_keys", call="bn254_batch_aggregate_keys_bitmap", clock="host, whole host-pointer calls",
                                      A_is_B=bool((keys_a == keys_b).all() and not status.any()), outputs_sha256=digest(keys_a),
                                      B_minus_A_ms=round(t["B"]["ms"] - t["A"]["ms"], 3), **t)) + "\n")
            # the weights
            _check(lib.bn254_ctx_set_key_weights(h, ptr(S["weights"]), n_keys))
            weight, walked = np.zeros(n, np.uint64), [None]

            def weights_call():
                _check(lib.bn254_batch_bitmap_weights(h, ptr(S["bits"]), bmw, n, ptr(weight), ptr(status)))

            def bit_walk():
                unpacked = np.unpackbits(S["bits"].view(np.uint8), axis=1, bitorder="little")[:, :n_keys]
                walked[0] = unpacked.astype(np.uint64) @ S["weights"]
            t = measure({"A": weights_call, "B": bit_walk}, args.reps)
            out.write(json.dumps(dict(line, kind="bitmap_weights", call="bn254_batch_bitmap_weights", clock="host, whole host-pointer calls",
                                      A_is_B=bool((weight == walked[0]).all() and not status.any()), outputs_sha256=digest(weight),
                                      B_minus_A_ms=round(t["B"]["ms"] - t["A"]["ms"], 3), **t)) + "\n")
            # the _device forms under events, inputs resident, on the caller's stream
            dev = {k: torch.from_numpy(S[k].view(np.uint8).reshape(-1).copy()).cuda() for k in ("msgs", "off", "sigs", "bits")}
            d_st, d_h, d_k, d_w = (torch.empty(sz, dtype=torch.uint8, device="cuda") for sz in (n, 64 * n, 128 * n, 8 * n))
            p = {k: ctypes.c_void_p(v.data_ptr()) for k, v in dev.items()}
            st_p, h_p, k_p, w_p = (ctypes.c_void_p(x.data_ptr()) for x in (d_st, d_h, d_k, d_w))
            torch.cuda.synchronize()
            with torch.cuda.stream(caller):
              t = measure({
                "export": lambda: _check(lib.bn254_batch_verify_keyed_bitmap_export_device(h, p["msgs"], p["off"], p["sigs"], p["bits"], bmw, n, 0, st_p, h_p, k_p, stream)),
                "verify": lambda: _check(lib.bn254_batch_verify_keyed_bitmap_device(h, p["msgs"], p["off"], p["sigs"], p["bits"], bmw, n, 0, st_p, stream)),
                "keys": lambda: _check(lib.bn254_batch_aggregate_keys_bitmap_device(h, p["bits"], bmw, n, 0, k_p, st_p, stream)),
                "weights": lambda: _check(lib.bn254_batch_bitmap_weights_device(h, p["bits"], bmw, n, w_p, st_p, stream)),
              }, args.reps, clock=event_ms)
            torch.cuda.synchronize()
            same = bool((d_k.cpu().numpy() == keys_a).all() and (d_w.cpu().numpy().view(np.uint64) == weight).all())
            out.write(json.dumps(dict(line, kind="bitmap_out_device", clock="events on the caller's stream, _device forms, inputs resident",
                                      device_outputs_are_host_outputs=same, export_minus_verify_ms=round(t["export"]["ms"] - t["verify"]["ms"], 3), **t)) + "\n")
            out.flush()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
