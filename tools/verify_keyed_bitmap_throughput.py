#!/usr/bin/env python3
"""Throughput of bn254_batch_verify_keyed_bitmap_device (one message, one aggregated signature and a signer bitmap per tuple, keys registered)
with the inputs resident in HBM.  Per shape n tuples x n_keys keys, a fraction `density` of the bits set at random:
  (a) the call with the subset tables of the registered set          (BN254_OPT_BITMAP_ROUTE 1)
  (b) the call summing key by key                                    (BN254_OPT_BITMAP_ROUTE 2)
  (c) bn254_batch_aggregate_verify_distinct_keyed_device with the message repeated once per set bit — the way to the same status bytes
      without this call.  Its workspace grows with the number of pairs: above --max-pairs it runs on the first c_n tuples only and
      c_ms is scaled to n tuples (c_scaled = true says so; the full-size figure is then an extrapolation, not a measurement)
  (d) the floor: bn254_batch_verify_device alone on the pre-summed keys
All variants run in the same process on the same inputs, alternating: per round every variant runs one window (>= min_s of back-to-back
calls after two warm-up calls, timed to a synchronise); the figures are the medians over the rounds, with the min and max beside them
for (a) and (c).  a_faster_than_c_beyond_spread = the slowest window of (a) beat the fastest window of (c).  Per-stage times of one
profiled call of (a) and (b): bn254_ctx_last_kernel_ms — for this call ms[0] = sigma's decode + hash-to-G1, ms[1] = the summation kernel,
ms[2] Miller loop, ms[3] final exponentiation.  One JSON line per shape (default stdout), with the library's SHA-256.
    python tools/verify_keyed_bitmap_throughput.py [out.jsonl] [--rounds R] [--min-s S] [--density D] [--max-pairs M] [shape ...]   shape = n:n_keys"""
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
from bn254_amd.engine import OPT_BITMAP_ROUTE  # noqa: E402
from tests.datagen import sk_bytes  # noqa: E402

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SHAPES = [(65536, 256), (65536, 1024), (4096, 1024), (1, 256)]
MSG_LEN = 32


def dev(data):
    t = torch.empty(max(len(data), 8), dtype=torch.uint8, device="cuda")
    if len(data):
        t[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def window(fn, min_s):
    torch.cuda.synchronize()
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    calls, t0 = 0, time.perf_counter()
    while True:
        fn()
        calls += 1
        if calls % 4 == 0 or calls == 1:
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= min_s:
                return dt / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-s", type=float, default=0.4)
    ap.add_argument("--density", type=float, default=2 / 3)
    ap.add_argument("--max-pairs", type=int, default=12 << 20)
    a = ap.parse_intermixed_args()
    out = open(a.out, "a") if a.out else sys.stdout
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes] or SHAPES
    eng = bn254_amd.Engine(0)
    lib, h = eng._lib, eng._h
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    box = {"device": torch.cuda.get_device_name(0), "lib_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16],
           "density": round(a.density, 4), "rounds": a.rounds, "min_s": a.min_s}
    rng = np.random.default_rng(20261017)

    for n, n_keys in shapes:
        sks = [int.from_bytes(sk_bytes(7000 + j), "big") % R for j in range(n_keys)]
        pool, st = eng.batch_g2_mul(None, b"".join(s.to_bytes(32, "big") for s in sks), n_keys, reduce_scalar=True)
        assert st == bytes(n_keys)
        assert eng.register_keys(pool) == bytes(n_keys)
        sel = rng.random((n, n_keys)) < a.density
        pops = sel.sum(axis=1)
        bm_words = (n_keys + 31) // 32
        padded = np.zeros((n, bm_words * 32), dtype=np.uint8)
        padded[:, :n_keys] = sel
        bits = np.packbits(padded, axis=1, bitorder="little").tobytes()            # bit j % 32 of little-endian word j / 32
        sk_sums = [sum(sks[j] for j in np.nonzero(row)[0]) % R for row in sel]
        msgs = [hashlib.sha256(b"bitmap/tp/%d/%d/%d" % (n, n_keys, i)).digest() for i in range(n)]
        sk_blob = b"".join((s or 1).to_bytes(32, "big") for s in sk_sums)
        sigma, st = eng.batch_sign(msgs, sk_blob)
        assert st == bytes(n)
        apk, st = eng.batch_g2_mul(None, sk_blob, n, reduce_scalar=True)             # the pre-summed keys of the floor: (sum sk) G2 = sum pk
        assert st == bytes(n)
        # an empty bitmap (or keys that cancel): the identity signature under the identity key, all-zero bytes both
        sigma = b"".join(bytes(64) if s == 0 else sigma[64 * i:64 * i + 64] for i, s in enumerate(sk_sums))
        apk = b"".join(bytes(128) if s == 0 else apk[128 * i:128 * i + 128] for i, s in enumerate(sk_sums))
        off = np.arange(n + 1, dtype=np.uint64) * MSG_LEN
        d_msgs, d_off, d_sig, d_bits, d_apk = dev(b"".join(msgs)), dev(off.tobytes()), dev(sigma), dev(bits), dev(apk)
        d_st = dev(bytes(n))
        # (c): the first c_n tuples with the message repeated once per set bit
        c_n = n
        while c_n > 1 and int(pops[:c_n].sum()) > a.max_pairs:
            c_n //= 2
        m = int(pops[:c_n].sum())
        d_cmsgs = dev(b"".join(msgs[i] * int(pops[i]) for i in range(c_n)))
        d_coff = dev((np.arange(m + 1, dtype=np.uint64) * MSG_LEN).tobytes())
        d_cidx = dev(np.nonzero(sel[:c_n])[1].astype(np.uint32).tobytes())
        d_cagg = dev(np.concatenate([[0], np.cumsum(pops[:c_n])]).astype(np.uint64).tobytes())
        d_cst = dev(bytes(c_n))

        def bitmap():
            return lib.bn254_batch_verify_keyed_bitmap_device(h, d_msgs.data_ptr(), d_off.data_ptr(), d_sig.data_ptr(), d_bits.data_ptr(), bm_words, n, 0,
                                                              d_st.data_ptr(), stream)

        def distinct():
            return lib.bn254_batch_aggregate_verify_distinct_keyed_device(h, d_cmsgs.data_ptr(), d_coff.data_ptr(), d_cidx.data_ptr(), m, d_sig.data_ptr(),
                                                                          d_cagg.data_ptr(), c_n, 0, d_cst.data_ptr(), stream)

        def floor():
            return lib.bn254_batch_verify_device(h, d_msgs.data_ptr(), d_off.data_ptr(), d_sig.data_ptr(), d_apk.data_ptr(), n, 0, d_st.data_ptr(), stream)
        variants = [("a_tables", bitmap, 1, d_st, n), ("b_keys", bitmap, 2, d_st, n), ("c_distinct_keyed", distinct, 0, d_cst, c_n), ("d_verify_floor", floor, 0, d_st, n)]
        ms = {name: [] for name, *_ in variants}
        ok, stages = {}, {}
        for _ in range(a.rounds):
            for name, fn, route, d_out, cnt in variants:
                eng.set_option(OPT_BITMAP_ROUTE, route)
                d_out.fill_(0xEE)
                ms[name].append(1e3 * window(lambda: _check(fn()), a.min_s))
                ok[name] = ok.get(name, True) and bytes(d_out.cpu().numpy().tobytes()[:cnt]) == bytes(cnt)
        for name, fn, route, d_out, cnt in variants[:2]:
            eng.set_option(OPT_BITMAP_ROUTE, route)
            eng.set_profiling(True)
            _check(fn())
            k = eng.last_kernel_ms()
            eng.set_profiling(False)
            stages[name] = {"decode_hash_ms": round(k["decode"], 3), "summation_ms": round(k["hash_to_g1"], 3), "miller_ms": round(k["miller_loop"], 3),
                            "final_exp_ms": round(k["final_exp"], 3)}
        eng.set_option(OPT_BITMAP_ROUTE, 0)
        med = {name: statistics.median(v) for name, v in ms.items()}
        scale = n / c_n
        c_ms = [v * scale for v in ms["c_distinct_keyed"]]
        row = {"shape": "%dx%d" % (n, n_keys), "n": n, "n_keys": n_keys, "bm_words": bm_words, "mean_popcount": round(float(pops.mean()), 1),
               "a_ms": round(med["a_tables"], 3), "a_min_ms": round(min(ms["a_tables"]), 3), "a_max_ms": round(max(ms["a_tables"]), 3),
               "b_ms": round(med["b_keys"], 3),
               "c_ms": round(statistics.median(c_ms), 3), "c_min_ms": round(min(c_ms), 3), "c_max_ms": round(max(c_ms), 3),
               "c_tuples_measured": c_n, "c_pairs_measured": m, "c_scaled": c_n != n,
               "d_ms": round(med["d_verify_floor"], 3),
               "a_tuples_per_s": round(n / med["a_tables"] * 1e3), "a_over_floor": round(med["a_tables"] / med["d_verify_floor"], 3),
               "c_over_a": round(statistics.median(c_ms) / med["a_tables"], 2),
               "a_faster_than_c_beyond_spread": max(ms["a_tables"]) < min(c_ms),
               "stages": stages, "all_valid": all(ok.values()), **box}
        print(json.dumps(row), file=out, flush=True)
        del d_msgs, d_off, d_sig, d_bits, d_apk, d_st, d_cmsgs, d_coff, d_cidx, d_cagg, d_cst


def _check(rc):
    if rc != 0:
        raise RuntimeError("library call failed: %d" % rc)


if __name__ == "__main__":
    main()
