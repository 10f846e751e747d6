#!/usr/bin/env python3
"""Throughput of bn254_batch_verify_keyed_bitmap_randomized_device beside the exact bn254_batch_verify_keyed_bitmap_device, inputs resident in
HBM, every tuple valid.  Per shape n tuples x n_keys keys, a fraction `density` of the bits set at random, the variants
  exact (subset tables), rand128, rand_glv (BN254_FLAG_RAND_GLV), rand64 (BN254_FLAG_RAND64)
run in the same process on the same inputs, alternating: per round every variant runs one window (>= min_s of back-to-back calls after two
warm-up calls, timed to a synchronise).  Reported: the median, minimum and maximum window per variant, the ratio of the medians, whether the
SLOWEST randomised window beat the FASTEST exact one, the counters of bn254_debug_bitmap_rand_last (a passing batch re-checks nothing) and
the stage times of one profiled call (ms[0] sigma's decode + hash, ms[1] statuses + ladders, ms[2] sort, sums and fold, ms[3] group checks,
collect and re-check).  One JSON line per shape and group size.
    python tools/verify_keyed_bitmap_rand_throughput.py [out.jsonl] [--rounds R] [--min-s S] [--density D] [--groups G,G,..] [--trace-calls N] [shape ...]
shape = n:n_keys; --trace-calls N runs N rand128 calls per shape and nothing else (under rocprofv3 --kernel-trace --stats)."""
import argparse
import ctypes
import hashlib
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402  (first: one HIP runtime per process)
import bn254_amd  # noqa: E402
from bn254_amd import _native  # noqa: E402
from bn254_amd.engine import FLAG_RAND64, FLAG_RAND_GLV, OPT_BITMAP_RAND_GROUP_TUPLES, OPT_BITMAP_RAND_MAX_KEYS, OPT_BITMAP_RAND_MIN_TUPLES  # noqa: E402
from tests.datagen import sk_bytes  # noqa: E402
from tools.verify_keyed_bitmap_throughput import MSG_LEN, R, _check, dev, window  # noqa: E402

SHAPES = [(65536, 256), (65536, 1024), (1 << 20, 256), (16384, 256), (4096, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-s", type=float, default=0.3)
    ap.add_argument("--density", type=float, default=2 / 3)
    ap.add_argument("--groups", default="")
    ap.add_argument("--trace-calls", type=int, default=0, help="no windows: this many rand128 calls per shape and nothing else (for a kernel trace)")
    a = ap.parse_intermixed_args()
    out = open(a.out, "a") if a.out else sys.stdout
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes] or SHAPES
    eng = bn254_amd.Engine(0)
    lib, h = eng._lib, eng._h
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    box = {"device": torch.cuda.get_device_name(0), "lib_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16],
           "density": round(a.density, 4), "rounds": a.rounds, "min_s": a.min_s}
    rng = np.random.default_rng(20261017)
    seed = hashlib.sha256(b"bitmap/rand/tp").digest()
    eng.set_option(OPT_BITMAP_RAND_MIN_TUPLES, 0)
    eng.set_option(OPT_BITMAP_RAND_MAX_KEYS, 1 << 30)
    for n, n_keys in shapes:
        sks = [int.from_bytes(sk_bytes(7000 + j), "big") % R for j in range(n_keys)]
        pool, st = eng.batch_g2_mul(None, b"".join(s.to_bytes(32, "big") for s in sks), n_keys, reduce_scalar=True)
        assert st == bytes(n_keys) and eng.register_keys(pool) == bytes(n_keys)
        sel = rng.random((n, n_keys)) < a.density
        bm_words = (n_keys + 31) // 32
        padded = np.zeros((n, bm_words * 32), dtype=np.uint8)
        padded[:, :n_keys] = sel
        bits = np.packbits(padded, axis=1, bitorder="little").tobytes()
        # the sums of the selected secret keys, in 16-bit limbs through one integer matrix product (exact: < 2^34 per limb)
        limbs = np.array([[(s >> (16 * k)) & 0xFFFF for k in range(16)] for s in sks], dtype=np.int64)
        sk_sums = [sum(int(v) << (16 * k) for k, v in enumerate(row)) % R for row in sel.astype(np.int64) @ limbs]
        msgs = [hashlib.sha256(b"bitmap/tp/%d/%d/%d" % (n, n_keys, i)).digest() for i in range(n)]
        sigma, st = eng.batch_sign(msgs, b"".join((s or 1).to_bytes(32, "big") for s in sk_sums))
        assert st == bytes(n)
        sigma = b"".join(bytes(64) if s == 0 else sigma[64 * i:64 * i + 64] for i, s in enumerate(sk_sums))
        off = np.arange(n + 1, dtype=np.uint64) * MSG_LEN
        d_msgs, d_off, d_sig, d_bits, d_st = dev(b"".join(msgs)), dev(off.tobytes()), dev(sigma), dev(bits), dev(bytes(n))

        def exact():
            return lib.bn254_batch_verify_keyed_bitmap_device(h, d_msgs.data_ptr(), d_off.data_ptr(), d_sig.data_ptr(), d_bits.data_ptr(), bm_words, n, 0,
                                                              d_st.data_ptr(), stream)

        def rand(flags):
            return lambda: lib.bn254_batch_verify_keyed_bitmap_randomized_device(h, d_msgs.data_ptr(), d_off.data_ptr(), d_sig.data_ptr(), d_bits.data_ptr(),
                                                                                 bm_words, n, flags, seed, d_st.data_ptr(), stream)
        variants = [("exact", exact), ("rand128", rand(0)), ("rand_glv", rand(FLAG_RAND_GLV)), ("rand64", rand(FLAG_RAND64))]
        if a.trace_calls:
            for _ in range(a.trace_calls):
                _check(variants[1][1]())
            torch.cuda.synchronize()
            continue
        for G in [int(g) for g in a.groups.split(",") if g] or [None]:
            if G:
                eng.set_option(OPT_BITMAP_RAND_GROUP_TUPLES, G)
            ms = {name: [] for name, _ in variants}
            ok, last = True, {}
            for _ in range(a.rounds):
                for name, fn in variants:
                    d_st.fill_(0xEE)
                    ms[name].append(1e3 * window(lambda: _check(fn()), a.min_s))
                    ok = ok and bytes(d_st.cpu().numpy().tobytes()[:n]) == bytes(n)
                    if name != "exact":
                        last[name] = eng.debug_bitmap_rand_last()
            eng.set_profiling(True)
            _check(variants[1][1]())
            k = eng.last_kernel_ms()
            eng.set_profiling(False)
            med = {name: statistics.median(v) for name, v in ms.items()}
            row = {"shape": "%dx%d" % (n, n_keys), "n": n, "n_keys": n_keys, "group_tuples": G or "default",
                   **{"%s_ms" % name: [round(med[name], 3), round(min(v), 3), round(max(v), 3)] for name, v in ms.items()},
                   **{"exact_over_%s" % name: round(med["exact"] / med[name], 2) for name in ms if name != "exact"},
                   "rand128_faster_beyond_spread": max(ms["rand128"]) < min(ms["exact"]),
                   "rand128_stages_ms": {"decode_hash": round(k["decode"], 3), "status_ladders": round(k["hash_to_g1"], 3),
                                         "sort_sums_fold": round(k["miller_loop"], 3), "checks": round(k["final_exp"], 3)},
                   "last": last.get("rand128"), "all_valid": ok, **box}
            print(json.dumps(row), file=out, flush=True)
        del d_msgs, d_off, d_sig, d_bits, d_st


if __name__ == "__main__":
    main()
