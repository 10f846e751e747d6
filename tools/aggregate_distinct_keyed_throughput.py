#!/usr/bin/env python3
"""Throughput of bn254_batch_aggregate_verify_distinct_keyed_device (n aggregates x k distinct messages each, keys registered) against the
unkeyed bn254_batch_aggregate_verify_distinct_device on the SAME inputs in the same process, alternating: per round every variant runs one
window, and the figures are the medians over the rounds.  Variants: keyed by size (the default route), the slot kernel forced to width 1 and
to width 2, the keys expanded into the unkeyed route (BN254_OPT_AGGD_KEYED_ROUTE 1 / 2 / 3), and the unkeyed call.  Reference line:
bn254_batch_verify_keyed_device on 65 536 tuples.  Inputs live on the device; a window is >= min_s of back-to-back calls after a warm-up,
timed to a synchronise.  One JSON line per shape to the file named first (default stdout).
    python tools/aggregate_distinct_keyed_throughput.py [out.jsonl] [--rounds R] [--min-s S] [--keys K] [shape ...]   shape = n:k"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process)
import bn254_amd  # noqa: E402
from bn254_amd import _native  # noqa: E402
from bn254_amd.engine import OPT_AGGD_KEYED_ROUTE, pack_messages  # noqa: E402
from tests.datagen import D, sk_bytes  # noqa: E402

SHAPES = [(65536, 1), (16384, 4), (4096, 16), (1024, 64), (64, 1024), (1, 64), (1, 65536), (1, 1 << 20),        # DESIGN.md §10's table
          (1, 1), (1, 16), (16, 1), (256, 1), (1024, 1), (1, 1536), (64, 16),                                  # the lane machine's row
          (1024, 2), (4096, 1), (1024, 4), (16384, 1), (32768, 1), (131072, 1), (262144, 1), (65536, 2)]      # around the width rule
VARIANTS = [("keyed", 0), ("keyed_w1", 1), ("keyed_w2", 2), ("keyed_expand", 3), ("unkeyed", None)]


def dev(data):
    t = torch.empty(max(len(data), 8), dtype=torch.uint8, device="cuda")
    if data:
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
    ap.add_argument("--keys", type=int, default=256)
    a = ap.parse_intermixed_args()
    out = open(a.out, "a") if a.out else sys.stdout
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes] or SHAPES
    eng = bn254_amd.Engine(0)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    K = a.keys
    sks = [sk_bytes(j) for j in range(K)]
    pool, st = eng.batch_g2_mul(None, b"".join(sks), K, reduce_scalar=True)
    assert st == bytes(K)
    assert eng.register_keys(pool) == bytes(K)
    lib, h = eng._lib, eng._h
    box = {"device": torch.cuda.get_device_name(0), "lib": os.path.basename(_native.LIB_PATH), "keys": K}

    # reference: the keyed verify on 65 536 tuples
    nv = 65536
    msgs = [D("aggdk/tp/verify", i) for i in range(nv)]
    sigs, st = eng.batch_sign(msgs, b"".join(sks[i % K] for i in range(nv)))
    blob, off = pack_messages(msgs)
    d = [dev(blob), dev(bytes(off)), dev(sigs), dev(b"".join((i % K).to_bytes(4, "little") for i in range(nv))), dev(bytes(nv))]
    t = window(lambda: lib.bn254_batch_verify_keyed_device(h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), nv, 0,
                                                           d[4].data_ptr(), stream), a.min_s)
    assert bytes(d[4].cpu().numpy().tobytes()[:nv]) == bytes(nv)
    print(json.dumps({"shape": "verify_keyed", "n": nv, "ms": round(1e3 * t, 3), "verifies_per_s": round(nv / t), **box}), file=out, flush=True)
    del d

    for n, k in shapes:
        m = n * k
        msgs = [D("aggdk/tp/%d/%d" % (n, k), j) for j in range(m)]
        sigs, st = eng.batch_sign(msgs, b"".join(sks[j % K] for j in range(m)))
        assert st == bytes(m)
        sigma, st = eng.batch_g1_sum(sigs, (ctypes.c_uint64 * (n + 1))(*[i * k for i in range(n + 1)]))
        blob, off = pack_messages(msgs)
        d_msgs, d_off, d_sig = dev(blob), dev(bytes(off)), dev(sigma)
        d_agg = dev(b"".join(int(v).to_bytes(8, "little") for v in range(0, m + 1, k)))
        d_idx = dev(b"".join((j % K).to_bytes(4, "little") for j in range(m)))
        d_pks = dev(b"".join(pool[128 * (j % K):128 * (j % K) + 128] for j in range(m)))
        d_st = dev(bytes(n))

        def run(route):
            if route is None:
                return lambda: lib.bn254_batch_aggregate_verify_distinct_device(h, d_msgs.data_ptr(), d_off.data_ptr(), d_pks.data_ptr(), m, d_sig.data_ptr(),
                                                                                d_agg.data_ptr(), n, 0, d_st.data_ptr(), stream)
            return lambda: lib.bn254_batch_aggregate_verify_distinct_keyed_device(h, d_msgs.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), m,
                                                                                  d_sig.data_ptr(), d_agg.data_ptr(), n, 0, d_st.data_ptr(), stream)
        ms = {name: [] for name, _ in VARIANTS}
        ok = {}
        for _ in range(a.rounds):
            for name, route in VARIANTS:
                eng.set_option(OPT_AGGD_KEYED_ROUTE, route or 0)
                d_st.fill_(0xEE)
                ms[name].append(1e3 * window(run(route), a.min_s))
                ok[name] = ok.get(name, True) and bytes(d_st.cpu().numpy().tobytes()[:n]) == bytes(n)
        eng.set_option(OPT_AGGD_KEYED_ROUTE, 0)
        med = {name: statistics.median(v) for name, v in ms.items()}
        row = {"shape": "%dx%d" % (n, k), "n": n, "k": k, "m": m, "rounds": a.rounds,
               **{name + "_ms": round(v, 3) for name, v in med.items()},
               "keyed_msgs_per_s": round(m / med["keyed"] * 1e3), "unkeyed_msgs_per_s": round(m / med["unkeyed"] * 1e3),
               "keyed_speedup": round(med["unkeyed"] / med["keyed"], 3), "all_valid": all(ok.values()), **box}
        print(json.dumps(row), file=out, flush=True)
        del d_msgs, d_off, d_sig, d_agg, d_idx, d_pks, d_st


if __name__ == "__main__":
    main()
