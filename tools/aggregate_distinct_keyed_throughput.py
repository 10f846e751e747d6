#!/usr/bin/env python3
"""Throughput of bn254_batch_aggregate_verify_distinct_keyed_device (n aggregates x k distinct messages each, keys registered) against the
unkeyed bn254_batch_aggregate_verify_distinct_device on the SAME inputs in the same process, alternating: per round every variant runs one
window, and the figures are the medians over the rounds.  Variants: keyed by size (the default route), the slot kernel forced to width 1 and
to width 2, the keys expanded into the unkeyed route (BN254_OPT_AGGD_KEYED_ROUTE 1 / 2 / 3), the unkeyed call, and the randomised keyed
call (bn254_batch_aggregate_verify_distinct_keyed_randomized_device, forced with BN254_OPT_AGG_RAND_MIN_PAIRS = 0) with 128-bit, GLV and 64-bit
scalars.  --variants picks a subset; --group-pairs sets BN254_OPT_AGG_RAND_GROUP_PAIRS.  Reference line:
bn254_batch_verify_keyed_device on 65 536 tuples.  Inputs live on the device; a window is >= min_s of back-to-back calls after a warm-up,
timed to a synchronise.  One JSON line per shape to the file named first (default stdout).
    python tools/aggregate_distinct_keyed_throughput.py [out.jsonl] [--rounds R] [--min-s S] [--keys K] [--variants a,b] [--group-pairs G]
                                                        [shape ...]   shape = n:k"""
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
from bn254_amd.engine import (FLAG_RAND64, FLAG_RAND_GLV, OPT_AGG_RAND_GROUP_PAIRS, OPT_AGG_RAND_MIN_PAIRS, OPT_AGGD_KEYED_ROUTE,  # noqa: E402
                              pack_messages)
from tests.datagen import D, sk_bytes  # noqa: E402

SHAPES = [(65536, 1), (16384, 4), (4096, 16), (1024, 64), (64, 1024), (1, 64), (1, 65536), (1, 1 << 20),        # DESIGN.md §10's table
          (1, 1), (1, 16), (16, 1), (256, 1), (1024, 1), (1, 1536), (64, 16),                                  # the lane machine's row
          (1024, 2), (4096, 1), (1024, 4), (16384, 1), (32768, 1), (131072, 1), (262144, 1), (65536, 2)]      # around the width rule
VARIANTS = [("keyed", 0), ("keyed_w1", 1), ("keyed_w2", 2), ("keyed_expand", 3), ("unkeyed", None),
            ("rand128", ("rand", 0)), ("rand_glv", ("rand", FLAG_RAND_GLV)), ("rand64", ("rand", FLAG_RAND64))]
SEED = bytes(range(32))


def ws_default(name):
    """the library's default `#define <name> <integer>` in bn254_amd/csrc/bn254_ws.h"""
    import re
    text = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "bn254_ws.h")).read()
    return int(re.search(r"#define\s+%s\s+(\d+)" % name, text).group(1))


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
    ap.add_argument("--variants", default=",".join(v for v, _ in VARIANTS))
    ap.add_argument("--group-pairs", type=int, default=0)
    a = ap.parse_intermixed_args()
    variants = [(v, r) for v, r in VARIANTS if v in a.variants.split(",")]
    assert variants and variants[0][0] == "keyed", "the keyed call (by size) comes first: every speedup is against it or the unkeyed one"
    out = open(a.out, "a") if a.out else sys.stdout
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes] or SHAPES
    eng = bn254_amd.Engine(0)
    eng.set_option(OPT_AGG_RAND_MIN_PAIRS, 0)
    group_pairs = a.group_pairs or ws_default("AGG_RAND_GROUP_PAIRS_DEFAULT")      # set explicitly: the profile rows name what ran
    eng.set_option(OPT_AGG_RAND_GROUP_PAIRS, group_pairs)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    K = a.keys
    sks = [sk_bytes(j) for j in range(K)]
    pool, st = eng.batch_g2_mul(None, b"".join(sks), K, reduce_scalar=True)
    assert st == bytes(K)
    assert eng.register_keys(pool) == bytes(K)
    lib, h = eng._lib, eng._h
    box = {"device": torch.cuda.get_device_name(0), "lib": os.path.basename(_native.LIB_PATH), "keys": K, "group_pairs": group_pairs}

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
            if isinstance(route, tuple):
                return lambda: lib.bn254_batch_aggregate_verify_distinct_keyed_randomized_device(
                    h, d_msgs.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), m, d_sig.data_ptr(), d_agg.data_ptr(), n, route[1], SEED, d_st.data_ptr(),
                    stream)
            if route is None:
                return lambda: lib.bn254_batch_aggregate_verify_distinct_device(h, d_msgs.data_ptr(), d_off.data_ptr(), d_pks.data_ptr(), m, d_sig.data_ptr(),
                                                                                d_agg.data_ptr(), n, 0, d_st.data_ptr(), stream)
            return lambda: lib.bn254_batch_aggregate_verify_distinct_keyed_device(h, d_msgs.data_ptr(), d_off.data_ptr(), d_idx.data_ptr(), m,
                                                                                  d_sig.data_ptr(), d_agg.data_ptr(), n, 0, d_st.data_ptr(), stream)
        ms = {name: [] for name, _ in variants}
        ok = {}
        for _ in range(a.rounds):
            for name, route in variants:
                eng.set_option(OPT_AGGD_KEYED_ROUTE, route if isinstance(route, int) else 0)
                d_st.fill_(0xEE)
                ms[name].append(1e3 * window(run(route), a.min_s))
                ok[name] = ok.get(name, True) and bytes(d_st.cpu().numpy().tobytes()[:n]) == bytes(n)
        eng.set_option(OPT_AGGD_KEYED_ROUTE, 0)
        med = {name: statistics.median(v) for name, v in ms.items()}
        row = {"shape": "%dx%d" % (n, k), "n": n, "k": k, "m": m, "rounds": a.rounds,
               **{name + "_ms": round(v, 3) for name, v in med.items()},
               **{name + "_msgs_per_s": round(m / v * 1e3) for name, v in med.items()},
               **({"keyed_speedup": round(med["unkeyed"] / med["keyed"], 3)} if "unkeyed" in med else {}),
               **{name + "_vs_keyed": round(med["keyed"] / v, 3) for name, v in med.items() if name.startswith("rand")},
               "all_valid": all(ok.values()), **box}
        print(json.dumps(row), file=out, flush=True)
        del d_msgs, d_off, d_sig, d_agg, d_idx, d_pks, d_st


if __name__ == "__main__":
    main()
