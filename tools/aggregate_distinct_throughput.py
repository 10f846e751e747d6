#!/usr/bin/env python3
"""Throughput of bn254_batch_aggregate_verify_distinct_device (n aggregates x k distinct messages each) against bn254_batch_verify_device on
65 536 tuples in the same process, and, for one aggregate, against the composition a caller could build before: hash_to_g1 of the k
messages + pairing_check(k + 1) on the device.  Inputs live on the device; every figure is a window of >= 1 s of back-to-back calls after a
warm-up, timed to a synchronise.  One JSON line per shape to the file named on the command line (default stdout).
    python tools/aggregate_distinct_throughput.py [out.jsonl] [shape ...]      shape = n:k, e.g. 65536:1"""
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime per process)
import bn254_amd  # noqa: E402
from bn254_amd import _native  # noqa: E402
from bn254_amd.engine import pack_messages  # noqa: E402
from tests.datagen import D, sk_bytes  # noqa: E402

SHAPES = [(65536, 1), (16384, 4), (4096, 16), (1024, 64), (64, 1024), (1, 64), (1, 65536), (1, 1 << 20)]
COMPOSE = {(1, 64), (1, 65536)}
POOL = 256


def dev(data):
    t = torch.empty(max(len(data), 8), dtype=torch.uint8, device="cuda")
    if data:
        t[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def u64(vals):
    return b"".join(int(v).to_bytes(8, "little") for v in vals)


def window(fn, min_s=1.0):
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
                return dt / calls, calls


def main():
    out = open(sys.argv[1], "a") if len(sys.argv) > 1 else sys.stdout
    shapes = [tuple(int(x) for x in s.split(":")) for s in sys.argv[2:]] or SHAPES
    eng = bn254_amd.Engine(0)
    stream = torch.cuda.current_stream().cuda_stream
    sks = [sk_bytes(j) for j in range(POOL)]
    pool, st = eng.batch_g2_mul(None, b"".join(sks), POOL, reduce_scalar=True)
    assert st == bytes(POOL)
    pks_of = lambda m: b"".join(pool[128 * (j % POOL):128 * (j % POOL) + 128] for j in range(m))   # noqa: E731
    lib, h = eng._lib, eng._h
    box = {"device": torch.cuda.get_device_name(0), "lib": os.path.basename(_native.LIB_PATH)}

    # baseline: bn254_batch_verify on 65 536 tuples
    nv = 65536
    msgs = [D("aggd/tp/verify", i) for i in range(nv)]
    sigs, st = eng.batch_sign(msgs, b"".join(sks[i % POOL] for i in range(nv)))
    blob, off = pack_messages(msgs)
    d = [dev(blob), dev(bytes(off)), dev(sigs), dev(pks_of(nv)), dev(bytes(nv))]
    t, calls = window(lambda: lib.bn254_batch_verify_device(h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), nv, 0,
                                                            d[4].data_ptr(), ctypes.c_void_p(stream)))
    assert bytes(d[4].cpu().numpy().tobytes()[:nv]) == bytes(nv)
    verify_per_s = nv / t
    print(json.dumps({"shape": "verify", "n": nv, "ms": round(1e3 * t, 3), "verifies_per_s": round(verify_per_s), "calls": calls, **box}), file=out, flush=True)
    del d

    for n, k in shapes:
        m = n * k
        msgs = [D("aggd/tp/%d/%d" % (n, k), j) for j in range(m)]
        sigs, st = eng.batch_sign(msgs, b"".join(sks[j % POOL] for j in range(m)))
        assert st == bytes(m)
        seg = (ctypes.c_uint64 * (n + 1))(*[i * k for i in range(n + 1)])
        sigma, st = eng.batch_g1_sum(sigs, seg)
        blob, off = pack_messages(msgs)
        pks = pks_of(m)
        d = [dev(blob), dev(bytes(off)), dev(pks), dev(sigma), dev(u64(range(0, m + 1, k))), dev(bytes(n))]
        call = lambda: lib.bn254_batch_aggregate_verify_distinct_device(   # noqa: E731
            h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), m, d[3].data_ptr(), d[4].data_ptr(), n, 0, d[5].data_ptr(), ctypes.c_void_p(stream))
        t, calls = window(call)
        ok = bytes(d[5].cpu().numpy().tobytes()[:n]) == bytes(n)
        row = {"shape": "%dx%d" % (n, k), "n": n, "k": k, "m": m, "ms": round(1e3 * t, 3), "msgs_per_s": round(m / t),
               "vs_verify": round(m / t / verify_per_s, 2), "all_valid": ok, "calls": calls, **box}
        if (n, k) in COMPOSE:
            # the composition: H(m_j) on the device into the first k points of the G1 array, sigma behind them; keys + (-G2) as the G2 array
            neg_g2 = bytes(bn254_amd.api._neg_g2_one())
            g1 = dev(bytes(64 * k) + sigma)
            g2 = dev(pks + neg_g2)
            hst, pst = dev(bytes(k)), dev(bytes(8))

            def compose():
                lib.bn254_batch_hash_to_g1_device(h, d[0].data_ptr(), d[1].data_ptr(), k, g1.data_ptr(), hst.data_ptr(), None, ctypes.c_void_p(stream))
                lib.bn254_batch_pairing_device(h, g1.data_ptr(), g2.data_ptr(), 1, k + 1, 0, None, pst.data_ptr(), ctypes.c_void_p(stream))
            tc, cc = window(compose)
            row.update({"compose_ms": round(1e3 * tc, 3), "compose_ok": pst.cpu().numpy().tobytes()[0] == 0, "speedup_vs_compose": round(tc / t, 2)})
        print(json.dumps(row), file=out, flush=True)
        del d


if __name__ == "__main__":
    main()
