"""Verify throughput against the number of distinct public keys in the batch (bench.py has no key-pool switch): bn254_batch_verify_device on
n items over a pool of K keys (item i uses key i % K), with key deduplication on and off (BN254_OPT_KEY_DEDUP), one JSON line per point.
  python tools/key_pool_throughput.py [--n 65536] [--pools 64,256,1024,4096,65536] [--steps 6] [--warmup 2]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--pools", default="64,256,1024,4096,65536")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    import bn254_amd
    from bn254_amd import engine as E
    from tests.datagen import D, sk_bytes
    eng = bn254_amd.Engine(0)
    n = a.n
    eng.reserve(n)
    msgs = [D("kpool", i) for i in range(n)]
    dev = "cuda:0"
    d_msgs = torch.frombuffer(bytearray(b"".join(msgs)), dtype=torch.uint8).to(dev)
    d_off = torch.arange(0, 32 * (n + 1), 32, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    for pool in [min(int(p), n) for p in a.pools.split(",")]:
        sks = [sk_bytes(j) for j in range(pool)]
        pk, st = eng.batch_g2_mul(None, b"".join(sks), pool, reduce_scalar=True)
        assert st == bytes(pool)
        sigs, st = eng.batch_sign(msgs, b"".join(sks[i % pool] for i in range(n)))
        assert st == bytes(n)
        pks = b"".join(pk[128 * (i % pool):128 * (i % pool) + 128] for i in range(n))
        d_sigs = torch.frombuffer(bytearray(sigs), dtype=torch.uint8).to(dev)
        d_pks = torch.frombuffer(bytearray(pks), dtype=torch.uint8).to(dev)
        torch.cuda.synchronize()
        for dedup in (0, 1, 0, 1):
            eng.set_option(E.OPT_KEY_DEDUP, dedup)

            def step():
                eng.batch_verify_device(d_msgs.data_ptr(), d_off.data_ptr(), d_sigs.data_ptr(), d_pks.data_ptr(), n, d_st.data_ptr(), flags=0)
            for _ in range(a.warmup):
                step()
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            eng.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / a.steps
            eng.set_profiling(1)
            step()
            k = eng.last_kernel_ms()
            eng.set_profiling(0)
            ok = bytes(d_st.cpu().numpy()) == bytes(n)
            print(json.dumps({"n": n, "pool": pool, "key_dedup": dedup, "ms_per_step": round(ms, 3), "pairings_per_s": round(2 * n / ms * 1e3),
                              "kernel_ms": {s: round(v, 3) for s, v in k.items()} if isinstance(k, dict) else k, "all_valid": ok}), flush=True)
    eng.set_option(E.OPT_KEY_DEDUP, 1)


if __name__ == "__main__":
    main()
