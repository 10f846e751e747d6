"""The key cache of the verify's key dedup (BN254_OPT_KEY_CACHE) at its two extremes, which bench.py cannot show (its keys never change):
bn254_batch_verify_device on n items over K keys per call, with
  --mode warm    the same keys on every call (a service with a stable key set: from the second call on nothing is built)
  --mode fresh   keys no earlier call left in the cache: the calls rotate over --pools disjoint key pools, more keys than the cache has
                 rows, so every call misses all its keys (the cold path: what a call pays for looking them up in vain)
  --mode off     BN254_OPT_KEY_CACHE = 0: every call builds all its keys
  --mode parent  no option set: for a library loaded through BN254_LIB that has no key cache
One JSON line: ms per step, pairings/s and what the last call found and built.
  python tools/key_cache_throughput.py --mode fresh [--n 65536] [--keys 256] [--pools 8] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="warm", choices=["warm", "fresh", "off", "parent"])
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--keys", type=int, default=256)
    ap.add_argument("--pools", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    import torch
    import bn254_amd
    from bn254_amd import engine as E
    from tests.datagen import D, sk_bytes
    eng = bn254_amd.Engine(0)
    n, K = a.n, a.keys
    rotate = a.mode in ("fresh", "parent", "off")
    pools = a.pools if rotate else 1
    eng.reserve(n)
    msgs = [D("kcache", i) for i in range(n)]
    dev = "cuda:0"
    d_msgs = torch.frombuffer(bytearray(b"".join(msgs)), dtype=torch.uint8).to(dev)
    d_off = torch.arange(0, 32 * (n + 1), 32, dtype=torch.int64, device=dev)
    d_st = torch.zeros(n, dtype=torch.uint8, device=dev)
    batches = []
    for p in range(pools):
        sks = [sk_bytes(20000 + p * K + j) for j in range(K)]
        pk, st = eng.batch_g2_mul(None, b"".join(sks), K, reduce_scalar=True)
        assert st == bytes(K)
        sigs, st = eng.batch_sign(msgs, b"".join(sks[i % K] for i in range(n)))
        assert st == bytes(n)
        pks = b"".join(pk[128 * (i % K):128 * (i % K) + 128] for i in range(n))
        batches.append((torch.frombuffer(bytearray(sigs), dtype=torch.uint8).to(dev), torch.frombuffer(bytearray(pks), dtype=torch.uint8).to(dev)))
    torch.cuda.synchronize()
    if a.mode != "parent":
        eng.set_option(E.OPT_KEY_CACHE, 0 if a.mode == "off" else 1)
    calls = [0]

    def step():
        d_sigs, d_pks = batches[calls[0] % pools]
        calls[0] += 1
        eng.batch_verify_device(d_msgs.data_ptr(), d_off.data_ptr(), d_sigs.data_ptr(), d_pks.data_ptr(), n, d_st.data_ptr(), flags=0)
    for _ in range(a.warmup):
        step()
    eng.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        step()
    eng.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / a.steps
    ok = bytes(d_st.cpu().numpy()) == bytes(n)
    last = eng.debug_key_cache_last() if hasattr(eng._lib, "bn254_debug_key_cache_last") else None
    print(json.dumps({"mode": a.mode, "n": n, "keys": K, "pools": pools, "ms_per_step": round(ms, 4), "pairings_per_s": round(2 * n / ms * 1e3),
                      "last_call": last, "route": eng.debug_key_dedup_last(), "all_valid": ok}), flush=True)


if __name__ == "__main__":
    main()
