#!/usr/bin/env python3
"""The proof-of-possession calls (include/bn254_hip.h: bn254_ctx_register_keys_pop, bn254_batch_pop_verify_device,
bn254_batch_pop_prove_device) against what a caller did without them, on the same build, every proof valid.
  register   per key count K (--keys, default 256 1024 4096), host pointers, whole synchronous calls under a host clock:
             (a) bn254_ctx_register_keys_pop;
             (b) bn254_ctx_register_keys, then bn254_batch_verify_keyed on the K host-composed proof messages TAG || pk_j, key_idx = j;
             (p) bn254_ctx_register_keys alone — the figure to hold against another build (BN254_LIB) of the plain call.
  bulk       at --items (default 65536), inputs resident in HBM, HIP events on the caller's stream around whole calls:
             (v) bn254_batch_pop_verify_device against bn254_batch_verify_device with the subgroup flag on messages composed beforehand;
             (s) bn254_batch_pop_prove_device against bn254_batch_g2_mul_device, then bn254_batch_sign_device on messages composed beforehand
                 (the caller's route also copies the keys to the host, composes there and copies back; that is not counted).
             The margin of each pair is the composer's cost (and the fold's, for prove).
All legs alternate, `--reps` calls each after two warm-up calls of every leg: the median, with the min and max beside it.  The status
bytes of (a) and (b), and of the two legs of (v) and (s), are compared.  A library without the calls (BN254_LIB = an older build, the
baseline of an A/B) runs leg (p) and the plain legs of (v) and (s).  One JSON line per measurement (default stdout).
    python tools/pop_throughput.py [out.jsonl] [--reps R] [--keys K ...] [--items N] [--note TEXT]"""
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
from bn254_amd.engine import FLAG_G2_SUBGROUP_CHECK, FLAG_REJECT_IDENTITY, POP_TAG  # noqa: E402
from tests.datagen import sk_bytes  # noqa: E402


def dev(data):
    t = torch.empty(max(len(data), 8), dtype=torch.uint8, device="cuda")
    if len(data):
        t[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def _check(rc):
    if rc != 0:
        raise RuntimeError("library call failed: %d" % rc)


def host_ms(fn):
    t0 = time.perf_counter()
    fn()                                             # synchronous: returns with the statuses on the host
    return (time.perf_counter() - t0) * 1e3


def event_ms(fn, ts):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ts)
    fn()
    e1.record(ts)
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(v):
    return {"ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}


def alternate(legs, reps, timer):
    """legs: {name: fn}; two warm-up rounds, then `reps` rounds of every leg in turn"""
    for _ in range(2):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            ms[name].append(timer(fn))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--keys", type=int, nargs="*", default=[256, 1024, 4096])
    ap.add_argument("--items", type=int, default=65536)
    ap.add_argument("--note", default=None, help="recorded with every line, e.g. which build ran")
    a = ap.parse_args()
    out = open(a.out, "a") if a.out else sys.stdout
    eng = bn254_amd.Engine(0)
    lib, h = eng._lib, eng._h
    have = hasattr(lib, "bn254_ctx_register_keys_pop")
    ts = torch.cuda.Stream()
    stream = ctypes.c_void_p(ts.cuda_stream)
    box = {"device": torch.cuda.get_device_name(0), "lib_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16], "reps": a.reps,
           "has_pop_calls": bool(have)}
    if a.note:
        box["note"] = a.note
    n_max = max(a.keys + [a.items])
    sks = b"".join(sk_bytes(30000 + j) for j in range(n_max))
    pks, st = eng.batch_g2_mul(None, sks, n_max, reduce_scalar=True)
    assert st == bytes(n_max)
    msgs = [POP_TAG + pks[128 * j:128 * j + 128] for j in range(n_max)]
    pops, st = eng.batch_sign(msgs, sks)
    assert st == bytes(n_max)
    blob = b"".join(msgs)

    # ---- register ----------------------------------------------------------------------------------------------------------------------
    for K in a.keys:
        k_pks, k_pops, k_blob = pks[:128 * K], pops[:64 * K], blob[:144 * K]
        off = (ctypes.c_uint64 * (K + 1))(*[144 * j for j in range(K + 1)])
        idx = (ctypes.c_uint32 * K)(*range(K))
        st_a, st_b, st_v = ctypes.create_string_buffer(K), ctypes.create_string_buffer(K), ctypes.create_string_buffer(K)

        def plain():
            _check(lib.bn254_ctx_register_keys(h, k_pks, K, FLAG_REJECT_IDENTITY, st_b))

        def by_hand():
            plain()
            _check(lib.bn254_batch_verify_keyed(h, k_blob, off, k_pops, idx, K, FLAG_REJECT_IDENTITY, st_v))

        def with_pop():
            _check(lib.bn254_ctx_register_keys_pop(h, k_pks, k_pops, K, FLAG_REJECT_IDENTITY, st_a))

        legs = {"p": plain, "b": by_hand}
        if have:
            legs["a"] = with_pop
        ms = alternate(legs, a.reps, host_ms)
        row = {"what": "register", "n_keys": K, "plain_register_keys": stats(ms["p"]), "b_register_then_verify_keyed": stats(ms["b"])}
        if have:
            row["a_register_keys_pop"] = stats(ms["a"])
            row["b_over_a"] = round(statistics.median(ms["b"]) / statistics.median(ms["a"]), 3)
            row["a_not_slower_beyond_spread"] = statistics.median(ms["a"]) <= max(ms["b"])
            row["same_status_bytes"] = st_a.raw == bytes(r if r else v for r, v in zip(st_b.raw, st_v.raw)) == bytes(K)
        print(json.dumps({**row, **box}), file=out, flush=True)

    # ---- bulk ----------------------------------------------------------------------------------------------------------------------------
    n = a.items
    d_sks, d_pks, d_pops, d_msgs = dev(sks[:32 * n]), dev(pks[:128 * n]), dev(pops[:64 * n]), dev(blob[:144 * n])
    d_off = dev((np.arange(n + 1, dtype=np.uint64) * 144).tobytes())
    d_st1, d_st2, d_st3 = dev(bytes(n)), dev(bytes(n)), dev(bytes(n))
    d_out_pks, d_out_pops, d_out_pks2, d_out_pops2 = dev(bytes(128 * n)), dev(bytes(64 * n)), dev(bytes(128 * n)), dev(bytes(64 * n))

    def verify():
        _check(lib.bn254_batch_verify_device(h, d_msgs.data_ptr(), d_off.data_ptr(), d_pops.data_ptr(), d_pks.data_ptr(), n,
                                             FLAG_G2_SUBGROUP_CHECK | FLAG_REJECT_IDENTITY, d_st1.data_ptr(), stream))

    def pop_verify():
        _check(lib.bn254_batch_pop_verify_device(h, d_pks.data_ptr(), d_pops.data_ptr(), n, FLAG_REJECT_IDENTITY, d_st2.data_ptr(), stream))

    def mul_sign():
        _check(lib.bn254_batch_g2_mul_device(h, None, d_sks.data_ptr(), n, 1, d_out_pks.data_ptr(), d_st1.data_ptr(), stream))
        _check(lib.bn254_batch_sign_device(h, d_msgs.data_ptr(), d_off.data_ptr(), d_sks.data_ptr(), n, d_out_pops.data_ptr(), d_st3.data_ptr(), stream))

    def pop_prove():
        _check(lib.bn254_batch_pop_prove_device(h, d_sks.data_ptr(), n, d_out_pks2.data_ptr(), d_out_pops2.data_ptr(), d_st2.data_ptr(), stream))

    for what, plain_fn, pop_fn, plain_name in (("pop_verify", verify, pop_verify, "batch_verify_device"), ("pop_prove", mul_sign, pop_prove, "g2_mul_device_then_sign_device")):
        legs = {"plain": plain_fn}
        if have:
            legs["pop"] = pop_fn
        ms = alternate(legs, a.reps, lambda fn: event_ms(fn, ts))
        row = {"what": what, "n": n, plain_name: stats(ms["plain"])}
        if have:
            row["pop_call"] = stats(ms["pop"])
            row["margin_ms"] = round(statistics.median(ms["pop"]) - statistics.median(ms["plain"]), 3)
            row["plain_spread_ms"] = round(max(ms["plain"]) - min(ms["plain"]), 3)
            torch.cuda.synchronize()
            if what == "pop_verify":
                row["same_status_bytes"] = bool(torch.equal(d_st1[:n], d_st2[:n])) and not bool(d_st2[:n].any())
            else:
                row["same_bytes"] = bool(torch.equal(d_out_pks[:128 * n], d_out_pks2[:128 * n]) and torch.equal(d_out_pops[:64 * n], d_out_pops2[:64 * n]) and
                                         torch.equal(d_out_pops2[:64 * n], d_pops[:64 * n])) and not bool(d_st2[:n].any())
        print(json.dumps({**row, **box}), file=out, flush=True)


if __name__ == "__main__":
    main()
