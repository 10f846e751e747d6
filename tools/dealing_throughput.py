#!/usr/bin/env python3
"""bn254_batch_g2_msm and bn254_ctx_check_dealing against the routes without them.  One JSON line per measurement (default stdout; the
committed figures are profiles/dealing.jsonl).  Every figure is the median, with the min and max beside it, of `--reps` runs after two warm-up
runs, the legs of a comparison alternating in one process.
  g2_msm: 65 536 terms in 4 096 segments of 16, 65 536 terms in one segment, 171 terms in one segment —
    (m) bn254_batch_g2_msm, host form, wall clock (staging included);
    (p) the route without it: bn254_batch_g2_mul + bn254_batch_g2_sum, host forms, wall clock;
    (d) bn254_batch_g2_msm_device under HIP events on a caller's stream (its 8-byte copy home and wait included).
  check_dealing at n:t (default 256:171 1024:683 4096:2731), keys dealt from one polynomial of degree t - 1 and registered —
    (c) bn254_ctx_check_dealing, wall clock (the call is host-synchronous);
    (i) the Python-integer route: the same coefficients c_j and lambda_k on the host (factorial closed forms, Python integers), then
        bn254_batch_g2_mul and bn254_batch_g2_sum over the t + n products — `--reps-slow` runs;
    (x) the exact route, at the first shape only: L_k(x_j) for every j >= t in Python integers, (n - t) t products through
        bn254_batch_g2_mul, bn254_batch_g2_sum per j, each sum compared with pk_j — `--reps-slow` runs;
    and the stage split of ONE profiled call of (c) from bn254_ctx_last_kernel_ms: key scan + coefficients, terms, sums, verdict.
    python tools/dealing_throughput.py [out.jsonl] [--reps R] [--reps-slow R] [--skip-msm] [--note TEXT] [shape ...]   shape = n:t"""
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
SHAPES = [(256, 171), (1024, 683), (4096, 2731)]
MSM_SHAPES = [(65536, 16), (65536, 65536), (171, 171)]


def dev(data):
    t = torch.empty(max(len(data), 8), dtype=torch.uint8, device="cuda")
    if len(data):
        t[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def _check(rc):
    if rc != 0:
        raise RuntimeError("library call failed: %d" % rc)


def timed(fn, ts):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(ts)
    fn()
    e1.record(ts)
    e1.synchronize()
    return e0.elapsed_time(e1)


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return {"ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "runs": len(v)}


def be(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def rho(seed, j):
    return int.from_bytes(hashlib.sha256(seed + j.to_bytes(8, "little")).digest()[:16], "little") or 1


def host_coefficients(n, t, seed):
    """(lambda_0 .. lambda_t-1, c_0 .. c_n-1) in Python integers, by the closed forms the device uses"""
    fact = [1] * (n + 1)
    for m in range(1, n + 1):
        fact[m] = fact[m - 1] * m % R
    inv = [0] + [pow(m, -1, R) for m in range(1, n + 1)]
    w = [rho(seed, j) * fact[j] % R * pow(fact[j - t], -1, R) % R for j in range(t, n)]
    lam, cs = [], []
    for k in range(t):
        e = pow(fact[k] * fact[t - 1 - k] % R, -1, R)
        lam.append((-1) ** k * fact[t] * inv[k + 1] * e % R)
        s = sum(wj * inv[j - k] for j, wj in zip(range(t, n), w)) % R
        cs.append(-(-1) ** (t - 1 - k) * s * e % R)
    return lam, cs + [rho(seed, j) for j in range(t, n)]


def msm_rows(eng, lib, h, ts, stream, box, reps, out):
    rng = np.random.default_rng(7)
    for m, seg_len in MSM_SHAPES:
        pts, st = eng.batch_g2_mul(None, rng.bytes(32 * m), m, reduce_scalar=True)
        assert st == bytes(m)
        scalars = rng.bytes(32 * m)
        d_pts, d_k = dev(pts), dev(scalars)
        n = m // seg_len
        seg = (ctypes.c_uint64 * (n + 1))(*[i * seg_len for i in range(n + 1)])
        d_seg, d_out, d_st = dev(bytes(seg)), dev(bytes(128 * n)), dev(bytes(n))
        o1, s1, prod, ps = (ctypes.create_string_buffer(x) for x in (128 * n, n, 128 * m, m))
        o2, s2 = ctypes.create_string_buffer(128 * n), ctypes.create_string_buffer(n)

        def msm_host():
            _check(lib.bn254_batch_g2_msm(h, pts, scalars, seg, n, 1, o1, s1))

        def mul_sum_host():
            _check(lib.bn254_batch_g2_mul(h, pts, scalars, m, 1, prod, ps))
            _check(lib.bn254_batch_g2_sum(h, prod, seg, n, o2, s2))

        def msm_device():
            _check(lib.bn254_batch_g2_msm_device(h, d_pts.data_ptr(), d_k.data_ptr(), d_seg.data_ptr(), n, 1, d_out.data_ptr(), d_st.data_ptr(), stream))
        for fn in (msm_host, mul_sum_host, msm_device, msm_host, mul_sum_host, msm_device):
            fn()
        torch.cuda.synchronize()
        same = o1.raw == o2.raw and s1.raw == s2.raw and d_out.cpu().numpy().tobytes()[:128 * n] == o1.raw
        t = {"msm": [], "mul_sum": [], "msm_device": []}
        for _ in range(reps):
            t["msm"].append(wall(msm_host))
            t["mul_sum"].append(wall(mul_sum_host))
            t["msm_device"].append(timed(msm_device, ts))
        row = {"kind": "g2_msm", "terms": m, "segment": seg_len, "segments": n, "msm_host": spread(t["msm"]), "mul_then_sum_host": spread(t["mul_sum"]),
               "msm_device": spread(t["msm_device"]), "same_bytes": bool(same), **box}
        print(json.dumps(row), file=out, flush=True)
        del d_pts, d_k, d_seg, d_out, d_st


def dealing_rows(eng, lib, h, box, shapes, reps, reps_slow, out):
    seed = hashlib.sha256(b"dealing throughput").digest()
    for at, (n, t) in enumerate(shapes):
        coeffs = [int.from_bytes(sk_bytes(8000 + e), "big") % R for e in range(t)]
        sks = []
        for x in range(1, n + 1):                        # Horner
            v = 0
            for c in reversed(coeffs):
                v = (v * x + c) % R
            sks.append(v)
        pool, st = eng.batch_g2_mul(None, be(sks), n, reduce_scalar=True)
        assert st == bytes(n) and eng.register_keys(pool) == bytes(n)
        keys = [pool[128 * j:128 * j + 128] for j in range(n)]
        pk, cst, bad = ctypes.create_string_buffer(128), ctypes.create_string_buffer(1), ctypes.c_uint32(0)
        res = {}

        def check():
            _check(lib.bn254_ctx_check_dealing(h, t, seed, 0, pk, cst, ctypes.byref(bad)))

        def by_integers():
            lam, cs = host_coefficients(n, t, seed)
            pts = b"".join(keys[:t]) + pool
            prod, st = eng.batch_g2_mul(pts, be(lam + cs), t + n)
            res["int"] = eng.batch_g2_sum(prod, [0, t, t + n])

        def exact():
            xs = list(range(1, t + 1))
            d_inv = []
            for k in range(t):
                d = 1
                for i in range(t):
                    if i != k:
                        d = d * (xs[k] - xs[i]) % R
                d_inv.append(pow(d, -1, R))
            ks, seg = [], [0]
            for j in range(t, n):
                big_n = 1
                for i in range(t):
                    big_n = big_n * (j + 1 - xs[i]) % R
                ks += [big_n * pow(j + 1 - xs[k], -1, R) % R * d_inv[k] % R for k in range(t)]
                seg.append(len(ks))
            prod, st = eng.batch_g2_mul(b"".join(keys[:t]) * (n - t), be(ks), len(ks))
            sums, st = eng.batch_g2_sum(prod, seg)
            res["exact_ok"] = sums == pool[128 * t:]
        for _ in range(2):
            check()
        by_integers()
        gk, st = eng.batch_g2_mul(None, be([coeffs[0]]), 1, reduce_scalar=True)
        same = cst.raw == b"\0" and pk.raw == gk and res["int"][0] == gk + bytes(128) and res["int"][1] == bytes(2)
        ms = {"check": [], "int": [], "exact": []}
        for r in range(reps):
            ms["check"].append(wall(check))
            if r < reps_slow:
                ms["int"].append(wall(by_integers))
        if at == 0:
            exact()
            for _ in range(reps_slow):
                ms["exact"].append(wall(exact))
        eng.set_profiling(True)
        check()
        kms = list(eng.last_kernel_ms().values())
        eng.set_profiling(False)
        row = {"kind": "check_dealing", "n": n, "threshold": t, "check_dealing": spread(ms["check"]), "python_integer_route": spread(ms["int"]),
               "stages_ms": [round(v, 3) for v in kms], "stage_slots": "key scan + coefficients, terms, sums, verdict", "status": cst.raw[0],
               "same_group_key_and_verdict": bool(same), **box}
        if ms["exact"]:
            row["exact_route"] = spread(ms["exact"])
            row["exact_route_agrees"] = bool(res["exact_ok"])
        print(json.dumps(row), file=out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reps-slow", type=int, default=7)
    ap.add_argument("--skip-msm", action="store_true")
    ap.add_argument("--note", default=None, help="recorded with every line, e.g. which build ran")
    a = ap.parse_intermixed_args()
    out = open(a.out, "a") if a.out else sys.stdout
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes] or SHAPES
    eng = bn254_amd.Engine(0)
    lib, h = eng._lib, eng._h
    ts = torch.cuda.Stream()
    stream = ctypes.c_void_p(ts.cuda_stream)
    box = {"device": torch.cuda.get_device_name(0), "lib_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16], "reps": a.reps}
    if a.note:
        box["note"] = a.note
    if not a.skip_msm:
        msm_rows(eng, lib, h, ts, stream, box, a.reps, out)
    dealing_rows(eng, lib, h, box, shapes, a.reps, a.reps_slow, out)


if __name__ == "__main__":
    main()
