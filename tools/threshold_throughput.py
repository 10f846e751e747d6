#!/usr/bin/env python3
"""bn254_batch_threshold_combine_keyed_device against the calls beside it, inputs resident in HBM, 256 registered keys, every share valid.
Per shape n tuples x k shares (the signers of a tuple: k distinct keys drawn at random; a tuple with more shares than keys repeats them),
threshold t = two thirds of the tuple's distinct keys:
  (t) the new call;
  (a) bn254_batch_collect_keyed_bitmap_device on the same inputs — the same verification work, so (t) - (a) is the interpolation;
  (b) the route without the call: bn254_batch_verify_keyed_device on the tuple's message repeated once per share, the statuses to the host,
      the t lowest valid keys per tuple and their Lagrange coefficients in Python integers, bn254_batch_g1_mul and bn254_batch_g1_sum (host
      pointers) over the chosen shares.  Its interval contains its host work — that is the route.
Timed with HIP events on the caller's stream around whole calls, alternating, `--reps` calls each after two warm-up calls ((b): `--reps-b`):
the median, with the min and max beside it.  Per-stage times of one profiled call of (t) and of (a) from bn254_ctx_last_kernel_ms (ms[0]
decode + hash + spread, ms[1] select-and-sum — for (t) with rank-and-select, coefficients, terms and sums inside —, ms[2] Miller loop, ms[3]
final exponentiation) — ONE call per leg, not a median, so `interpolation_ms_by_stage` rests on a single sample each; `interpolation_ms`, from
the whole-call medians, is the figure to quote.  The keys are independent (no dealing): the work is the same, the outputs are compared with route (b)'s bytes.
--msm adds bn254_batch_g1_msm against bn254_batch_g1_mul + bn254_batch_g1_sum (host forms, wall clock, staging included on both sides) and
the _device form (events) at `--msm-terms` terms in segments of 16 and in one segment.  One JSON line per shape (default stdout).
--optimistic measures bn254_batch_threshold_combine_keyed_optimistic_device against the exact call instead, alternating in one process: the
keys are DEALT (per shape one polynomial of degree t - 1 over the K keys, key j = f(j + 1) * G2) and the true group key f(0) * G2 is set, the
optimistic route forced (option 46 = 0) so that what is measured is the route and not the default's choice.  --fail chooses what goes wrong:
none; tuple (every share of the lowest keys of ONE tuple replaced by another point of the curve); percent (1 % of the shares, drawn at
random); key (the group key of another polynomial: every tuple goes the exact way — the cost of a misconfiguration).  The line carries both
calls' medians with min and max, what the route did (bn254_debug_threshold_opt_last), whether the three outputs of identity A agree with the
exact call's, and the four stage times of ONE profiled optimistic call (front end + candidate rows, coefficients + weighted sum, the tuples'
Miller loop + final exponentiation, exact fallback + re-interpolation).
    python tools/threshold_throughput.py [out.jsonl] [--reps R] [--reps-b R] [--msm] [--msm-terms M] [--keys K] [--note TEXT]
                                         [--optimistic [--fail none|tuple|percent|key]] [shape ...]   shape = n:k"""
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
SHAPES = [(256, 171), (4096, 11), (1, 4096)]
MSG_LEN = 32
STAGES = ("decode", "hash_to_g1", "miller_loop", "final_exp")


def dev(data):
    t = torch.empty(max(len(data), 8), dtype=torch.uint8, device="cuda")
    if len(data):
        t[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def _check(rc):
    if rc != 0:
        raise RuntimeError("library call failed: %d" % rc)


def timed(fn, ts):
    """ms between two HIP events on the stream the calls are enqueued on"""
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


def lagrange_at_zero(xs):
    out = []
    for j, xj in enumerate(xs):
        num = den = 1
        for k, xk in enumerate(xs):
            if k != j:
                num, den = num * xk % R, den * (xk - xj) % R
        out.append(num * pow(den, -1, R) % R)
    return out


def spread(v):
    return {"ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "mean_ms": round(statistics.mean(v), 3)}


def msm_rows(eng, lib, h, ts, stream, box, m, reps, out):
    rng = np.random.default_rng(7)
    pts, st = eng.batch_g1_mul(None, rng.bytes(32 * m), m, reduce_scalar=True)
    assert st == bytes(m)
    scalars = rng.bytes(32 * m)
    d_pts, d_k = dev(pts), dev(scalars)
    for seg_len in (16, m):
        n = m // seg_len
        seg = (ctypes.c_uint64 * (n + 1))(*[i * seg_len for i in range(n + 1)])
        d_seg, d_out, d_st = dev(bytes(seg)), dev(bytes(64 * n)), dev(bytes(n))
        o1, s1, prod, ps = (ctypes.create_string_buffer(x) for x in (64 * n, n, 64 * m, m))
        o2, s2 = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)

        def msm_host():
            _check(lib.bn254_batch_g1_msm(h, pts, scalars, seg, n, 1, o1, s1))

        def mul_sum_host():
            _check(lib.bn254_batch_g1_mul(h, pts, scalars, m, 1, prod, ps))
            _check(lib.bn254_batch_g1_sum(h, prod, seg, n, o2, s2))

        def msm_device():
            _check(lib.bn254_batch_g1_msm_device(h, d_pts.data_ptr(), d_k.data_ptr(), d_seg.data_ptr(), n, 1, d_out.data_ptr(), d_st.data_ptr(), stream))
        for fn in (msm_host, mul_sum_host, msm_device, msm_host, mul_sum_host, msm_device):
            fn()
        torch.cuda.synchronize()
        same = o1.raw == o2.raw and s1.raw == s2.raw and d_out.cpu().numpy().tobytes()[:64 * n] == o1.raw
        t = {"msm": [], "mul_sum": [], "msm_device": []}
        for _ in range(reps):
            t["msm"].append(wall(msm_host))
            t["mul_sum"].append(wall(mul_sum_host))
            t["msm_device"].append(timed(msm_device, ts))
        row = {"kind": "g1_msm", "terms": m, "segment": seg_len, "segments": n, "msm_host": spread(t["msm"]), "mul_then_sum_host": spread(t["mul_sum"]),
               "msm_device": spread(t["msm_device"]), "same_bytes": bool(same), **box}
        print(json.dumps(row), file=out, flush=True)


OPT_THRESHOLD_OPT_MIN_SHARES = 46


def optimistic_rows(eng, lib, h, ts, stream, box, shapes, n_keys, reps, fail, out):
    """--optimistic: one line per shape, the optimistic call against the exact call on dealt keys under the true (or, --fail key, a wrong) group key"""
    rng = np.random.default_rng(20261020)
    bm_words = (n_keys + 31) // 32
    g1, st = eng.batch_g1_mul(None, (1).to_bytes(32, "big"), 1)
    for n, k in shapes:
        n_shares = n * k
        t = max(1, 2 * min(k, n_keys) // 3)
        coeffs = [int.from_bytes(sk_bytes(7000 + e), "big") % R for e in range(t)]
        sks = [sum(c * pow(x, e, R) for e, c in enumerate(coeffs)) % R or 1 for x in range(1, n_keys + 1)]
        pool, st = eng.batch_g2_mul(None, b"".join(s.to_bytes(32, "big") for s in sks), n_keys, reduce_scalar=True)
        assert st == bytes(n_keys) and eng.register_keys(pool) == bytes(n_keys)
        f0 = coeffs[0] if fail != "key" else (coeffs[0] + 1) % R
        gk, st = eng.batch_g2_mul(None, f0.to_bytes(32, "big"), 1, reduce_scalar=True)
        st_gk = ctypes.create_string_buffer(1)
        _check(lib.bn254_ctx_set_group_key(h, gk, 0, st_gk))
        assert st_gk.raw == b"\0"
        keys = np.concatenate([np.resize(rng.permutation(n_keys), k) for _ in range(n)]).astype(np.uint32)
        msgs = [hashlib.sha256(b"threshold/opt/%d/%d/%d" % (n, k, i)).digest() for i in range(n)]
        shares, st = eng.batch_sign([msgs[s // k] for s in range(n_shares)], b"".join(sks[j].to_bytes(32, "big") for j in keys))
        assert st == bytes(n_shares)
        bad = []
        if fail == "tuple":                              # one tuple, the share of its lowest key: the interpolation takes it, the check fails
            i = n // 2
            bad = [i * k + int(np.argmin(keys[i * k:(i + 1) * k]))]
        elif fail == "percent":
            bad = sorted(int(s) for s in rng.choice(n_shares, max(1, n_shares // 100), replace=False))
        if bad:
            buf = bytearray(shares)
            wrong, st = eng.batch_g1_add(b"".join(shares[64 * s:64 * s + 64] for s in bad), g1 * len(bad), len(bad))
            assert st == bytes(len(bad))
            for q, s in enumerate(bad):
                buf[64 * s:64 * s + 64] = wrong[64 * q:64 * q + 64]
            shares = bytes(buf)
        d_msgs, d_moff = dev(b"".join(msgs)), dev((np.arange(n + 1, dtype=np.uint64) * MSG_LEN).tobytes())
        d_shares, d_keys, d_soff = dev(shares), dev(keys.tobytes()), dev((np.arange(n + 1, dtype=np.uint64) * k).tobytes())
        outs = {name: [dev(bytes(x)) for x in (n_shares, n, 64 * n, 4 * bm_words * n, 4 * n)] for name in ("opt", "exact")}

        def call(fn, o):
            _check(fn(h, d_msgs.data_ptr(), d_moff.data_ptr(), d_shares.data_ptr(), d_keys.data_ptr(), d_soff.data_ptr(), n_shares, n, bm_words, t, 0,
                      o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), o[3].data_ptr(), o[4].data_ptr(), stream))

        def optimistic():
            call(lib.bn254_batch_threshold_combine_keyed_optimistic_device, outs["opt"])

        def exact():
            call(lib.bn254_batch_threshold_combine_keyed_device, outs["exact"])
        eng.set_option(OPT_THRESHOLD_OPT_MIN_SHARES, 0)
        for fn in (optimistic, exact, optimistic, exact):
            fn()
        optimistic()
        torch.cuda.synchronize()
        did = (ctypes.c_uint64 * 4)()
        _check(lib.bn254_debug_threshold_opt_last(h, did))
        host = {name: [x.cpu().numpy().tobytes() for x in o] for name, o in outs.items()}
        same_a = all(host["opt"][q][:size] == host["exact"][q][:size] for q, size in ((1, n), (2, 64 * n), (3, 4 * bm_words * n)))
        same_all = same_a and host["opt"][0][:n_shares] == host["exact"][0][:n_shares] and host["opt"][4][:4 * n] == host["exact"][4][:4 * n]
        ms = {"opt": [], "exact": []}
        for _ in range(reps):
            ms["opt"].append(timed(optimistic, ts))
            ms["exact"].append(timed(exact, ts))
        eng.set_profiling(True)
        optimistic()
        kms = eng.last_kernel_ms()
        eng.set_profiling(False)
        row = {"kind": "threshold_optimistic", "shape": "%dx%d" % (n, k), "n": n, "shares_per_tuple": k, "n_shares": n_shares, "threshold": t, "fail": fail,
               "bad_shares": len(bad), "optimistic_call": spread(ms["opt"]), "exact_call": spread(ms["exact"]),
               "hook": dict(zip(("checked", "passed", "exact_tuples", "exact_shares"), (int(x) for x in did))),
               "stages_ms": [round(kms[x], 3) for x in STAGES],
               "stage_slots": "front end + candidate rows, coefficients + weighted sum, tuple check (miller + final exp), exact fallback + re-interpolation",
               "statuses_signatures_rows_as_exact": bool(same_a), "all_five_outputs_as_exact": bool(same_all), **box}
        print(json.dumps(row), file=out, flush=True)
        del d_msgs, d_moff, d_shares, d_keys, d_soff, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--reps-b", type=int, default=3)
    ap.add_argument("--msm", action="store_true")
    ap.add_argument("--msm-terms", type=int, default=65536)
    ap.add_argument("--keys", type=int, default=256)
    ap.add_argument("--note", default=None, help="recorded with every line, e.g. which build ran")
    ap.add_argument("--optimistic", action="store_true", help="the optimistic threshold call against the exact one, on dealt keys")
    ap.add_argument("--fail", default="none", choices=("none", "tuple", "percent", "key"))
    a = ap.parse_intermixed_args()
    out = open(a.out, "a") if a.out else sys.stdout
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes] or SHAPES
    N_KEYS = a.keys
    eng = bn254_amd.Engine(0)
    lib, h = eng._lib, eng._h
    ts = torch.cuda.Stream()                        # a stream of the caller's own: a null handle would send the calls to the context's stream
    stream = ctypes.c_void_p(ts.cuda_stream)
    box = {"device": torch.cuda.get_device_name(0), "lib_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16],
           "n_keys": N_KEYS, "reps": a.reps}
    if a.note:
        box["note"] = a.note
    if a.optimistic:
        optimistic_rows(eng, lib, h, ts, stream, box, shapes, N_KEYS, a.reps, a.fail, out)
        return
    rng = np.random.default_rng(20261020)
    sks = [int.from_bytes(sk_bytes(9000 + j), "big") % R for j in range(N_KEYS)]
    pool, st = eng.batch_g2_mul(None, b"".join(s.to_bytes(32, "big") for s in sks), N_KEYS, reduce_scalar=True)
    assert st == bytes(N_KEYS) and eng.register_keys(pool) == bytes(N_KEYS)
    bm_words = (N_KEYS + 31) // 32

    for n, k in shapes:
        n_shares = n * k
        t = max(1, 2 * min(k, N_KEYS) // 3)
        keys = np.concatenate([np.resize(rng.permutation(N_KEYS), k) for _ in range(n)]).astype(np.uint32)
        msgs = [hashlib.sha256(b"threshold/tp/%d/%d/%d" % (n, k, i)).digest() for i in range(n)]
        rep = [msgs[s // k] for s in range(n_shares)]
        shares, st = eng.batch_sign(rep, b"".join(sks[j].to_bytes(32, "big") for j in keys))
        assert st == bytes(n_shares)
        share_off = np.arange(n + 1, dtype=np.uint64) * k
        d_msgs, d_moff = dev(b"".join(msgs)), dev((np.arange(n + 1, dtype=np.uint64) * MSG_LEN).tobytes())
        d_rep, d_roff = dev(b"".join(rep)), dev((np.arange(n_shares + 1, dtype=np.uint64) * MSG_LEN).tobytes())
        d_shares, d_keys, d_soff = dev(shares), dev(keys.tobytes()), dev(share_off.tobytes())
        d_sst, d_tst, d_sig, d_bits, d_cnt = dev(bytes(n_shares)), dev(bytes(n)), dev(bytes(64 * n)), dev(bytes(4 * bm_words * n)), dev(bytes(4 * n))
        d_agg, d_kst = dev(bytes(64 * n)), dev(bytes(n_shares))
        b_out = {}

        def threshold():
            _check(lib.bn254_batch_threshold_combine_keyed_device(h, d_msgs.data_ptr(), d_moff.data_ptr(), d_shares.data_ptr(), d_keys.data_ptr(),
                                                                  d_soff.data_ptr(), n_shares, n, bm_words, t, 0, d_sst.data_ptr(), d_tst.data_ptr(),
                                                                  d_sig.data_ptr(), d_bits.data_ptr(), d_cnt.data_ptr(), stream))

        def collect():
            _check(lib.bn254_batch_collect_keyed_bitmap_device(h, d_msgs.data_ptr(), d_moff.data_ptr(), d_shares.data_ptr(), d_keys.data_ptr(),
                                                               d_soff.data_ptr(), n_shares, n, bm_words, 0, d_sst.data_ptr(), d_tst.data_ptr(),
                                                               d_agg.data_ptr(), d_bits.data_ptr(), d_cnt.data_ptr(), stream))

        def keyed():
            _check(lib.bn254_batch_verify_keyed_device(h, d_rep.data_ptr(), d_roff.data_ptr(), d_shares.data_ptr(), d_keys.data_ptr(), n_shares, 0,
                                                       d_kst.data_ptr(), stream))

        def without_the_call():
            keyed()
            with torch.cuda.stream(ts):
                status = d_kst[:n_shares].cpu().numpy()
            pts, ks, seg = [], [], [0]
            for i in range(n):
                first = {}
                for s in range(i * k, (i + 1) * k):
                    if status[s] == 0:
                        first.setdefault(int(keys[s]), s)
                kept = sorted(first)[:t]
                if len(kept) == t:
                    pts += [shares[64 * first[j]:64 * first[j] + 64] for j in kept]
                    ks += lagrange_at_zero([j + 1 for j in kept])
                seg.append(len(ks))
            m = len(ks)
            prod, ps = ctypes.create_string_buffer(max(64 * m, 1)), ctypes.create_string_buffer(max(m, 1))
            o, s_ = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
            _check(lib.bn254_batch_g1_mul(h, b"".join(pts), b"".join(x.to_bytes(32, "big") for x in ks), m, 0, prod, ps))
            _check(lib.bn254_batch_g1_sum(h, prod, (ctypes.c_uint64 * (n + 1))(*seg), n, o, s_))
            b_out["sigs"] = o.raw

        for fn in (threshold, collect, threshold, collect):
            fn()
        without_the_call()
        threshold()
        torch.cuda.synchronize()
        same = d_sig.cpu().numpy().tobytes()[:64 * n] == b_out["sigs"] and not d_tst[:n].cpu().numpy().any()
        ms = {"t": [], "a": [], "b": [], "keyed": []}
        for _ in range(a.reps):
            ms["t"].append(timed(threshold, ts))
            ms["a"].append(timed(collect, ts))
            ms["keyed"].append(timed(keyed, ts))
        for _ in range(a.reps_b):
            ms["b"].append(timed(without_the_call, ts))
        stages = {}
        for name, fn in (("threshold", threshold), ("collect", collect)):
            eng.set_profiling(True)
            fn()
            kms = eng.last_kernel_ms()
            eng.set_profiling(False)
            stages[name] = [round(kms[x], 3) for x in STAGES]
        row = {"kind": "threshold", "shape": "%dx%d" % (n, k), "n": n, "shares_per_tuple": k, "n_shares": n_shares, "threshold": t,
               "threshold_call": spread(ms["t"]), "collect_call": spread(ms["a"]), "route_without_the_call": spread(ms["b"]), "reps_b": a.reps_b,
               "keyed_verify_alone": spread(ms["keyed"]),
               "interpolation_ms": round(statistics.median(ms["t"]) - statistics.median(ms["a"]), 3),
               "interpolation_ms_by_stage": round(stages["threshold"][1] - stages["collect"][1], 3),
               "stages_ms": stages, "stage_slots": "decode+hash+spread, select-and-sum (+ interpolation), miller, final_exp",
               "same_signatures_as_the_route": bool(same), **box}
        print(json.dumps(row), file=out, flush=True)
        del d_msgs, d_moff, d_rep, d_roff, d_shares, d_keys, d_soff, d_sst, d_tst, d_sig, d_bits, d_cnt, d_agg, d_kst
    if a.msm:
        msm_rows(eng, lib, h, ts, stream, box, a.msm_terms, a.reps, out)


if __name__ == "__main__":
    main()
