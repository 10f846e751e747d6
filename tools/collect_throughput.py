#!/usr/bin/env python3
"""bn254_batch_collect_keyed_bitmap_device against what a caller did without it, inputs resident in HBM, 256 registered keys, every share
valid.  Per shape n tuples x k shares (the signers of a tuple: k distinct keys drawn at random; a tuple with more shares than keys repeats
them):
  (a) the new call;
  (b) bn254_batch_verify_keyed_device on the tuple's message repeated once per share, a copy of the statuses to the host, the filter there,
      and bn254_batch_g1_sum (host pointers) over the shares that passed, one segment per tuple.  The bitmap, which the caller would also
      assemble by hand, is not counted.
Both are timed with HIP events on the caller's stream around whole calls, alternating, `--reps` calls each after two warm-up calls: the
median, with the min and max beside it (and the new call's mean, for an A/B of two builds through BN254_LIB).  (b)'s interval contains its host work — that is the route.  Per-stage times of one profiled call
of (a) and of the keyed verify: bn254_ctx_last_kernel_ms ((a): ms[0] decode + hash + spread, ms[1] select-and-sum, ms[2] Miller loop,
ms[3] final exponentiation).  --wave-min sweeps BN254_OPT_COLLECT_WAVE_MIN_SHARES for (a).  One JSON line per shape (default stdout).
--rand adds bn254_batch_collect_keyed_bitmap_randomized_device with its route forced (options 38 = 0, 39 = 0), 128-bit and 64-bit weights:
whole-call median, per-stage times (ms[2] = grouping + scalar ladders, ms[3] = group checks + exact re-checks), the debug hook's counters, and
whether all five outputs are the exact call's bytes.  --keys sets the size of the registered set; --bad-percent P corrupts every (100 / P)-th
share (a valid point, the neighbour's signature), which prices failed groups — route (b) is then left out, its filter assumes valid shares.
--optimistic adds bn254_batch_collect_keyed_bitmap_optimistic_device with its route forced (options 40 = 0, 41 = 0): whole-call median,
per-stage times (ms[0] = front end + provisional sum, ms[1] = aggregate keys, ms[2] = the tuples' Miller loop and final exponentiation,
ms[3] = exact fallback + re-sum), the debug hook's counters, and whether all five outputs are the exact call's bytes.  --bad-one-tuple puts
the wrong shares of --bad-percent into tuple 0 alone (at most its k shares; each the share at its position in the NEXT tuple, so that the
tuple's sum is wrong too).  --skip-b leaves route (b) out.
A library without the randomised or the optimistic call (BN254_LIB = an older build, the baseline of an A/B) runs the other legs.
    python tools/collect_throughput.py [out.jsonl] [--reps R] [--wave-min W ...] [--rand] [--optimistic] [--keys K] [--bad-percent P]
                                       [--bad-one-tuple] [--skip-b] [--note TEXT] [shape ...]   shape = n:k"""
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
from bn254_amd.engine import (COLLECT_OPT_MIN_SHARES_DEFAULT, COLLECT_OPT_MIN_TUPLE_SHARES_DEFAULT, OPT_COLLECT_OPT_MIN_SHARES,  # noqa: E402
                              OPT_COLLECT_OPT_MIN_TUPLE_SHARES)
from bn254_amd.engine import (FLAG_RAND64, OPT_COLLECT_RAND_MIN_PER_KEY, OPT_COLLECT_RAND_MIN_SHARES, OPT_COLLECT_WAVE_MIN_SHARES,  # noqa: E402
                              COLLECT_RAND_MIN_PER_KEY_DEFAULT, COLLECT_RAND_MIN_SHARES_DEFAULT)
from tests.datagen import sk_bytes  # noqa: E402

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SHAPES = [(256, 171), (4096, 11), (1, 4096)]
MSG_LEN = 32


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--wave-min", type=int, nargs="*", default=[])
    ap.add_argument("--rand", action="store_true")
    ap.add_argument("--optimistic", action="store_true")
    ap.add_argument("--bad-one-tuple", action="store_true")
    ap.add_argument("--skip-b", action="store_true")
    ap.add_argument("--keys", type=int, default=256)
    ap.add_argument("--bad-percent", type=float, default=0.0)
    ap.add_argument("--note", default=None, help="recorded with every line, e.g. which build ran")
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
    rng = np.random.default_rng(20261018)
    sks = [int.from_bytes(sk_bytes(9000 + j), "big") % R for j in range(N_KEYS)]
    pool, st = eng.batch_g2_mul(None, b"".join(s.to_bytes(32, "big") for s in sks), N_KEYS, reduce_scalar=True)
    assert st == bytes(N_KEYS) and eng.register_keys(pool) == bytes(N_KEYS)
    bm_words = (N_KEYS + 31) // 32
    have_rand = a.rand and hasattr(lib, "bn254_batch_collect_keyed_bitmap_randomized_device")
    have_opt = a.optimistic and hasattr(lib, "bn254_batch_collect_keyed_bitmap_optimistic_device")
    seed = hashlib.sha256(b"collect/tp/seed").digest()

    for n, k in shapes:
        n_shares = n * k
        keys = np.concatenate([np.resize(rng.permutation(N_KEYS), k) for _ in range(n)]).astype(np.uint32)
        msgs = [hashlib.sha256(b"collect/tp/%d/%d/%d" % (n, k, i)).digest() for i in range(n)]
        rep = [msgs[s // k] for s in range(n_shares)]
        shares, st = eng.batch_sign(rep, b"".join(sks[j].to_bytes(32, "big") for j in keys))
        assert st == bytes(n_shares)
        n_bad = 0
        if a.bad_percent > 0:
            every = max(int(round(100.0 / a.bad_percent)), 2)
            sh = bytearray(shares)
            where = range(every // 2, n_shares, every)
            if a.bad_one_tuple:
                where = range(min(len(where), k))
            for s in where:
                o = s + 1 if s + 1 < n_shares else s - 1
                if a.bad_one_tuple and n > 1:
                    o = s + k
                sh[64 * s:64 * s + 64] = shares[64 * o:64 * o + 64]
                n_bad += 1
            shares = bytes(sh)
        share_off = np.arange(n + 1, dtype=np.uint64) * k
        d_msgs, d_moff = dev(b"".join(msgs)), dev((np.arange(n + 1, dtype=np.uint64) * MSG_LEN).tobytes())
        d_rep, d_roff = dev(b"".join(rep)), dev((np.arange(n_shares + 1, dtype=np.uint64) * MSG_LEN).tobytes())
        d_shares, d_keys, d_soff = dev(shares), dev(keys.tobytes()), dev(share_off.tobytes())
        d_sst, d_tst, d_agg, d_bits, d_cnt = dev(bytes(n_shares)), dev(bytes(n)), dev(bytes(64 * n)), dev(bytes(4 * bm_words * n)), dev(bytes(4 * n))
        d_kst = dev(bytes(n_shares))
        sum_out, sum_st = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
        seg = (ctypes.c_uint64 * (n + 1))(*[int(x) for x in share_off])

        def collect():
            _check(lib.bn254_batch_collect_keyed_bitmap_device(h, d_msgs.data_ptr(), d_moff.data_ptr(), d_shares.data_ptr(), d_keys.data_ptr(),
                                                               d_soff.data_ptr(), n_shares, n, bm_words, 0, d_sst.data_ptr(), d_tst.data_ptr(),
                                                               d_agg.data_ptr(), d_bits.data_ptr(), d_cnt.data_ptr(), stream))

        def keyed():
            _check(lib.bn254_batch_verify_keyed_device(h, d_rep.data_ptr(), d_roff.data_ptr(), d_shares.data_ptr(), d_keys.data_ptr(), n_shares, 0,
                                                       d_kst.data_ptr(), stream))

        def parent_route():
            keyed()
            with torch.cuda.stream(ts):
                status = d_kst[:n_shares].cpu().numpy()
            assert not status.any()                                   # the filter: every share passed, so the sum takes them all
            _check(lib.bn254_batch_g1_sum(h, shares, seg, n, sum_out, sum_st))

        def collect_rand(flags):
            _check(lib.bn254_batch_collect_keyed_bitmap_randomized_device(h, d_msgs.data_ptr(), d_moff.data_ptr(), d_shares.data_ptr(), d_keys.data_ptr(),
                                                                          d_soff.data_ptr(), n_shares, n, bm_words, flags, seed, d_sst.data_ptr(),
                                                                          d_tst.data_ptr(), d_agg.data_ptr(), d_bits.data_ptr(), d_cnt.data_ptr(), stream))

        def collect_opt():
            _check(lib.bn254_batch_collect_keyed_bitmap_optimistic_device(h, d_msgs.data_ptr(), d_moff.data_ptr(), d_shares.data_ptr(), d_keys.data_ptr(),
                                                                          d_soff.data_ptr(), n_shares, n, bm_words, 0, d_sst.data_ptr(), d_tst.data_ptr(),
                                                                          d_agg.data_ptr(), d_bits.data_ptr(), d_cnt.data_ptr(), stream))

        def outputs():
            torch.cuda.synchronize()
            return tuple(t.cpu().numpy().tobytes()[:m] for t, m in ((d_sst, n_shares), (d_tst, n), (d_agg, 64 * n), (d_bits, 4 * bm_words * n), (d_cnt, 4 * n)))

        if n_bad or a.skip_b:
            def parent_route():   # noqa: F811  (its filter assumes that every share passes)
                keyed()
        for fn in (collect, parent_route, collect, parent_route):
            fn()
        torch.cuda.synchronize()
        # with more shares than keys a tuple repeats its signers: (a) takes one share per key, (b)'s plain sum takes them all — no comparison there
        exact_out = outputs()
        same = n_bad == 0 and not d_sst[:n_shares].cpu().numpy().any() and (k > N_KEYS or bytes(d_agg.cpu().numpy().tobytes()[:64 * n]) == sum_out.raw)
        counts = np.frombuffer(d_cnt.cpu().numpy().tobytes()[:4 * n], dtype=np.uint32)
        ms = {"a": [], "b": [], "keyed": []}
        for _ in range(a.reps):
            ms["a"].append(timed(collect, ts))
            ms["b"].append(timed(parent_route, ts))
            ms["keyed"].append(timed(keyed, ts))
        stages = {}
        for name, fn in (("a_collect", collect), ("keyed_verify", keyed)):
            eng.set_profiling(True)
            fn()
            kms = eng.last_kernel_ms()
            eng.set_profiling(False)
            stages[name] = [round(kms[x], 3) for x in ("decode", "hash_to_g1", "miller_loop", "final_exp")]
        sweep = {}
        for w in a.wave_min:
            eng.set_option(OPT_COLLECT_WAVE_MIN_SHARES, w)
            collect()
            sweep[str(w)] = round(statistics.median([timed(collect, ts) for _ in range(a.reps)]), 3)
            eng.set_profiling(True)
            collect()
            sweep[str(w) + "_sum_ms"] = round(eng.last_kernel_ms()["hash_to_g1"], 3)
            eng.set_profiling(False)
        eng.set_option(OPT_COLLECT_WAVE_MIN_SHARES, 16)
        rand = {}
        if have_rand:
            eng.set_option(OPT_COLLECT_RAND_MIN_SHARES, 0)
            eng.set_option(OPT_COLLECT_RAND_MIN_PER_KEY, 0)
            for name, flags in (("r128", 0), ("r64", FLAG_RAND64)):
                call = lambda: collect_rand(flags)   # noqa: E731
                call()
                call()
                same_bytes = outputs() == exact_out
                hook = eng.debug_collect_rand_last()
                t = [timed(call, ts) for _ in range(a.reps)]
                eng.set_profiling(True)
                call()
                kms = eng.last_kernel_ms()
                eng.set_profiling(False)
                rand[name] = {"ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "mean_ms": round(statistics.mean(t), 3),
                              "stages_ms": [round(kms[x], 3) for x in ("decode", "hash_to_g1", "miller_loop", "final_exp")],
                              "hook": hook, "same_bytes_as_exact": bool(same_bytes)}
            eng.set_option(OPT_COLLECT_RAND_MIN_SHARES, COLLECT_RAND_MIN_SHARES_DEFAULT)
            eng.set_option(OPT_COLLECT_RAND_MIN_PER_KEY, COLLECT_RAND_MIN_PER_KEY_DEFAULT)
        optimistic = {}
        if have_opt:
            eng.set_option(OPT_COLLECT_OPT_MIN_SHARES, 0)
            eng.set_option(OPT_COLLECT_OPT_MIN_TUPLE_SHARES, 0)
            collect_opt()
            collect_opt()
            same_bytes = outputs() == exact_out
            hook = eng.debug_collect_opt_last()
            t = [timed(collect_opt, ts) for _ in range(a.reps)]
            eng.set_profiling(True)
            collect_opt()
            kms = eng.last_kernel_ms()
            eng.set_profiling(False)
            optimistic = {"ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3), "mean_ms": round(statistics.mean(t), 3),
                          "stages_ms": [round(kms[x], 3) for x in ("decode", "hash_to_g1", "miller_loop", "final_exp")],
                          "hook": hook, "same_bytes_as_exact": bool(same_bytes)}
            eng.set_option(OPT_COLLECT_OPT_MIN_SHARES, COLLECT_OPT_MIN_SHARES_DEFAULT)
            eng.set_option(OPT_COLLECT_OPT_MIN_TUPLE_SHARES, COLLECT_OPT_MIN_TUPLE_SHARES_DEFAULT)
        med = {x: statistics.median(v) for x, v in ms.items()}
        row = {"shape": "%dx%d" % (n, k), "n": n, "shares_per_tuple": k, "n_shares": n_shares, "mean_signers": round(float(counts.mean()), 1),
               "a_ms": round(med["a"], 3), "a_min_ms": round(min(ms["a"]), 3), "a_max_ms": round(max(ms["a"]), 3), "a_mean_ms": round(statistics.mean(ms["a"]), 3),
               "b_ms": round(med["b"], 3), "b_min_ms": round(min(ms["b"]), 3), "b_max_ms": round(max(ms["b"]), 3),
               "keyed_verify_alone_ms": round(med["keyed"], 3), "b_over_a": round(med["b"] / med["a"], 2),
               "a_not_slower_beyond_spread": max(ms["a"]) <= min(ms["b"]),
               "stages_ms": stages, "stage_slots": {"a_collect": "decode+hash+spread, select-and-sum, miller, final_exp", "keyed_verify": "decode, hash, miller, final_exp"},
               "wave_min_sweep_ms": sweep, "same_aggregates_all_valid": bool(same), **box}
        if a.skip_b and not n_bad:
            row.update({"b_ms": None, "b_min_ms": None, "b_max_ms": None, "b_over_a": None, "a_not_slower_beyond_spread": None, "same_aggregates_all_valid": None})
        if n_bad:
            row.update({"bad_shares": n_bad, "bad_in_one_tuple": bool(a.bad_one_tuple), "b_ms": None, "b_min_ms": None, "b_max_ms": None, "b_over_a": None, "a_not_slower_beyond_spread": None})
        if have_rand:
            row["randomized"] = rand
            row["rand_stage_slots"] = "decode+hash+spread, select-and-sum, grouping+ladders, group checks+re-checks"
        if have_opt:
            row["optimistic"] = optimistic
            row["optimistic_stage_slots"] = "front end+provisional sum, aggregate keys, tuples' miller+final_exp, exact fallback+re-sum"
        print(json.dumps(row), file=out, flush=True)
        del d_msgs, d_moff, d_rep, d_roff, d_shares, d_keys, d_soff, d_sst, d_tst, d_agg, d_bits, d_cnt, d_kst


if __name__ == "__main__":
    main()
