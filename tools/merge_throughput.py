#!/usr/bin/env python3
"""bn254_batch_merge_keyed_bitmap_device against what a caller did without it, inputs resident in HBM, 256 registered keys, every partial
valid.  Per shape n tuples x k partials: two thirds of the keys sign in total, drawn at random per tuple and split into k DISJOINT committees
(a partial = the sum of its committee's signatures and its bitmap row); a shape n:k:1 has ONE-BIT partials instead, partial p signed by key
p % n_keys, so that all but the first n_keys partials of a tuple overlap.
  (a) the new call;
  (b) the route without it: bn254_batch_verify_keyed_bitmap_device on the tuple's message repeated once per partial, a copy of the statuses
      to the host, the first-fit filter there with its overlap bookkeeping (numpy, vectorised over the tuples; big integers for a lone
      tuple), and bn254_batch_g1_sum (host pointers) over the partials taken, one segment per tuple.  The union bitmaps, which the filter
      produces on the way, are compared with (a)'s; so are the sums.
Both are timed with HIP events on the caller's stream around whole calls, alternating, `--reps` calls each after two warm-up calls: the
median, with the min and max beside it.  (b)'s interval contains its host work — that is the route; the host filter's own share is
reported beside it (host clock), since an interpreter's loop is slower than a caller's compiled one would be.  Per-stage times of one profiled
call of (a) and of the bitmap verify: bn254_ctx_last_kernel_ms ((a): ms[0] hash once per tuple + decode + spread + aggregate keys, ms[1]
select-and-sum, ms[2] Miller loop, ms[3] final exponentiation).
--sweep: instead of the shapes, both layouts of the select-and-sum forced through BN254_OPT_MERGE_WAVE_MIN_PARTS (1 = a wave per tuple,
2^31 - 1 = a lane per tuple) over tuple lengths 4 .. 256 at bm_words 8 and 128, about --sweep-parts partials per call, all 256 keys signing
in k disjoint committees: the select-and-sum interval (median of --reps profiled calls) and the whole call.  One JSON line per shape or
sweep point (default stdout).
--optimistic: instead of (a) against (b), bn254_batch_merge_keyed_bitmap_optimistic_device — its route forced with
BN254_OPT_MERGE_OPT_MIN_PARTS = 0 — against the exact merge of the same build, alternating, over the shapes above and n x 16 for n = 1, 2,
4, 8, 16, 64: whole-call medians with min and max, the four intervals of one profiled optimistic call (ms[0] front end + provisional
select-and-sum, ms[1] aggregate keys of the union rows, ms[2] the tuples' Miller loop and final exponentiation, ms[3] fallback + re-select),
the debug hook's counters, and whether all six outputs are the exact call's bytes.  --bad-one-tuple replaces the first partial's signature by
its neighbour's (one failing tuple); --bad-percent P does so for P % of the partials, spread evenly.  --other-lib PATH loads a second build
of the library (the parent commit's, say) into the same process, with a context of its own over the same keys, and times ITS exact merge in
the same alternation: what the new route costs the old one.
    python tools/merge_throughput.py [out.jsonl] [--reps R] [--keys K] [--sweep] [--sweep-parts P] [--optimistic] [--bad-one-tuple]
                                     [--bad-percent P] [--other-lib PATH] [--note TEXT] [shape ...]   shape = n:k[:1]"""
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

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SHAPES = [(256, 16, 0), (4096, 4, 0), (1024, 64, 0), (1, 4096, 1)]
OPT_SHAPES = SHAPES + [(n, 16, 0) for n in (1, 2, 4, 8, 16, 64)]
SWEEP_LENGTHS = [4, 8, 16, 32, 64, 128, 256]
SWEEP_WIDTHS = [8, 128]
MSG_LEN = 32
ALL_LANES = (1 << 31) - 1


def committees(rng, n, k, n_keys, n_signing, one_bit):
    """-> per tuple a list of k lists of key indices"""
    out = []
    for _ in range(n):
        if one_bit:
            out.append([[p % n_keys] for p in range(k)])
            continue
        who = rng.permutation(n_keys)[:max(n_signing, k)]
        out.append([list(map(int, c)) for c in np.array_split(who, k)])
    return out


def rows_of(sets, bm_words):
    """the bitmap rows of the partials, [n_parts, bm_words] uint32"""
    rows = np.zeros((len(sets), bm_words), dtype=np.uint32)
    for p, idx in enumerate(sets):
        for j in idx:
            rows[p, j // 32] |= np.uint32(1 << (j % 32))
    return rows


def first_fit(status, rows, n, k):
    """the host filter of route (b): status [n * k], rows [n * k, bm_words] -> (taken [n * k] bool, union rows [n, bm_words])"""
    bm_words = rows.shape[1]
    ok = (status == 0).reshape(n, k)
    if n == 1:                                                     # a lone tuple: the row as one big integer
        taken, union = np.zeros(k, dtype=bool), 0
        ints = [int.from_bytes(rows[p].tobytes(), "little") for p in range(k)]
        for p in range(k):
            if ok[0, p] and not (union & ints[p]):
                union |= ints[p]
                taken[p] = True
        return taken, np.frombuffer(union.to_bytes(4 * bm_words, "little"), dtype=np.uint32).reshape(1, bm_words).copy()
    r = rows.reshape(n, k, bm_words)
    union = np.zeros((n, bm_words), dtype=np.uint32)
    taken = np.zeros((n, k), dtype=bool)
    for j in range(k):                                             # serial in the partials, vectorised over the tuples
        take = ok[:, j] & ~(union & r[:, j]).any(axis=1)
        union |= np.where(take[:, None], r[:, j], np.uint32(0))
        taken[:, j] = take
    return taken.reshape(-1), union


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--keys", type=int, default=256)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--sweep-parts", type=int, default=16384)
    ap.add_argument("--optimistic", action="store_true")
    ap.add_argument("--bad-one-tuple", action="store_true")
    ap.add_argument("--bad-percent", type=float, default=0.0)
    ap.add_argument("--other-lib", default=None, help="a second build whose exact merge is timed in the same alternation")
    ap.add_argument("--note", default=None, help="recorded with every line, e.g. which build ran")
    a = ap.parse_intermixed_args()
    shapes = [tuple(int(x) for x in (s + ":0").split(":")[:3]) for s in a.shapes] or (OPT_SHAPES if a.optimistic else SHAPES)

    import torch  # (first: one HIP runtime per process)
    import bn254_amd
    from bn254_amd import _native
    from bn254_amd.engine import MERGE_WAVE_MIN_PARTS_DEFAULT, OPT_MERGE_WAVE_MIN_PARTS
    from tests.datagen import sk_bytes

    def dev(data):
        t = torch.empty(max(len(data), 8), dtype=torch.uint8, device="cuda")
        if len(data):
            t[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        return t

    def check(rc):
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

    out = open(a.out, "a") if a.out else sys.stdout
    n_keys = a.keys
    eng = bn254_amd.Engine(0)
    lib, h = eng._lib, eng._h
    ts = torch.cuda.Stream()                        # a stream of the caller's own: a null handle would send the calls to the context's stream
    stream = ctypes.c_void_p(ts.cuda_stream)
    box = {"device": torch.cuda.get_device_name(0), "lib_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16],
           "n_keys": n_keys, "reps": a.reps}
    if a.note:
        box["note"] = a.note
    rng = np.random.default_rng(20261018)
    sks = [int.from_bytes(sk_bytes(9000 + j), "big") % R for j in range(n_keys)]
    pool, st = eng.batch_g2_mul(None, b"".join(s.to_bytes(32, "big") for s in sks), n_keys, reduce_scalar=True)
    assert st == bytes(n_keys) and eng.register_keys(pool) == bytes(n_keys)
    stage_names = ("decode", "hash_to_g1", "miller_loop", "final_exp")

    def setup(n, k, bm_words, n_signing, one_bit, tag, bad=()):
        """the inputs of one shape, resident; -> dict.  bad: the partials whose signature is replaced by the next partial's"""
        n_parts = n * k
        sets = [c for t in committees(rng, n, k, n_keys, n_signing, one_bit) for c in t]
        msgs = [hashlib.sha256(b"merge/tp/%s/%d/%d/%d" % (tag.encode(), n, k, i)).digest() for i in range(n)]
        rep = [msgs[p // k] for p in range(n_parts)]
        parts, st = eng.batch_sign(rep, b"".join((sum(sks[j] for j in c) % R).to_bytes(32, "big") for c in sets))
        assert st == bytes(n_parts)
        if bad:
            honest, parts = parts, bytearray(parts)
            for p in bad:
                q = (p + 1) % n_parts
                parts[64 * p:64 * p + 64] = honest[64 * q:64 * q + 64]
            parts = bytes(parts)
        rows = rows_of(sets, bm_words)
        d = dict(n=n, k=k, n_parts=n_parts, bm_words=bm_words, parts=parts, rows=rows, sets=sets)
        d["d_msgs"], d["d_moff"] = dev(b"".join(msgs)), dev((np.arange(n + 1, dtype=np.uint64) * MSG_LEN).tobytes())
        d["d_rep"], d["d_roff"] = dev(b"".join(rep)), dev((np.arange(n_parts + 1, dtype=np.uint64) * MSG_LEN).tobytes())
        d["d_parts"], d["d_rows"], d["d_poff"] = dev(parts), dev(rows.tobytes()), dev((np.arange(n + 1, dtype=np.uint64) * k).tobytes())
        d["d_pst"], d["d_tkn"], d["d_tst"], d["d_agg"] = dev(bytes(n_parts)), dev(bytes(n_parts)), dev(bytes(n)), dev(bytes(64 * n))
        d["d_bits"], d["d_cnt"], d["d_vst"] = dev(bytes(4 * bm_words * n)), dev(bytes(4 * n)), dev(bytes(n_parts))
        return d

    def merge_call(d):
        check(lib.bn254_batch_merge_keyed_bitmap_device(h, d["d_msgs"].data_ptr(), d["d_moff"].data_ptr(), d["d_parts"].data_ptr(), d["d_rows"].data_ptr(),
                                                        d["d_poff"].data_ptr(), d["n_parts"], d["n"], d["bm_words"], 0, d["d_pst"].data_ptr(),
                                                        d["d_tkn"].data_ptr(), d["d_tst"].data_ptr(), d["d_agg"].data_ptr(), d["d_bits"].data_ptr(),
                                                        d["d_cnt"].data_ptr(), stream))

    def profiled(fn):
        eng.set_profiling(True)
        fn()
        kms = eng.last_kernel_ms()
        eng.set_profiling(False)
        return [kms[x] for x in stage_names]

    if a.sweep:
        for bm_words in SWEEP_WIDTHS:
            for k in SWEEP_LENGTHS:
                n = max(a.sweep_parts // k, 1)
                d = setup(n, k, bm_words, n_keys, False, "sweep%d" % bm_words)
                row = {"sweep": True, "bm_words": bm_words, "partials_per_tuple": k, "n": n, "n_parts": n * k}
                outs = {}
                for name, w in (("lane", ALL_LANES), ("wave", 1)):
                    eng.set_option(OPT_MERGE_WAVE_MIN_PARTS, w)
                    merge_call(d)
                    merge_call(d)
                    torch.cuda.synchronize()
                    outs[name] = tuple(d[x].cpu().numpy().tobytes() for x in ("d_pst", "d_tkn", "d_tst", "d_agg", "d_bits", "d_cnt"))
                    sums = [profiled(lambda: merge_call(d))[1] for _ in range(a.reps)]
                    whole = [timed(lambda: merge_call(d), ts) for _ in range(a.reps)]
                    row[name + "_sum_ms"] = round(statistics.median(sums), 4)
                    row[name + "_sum_min_max_ms"] = [round(min(sums), 4), round(max(sums), 4)]
                    row[name + "_call_ms"] = round(statistics.median(whole), 3)
                eng.set_option(OPT_MERGE_WAVE_MIN_PARTS, MERGE_WAVE_MIN_PARTS_DEFAULT)
                row["same_bytes_both_layouts"] = outs["lane"] == outs["wave"]
                row["all_taken"] = bool(np.frombuffer(outs["lane"][1][:n * k], dtype=np.uint8).all())
                row.update(box)
                print(json.dumps(row), file=out, flush=True)
                del d
        return

    if a.optimistic:
        from bn254_amd.engine import MERGE_OPT_MIN_PARTS_DEFAULT, OPT_MERGE_OPT_MIN_PARTS
        other = None
        if a.other_lib:                                    # a second build in the same process: its own context over the same keys
            vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
            other = ctypes.CDLL(os.path.abspath(a.other_lib))
            other.bn254_ctx_create.argtypes = [ctypes.c_int32, ctypes.POINTER(vp)]
            other.bn254_ctx_register_keys.argtypes = [vp, vp, sz, u32, vp]
            other.bn254_batch_merge_keyed_bitmap_device.argtypes = [vp, vp, vp, vp, vp, vp, sz, sz, sz, u32, vp, vp, vp, vp, vp, vp, vp]
            other.bn254_ctx_destroy.argtypes = [vp]
            other.bn254_ctx_destroy.restype = None
            h2 = vp()
            check(other.bn254_ctx_create(0, ctypes.byref(h2)))
            reg = ctypes.create_string_buffer(n_keys)
            check(other.bn254_ctx_register_keys(h2, pool, n_keys, 0, reg))
            assert reg.raw == bytes(n_keys)
            box["other_lib_sha256"] = hashlib.sha256(open(a.other_lib, "rb").read()).hexdigest()[:16]
        names = ("d_pst", "d_tkn", "d_tst", "d_agg", "d_bits", "d_cnt")
        for n, k, one_bit in shapes:
            bm_words = (n_keys + 31) // 32
            n_parts = n * k
            bad = [0] if a.bad_one_tuple else []
            if a.bad_percent > 0:
                step = max(int(round(100.0 / a.bad_percent)), 1)
                bad = list(range(step // 2, n_parts, step))
            d = setup(n, k, bm_words, (2 * n_keys) // 3, bool(one_bit), "opt", bad)

            def device_call(fn, ctx):
                check(fn(ctx, d["d_msgs"].data_ptr(), d["d_moff"].data_ptr(), d["d_parts"].data_ptr(), d["d_rows"].data_ptr(), d["d_poff"].data_ptr(), n_parts, n,
                         bm_words, 0, d["d_pst"].data_ptr(), d["d_tkn"].data_ptr(), d["d_tst"].data_ptr(), d["d_agg"].data_ptr(), d["d_bits"].data_ptr(),
                         d["d_cnt"].data_ptr(), stream))
            legs = {"exact": lambda: merge_call(d), "opt": lambda: device_call(lib.bn254_batch_merge_keyed_bitmap_optimistic_device, h)}
            if other is not None:
                legs["other_exact"] = lambda: device_call(other.bn254_batch_merge_keyed_bitmap_device, h2)
            eng.set_option(OPT_MERGE_OPT_MIN_PARTS, 0)
            try:
                outs = {}
                for _ in range(2):                             # two warm-up calls each; the second one's outputs are compared
                    for name, fn in legs.items():
                        fn()
                        torch.cuda.synchronize()
                        outs[name] = tuple(d[x].cpu().numpy().tobytes() for x in names)
                        if name == "opt":
                            hook = eng.debug_merge_opt_last()
                ms = {name: [] for name in legs}
                for _ in range(a.reps):
                    for name, fn in legs.items():
                        ms[name].append(timed(fn, ts))
                stages = [round(x, 3) for x in profiled(legs["opt"])]
                exact_stages = [round(x, 3) for x in profiled(legs["exact"])]
            finally:
                eng.set_option(OPT_MERGE_OPT_MIN_PARTS, MERGE_OPT_MIN_PARTS_DEFAULT)
            med = {name: statistics.median(v) for name, v in ms.items()}
            row = {"optimistic": True, "shape": "%dx%d%s" % (n, k, " one-bit" if one_bit else ""), "n": n, "partials_per_tuple": k, "n_parts": n_parts,
                   "bm_words": bm_words, "bad_parts": len(bad), "bad_in_one_tuple": bool(a.bad_one_tuple)}
            for name in legs:
                row.update({name + "_ms": round(med[name], 3), name + "_min_ms": round(min(ms[name]), 3), name + "_max_ms": round(max(ms[name]), 3),
                            name + "_mean_ms": round(statistics.mean(ms[name]), 3)})
            row.update({"exact_over_opt": round(med["exact"] / med["opt"], 2), "opt_wins_beyond_spread": max(ms["opt"]) < min(ms["exact"]),
                        "opt_loses_beyond_spread": min(ms["opt"]) > max(ms["exact"]),
                        "opt_stages_ms": stages, "opt_stage_slots": "front end + provisional select-and-sum, aggregate keys, tuples' miller + final_exp, fallback + re-select",
                        "exact_stages_ms": exact_stages, "hook": hook, "same_outputs_as_exact": outs["opt"] == outs["exact"]})
            if other is not None:
                row.update({"same_outputs_other_exact": outs["other_exact"] == outs["exact"],
                            "exact_vs_other_percent": round(100.0 * (med["exact"] / med["other_exact"] - 1.0), 2),
                            "other_spread_percent": [round(100.0 * (min(ms["other_exact"]) / med["other_exact"] - 1.0), 2),
                                                     round(100.0 * (max(ms["other_exact"]) / med["other_exact"] - 1.0), 2)]})
            row.update(box)
            print(json.dumps(row), file=out, flush=True)
            del d
        if other is not None:
            other.bn254_ctx_destroy(h2)
        return

    for n, k, one_bit in shapes:
        bm_words = (n_keys + 31) // 32
        d = setup(n, k, bm_words, (2 * n_keys) // 3, bool(one_bit), "shape")
        n_parts = n * k
        parts_np = np.frombuffer(d["parts"], dtype=np.uint8).reshape(n_parts, 64)
        sum_out, sum_st = ctypes.create_string_buffer(64 * n), ctypes.create_string_buffer(n)
        host = {}

        def bitmap_verify():
            check(lib.bn254_batch_verify_keyed_bitmap_device(h, d["d_rep"].data_ptr(), d["d_roff"].data_ptr(), d["d_parts"].data_ptr(), d["d_rows"].data_ptr(),
                                                             bm_words, n_parts, 0, d["d_vst"].data_ptr(), stream))

        def parent_route():
            bitmap_verify()
            with torch.cuda.stream(ts):
                status = d["d_vst"][:n_parts].cpu().numpy()
            t0 = time.perf_counter()
            taken, union = first_fit(status, d["rows"], n, k)
            picked = np.ascontiguousarray(parts_np[taken]).tobytes()
            seg = np.concatenate(([0], np.cumsum(taken.reshape(n, k).sum(axis=1)))).astype(np.uint64)
            host["filter_ms"] = (time.perf_counter() - t0) * 1e3
            check(lib.bn254_batch_g1_sum(h, picked, seg.ctypes.data_as(ctypes.c_void_p), n, sum_out, sum_st))
            host["taken"], host["union"] = taken, union

        for fn in (lambda: merge_call(d), parent_route, lambda: merge_call(d), parent_route):
            fn()
        torch.cuda.synchronize()
        a_out = {x: d[x].cpu().numpy().tobytes() for x in ("d_pst", "d_tkn", "d_agg", "d_bits", "d_cnt")}
        same = (not any(a_out["d_pst"][:n_parts]) and a_out["d_agg"][:64 * n] == sum_out.raw and a_out["d_bits"][:4 * bm_words * n] == host["union"].tobytes()
                and a_out["d_tkn"][:n_parts] == host["taken"].astype(np.uint8).tobytes())
        counts = np.frombuffer(a_out["d_cnt"][:4 * n], dtype=np.uint32)
        ms = {"a": [], "b": [], "verify": [], "filter": []}
        for _ in range(a.reps):
            ms["a"].append(timed(lambda: merge_call(d), ts))
            ms["b"].append(timed(parent_route, ts))
            ms["filter"].append(host["filter_ms"])
            ms["verify"].append(timed(bitmap_verify, ts))
        stages = {"a_merge": [round(x, 3) for x in profiled(lambda: merge_call(d))], "bitmap_verify": [round(x, 3) for x in profiled(bitmap_verify)]}
        med = {x: statistics.median(v) for x, v in ms.items()}
        row = {"shape": "%dx%d%s" % (n, k, " one-bit" if one_bit else ""), "n": n, "partials_per_tuple": k, "n_parts": n_parts, "bm_words": bm_words,
               "mean_signers": round(float(counts.mean()), 1), "partials_taken": int(host["taken"].sum()),
               "a_ms": round(med["a"], 3), "a_min_ms": round(min(ms["a"]), 3), "a_max_ms": round(max(ms["a"]), 3), "a_mean_ms": round(statistics.mean(ms["a"]), 3),
               "b_ms": round(med["b"], 3), "b_min_ms": round(min(ms["b"]), 3), "b_max_ms": round(max(ms["b"]), 3),
               "b_host_filter_ms": round(med["filter"], 3), "bitmap_verify_alone_ms": round(med["verify"], 3), "b_over_a": round(med["b"] / med["a"], 2),
               "a_not_slower_beyond_spread": max(ms["a"]) <= min(ms["b"]),
               "stages_ms": stages, "stage_slots": {"a_merge": "hash+decode+spread+aggregate keys, select-and-sum, miller, final_exp",
                                                    "bitmap_verify": "decode+hash, aggregate keys, miller, final_exp"},
               "same_outputs_both_routes": bool(same), **box}
        print(json.dumps(row), file=out, flush=True)
        del d


if __name__ == "__main__":
    main()
