#!/usr/bin/env python3
"""bn254_ctx_reshare_commitments and bn254_batch_g2_vector_combine against the route that exists without them.  One JSON line per measurement
(default stdout; the committed figures are profiles/reshare.jsonl).  Every figure is the median, with the min and max beside it, of `--reps`
runs after two warm-up runs, the legs of a comparison alternating in one process; whole calls under a host clock, staging on both sides.
  reshare at n:t (default 256:171 1024:683), (n, t) -> (n, t), every old member a dealer —
    (r) bn254_ctx_reshare_commitments: decode, qualification, selection, coefficients, t * t ladders, sums;
    (v) bn254_batch_g2_vector_combine over the t vectors of S with the coefficients given;
    the route without the calls, which checks NOTHING about the dealers, each part timed:
    (l) the Lagrange coefficients of S in Python integers;
    (s) the staging: the vectors of S transposed into t segments of t points, the scalars replicated t times;
    (m) bn254_batch_g2_msm over those t segments.
  --unchanged: bn254_batch_g2_msm (171 terms in one segment), bn254_ctx_check_dealing (256:171) and bn254_batch_g2_poly_eval (256:171) alone, to
    compare two builds (BN254_LIB).
    python tools/reshare_throughput.py [out.jsonl] [--reps R] [--unchanged] [--note TEXT] [shape ...]   shape = n:t"""
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

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SHAPES = [(256, 171), (1024, 683)]


def _check(rc):
    if rc != 0:
        raise RuntimeError("library call failed: %d" % rc)


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def spread(v):
    return {"ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3), "runs": len(v)}


def be(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def dealing(n, t, tag):
    """the n shares of a polynomial of degree t - 1 drawn from a hash"""
    coeffs = [int.from_bytes(hashlib.sha256(b"%s%d" % (tag, e)).digest(), "big") % R for e in range(t)]
    out = []
    for x in range(1, n + 1):
        v = 0
        for c in reversed(coeffs):
            v = (v * x + c) % R
        out.append(v)
    return out


def lagrange_at_zero(keys):
    xs = [k + 1 for k in keys]
    out = []
    for j, xj in enumerate(xs):
        num = den = 1
        for k, xk in enumerate(xs):
            if k != j:
                num, den = num * xk % R, den * (xk - xj) % R
        out.append(num * pow(den, -1, R) % R)
    return out


def reshare_rows(eng, box, shapes, reps, out):
    lib, h = eng._lib, eng._h
    for n, t in shapes:
        sks = dealing(n, t, b"old")
        pool, st = eng.batch_g2_mul(None, be(sks), n, reduce_scalar=True)
        assert st == bytes(n) and eng.register_keys(pool) == bytes(n)
        # every old member's vector: its key, then t - 1 commitments of random coefficients
        rest, st = eng.batch_g2_mul(None, np.random.default_rng(n).bytes(32 * n * (t - 1)), n * (t - 1), reduce_scalar=True)
        assert st == bytes(n * (t - 1))
        rows = [pool[128 * i:128 * i + 128] + rest[128 * (t - 1) * i:128 * (t - 1) * (i + 1)] for i in range(n)]
        vectors = b"".join(rows)
        keys = (ctypes.c_uint32 * n)(*range(n))
        bm_words = (n + 31) // 32
        dst, row = ctypes.create_string_buffer(n), (ctypes.c_uint32 * bm_words)()
        r_out, r_st = ctypes.create_string_buffer(128 * t), ctypes.create_string_buffer(1)

        def reshare():
            _check(lib.bn254_ctx_reshare_commitments(h, vectors, keys, n, t, t, 0, dst, row, bm_words, r_out, r_st))
        old = {}

        def coefficients():
            old["lam"] = lagrange_at_zero(range(t))

        def staging():
            old["points"] = b"".join(rows[i][128 * k:128 * k + 128] for k in range(t) for i in range(t))
            old["scalars"] = be(old["lam"]) * t
        coefficients()
        staging()
        seg = (ctypes.c_uint64 * (t + 1))(*[k * t for k in range(t + 1)])
        m_out, m_st = ctypes.create_string_buffer(128 * t), ctypes.create_string_buffer(t)

        def msm():
            _check(lib.bn254_batch_g2_msm(h, old["points"], old["scalars"], seg, t, 0, m_out, m_st))
        s_vectors, s_scalars = b"".join(rows[:t]), be(old["lam"])
        v_out, v_st = ctypes.create_string_buffer(128 * t), ctypes.create_string_buffer(t)

        def combine():
            _check(lib.bn254_batch_g2_vector_combine(h, s_vectors, s_scalars, t, t, 0, v_out, v_st))
        for fn in (reshare, msm, combine, reshare, msm, combine):
            fn()
        same = r_out.raw == m_out.raw == v_out.raw and r_st.raw == b"\0" and m_st.raw == v_st.raw == bytes(t) and dst.raw == bytes(n)
        ms = {"r": [], "v": [], "l": [], "s": [], "m": []}
        for _ in range(reps):
            ms["r"].append(wall(reshare))
            ms["m"].append(wall(msm))
            ms["v"].append(wall(combine))
            ms["l"].append(wall(coefficients))
            ms["s"].append(wall(staging))
        print(json.dumps({"kind": "reshare", "n": n, "threshold": t, "t_new": t, "dealers": n, "reshare_commitments": spread(ms["r"]),
                          "vector_combine_host": spread(ms["v"]), "old_route_lagrange_python": spread(ms["l"]), "old_route_staging_python": spread(ms["s"]),
                          "old_route_g2_msm_host": spread(ms["m"]), "same_bytes": bool(same), "group_key_kept": r_out.raw[:128] == eng.check_dealing(t, bytes(32))[0],
                          **box}), file=out, flush=True)


def unchanged_rows(eng, box, reps, out):
    lib, h = eng._lib, eng._h
    pts, st = eng.batch_g2_mul(None, np.random.default_rng(1).bytes(32 * 171), 171, reduce_scalar=True)
    ks = np.random.default_rng(2).bytes(32 * 171)
    seg = (ctypes.c_uint64 * 2)(0, 171)
    o, s = ctypes.create_string_buffer(128), ctypes.create_string_buffer(1)

    def msm():
        _check(lib.bn254_batch_g2_msm(h, pts, ks, seg, 1, 1, o, s))
    n, t = 256, 171
    pool, st = eng.batch_g2_mul(None, be(dealing(n, t, b"c")), n, reduce_scalar=True)
    assert st == bytes(n) and eng.register_keys(pool) == bytes(n)
    seed = hashlib.sha256(b"reshare throughput").digest()
    pk, cst, bad = ctypes.create_string_buffer(128), ctypes.create_string_buffer(1), ctypes.c_uint32(0)

    def check():
        _check(lib.bn254_ctx_check_dealing(h, t, seed, 0, pk, cst, ctypes.byref(bad)))
    off = (ctypes.c_uint64 * 2)(0, t)
    polys, xs = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)(*range(1, n + 1))
    e_out, e_st = ctypes.create_string_buffer(128 * n), ctypes.create_string_buffer(n)

    def poly_eval():
        _check(lib.bn254_batch_g2_poly_eval(h, pts, off, 1, polys, xs, n, e_out, e_st))
    for fn in (msm, check, poly_eval, msm, check, poly_eval):
        fn()
    ms = {"msm": [], "check": [], "eval": []}
    for _ in range(reps):
        ms["msm"].append(wall(msm))
        ms["check"].append(wall(check))
        ms["eval"].append(wall(poly_eval))
    digest = hashlib.sha256(o.raw + pk.raw + e_out.raw).hexdigest()[:16]
    print(json.dumps({"kind": "unchanged_calls", "g2_msm_171_terms_one_segment": spread(ms["msm"]), "check_dealing_256_171": spread(ms["check"]),
                      "poly_eval_256_171": spread(ms["eval"]), "check_status": cst.raw[0], "outputs_sha256": digest, **box}), file=out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--unchanged", action="store_true")
    ap.add_argument("--note", default=None, help="recorded with every line, e.g. which build ran")
    a = ap.parse_intermixed_args()
    out = open(a.out, "a") if a.out else sys.stdout
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes] or SHAPES
    eng = bn254_amd.Engine(0)
    box = {"device": torch.cuda.get_device_name(0), "lib_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16], "reps": a.reps}
    if a.note:
        box["note"] = a.note
    if a.unchanged:
        unchanged_rows(eng, box, a.reps, out)
        return
    reshare_rows(eng, box, shapes, a.reps, out)


if __name__ == "__main__":
    main()
