#!/usr/bin/env python3
"""bn254_batch_g2_poly_eval and bn254_ctx_register_keys_commitments against the routes without them.  One JSON line per measurement (default
stdout; the committed figures are profiles/poly_eval.jsonl).  Every figure is the median, with the min and max beside it, of `--reps` runs
after two warm-up runs, the legs of a comparison alternating in one process.
  share keys at n:t (default 256:171 1024:683 4096:2731), the commitments of one polynomial, x = 1 .. n —
    (e) bn254_batch_g2_poly_eval, host form, wall clock (staging included);
    (d) bn254_batch_g2_poly_eval_device under HIP events on a caller's stream (its 8-byte copy home and wait included);
    (s) the scalars x^k mod r of the route that exists without the call, in Python integers, wall clock;
    (m) bn254_batch_g2_msm over n segments of t terms, host form, wall clock — the commitments staged n times.  Above --msm-max-terms
        terms only the first 256 keys are run and the figure is SCALED by n / 256 (the line says so);
    (r) bn254_ctx_register_keys_commitments, wall clock (the call is host-synchronous);
    (h) the route without it: bn254_batch_g2_poly_eval, the keys home, bn254_ctx_register_keys.
  dkg: 64 polynomials of 171 coefficients at one x (the share check of a DKG round) — (e), (d) and (m) over 64 segments of 171.
  --sweep: BN254_OPT_POLY_EVAL_WAVE_MIN_COEFFS over 4 .. 128 at t in 8, 16, 32, 64, 171, 256 evaluations of one polynomial at x of 9 and
    of 13 bits — (e) at each value.
  --unchanged: bn254_batch_g2_msm (171 terms in one segment) and bn254_ctx_check_dealing (256:171) alone, to compare two builds (BN254_LIB).
    python tools/poly_eval_throughput.py [out.jsonl] [--reps R] [--sweep] [--unchanged] [--note TEXT] [shape ...]   shape = n:t"""
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
from bn254_amd import engine as E  # noqa: E402

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
SHAPES = [(256, 171), (1024, 683), (4096, 2731)]
SWEEP_SPLITS = [4, 8, 16, 32, 64, 128]
SWEEP_LENGTHS = [8, 16, 32, 64, 171]


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


def spread(v, scale=1.0):
    return {"ms": round(statistics.median(v) * scale, 3), "min_ms": round(min(v) * scale, 3), "max_ms": round(max(v) * scale, 3), "runs": len(v)}


def be(values):
    return b"".join(int(v).to_bytes(32, "big") for v in values)


def u32(values):
    return np.asarray(list(values), dtype=np.uint32).tobytes()


def u64(values):
    return np.asarray(list(values), dtype=np.uint64).tobytes()


def commitments(eng, count, tag):
    rng = np.random.default_rng(tag)
    pts, st = eng.batch_g2_mul(None, rng.bytes(32 * count), count, reduce_scalar=True)
    assert st == bytes(count)
    return pts


def power_scalars(xs, t):
    out = []
    for x in xs:
        v = 1
        for _ in range(t):
            out.append(v)
            v = v * x % R
    return be(out)


class Eval:
    """one call shape: p polynomials (off), q evaluations; the host form, the _device form and the g2_msm route over the same evaluations"""

    def __init__(self, eng, stream, coeffs, off, polys, xs):
        self.eng, self.lib, self.h, self.stream = eng, eng._lib, eng._h, stream
        self.coeffs, self.off, self.polys, self.xs = coeffs, list(off), list(polys), list(xs)
        self.p, self.q = len(off) - 1, len(xs)
        self.c_off = (ctypes.c_uint64 * (self.p + 1))(*off)
        self.c_poly, self.c_x = (ctypes.c_uint32 * self.q)(*polys), (ctypes.c_uint32 * self.q)(*xs)
        self.out, self.st = ctypes.create_string_buffer(128 * self.q), ctypes.create_string_buffer(self.q)
        self.d = [dev(coeffs), dev(u64(off)), dev(u32(polys)), dev(u32(xs)), dev(bytes(128 * self.q)), dev(bytes(self.q))]

    def host(self):
        _check(self.lib.bn254_batch_g2_poly_eval(self.h, self.coeffs, self.c_off, self.p, self.c_poly, self.c_x, self.q, self.out, self.st))

    def device(self):
        d = self.d
        _check(self.lib.bn254_batch_g2_poly_eval_device(self.h, d[0].data_ptr(), d[1].data_ptr(), self.p, d[2].data_ptr(), d[3].data_ptr(), self.q,
                                                        d[4].data_ptr(), d[5].data_ptr(), self.stream))

    def msm_inputs(self, first):
        """the g2_msm route for the first `first` evaluations: every evaluation a segment of its polynomial's coefficients (staged again per
        evaluation) under the scalars x^k mod r"""
        pts, seg, ks = [], [0], []
        for poly, x in list(zip(self.polys, self.xs))[:first]:
            lo, hi = self.off[poly], self.off[poly + 1]
            pts.append(self.coeffs[128 * lo:128 * hi])
            seg.append(seg[-1] + hi - lo)
            ks.append((x, hi - lo))
        return b"".join(pts), seg, ks


def compare_rows(kind, ev, box, reps, msm_max_terms, out, extra):
    first = ev.q
    total_terms = sum(ev.off[p + 1] - ev.off[p] for p in ev.polys)
    if total_terms > msm_max_terms:
        first = min(ev.q, 256)
    pts, seg, ks = ev.msm_inputs(first)
    scalars = {}

    def scalars_python():
        scalars["k"] = b"".join(power_scalars([x], t) for x, t in ks)
    scalars_python()
    c_seg = (ctypes.c_uint64 * len(seg))(*seg)
    m_out, m_st = ctypes.create_string_buffer(128 * first), ctypes.create_string_buffer(first)

    def msm():
        _check(ev.lib.bn254_batch_g2_msm(ev.h, pts, scalars["k"], c_seg, first, 0, m_out, m_st))
    for fn in (ev.host, msm, ev.device, ev.host, msm, ev.device):
        fn()
    torch.cuda.synchronize()
    same = ev.out.raw[:128 * first] == m_out.raw and ev.st.raw[:first] == m_st.raw and ev.d[4].cpu().numpy().tobytes()[:128 * ev.q] == ev.out.raw
    t = {"host": [], "device": [], "msm": [], "scalars": []}
    for _ in range(reps):
        t["host"].append(wall(ev.host))
        t["msm"].append(wall(msm))
        t["device"].append(timed(ev.device, ev.stream_obj))
        t["scalars"].append(wall(scalars_python))
    scale = ev.q / first
    row = {"kind": kind, **extra, "evaluations": ev.q, "poly_eval_host": spread(t["host"]), "poly_eval_device": spread(t["device"]),
           "g2_msm_route_scalars_python": spread(t["scalars"], scale), "g2_msm_route_msm_host": spread(t["msm"], scale),
           "g2_msm_route_scaled_from_first": first if first != ev.q else None, "same_bytes": bool(same), "statuses_zero": ev.st.raw == bytes(ev.q), **box}
    print(json.dumps(row), file=out, flush=True)


def share_key_rows(eng, ts, stream, box, shapes, reps, msm_max_terms, out):
    lib, h = eng._lib, eng._h
    for n, t in shapes:
        coeffs = commitments(eng, t, 9000 + t)
        ev = Eval(eng, stream, coeffs, [0, t], [0] * n, range(1, n + 1))
        ev.stream_obj = ts
        compare_rows("share_keys", ev, box, reps, msm_max_terms, out, {"n": n, "threshold": t})
        key_st, st, key_st2 = ctypes.create_string_buffer(n), ctypes.create_string_buffer(1), ctypes.create_string_buffer(n)

        def from_commitments():
            _check(lib.bn254_ctx_register_keys_commitments(h, coeffs, t, n, 0, key_st, st))

        def through_host():
            ev.host()
            _check(lib.bn254_ctx_register_keys(h, ev.out.raw, n, 0, key_st2))
        for fn in (from_commitments, through_host, from_commitments, through_host):
            fn()
        ms = {"c": [], "h": []}
        for _ in range(reps):
            ms["c"].append(wall(from_commitments))
            ms["h"].append(wall(through_host))
        row = {"kind": "register", "n": n, "threshold": t, "register_keys_commitments": spread(ms["c"]), "poly_eval_then_register_keys": spread(ms["h"]),
               "same_key_statuses": key_st.raw == key_st2.raw == bytes(n) and st.raw == b"\0", **box}
        print(json.dumps(row), file=out, flush=True)
        del ev


def dkg_row(eng, ts, stream, box, reps, out):
    dealers, t = 64, 171
    coeffs = commitments(eng, dealers * t, 171)
    ev = Eval(eng, stream, coeffs, [d * t for d in range(dealers + 1)], range(dealers), [4097] * dealers)
    ev.stream_obj = ts
    compare_rows("dkg_share_check", ev, box, reps, 1 << 62, out, {"dealers": dealers, "threshold": t, "x": 4097})


def sweep_rows(eng, ts, stream, box, reps, out):
    q = 256
    default = None
    for t in SWEEP_LENGTHS:
        coeffs = commitments(eng, t, 500 + t)
        for bits in (9, 13):
            base = 1 << (bits - 1)
            ev = Eval(eng, stream, coeffs, [0, t], [0] * q, [base + j for j in range(q)])
            res, ms = {}, {w: [] for w in SWEEP_SPLITS}
            try:
                for w in SWEEP_SPLITS + SWEEP_SPLITS:                       # two warm-up rounds, the bytes of every setting kept
                    eng.set_option(E.OPT_POLY_EVAL_WAVE_MIN_COEFFS, w)
                    ev.host()
                    res[w] = ev.out.raw
                for _ in range(reps):
                    for w in SWEEP_SPLITS:
                        eng.set_option(E.OPT_POLY_EVAL_WAVE_MIN_COEFFS, w)
                        ms[w].append(wall(ev.host))
            finally:
                if default is None:
                    import re
                    text = open(os.path.join(os.path.dirname(_native.__file__), "csrc", "bn254_ws.h")).read()
                    default = int(re.search(r"#define POLY_EVAL_WAVE_MIN_COEFFS_DEFAULT (\d+)", text).group(1))
                eng.set_option(E.OPT_POLY_EVAL_WAVE_MIN_COEFFS, default)
            row = {"kind": "split_sweep", "coefficients": t, "x_bits": bits, "evaluations": q,
                   "by_wave_min": {str(w): dict(spread(ms[w]), layout="wave" if t >= w else "lane") for w in SWEEP_SPLITS},
                   "same_bytes": len(set(res.values())) == 1, "default_in_this_build": default, **box}
            print(json.dumps(row), file=out, flush=True)
            del ev


def unchanged_rows(eng, box, reps, out):
    lib, h = eng._lib, eng._h
    pts = commitments(eng, 171, 1)
    ks = np.random.default_rng(2).bytes(32 * 171)
    seg = (ctypes.c_uint64 * 2)(0, 171)
    o, s = ctypes.create_string_buffer(128), ctypes.create_string_buffer(1)

    def msm():
        _check(lib.bn254_batch_g2_msm(h, pts, ks, seg, 1, 1, o, s))
    n, t = 256, 171
    coeffs = [int.from_bytes(hashlib.sha256(b"c%d" % e).digest(), "big") % R for e in range(t)]
    sks = []
    for x in range(1, n + 1):
        v = 0
        for c in reversed(coeffs):
            v = (v * x + c) % R
        sks.append(v)
    pool, st = eng.batch_g2_mul(None, be(sks), n, reduce_scalar=True)
    assert st == bytes(n) and eng.register_keys(pool) == bytes(n)
    seed = hashlib.sha256(b"poly eval throughput").digest()
    pk, cst, bad = ctypes.create_string_buffer(128), ctypes.create_string_buffer(1), ctypes.c_uint32(0)

    def check():
        _check(lib.bn254_ctx_check_dealing(h, t, seed, 0, pk, cst, ctypes.byref(bad)))
    for fn in (msm, check, msm, check):
        fn()
    ms = {"msm": [], "check": []}
    for _ in range(reps):
        ms["msm"].append(wall(msm))
        ms["check"].append(wall(check))
    row = {"kind": "unchanged_calls", "g2_msm_171_terms_one_segment": spread(ms["msm"]), "check_dealing_256_171": spread(ms["check"]),
           "check_status": cst.raw[0], **box}
    print(json.dumps(row), file=out, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("shapes", nargs="*")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--msm-max-terms", type=int, default=1 << 20, help="run the g2_msm route in full up to this many terms, else on the first 256 keys, scaled")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--unchanged", action="store_true")
    ap.add_argument("--note", default=None, help="recorded with every line, e.g. which build ran")
    a = ap.parse_intermixed_args()
    out = open(a.out, "a") if a.out else sys.stdout
    shapes = [tuple(int(x) for x in s.split(":")) for s in a.shapes] or SHAPES
    eng = bn254_amd.Engine(0)
    ts = torch.cuda.Stream()
    stream = ctypes.c_void_p(ts.cuda_stream)
    box = {"device": torch.cuda.get_device_name(0), "lib_sha256": hashlib.sha256(open(_native.LIB_PATH, "rb").read()).hexdigest()[:16], "reps": a.reps}
    if a.note:
        box["note"] = a.note
    if a.unchanged:
        unchanged_rows(eng, box, a.reps, out)
        return
    if a.sweep:
        sweep_rows(eng, ts, stream, box, a.reps, out)
        return
    share_key_rows(eng, ts, stream, box, shapes, a.reps, a.msm_max_terms, out)
    dkg_row(eng, ts, stream, box, a.reps, out)


if __name__ == "__main__":
    main()
