"""Time per call of bn254_batch_verify_device (256 keys) and of bn254_batch_hash_to_g1_device against the hash schedule
(BN254_OPT_HASH_SCHEDULE) and the width of the wide round (BN254_OPT_HASH_WIDE_WIDTH), one JSON line per point; schedule 0 is what the
library picks.  With HASH_SWEEP_PLAIN=1 no option is set (a library that predates them, loaded through BN254_LIB).
  python tools/hash_schedule_sweep.py [sizes, default 8192,16385,32768,65536,131072,262144] [steps, default 15]"""
import json, os, sys, statistics
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bn254_amd
from bn254_amd import engine as E
from tests.datagen import D, sk_bytes

sizes = [int(x) for x in (sys.argv[1] if len(sys.argv) > 1 else "8192,16385,32768,65536,131072,262144").split(",")]
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 15
has_opts = os.environ.get("HASH_SWEEP_PLAIN", "") == ""
eng = bn254_amd.Engine(0)
nmax = max(sizes)
pool = 256
sks = [sk_bytes(j) for j in range(pool)]
pk, st = eng.batch_g2_mul(None, b"".join(sks), pool, reduce_scalar=True)
msgs = [D("sweep", i) for i in range(nmax)]
sigs, st = eng.batch_sign(msgs, b"".join(sks[i % pool] for i in range(nmax)))
dev = "cuda:0"
d_msgs = torch.frombuffer(bytearray(b"".join(msgs)), dtype=torch.uint8).to(dev)
d_off = torch.arange(0, 32 * (nmax + 1), 32, dtype=torch.int64, device=dev)
d_sigs = torch.frombuffer(bytearray(sigs), dtype=torch.uint8).to(dev)
d_pks = torch.frombuffer(bytearray(b"".join(pk[128 * (i % pool):128 * (i % pool) + 128] for i in range(nmax))), dtype=torch.uint8).to(dev)
d_st = torch.zeros(nmax, dtype=torch.uint8, device=dev)
d_pts = torch.zeros(nmax * 64, dtype=torch.uint8, device=dev)

def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize(); eng.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        eng.synchronize()
        b.record(); b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts)

s = torch.cuda.current_stream().cuda_stream
for n in sizes:
    cfgs = [(0, 0), (1, 0)] + [(2, w) for w in (4, 5, 6, 8)] + [(0, 0), (1, 0)] if has_opts else [(None, None)]
    ref = None
    for sched, w in cfgs:
        if has_opts:
            eng.set_option(E.OPT_HASH_SCHEDULE, sched); eng.set_option(E.OPT_HASH_WIDE_WIDTH, w)
        v = timed(lambda: eng.batch_verify_device(d_msgs.data_ptr(), d_off.data_ptr(), d_sigs.data_ptr(), d_pks.data_ptr(), n, d_st.data_ptr(), flags=0, stream=s))
        st_now = bytes(d_st[:n].cpu().numpy())
        ref = ref or st_now
        h = timed(lambda: eng.batch_hash_to_g1_device(d_msgs.data_ptr(), d_off.data_ptr(), n, d_pts.data_ptr(), d_st.data_ptr(), None, stream=s))
        print(json.dumps(dict(n=n, schedule=sched, w0=w, verify_ms_median=round(v[0], 4), verify_ms_min=round(v[1], 4), hash_ms_median=round(h[0], 4), hash_ms_min=round(h[1], 4), same_status=st_now == ref, ok=st_now.count(0))), flush=True)
