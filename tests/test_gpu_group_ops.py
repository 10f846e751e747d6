"""The group operations and the Fq12 hook on the device against the model: every case of tests/group_cases.py through
Engine.batch_g1_add / g2_add / g2_mul / g1_sum / g2_sum and debug_fp12_op, outputs AND status bytes of every item of every batch,
bit-exact.  The same cases run on the host build of the same source (tests/test_hostsim_group.py); what only this file sees is the
wave vote of jac_add / jac_accumulate (BN_WAVE_ANY) — hence the wave layouts of the builder — and the device compiler.
Also here: the device-pointer entry points of the multiplications and of sign, and the operators of the typed API."""
import ctypes

import pytest

from oracle import bn254_model as m
from tests import group_cases as gc

pytestmark = pytest.mark.gpu
GROUPS = [gc.G1, gc.G2]


@pytest.fixture(scope="module")
def eng():
    import bn254_amd
    return bn254_amd.Engine(0)


def _split(b, size):
    return [b[i:i + size] for i in range(0, len(b), size)]


@pytest.mark.parametrize("G", GROUPS, ids=lambda G: G.name)
def test_additions_every_lane_of_every_layout(eng, G):
    add = eng.batch_g2_add if G is gc.G2 else eng.batch_g1_add
    for bi, batch in enumerate(gc.add_batches(G.name)):
        n = len(batch)
        out, st = add(b"".join(it["a"] for it in batch), b"".join(it["b"] for it in batch), n)
        out = _split(out, G.size)
        bad = [(lane, it["kind"], st[lane], it["status"]) for lane, it in enumerate(batch) if (st[lane], out[lane]) != (it["status"], it["want"])]
        assert not bad and len(st) == len(out) == n, (bi, n, bad[:6])


def test_g2_multiplication_raw_and_reduced(eng):
    mc = gc.g2_mul_cases()
    items, n = mc["items"], len(mc["items"])
    for reduce in (False, True):
        out, st = eng.batch_g2_mul(mc["points"], mc["scalars"], n, reduce_scalar=reduce)
        out = _split(out, 128)
        bad = [(i, it["kind"], hex(it["k"]), st[i]) for i, it in enumerate(items) if (st[i], out[i]) != (it["status"], it["want", reduce])]
        assert not bad and len(st) == len(out) == n, (reduce, bad[:6])


@pytest.mark.parametrize("G", GROUPS, ids=lambda G: G.name)
def test_segmented_sums(eng, G):
    fn = eng.batch_g2_sum if G is gc.G2 else eng.batch_g1_sum
    for call in gc.sum_calls(G.name):
        out, st = fn(call.points, call.seg_off)
        out = _split(out, G.size)
        n = len(call.segments)
        bad = [(i, len(call.segments[i]), call.notes.get(i), st[i], call.status[i]) for i in range(n) if (st[i], out[i]) != (call.status[i], call.want[i])]
        assert not bad and len(st) == len(out) == n, (call.name, bad[:6])


def test_fp12_ops_vs_model(eng):
    cases = gc.fp12_cases()
    for name, op in gc.FP12_OPS.items():
        mine = [cs for cs in cases if cs["op"] == name]
        assert mine
        a = b"".join(cs["a"] for cs in mine)
        b = b"".join(cs["b"] for cs in mine) if name == "mul" else None
        out = _split(eng.debug_fp12_op(op, a, b, len(mine)), 384)
        bad = [(i, cs["kind"]) for i, cs in enumerate(mine) if out[i] != cs["want"]]
        assert not bad and len(out) == len(mine), (name, bad[:6])


def test_device_pointer_multiplications_and_sign(eng):
    """bn254_batch_g1_mul_device / g2_mul_device / sign_device on a caller-owned stream equal the host-pointer calls on the same inputs (and, for
    G2, the model); a misaligned pointer is BN254_E_MISALIGNED, a null scalar or output pointer BN254_E_BAD_ARGUMENT, n = 0 succeeds and
    writes nothing."""
    import torch
    dev = torch.device("cuda", 0)
    L, h = eng._lib, eng._h
    mc = gc.g2_mul_cases()
    n = 130
    items = mc["items"][:n]
    pts2, ks = mc["points"][:128 * n], mc["scalars"][:32 * n]
    pool1 = [it["a"] for it in gc.add_batches("g1")[-1][:64]]
    pts1 = b"".join(pool1[i % 64] for i in range(n))
    msgs = [b"dev-sign-%d" % i * (1 + i % 3) for i in range(n)]
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)     # noqa: E731
    d_k, d_p1, d_p2 = up(ks), up(pts1), up(pts2)
    stream = torch.cuda.Stream(device=dev)
    for reduce in (False, True):
        for size, d_p, host, fn in ((64, d_p1, eng.batch_g1_mul(pts1, ks, n, reduce_scalar=reduce), eng.batch_g1_mul_device),
                                    (128, d_p2, eng.batch_g2_mul(pts2, ks, n, reduce_scalar=reduce), eng.batch_g2_mul_device)):
            d_out = torch.full((size * n,), 0xA5, dtype=torch.uint8, device=dev)
            d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
            with torch.cuda.stream(stream):
                fn(d_p.data_ptr(), d_k.data_ptr(), n, d_out.data_ptr(), d_st.data_ptr(), reduce_scalar=reduce, stream=stream.cuda_stream)
            stream.synchronize()
            assert (d_out.cpu().numpy().tobytes(), d_st.cpu().numpy().tobytes()) == host, (size, reduce)
            if size == 128:
                assert host == (b"".join(it["want", reduce] for it in items), bytes(it["status"] for it in items))
    # the G1 products against the model as well (the scalar acts mod r on G1, reduced or not)
    out1, st1 = eng.batch_g1_mul(pts1, ks, n)
    assert st1 == bytes(n)
    for i in range(0, n):
        if i % 7 == 0 or items[i]["k"] >= m.R:
            assert out1[64 * i:64 * i + 64] == gc.G1.enc(m.g1_mul(gc.G1.decode(pool1[i % 64])[1], items[i]["k"] % m.R)), i
    # sign: sk = the same scalars (Fr::from_slice reduces them)
    host = eng.batch_sign(msgs, ks)
    off, pos = [0], 0
    for msg in msgs:
        pos += len(msg)
        off.append(pos)
    d_msgs, d_off = up(b"".join(msgs)), torch.tensor(off, dtype=torch.int64, device=dev)
    d_sig = torch.full((64 * n,), 0xA5, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    with torch.cuda.stream(stream):
        eng.batch_sign_device(d_msgs.data_ptr(), d_off.data_ptr(), d_k.data_ptr(), n, d_sig.data_ptr(), d_st.data_ptr(), stream=stream.cuda_stream)
    stream.synchronize()
    assert (d_sig.cpu().numpy().tobytes(), d_st.cpu().numpy().tobytes()) == host and host[1] == bytes(n)
    for i in (0, 57, 129):
        assert host[0][64 * i:64 * i + 64] == gc.G1.enc(m.sign(msgs[i], items[i]["k"] % m.R))
    # argument checks: refused before any access, outputs untouched
    E_BAD, E_MIS = -10001, -10002
    d_out = torch.full((128 * n,), 0x5A, dtype=torch.uint8, device=dev)
    d_st = torch.full((n,), 0x5A, dtype=torch.uint8, device=dev)
    s = ctypes.c_void_p(stream.cuda_stream)
    vp = lambda t, o=0: ctypes.c_void_p(t.data_ptr() + o)      # noqa: E731
    for fn, d_p in ((L.bn254_batch_g1_mul_device, d_p1), (L.bn254_batch_g2_mul_device, d_p2)):
        assert fn(h, vp(d_p, 1), vp(d_k), n - 1, 0, vp(d_out), vp(d_st), s) == E_MIS
        assert fn(h, vp(d_p), vp(d_k, 2), n - 1, 0, vp(d_out), vp(d_st), s) == E_MIS
        assert fn(h, vp(d_p), vp(d_k), n - 1, 0, vp(d_out, 1), vp(d_st), s) == E_MIS
        assert fn(h, vp(d_p), None, n, 0, vp(d_out), vp(d_st), s) == E_BAD
        assert fn(h, vp(d_p), vp(d_k), n, 0, None, vp(d_st), s) == E_BAD
        assert fn(h, vp(d_p), vp(d_k), n, 0, vp(d_out), None, s) == E_BAD
        assert fn(h, vp(d_p), vp(d_k), 0, 0, vp(d_out), vp(d_st), s) == 0
    sg = L.bn254_batch_sign_device
    assert sg(h, vp(d_msgs), vp(d_off), vp(d_k, 1), n - 1, vp(d_out), vp(d_st), s) == E_MIS
    assert sg(h, vp(d_msgs), vp(d_off), vp(d_k), n - 1, vp(d_out, 3), vp(d_st), s) == E_MIS
    assert sg(h, vp(d_msgs), vp(d_off, 4), vp(d_k), n - 1, vp(d_out), vp(d_st), s) == E_MIS
    assert sg(h, vp(d_msgs), vp(d_off), None, n, vp(d_out), vp(d_st), s) == E_BAD
    assert sg(h, vp(d_msgs), vp(d_off), vp(d_k), n, None, vp(d_st), s) == E_BAD
    assert sg(h, vp(d_msgs), vp(d_off), vp(d_k), 0, vp(d_out), vp(d_st), s) == 0
    torch.cuda.synchronize()
    assert bool((d_out == 0x5A).all()) and bool((d_st == 0x5A).all())
    # the context still works
    assert eng.batch_g2_mul(pts2, ks, n) == (b"".join(it["want", False] for it in items), bytes(it["status"] for it in items))


def test_typed_api_operators_vs_model():
    """PublicKey / Signature __add__, __sub__, __neg__ (one-item batches: the n = 1 launch) on P + Q, P + P, P - P and the identity"""
    from bn254_amd.api import PublicKey, Signature
    for G, T in ((gc.G1, Signature), (gc.G2, PublicKey)):
        p, q = gc.chain(G, b"api", 2)
        P, Qp, O = T(G.enc(p)), T(G.enc(q)), T(G.zero)
        assert (P + Qp).raw == G.enc(G.add(p, q))
        assert (P + P).raw == G.enc(G.add(p, p)) != P.raw
        assert (P - P).raw == G.zero and (P + (-P)).raw == G.zero
        assert (P - Qp).raw == G.enc(G.add(p, G.neg(q)))
        assert (-P).raw == G.enc(G.neg(p)) and (-(-P)).raw == P.raw
        assert (O + P).raw == P.raw and (P + O).raw == P.raw and (P - O).raw == P.raw
        assert (O + O).raw == G.zero and (-O).raw == G.zero and (O - P).raw == G.enc(G.neg(p))
        assert ((P + P) - P).raw == P.raw
