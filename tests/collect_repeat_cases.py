"""Tuples over a key set that repeats keys, for the sums of bn254_batch_collect_keyed_bitmap (bn254_amd/csrc/bn254_collect.h: cl_step,
cl_wave_partial, cl_tree_level): 256 registered keys, indices 0 .. 127 all ONE key pk_A, 128 .. 191 all its negation, 192 .. 255 the 64
distinct keys B_j.  With sigma = a H(m) a valid share of an index below 128 is sigma, of 128 .. 191 it is -sigma: additions of equal and of
opposite points are the normal path.  A tuple is a list of (kind, key index): "A" sigma, "N" -sigma, "B" the share of B_(key - 192), "W"
sigma + G1 (status 9: not counted, added as the identity).  In the wave layout share k of a tuple is lane k % 64's, and the tree folds slot
t + stride into slot t for stride 32, 16, .. 1.
Shared by tests/test_collect_keyed_bitmap.py (host compilation, statuses given) and tests/test_gpu_collect_repeated_keys.py."""

N_A, N_NEG, N_B = 128, 64, 64
K_NEG, K_B = N_A, N_A + N_NEG
N_KEYS = N_A + N_NEG + N_B
BM = N_KEYS // 32
STRIDES = [1, 2, 4, 8, 16, 32]
FIRST = {1: 0, 2: 1, 4: 2, 8: 5, 16: 11, 32: 19}          # the position p < stride of a level's first valid share; the other is p + stride


def _a(p):
    return ("A", p)


def _n(p):
    return ("N", K_NEG + p % N_NEG)


def _w(p):
    return ("W", p % N_A)


def shapes64():
    """the 64-share shapes -> [(name, shares)]"""
    out = [("double_every_level", [_a(p) for p in range(64)])]
    for s in STRIDES:
        p = FIRST[s]
        assert p < s
        out.append(("double_at_%d" % s, [_a(q) if q in (p, p + s) else _w(q) for q in range(64)]))
        out.append(("cancel_at_%d" % s, [_a(q) if q == p else _n(q) if q == p + s else _w(q) for q in range(64)]))
    out.append(("cancel_first_level", [_a(q) if q < 32 else _n(q) for q in range(64)]))
    out.append(("cancel_last_level", [_n(q) if q % 2 else _a(q) for q in range(64)]))
    # one vote at stride 32: slots 0..7 double, 8..15 add ordinarily, 16..23 cancel, 24..31 add the identity to the identity
    mixed = []
    for q in range(64):
        kind = (q % 32) // 8
        mixed.append(("B", K_B + (q % 8) + 8 * (q // 32)) if kind == 1 else _w(q) if kind == 3 else _n(q) if (kind == 2 and q >= 32) else _a(q))
    out.append(("mixed_vote", mixed))
    return out


def shapes():
    """-> [(name, shares)]: the 64-share shapes; each again behind one share (65) and between two (66), so that position q is lane q + 1's
    and the last one lane 0's second step; 128 shares (every lane adds sigma to sigma, then the tree doubles); 130 shares, lanes 0 and 1
    walking sigma, sigma, sigma and sigma, -sigma, sigma"""
    base = shapes64()
    out = list(base)
    for name, sh in base:
        out.append((name + "+1", [_w(77)] + sh))
        out.append((name + "+2", [("B", K_B + 63)] + sh + [("B", K_B + 62)]))
    out.append(("own_stride_128", [_a(p) for p in range(128)]))
    # 130 shares: positions 2 and 3 are B shares, which leaves the indices 2 and 3 for positions 128 and 129
    sss = [_a(p) for p in range(128)] + [_a(2), _a(3)]
    sss[2], sss[3] = ("B", K_B), ("B", K_B + 1)
    out.append(("own_stride_sss", sss))
    # ... and positions 64, 65 -sigma, which leaves the indices 64 and 65
    sns = [_a(p) for p in range(128)] + [_a(64), _a(65)]
    sns[64], sns[65] = _n(0), _n(1)
    out.append(("own_stride_sns", sns))
    for name, sh in out:
        valid = [k for kind, k in sh if kind != "W"]
        assert len(valid) == len(set(valid)), name                     # every valid share of a tuple names an index of its own: all count
        assert all((kind in "AW" and k < N_A) or (kind == "N" and K_NEG <= k < K_B) or (kind == "B" and K_B <= k < N_KEYS) for kind, k in sh), name
    return out


def plant(cases, point):
    """point(i, kind, key) -> the 64 bytes of a share of tuple i.  -> (shares, keys, sizes, statuses): flat, the statuses planted"""
    shares, keys, sizes, status = [], [], [], []
    for i, (_, sh) in enumerate(cases):
        sizes.append(len(sh))
        for kind, key in sh:
            shares.append(point(i, kind, key))
            keys.append(key)
            status.append(9 if kind == "W" else 0)
    return shares, keys, sizes, status


def net(shares):
    """-> (multiple of sigma, {j: 1 for the B_j that count}, count): what a tuple's aggregate and count must be"""
    m = sum(1 if kind == "A" else -1 for kind, _ in shares if kind in "AN")
    return m, sorted(k - K_B for kind, k in shares if kind == "B"), sum(1 for kind, _ in shares if kind != "W")
