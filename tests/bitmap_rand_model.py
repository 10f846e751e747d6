"""A model of the G1 side of bn254_batch_verify_keyed_bitmap_randomized (include/bn254_hip.h), from the header's words alone:
r_i with hashlib, points and sums with the oracle's g1_mul / g1_add.  Used by the GPU tests (what bn254_debug_bitmap_rand_last and
bn254_debug_bitmap_rand_sums must report) and, without a device, by tests/test_verify_keyed_bitmap_randomized.py (the conditions the GPU
tests' plans must meet)."""
import hashlib

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
LAMBDA = 0xb3c4d79d41a917585bfc41088d8daaa78b17ea66b99c90dd        # BN254_FLAG_RAND_GLV's eigenvalue (include/bn254_hip.h)
O = bytes(64)


def r_model(seed, i, mode):
    """SHA-256(seed32 || le64(i)) read little-endian, 16 bytes (mode 1, RAND64: 8), 0 -> 1; mode 2, GLV: k1 + k2 lambda with k1, k2 the
    two 64-bit halves"""
    d = hashlib.sha256(seed + i.to_bytes(8, "little")).digest()
    if mode == 2:
        k1, k2 = int.from_bytes(d[:8], "little"), int.from_bytes(d[8:16], "little")
        return (k1 or (0 if k2 else 1)) + k2 * LAMBDA
    return int.from_bytes(d[:8 if mode == 1 else 16], "little") or 1


def held(bits, bm_words):
    """the set bits a bitmap of bm_words words can hold"""
    return sorted(j for j in set(bits) if j // 32 < bm_words)


def groups_of(n, at_check, G):
    """group -> its tuples at the check (tuple i belongs to group i // G)"""
    out = {}
    for i in range(n):
        if at_check[i]:
            out.setdefault(i // G, []).append(i)
    return out


def grouping(bitsets, at_check, bad, key_inf, G, bm_words):
    """what bn254_debug_bitmap_rand_last must report (less `ran`): groups at the check, table pairs of all group checks (one per key with a
    contributor that is not a registered identity, and S_g's), failed groups (of two or more tuples, holding a bad one), tuples re-checked,
    groups of one"""
    n = len(bitsets)
    members = groups_of(n, at_check, G)
    pairs = failed = rechecked = single = 0
    for g, idx in members.items():
        keys = {j for i in idx for j in held(bitsets[i], bm_words) if not key_inf[j]}
        pairs += len(keys) + 1
        if len(idx) == 1:
            single += 1
        elif any(bad[i] for i in idx):
            failed += 1
            rechecked += len(idx)
    return dict(groups=len(members), table_pairs=pairs, failed_groups=failed, rechecked=rechecked, single_groups=single)


def model(c, hs, sigs, bitsets, at_check, key_inf, seed, mode, G, bm_words, index_base=0):
    """per group (ceil(n / G) of them): dict(nagg, s = S_g, pairs = [(key, T_{g,key})] in key order over the keys with a contributor, zeros =
    the identity).  hs[i] = H(m_i) (read for tuples at the check only)."""
    n = len(sigs)
    members = groups_of(n, at_check, G)
    out = []
    for g in range((n + G - 1) // G):
        idx = members.get(g, [])
        s, t = O, {}
        for i in idx:
            r = 1 if len(idx) == 1 else r_model(seed, index_base + i, mode)
            k = (r % R).to_bytes(32, "big")
            s = c.g1_add(s, c.g1_mul(sigs[i], k) if sigs[i] != O else O)
            rh = c.g1_mul(hs[i], k)
            for j in held(bitsets[i], bm_words):
                if not key_inf[j]:
                    t[j] = c.g1_add(t.get(j, O), rh)
        out.append(dict(nagg=len(idx), s=s, pairs=sorted(t.items())))
    return out


def fold_model(c, buckets):
    """the eight key sums of one window from its byte buckets {v: point}: T_b = sum of B[v] over the v with bit b"""
    out = []
    for b in range(8):
        t = O
        for v, p in sorted(buckets.items()):
            if (v >> b) & 1:
                t = c.g1_add(t, p)
        out.append(t)
    return out


# ---- the plans of the GPU tests, as far as no device is needed: set bits and, for the ragged plan, what is done to a member ---------------
N_GOOD = 40
K_OFF_TWIST, K_OFF_SUB, K_BIG, K_IDENT, K_DUP0, K_NEG1 = range(N_GOOD, N_GOOD + 6)
N_KEYS = N_GOOD + 6


def passing_sets(n):
    """popcounts 0 .. all in turn, the identity key, the doubled key and the negation among them"""
    import random
    rnd = random.Random(5)
    sets = []
    for i in range(n):
        pop = (0, 1, 2, 8, 9, 17, 31, N_GOOD)[i % 8]
        s = sorted(rnd.sample(range(N_GOOD), pop))
        if i % 11 == 3:
            s.append(K_IDENT)
        if i % 13 == 5:
            s.append(K_DUP0)
        if i % 17 == 7:
            s.append(K_NEG1)
        sets.append(s)
    return sets


def ragged_sets():
    """90 members (set bits over the signing keys, kind): kind "ok", or off the check: "refused" (a refused key's bit is added), "oob" (a
    bit above the set), "curve" (sigma off the curve)"""
    import random
    rnd = random.Random(3)
    out = []
    for i in range(90):
        pop = (0, 1, 3, 8, 9, 16, N_GOOD)[i % 7]
        s = sorted(rnd.sample(range(N_GOOD), pop))
        if i % 9 == 4:
            s += [K_IDENT]
        if i % 10 == 6:
            s += [K_DUP0, K_NEG1]
        out.append((s, ["refused", "oob", "curve"][(i // 8) % 3] if i % 8 == 5 else "ok"))
    return out
