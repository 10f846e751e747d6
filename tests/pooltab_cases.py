"""Pools for the subset-sum tables of the aggregate verify (bn254_amd/csrc/bn254_pooltab.h), and the tables they must give, from the oracle
alone: every entry is the sum (c_oracle.g1_add / g2_add) of the signers its mask selects; a signer that is missing, refused or the identity
counts as the identity.  M = 2 messages (m = 1 exercises every m * groups stride), S = 5 (one partial window), 8, 16, 17 (a third window of
one key; a last chunk without a second half) and 43 (6 windows, 3 chunks, 11 quads, 22 pairs, the last of each partial).

Signer j holds the secret key sk_j: pk_j = sk_j G2, sig[m][j] = sk_j H(m), so ONE relation between secret keys plants the same relation in
the key tables and in both messages' signature tables.  The S = 43 pool (PLANTED below) puts equal and opposite points wherever two operands
of a builder meet, and makes sums equal to keys, to minus keys and to other sums, so that the widening's test x_B = x_A compares a
weakly reduced chord result with a decoded point, and two chord results with each other.  exceptional_counts() says, from the secret keys
alone, how many (hi, lo) entries of every widening stage meet equal and how many opposite operands; the tests assert each is at least 1.

Shared by tests/test_aggregate_pool_tables.py (host compilation) and tests/test_gpu_aggregate_pool_tables.py (device tables read back)."""
import functools
import random

R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001
M = 2
SIZES = (5, 8, 16, 17, 43)
MESSAGES = [b"pooltab/message-%d" % m for m in range(M)]
G1_ID, G2_ID = bytes(64), bytes(128)

# table -> (the context's pool index, signers per window, 1 for G2); the signature tables exist per message
TABLES = {"T8k": (3, 8, 1), "T2": (7, 2, 0), "T4": (4, 4, 0), "T8s": (6, 8, 0), "T16": (5, 16, 1)}

# S = 43.  Pairs (2j, 2j + 1), quads 4j .. 4j + 3, windows 8j .. 8j + 7, chunks 16j .. 16j + 15.  (signer, expression over earlier signers)
IDENTITY_SIGNER, BAD_KEY_SIGNER, BAD_SIG_SIGNER, BAD_SIG_MSG = 34, 35, 36, 1
PLANTED = [
    (1, lambda k: k[0]),                       # the two signers of pair 0 are equal: its T2 sum is a doubling
    (3, lambda k: -k[2]),                      # ... of pair 1 opposite: its T2 sum is the identity
    (6, lambda k: k[4]),                       # the two pairs of quad 1 hold equal points (T2 -> T4)
    (7, lambda k: -k[5]),                      # ... and opposite ones
    (9, lambda k: k[5]),                       # the two windows of chunk 0 hold equal points (T8 -> T16) — and, with 7, opposite ones
    (10, lambda k: k[8] + k[9]),               # T2 -> T4: the sum of pair 4 equals a key of pair 5
    (11, lambda k: -(k[8] + k[9])),            # ... and minus a key of pair 5
    (12, lambda k: k[0] + k[2]),               # T8 -> T16: a sum inside window 0 equals a key of window 1
    (13, lambda k: -(k[4] + k[5])),            # ... and minus a key of window 1
    (15, lambda k: k[12] + k[13] - k[14]),     # T2 -> T4: the sums of the two pairs of quad 3 are equal
    (20, lambda k: k[16]),                     # the two quads of window 2 hold equal points (T4 -> T8)
    (21, lambda k: -k[17]),                    # ... and opposite ones
    (22, lambda k: k[16] + k[18]),             # T4 -> T8: a T4 entry built by a chord (signers of both pairs of quad 4) equals a signer of quad 5
    (23, lambda k: -(k[17] + k[19])),          # ... and minus a signer of quad 5
    (29, lambda k: k[24] + k[26] - k[28]),     # T4 -> T8: a chord-built sum of quad 6 equals the pair sum of quad 7
    (31, lambda k: k[16] + k[17] - k[30]),     # T8 -> T16: a sum of window 2 equals a sum of window 3
    (32, lambda k: k[0]),                      # equal and opposite ACROSS chunks: they meet in no table
    (33, lambda k: -k[2]),
    (IDENTITY_SIGNER, lambda k: 0),            # an identity key with identity signatures
]


def secret_keys(S):
    rnd = random.Random(20261018 + S)
    k = [rnd.randrange(1, R) for _ in range(S)]
    if S == 43:
        for j, f in PLANTED:
            k[j] = f(k) % R
    return k


def neg_scalar(x):
    return (R - x) % R


class Pool:
    """the byte pools of one size, the decode statuses the oracle gives their entries, and which signers count in which table"""

    def __init__(self, c, S):
        self.S, self.sks = S, secret_keys(S)
        g2 = c.g2_generator()
        self.h = []
        for msg in MESSAGES:
            st, hm, _ = c.hash_to_g1(msg)
            assert st == 0
            self.h.append(hm)
        pks = [c.g2_mul(g2, k.to_bytes(32, "big")) if k else G2_ID for k in self.sks]
        sigs = [[c.g1_mul(self.h[m], k.to_bytes(32, "big")) if k else G1_ID for k in self.sks] for m in range(M)]
        if S == 43:
            pks[BAD_KEY_SIGNER] = pks[BAD_KEY_SIGNER][:127] + bytes([pks[BAD_KEY_SIGNER][127] ^ 1])                    # off the curve: status 4
            s = sigs[BAD_SIG_MSG][BAD_SIG_SIGNER]
            sigs[BAD_SIG_MSG][BAD_SIG_SIGNER] = s[:63] + bytes([s[63] ^ 1])
        self.pks, self.sigs = pks, sigs
        self.pk_st = [c.g2_validate(p, 0) for p in pks]
        self.sig_st = [[c.g1_validate(p, 0) for p in row] for row in sigs]
        if S == 43:
            assert self.pk_st[BAD_KEY_SIGNER] == 4 and self.sig_st[BAD_SIG_MSG][BAD_SIG_SIGNER] == 4 and sum(self.pk_st) == 4
            assert pks[IDENTITY_SIGNER] == G2_ID and all(sigs[m][IDENTITY_SIGNER] == G1_ID for m in range(M))
        self.pk_pool = b"".join(pks)
        self.sig_pool = b"".join(b"".join(row) for row in sigs)
        self.n_groups = (S + 7) // 8
        self.groups4, self.groups2, self.n_chunks = 2 * self.n_groups, 4 * self.n_groups, (self.n_groups + 1) // 2

    # what signer j contributes: its point and its secret key, or the identity and 0
    def key_point(self, j):
        return self.pks[j] if j < self.S and self.pk_st[j] == 0 else G2_ID

    def key_scalar(self, j):
        return self.sks[j] if j < self.S and self.pk_st[j] == 0 else 0

    def sig_point(self, m, j):
        return self.sigs[m][j] if j < self.S and self.sig_st[m][j] == 0 else G1_ID

    def sig_scalar(self, m, j):
        return self.sks[j] if j < self.S and self.sig_st[m][j] == 0 else 0

    def windows(self, table):
        """-> the number of windows of a table (per message for the signature tables)"""
        return {"T8k": self.n_groups, "T2": self.groups2, "T4": self.groups4, "T8s": self.n_groups, "T16": self.n_chunks}[table]

    def decoded_flags(self):
        """-> (flags of the decoded key pool, of the decoded signature pool): decode status | 0x80 for an identity entry"""
        fk = bytes(st | (0x80 if st == 0 and p == G2_ID else 0) for p, st in zip(self.pks, self.pk_st))
        fs = bytes(st | (0x80 if st == 0 and p == G1_ID else 0) for m in range(M) for p, st in zip(self.sigs[m], self.sig_st[m]))
        return fk, fs


@functools.lru_cache(maxsize=None)
def pool(S):
    from oracle import c_oracle
    return Pool(c_oracle, S)


def _subset_sums(add, zero, points):
    """-> the 2^W sums of the subsets of `points` (bit b selects points[b]), one oracle addition per entry that needs one"""
    out = [zero] * (1 << len(points))
    for mask in range(1, len(out)):
        low = (mask & -mask).bit_length() - 1
        rest, p = out[mask & (mask - 1)], points[low]
        out[mask] = rest if p == zero else p if rest == zero else add(rest, p)
    return out


@functools.lru_cache(maxsize=None)
def expected(S, table, window, m=0):
    """-> (points, flags) of window `window` of a table (of message m for the signature tables), as the debug hook hands entries out: canonical
    bytes, zeros and flag 0x80 for the identity"""
    from oracle import c_oracle as c
    P = pool(S)
    _, W, g2 = TABLES[table]
    if g2:
        sums = _subset_sums(c.g2_add, G2_ID, [P.key_point(W * window + b) for b in range(W)])
        zero = G2_ID
    else:
        sums = _subset_sums(c.g1_add, G1_ID, [P.sig_point(m, W * window + b) for b in range(W)])
        zero = G1_ID
    return b"".join(sums), bytes(0x80 if s == zero else 0 for s in sums)


def entry_base(S, table, window, m=0):
    """-> the index of mask 0 of that window in the table"""
    P = pool(S)
    W = TABLES[table][1]
    return ((m * P.windows(table) if not TABLES[table][2] else 0) + window) << W


def scalars(S, table, window, m=0):
    """-> the 2^W secret-key sums mod R behind a window's entries (0: the identity)"""
    P = pool(S)
    _, W, g2 = TABLES[table]
    ks = [P.key_scalar(W * window + b) if g2 else P.sig_scalar(m, W * window + b) for b in range(W)]
    out = [0] * (1 << W)
    for mask in range(1, len(out)):
        out[mask] = (out[mask & (mask - 1)] + ks[(mask & -mask).bit_length() - 1]) % R
    return out


STAGES = {"T2->T4": ("T2", "T4"), "T4->T8": ("T4", "T8s"), "T8->T16": ("T8k", "T16")}


def exceptional_counts(S):
    """-> {stage: (equal, opposite)}: the (hi, lo) entries of every widening stage — all windows, both messages — whose operands
    src[2k][lo] and src[2k + 1][hi] are both not the identity and are equal / opposite points, from the secret keys alone"""
    P = pool(S)
    out = {}
    for stage, (src, dst) in STAGES.items():
        eq = op = 0
        for m in range(1 if TABLES[src][2] else M):
            for k in range(P.windows(dst)):
                if 2 * k + 1 >= P.windows(src):
                    continue
                lo, hi = scalars(S, src, 2 * k, m), scalars(S, src, 2 * k + 1, m)
                hi_nz = {}
                for a in hi:
                    if a:
                        hi_nz[a] = hi_nz.get(a, 0) + 1
                for b in lo:
                    if b:
                        eq += hi_nz.get(b, 0)
                        op += hi_nz.get(neg_scalar(b), 0)
        out[stage] = (eq, op)
    return out


def pair_counts(S):
    """-> (doublings, cancellations) among the pairs of consecutive signers, over both messages: what the T2 builder's one addition meets"""
    P = pool(S)
    dbl = can = 0
    for m in range(M):
        for g in range(P.groups2):
            a, b = P.sig_scalar(m, 2 * g), P.sig_scalar(m, 2 * g + 1)
            if a and b:
                dbl += a == b
                can += a == neg_scalar(b)
    return dbl, can


def walk_tuples(S, window):
    """256 tuples that enumerate every mask of one 8-signer window (bit b names signer 8 * window + b, which may not exist: the oracle
    says IndexOutOfBounds too), each followed by eight signers of other windows so that every wave's longest list exceeds the number of
    windows and the kernel reads the tables; messages alternate.  -> (tuple_msg, signer_lists)"""
    P = pool(S)
    tail = [s for s in (16, 18, 19, 24, 25, 27, 30, 2 if window else 40) if s < S and s // 8 != window]
    lists = [[8 * window + b for b in range(8) if (mask >> b) & 1] + tail for mask in range(256)]
    assert all(len(lst) > P.n_groups for lst in lists[255:]) and len(tail) > P.n_groups
    return [mask % M for mask in range(256)], lists
