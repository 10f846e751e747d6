"""bn254_batch_collect_keyed_bitmap's select step restated in a few lines (include/bn254_hip.h): which shares count, the rows, the counts.
Shared by tests/test_collect_keyed_bitmap.py (host compilation) and tests/test_gpu_collect_keyed_bitmap.py."""


def select(share_keys, share_status, sizes, tuple_status, bm_words):
    """-> (rows, counts, chosen): per tuple its bm_words bitmap words, its popcount, and the indices of the shares that are added — the FIRST
    status-0 share of every key (any other valid share of that key is the same point)"""
    rows, counts, chosen, at = [], [], [], 0
    for i, k in enumerate(sizes):
        row, pick = [0] * bm_words, []
        for s in range(at, at + k):
            j = share_keys[s]
            if tuple_status[i] != 2 and share_status[s] == 0 and j // 32 < bm_words and not (row[j // 32] >> (j % 32)) & 1:
                row[j // 32] |= 1 << (j % 32)
                pick.append(s)
        at += k
        rows.append(row)
        counts.append(len(pick))
        chosen.append(pick)
    return rows, counts, chosen


def aggregates(c, shares, chosen):
    """the oracle's g1_add over the chosen shares of every tuple (64 zero bytes = the identity)"""
    out = []
    for pick in chosen:
        acc = bytes(64)
        for s in pick:
            acc = c.g1_add(acc, shares[s])
        out.append(acc)
    return out
