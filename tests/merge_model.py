"""bn254_batch_merge_keyed_bitmap's select step restated in a few lines (include/bn254_hip.h): FIRST FIT in the caller's order — a partial is
taken iff its status is 0 and its row is disjoint from the union of the rows taken before it in its tuple.
Shared by tests/test_merge_keyed_bitmap.py (host compilation) and tests/test_gpu_merge_keyed_bitmap.py."""


def select(part_rows, part_status, sizes, tuple_status, bm_words):
    """part_rows: one list of bm_words words per partial.  -> (rows, counts, taken): per tuple its bm_words union words and their popcount,
    per partial 1 or 0"""
    rows, counts, taken, at = [], [], [], 0
    for i, k in enumerate(sizes):
        row = [0] * bm_words
        for p in range(at, at + k):
            take = tuple_status[i] != 2 and part_status[p] == 0 and not any(a & b for a, b in zip(row, part_rows[p]))
            if take:
                row = [a | b for a, b in zip(row, part_rows[p])]
            taken.append(int(take))
        at += k
        rows.append(row)
        counts.append(sum(bin(w).count("1") for w in row))
    return rows, counts, taken


def aggregates(c, parts, sizes, taken):
    """the oracle's g1_add over the taken partials of every tuple (64 zero bytes = the identity)"""
    out, at = [], 0
    for k in sizes:
        acc = bytes(64)
        for p in range(at, at + k):
            if taken[p]:
                acc = c.g1_add(acc, parts[p])
        at += k
        out.append(acc)
    return out
