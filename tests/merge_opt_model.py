"""bn254_batch_merge_keyed_bitmap_optimistic restated (include/bn254_hip.h, steps 1-7): the candidates, the provisional first fit with its
overlap report, the per-tuple flag, the tuple check, the fallback and the six outputs, over given decode / rule-2 / hash statuses and two
callbacks — tuple_check(i, row, taken_parts) -> status of the verify of tuple i's provisional sum against its union row, part_check(p) -> 0
or 9 for partial p verified exactly.  oracle_checks builds both from the oracle's hash_to_g1, g1_add, g2_add and pairing_check.  Shared by
tests/test_merge_keyed_bitmap_optimistic.py (host compilation, and the model end to end over the oracle) and
tests/test_gpu_merge_keyed_bitmap_optimistic.py."""
from tests import merge_model

FINAL, CHECK, EXACT = 0, 1, 2
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def ranges(sizes):
    at, out = 0, []
    for k in sizes:
        out.append((at, at + k))
        at += k
    return out


def rule2(row, key_status):
    """the status of the lowest bad bit of a row: 2 for a bit beyond the key set, else the key's non-zero registration status; 0: none"""
    for w, word in enumerate(row):
        for b in range(32):
            if (word >> b) & 1:
                j = 32 * w + b
                if j >= len(key_status):
                    return 2
                if key_status[j]:
                    return key_status[j]
    return 0


def precheck(decode_status, part_rows, key_status, sizes, tuple_status, hash_status=None):
    """step 1 -> partial statuses: sigma's decode status, else rule 2 of its row, else the tuple's hash status; 2 for every partial of a
    tuple the range rule refused (tuple_status 2)"""
    hash_status = tuple_status if hash_status is None else hash_status
    out = []
    for i, (lo, hi) in enumerate(ranges(sizes)):
        for p in range(lo, hi):
            st = 2 if tuple_status[i] == 2 else decode_status[p]
            if st == 0:
                st = rule2(part_rows[p], key_status)
            if st == 0:
                st = hash_status[i]
            out.append(st)
    return out


def tuple_flags(part_rows, pre, sizes, tuple_status, bm_words):
    """steps 2-3 -> (flag, candidates) per tuple: FINAL with no candidate (however empty the row), EXACT when first fit refuses a candidate,
    else CHECK"""
    _, _, taken = merge_model.select(part_rows, pre, sizes, tuple_status, bm_words)
    out = []
    for i, (lo, hi) in enumerate(ranges(sizes)):
        cand = [p for p in range(lo, hi) if pre[p] == 0 and tuple_status[i] != 2]
        if any(not taken[p] for p in cand):
            out.append((EXACT, cand))
        else:
            out.append((CHECK if cand else FINAL, cand))
    return out


def merge(part_rows, pre, sizes, tuple_status, bm_words, tuple_check, part_check, routed=True):
    """steps 2-7 -> dict(part_status, taken, rows, counts, flags, verdicts, queue, hook).  routed False: the whole call is the exact merge
    (step 7) — every candidate by part_check, the hook all zero.  queue: the partials verified exactly, ascending; hook: what
    bn254_debug_merge_opt_last reports"""
    n = len(sizes)
    if not routed:
        status = [st or part_check(p) for p, st in enumerate(pre)]
        rows, counts, taken = merge_model.select(part_rows, status, sizes, tuple_status, bm_words)
        return dict(part_status=status, taken=taken, rows=rows, counts=counts, flags=[None] * n, verdicts=[None] * n, queue=[],
                    hook=dict(checked=0, passed=0, exact_tuples=0, exact_parts=0))
    flags = tuple_flags(part_rows, pre, sizes, tuple_status, bm_words)
    rows, counts, taken = merge_model.select(part_rows, pre, sizes, tuple_status, bm_words)      # provisional; final for FINAL and passing tuples
    verdicts, exact = [None] * n, []
    rng = ranges(sizes)
    for i, (flag, cand) in enumerate(flags):
        if flag == CHECK:
            verdicts[i] = tuple_check(i, rows[i], [p for p in range(*rng[i]) if taken[p]])
        if flag == EXACT or (flag == CHECK and verdicts[i] != 0):
            exact.append(i)
    status, queue = list(pre), []
    for i in exact:
        for p in flags[i][1]:
            status[p] = part_check(p)
            queue.append(p)
    if exact:                                                                                   # the exact rule again, for these tuples only
        only = [0 if i in exact and tuple_status[i] != 2 else 2 for i in range(n)]
        rows2, counts2, taken2 = merge_model.select(part_rows, status, sizes, only, bm_words)
        for i in exact:
            rows[i], counts[i] = rows2[i], counts2[i]
            taken[rng[i][0]:rng[i][1]] = taken2[rng[i][0]:rng[i][1]]
    checked = [i for i, (flag, _) in enumerate(flags) if flag == CHECK]
    hook = dict(checked=len(checked), passed=sum(1 for i in checked if verdicts[i] == 0), exact_tuples=len(exact), exact_parts=len(queue))
    return dict(part_status=status, taken=taken, rows=rows, counts=counts, flags=[f for f, _ in flags], verdicts=verdicts, queue=sorted(queue), hook=hook)


def oracle_checks(c, msgs, parts, part_rows, sizes, pks):
    """the two callbacks from the oracle alone: H(m) by hash_to_g1, sums by g1_add / g2_add over the set bits of a row, the verdicts by
    pairing_check (decode flags 0: an identity aggregate and an identity key sum are legitimate)"""
    neg_g2 = c.g2_mul(c.g2_generator(), (R - 1).to_bytes(32, "big"))
    h, tuple_of = [], []
    for i, (lo, hi) in enumerate(ranges(sizes)):
        st, pt, _ = c.hash_to_g1(msgs[i])
        h.append(pt if st == 0 else None)
        tuple_of += [i] * (hi - lo)

    def key_of(row):
        key = bytes(128)
        for j in range(32 * len(row)):
            if (row[j // 32] >> (j % 32)) & 1:
                key = c.g2_add(key, pks[j])
        return key

    def tuple_check(i, row, taken_parts):
        agg = bytes(64)
        for p in taken_parts:
            agg = c.g1_add(agg, parts[p])
        return c.pairing_check(h[i] + agg, key_of(row) + neg_g2, 2)

    def part_check(p):
        return c.pairing_check(h[tuple_of[p]] + parts[p], key_of(part_rows[p]) + neg_g2, 2)
    return tuple_check, part_check
