"""bn254_batch_collect_keyed_bitmap_optimistic restated (include/bn254_hip.h, steps 1-7): the candidate sets, eligibility, the tuple check,
the fallback and the five outputs, over given decode / key / hash statuses and two callbacks — tuple_check(i, row, chosen) -> status of the
verify of tuple i's provisional sum, share_check(s) -> 0 or 9 for share s verified exactly.  oracle_checks builds both from the oracle's
hash_to_g1, g1_add, g2_add and pairing_check.  Shared by tests/test_collect_keyed_bitmap_optimistic.py (host compilation, and the model end
to end over the oracle) and tests/test_gpu_collect_keyed_bitmap_optimistic.py."""
from tests import collect_model

FINAL, CHECK, EXACT = 0, 1, 2
R = 0x30644E72E131A029B85045B68181585D2833E84879B9709143E1F593F0000001


def ranges(sizes):
    at, out = 0, []
    for k in sizes:
        out.append((at, at + k))
        at += k
    return out


def precheck(decode_status, share_keys, key_status, sizes, tuple_status, hash_status=None):
    """step 1 -> share statuses: the decode status, else 2 for a key index outside the set or the key's registration status, else the tuple's
    hash status; 2 for every share of a tuple the range rule refused (tuple_status 2)"""
    hash_status = tuple_status if hash_status is None else hash_status
    out = []
    for i, (lo, hi) in enumerate(ranges(sizes)):
        for s in range(lo, hi):
            st = 2 if tuple_status[i] == 2 else decode_status[s]
            if st == 0:
                st = 2 if share_keys[s] >= len(key_status) else key_status[share_keys[s]]
            if st == 0:
                st = hash_status[i]
            out.append(st)
    return out


def tuple_flags(share_keys, pre, sizes, min_tuple):
    """step 2 -> (flag, candidates) per tuple: FINAL with no candidate, EXACT with two candidates of one key or fewer than min_tuple, else CHECK"""
    out = []
    for lo, hi in ranges(sizes):
        cand = [s for s in range(lo, hi) if pre[s] == 0]
        named = [share_keys[s] for s in cand]
        if len(set(named)) != len(named):
            out.append((EXACT, cand))
        elif not cand:
            out.append((FINAL, cand))
        else:
            out.append((EXACT if len(cand) < min_tuple else CHECK, cand))
    return out


def collect(share_keys, pre, sizes, tuple_status, bm_words, min_tuple, tuple_check, share_check):
    """steps 2-6 -> dict(share_status, rows, counts, chosen, flags, verdicts, queue, hook).  chosen: the shares whose sum is the aggregate
    (tests/collect_model.py: aggregates); queue: the shares verified exactly, ascending; hook: what bn254_debug_collect_opt_last reports"""
    flags = tuple_flags(share_keys, pre, sizes, min_tuple)
    n = len(sizes)
    masked = [2 if tuple_status[i] == 2 else 0 for i in range(n)]
    rows, counts, chosen = collect_model.select(share_keys, pre, sizes, masked, bm_words)       # provisional; final for FINAL and passing tuples
    verdicts, exact = [None] * n, []
    for i, (flag, cand) in enumerate(flags):
        if flag == CHECK:
            verdicts[i] = tuple_check(i, rows[i], chosen[i])
        if flag == EXACT or (flag == CHECK and verdicts[i] != 0):
            exact.append(i)
    status, queue = list(pre), []
    for i in exact:
        for s in flags[i][1]:
            status[s] = share_check(s)
            queue.append(s)
    if exact:                                                                               # the exact rule again, for these tuples only
        only = [0 if i in exact and tuple_status[i] != 2 else 2 for i in range(n)]
        rows2, counts2, chosen2 = collect_model.select(share_keys, status, sizes, only, bm_words)
        for i in exact:
            rows[i], counts[i], chosen[i] = rows2[i], counts2[i], chosen2[i]
    checked = [i for i, (flag, _) in enumerate(flags) if flag == CHECK]
    hook = dict(checked=len(checked), passed=sum(1 for i in checked if verdicts[i] == 0), exact_tuples=len(exact), exact_shares=len(queue))
    return dict(share_status=status, rows=rows, counts=counts, chosen=chosen, flags=[f for f, _ in flags], verdicts=verdicts, queue=sorted(queue), hook=hook)


def oracle_checks(c, msgs, shares, share_keys, sizes, pks):
    """the two callbacks from the oracle alone: H(m) by hash_to_g1, sums by g1_add / g2_add, the verdicts by pairing_check (decode flags 0: an
    identity aggregate and an identity key sum are legitimate)"""
    neg_g2 = c.g2_mul(c.g2_generator(), (R - 1).to_bytes(32, "big"))
    h, tuple_of = [], []
    for i, (lo, hi) in enumerate(ranges(sizes)):
        st, pt, _ = c.hash_to_g1(msgs[i])
        h.append(pt if st == 0 else None)
        tuple_of += [i] * (hi - lo)

    def tuple_check(i, row, chosen):
        agg, key = bytes(64), bytes(128)
        for s in chosen:
            agg = c.g1_add(agg, shares[s])
            key = c.g2_add(key, pks[share_keys[s]])
        return c.pairing_check(h[i] + agg, key + neg_g2, 2)

    def share_check(s):
        return c.pairing_check(h[tuple_of[s]] + shares[s], pks[share_keys[s]] + neg_g2, 2)
    return tuple_check, share_check
