"""bn254_batch_threshold_combine_keyed_optimistic restated (include/bn254_hip.h, steps 1-6): the candidate sets, the tuples that go the exact
way at once, S' and its interpolation, the tuple check under the group key, the fallback and the five outputs, over given pre-check
statuses and two callbacks — tuple_check(i, chosen) -> status of the verify of tuple i's interpolated signature under the group key, chosen =
[(key, share index)] in key order; share_check(s) -> 0 or 9 for share s verified exactly.  The pre-check is tests/collect_opt_model.py's
(rules 1-3 are the optimistic collect's), the exact rule tests/threshold_model.py's.  Shared by tests/test_threshold_opt_cases.py (host
compilation) and tests/test_gpu_threshold_optimistic.py.  Nothing here comes from the code under test."""
from tests import threshold_model as TM
from tests.collect_opt_model import FINAL, CHECK, EXACT, precheck, ranges   # noqa: F401  (re-exported for the tests)


def row_of(keys, bm_words):
    row = [0] * bm_words
    for j in keys:
        row[j // 32] |= 1 << (j % 32)
    return row


def tuple_flags(share_keys, pre, sizes, tuple_status, threshold):
    """step 2 -> (flag, candidates) per tuple: FINAL for a tuple whose status is non-zero already (range rule, hash), EXACT with two
    candidates of one key or fewer candidate keys than the threshold, else CHECK"""
    out = []
    for i, (lo, hi) in enumerate(ranges(sizes)):
        cand = [s for s in range(lo, hi) if pre[s] == 0] if tuple_status[i] == 0 else []
        named = [share_keys[s] for s in cand]
        if tuple_status[i] != 0:
            out.append((FINAL, cand))
        elif len(set(named)) != len(named) or len(named) < threshold:
            out.append((EXACT, cand))
        else:
            out.append((CHECK, cand))
    return out


def combine(share_keys, pre, sizes, tuple_status, bm_words, threshold, tuple_check, share_check):
    """steps 2-6 -> dict(share_status, tuple_status, rows, counts, chosen, flags, verdicts, queue, hook).  chosen: per tuple the (key, share
    index) pairs whose weighted sum is the group signature ([] for a tuple without one); queue: the shares verified exactly, ascending;
    hook: what bn254_debug_threshold_opt_last reports"""
    n = len(sizes)
    flags = tuple_flags(share_keys, pre, sizes, tuple_status, threshold)
    tuple_st, rows, counts, chosen, verdicts, exact = list(tuple_status), [], [], [], [None] * n, []
    for i, (flag, cand) in enumerate(flags):
        if flag == CHECK:
            kept = sorted(cand, key=lambda s: share_keys[s])[:threshold]
            pairs = [(share_keys[s], s) for s in kept]
            verdicts[i] = tuple_check(i, pairs)
            rows.append(row_of([j for j, _ in pairs], bm_words)), counts.append(len(cand)), chosen.append(pairs)
        else:
            rows.append([0] * bm_words), counts.append(0), chosen.append([])
        if flag == EXACT or (flag == CHECK and verdicts[i] != 0):
            exact.append(i)
    status, queue = list(pre), []
    for i in exact:
        for s in flags[i][1]:
            status[s] = share_check(s)
            queue.append(s)
    if exact:                                                                               # the exact call's rule, for these tuples only
        sel = TM.select(share_keys, status, sizes, [0 if i in exact else 2 for i in range(n)], bm_words, threshold)
        for i in exact:
            tuple_st[i], counts[i], rows[i], chosen[i] = sel[i]
    checked = [i for i, (flag, _) in enumerate(flags) if flag == CHECK]
    hook = dict(checked=len(checked), passed=sum(1 for i in checked if verdicts[i] == 0), exact_tuples=len(exact), exact_shares=len(queue))
    return dict(share_status=status, tuple_status=tuple_st, rows=rows, counts=counts, chosen=chosen, flags=[f for f, _ in flags], verdicts=verdicts,
                queue=sorted(queue), hook=hook)
