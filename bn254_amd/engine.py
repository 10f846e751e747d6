"""Thin Python binding of the C ABI (include/bn254_hip.h): one `Engine` per GPU.

Host-pointer methods take/return `bytes`; `*_device` methods take raw device pointers (e.g.
`tensor.data_ptr()` of torch uint8 tensors resident in HBM) and only enqueue work.
"""
import ctypes

from . import _native

G1_BYTES, G2_BYTES, GT_BYTES, SCALAR_BYTES = 64, 128, 384, 32
FLAG_G2_SUBGROUP_CHECK = 1
FLAG_REJECT_IDENTITY = 2
FLAG_G1_COMPRESSED = 4          # the call's G1 input array holds 33-byte compressed points (the registered-key calls; include/bn254_hip.h)
G1_COMPRESSED_BYTES = 33
FLAG_RAND64 = 0x100
FLAG_RAND_GLV = 0x200
POP_TAG = b"BN254G2_POP_V01:"   # BN254_POP_TAG (include/bn254_hip.h): the proof of possession of a key is its holder's signature on POP_TAG + pk
OPT_SPLIT_MILLER = 1
OPT_HASH_MAX_TRIES = 2
OPT_RAND_ITEMS_PER_LANE = 3
OPT_PAIR_LANES = 4
OPT_RAND_MIN_BATCH = 5
OPT_TRIO_MAX_BATCH = 6
OPT_HASH_DIRECT_WIDTH = 7
OPT_TRIO_WAVE_ROLES = 8
OPT_AGG_SUBSET_MIN_TUPLES = 9
OPT_CLOCK_PROBE = 10
OPT_AGG_SORT_BY_MSG = 11
OPT_PINNED_STAGING = 12
OPT_NONET_MAX_BATCH = 13
OPT_LM_MAX_BATCH = 15
OPT_NONET_WIDE = 16
OPT_AGG_WIDE_MIN_TUPLES = 14
OPT_MAX_CHUNK = 17          # verify-shaped batches above this size are processed in slices (0 = only when the workspace would not fit)
OPT_ASSUME_FREE_MB = 18
OPT_G2_FIXED_BASE = 19      # developer option: key derivation through the comb table of the generator (default 1)     # test knob of the automatic slicing rule
OPT_KEY_DEDUP = 20           # verify on lane pairs: distinct keys found and tabulated per call, keyed Miller loop when it pays (default 1)
OPT_KEY_DEDUP_MAX_KEYS = 21  # ... for at most this many distinct keys (default 1024)
OPT_KEY_DEDUP_MIN_MULT = 22  # ... and at least this many items per key (default 16)
OPT_KEY_DEDUP_FORCE_GENERIC = 23   # test hook: the device-side decision always takes the generic loop
OPT_KEY_DEDUP_HASH_BITS = 24       # test seam: bits of the dedup hash kept (0 = all)
OPT_AGGD_KEYED_ROUTE = 25          # keyed aggregates over distinct messages: 0 by size, 1 / 2 slot kernel width, 3 expanded keys
OPT_AGG_RAND_MIN_PAIRS = 26        # randomised keyed aggregates over distinct messages: the exact route below this many messages
OPT_AGG_RAND_GROUP_PAIRS = 27      # ... messages per group of its combined checks (developer option; at least the number of keys)
OPT_BITMAP_TABLE_MAX_KEYS = 28     # signer bitmaps: subset tables of the registered set while it has at most this many keys (default 4096; 0 = never)
OPT_BITMAP_ROUTE = 29              # ... test hook: 0 by that rule, 1 always tables, 2 always key by key
OPT_HASH_SCHEDULE = 30             # hash-to-G1 above 4096 messages: 0 by size, 1 multi-round schedule, 2 one wide round + finish and tail in one launch
OPT_HASH_WIDE_WIDTH = 31           # ... measurement knob: counters per message in the wide round (0 = by size)
OPT_HASH_TAIL_CHUNK = 32           # ... test seam: counters per lane group and pass in the tail (power of two, 2 .. 32; default 32)
OPT_BITMAP_RAND_MIN_TUPLES = 33    # randomised signer bitmaps: the exact bitmap call below this many tuples
OPT_BITMAP_RAND_GROUP_TUPLES = 34  # ... tuples per group of its combined checks (developer option)
OPT_BITMAP_RAND_MAX_KEYS = 35      # ... the exact bitmap call when more keys than this are registered
OPT_KEY_DEDUP_FOLD = 44            # key dedup: the keyed Miller loop multiplies unit lines (default 2; 1 = the keys' folded rows, 0 = line pairs)
OPT_KEY_CACHE = 36                 # key dedup: the line tables stay between calls, a call builds only unseen keys (default 1; 0 = build all, drops the cache)
OPT_COLLECT_RAND_MIN_SHARES = 38   # collect_keyed_bitmap_randomized: the exact collect below this many shares (default 65664)
OPT_COLLECT_RAND_MIN_PER_KEY = 39  # ... and below this many shares per registered key, n_shares // n_keys (default 42); DESIGN.md §10f
COLLECT_RAND_MIN_SHARES_DEFAULT = 65664  # the library's defaults of the two (bn254_amd/csrc/bn254_ws.h; measured: DESIGN.md §10f)
COLLECT_RAND_MIN_PER_KEY_DEFAULT = 42
OPT_COLLECT_OPT_MIN_SHARES = 40         # collect_keyed_bitmap_optimistic: the exact collect below this many shares (default 1539)
OPT_AGG_T4_ROUTE = 42              # aggregate verify, test hook: 0 the 4-signer signature tables from pairs + quads, 1 from k_pool_subsets_g1
OPT_COLLECT_OPT_MIN_TUPLE_SHARES = 41   # ... and, per tuple, the exact way below this many candidates (default 1 = every tuple is checked); DESIGN.md §10g
COLLECT_OPT_MIN_SHARES_DEFAULT = 1539   # the library's defaults of the two (bn254_amd/csrc/bn254_ws.h; measured: DESIGN.md §10g)
COLLECT_OPT_MIN_TUPLE_SHARES_DEFAULT = 1
OPT_MERGE_WAVE_MIN_PARTS = 43       # merge_keyed_bitmap: tuples with at least this many partials are merged by a wave each (default 16, from the sweep of tools/merge_throughput.py)
MERGE_WAVE_MIN_PARTS_DEFAULT = 16   # ... as bn254_ws.h has it
OPT_MERGE_OPT_MIN_PARTS = 45        # merge_keyed_bitmap_optimistic: the exact merge below this many partials (default 64, measured: DESIGN.md §10i); 0 = no lower bound
MERGE_OPT_MIN_PARTS_DEFAULT = 64    # ... as bn254_ws.h has it
OPT_THRESHOLD_OPT_MIN_SHARES = 46   # threshold_combine_keyed_optimistic: the exact threshold call below this many shares (default 513, measured: DESIGN.md §10l); 0 = no lower bound
THRESHOLD_OPT_MIN_SHARES_DEFAULT = 513    # ... as bn254_ws.h has it
OPT_POLY_EVAL_WAVE_MIN_COEFFS = 0   # batch_g2_poly_eval, register_keys_commitments: polynomials with at least this many coefficients are evaluated by a wave each (same bytes)
OPT_COLLECT_WAVE_MIN_SHARES = 37   # collect_keyed_bitmap: tuples with at least this many shares are summed by a wave each (default 16; swept at three shapes only)


class NativeError(RuntimeError):
    """A call into libbn254hip.so failed (HIP runtime error or bad argument) — not a per-item status."""

    def __init__(self, fn, rc):
        what = "HIP error %d" % (-rc) if -10000 < rc < 0 else {-10001: "bad argument", -10002: "misaligned device pointer",
                                                                -10003: "no HIP device (bn254_amd has no CPU fallback)"}.get(rc, "error")
        super().__init__("%s failed: %s (rc=%d)" % (fn, what, rc))
        self.rc = rc


def _check(fn, rc):
    if rc != 0:
        raise NativeError(fn, rc)


def g1_item_bytes(flags):
    """bytes per point of a call's G1 input array: 33 under FLAG_G1_COMPRESSED, else 64"""
    return G1_COMPRESSED_BYTES if flags & FLAG_G1_COMPRESSED else G1_BYTES


def pack_messages(messages):
    """list of bytes -> (concatenated bytes, ctypes uint64 offsets[n+1])"""
    n = len(messages)
    off = (ctypes.c_uint64 * (n + 1))()
    pos = 0
    for i, m in enumerate(messages):
        off[i] = pos
        pos += len(m)
    off[n] = pos
    return b"".join(bytes(m) for m in messages), off


class Engine:
    def __init__(self, device=0):
        self._lib = _native.load()
        h = ctypes.c_void_p()
        _check("bn254_ctx_create", self._lib.bn254_ctx_create(device, ctypes.byref(h)))
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bn254_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def version(self):
        return self._lib.bn254_version().decode()

    def reserve(self, n):
        _check("bn254_ctx_reserve", self._lib.bn254_ctx_reserve(self._h, n))

    def reserve_host(self, n, msg_bytes):
        """presize workspace + staging for host-pointer batch_verify calls of up to n tuples / msg_bytes message bytes"""
        _check("bn254_ctx_reserve_host", self._lib.bn254_ctx_reserve_host(self._h, n, msg_bytes))

    def synchronize(self):
        _check("bn254_ctx_synchronize", self._lib.bn254_ctx_synchronize(self._h))

    def set_profiling(self, on):
        _check("bn254_ctx_set_profiling", self._lib.bn254_ctx_set_profiling(self._h, 1 if on else 0))

    def expect_msgs_len(self, msgs_len):
        """size in bytes of the d_msgs buffer of the NEXT *_device call that hashes messages: its spans get bounds-checked on the
        device (status 5 for a span outside the buffer) — include/bn254_hip.h: bn254_ctx_expect_msgs_len"""
        _check("bn254_ctx_expect_msgs_len", self._lib.bn254_ctx_expect_msgs_len(self._h, int(msgs_len)))

    def set_option(self, option, value):
        _check("bn254_ctx_set_option", self._lib.bn254_ctx_set_option(self._h, option, value))

    def probe_issue_rate(self, op, waves_per_simd=2):
        """(wave-instructions per second, SIMD count) of op 0 v_mad_u64_u32 / 1 v_add_u32 / 2 v_mul_lo_u32"""
        rate, simds = ctypes.c_double(0), ctypes.c_int(0)
        _check("bn254_probe_issue_rate", self._lib.bn254_probe_issue_rate(self._h, op, waves_per_simd, ctypes.byref(rate), ctypes.byref(simds)))
        return rate.value, simds.value

    def route_table(self):
        """developer hook: the context's batch-size -> layout routing table as it stands: [(max_n, miller, fe)], last row max_n = 2**64 - 1
        (miller: 0 lane machine, 1 wave roles, 2 lane pairs; fe: 0 eighteen lane pairs, 1 nine, 2 octets, 3 lane pairs)"""
        m, a, b = (ctypes.c_uint64 * 8)(), (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
        rows = self._lib.bn254_debug_route_table(self._h, m, a, b, 8)
        if rows < 0:
            _check("bn254_debug_route_table", rows)
        return [(int(m[i]), int(a[i]), int(b[i])) for i in range(rows)]

    def debug_key_dedup_last(self):
        """the key dedup's device-side decision of the last batch_verify_device: dict(ran, keys, flags, keyed_n, generic_n)"""
        o = (ctypes.c_uint32 * 5)()
        _check("bn254_debug_key_dedup_last", self._lib.bn254_debug_key_dedup_last(self._h, o))
        return dict(zip(("ran", "keys", "flags", "keyed_n", "generic_n"), (int(x) for x in o)))

    def debug_key_cache_last(self):
        """what the last batch_verify_device did with the key cache: dict(ran, keys, hits, built, dropped)"""
        o = (ctypes.c_uint32 * 5)()
        _check("bn254_debug_key_cache_last", self._lib.bn254_debug_key_cache_last(self._h, o))
        return dict(zip(("ran", "keys", "hits", "built", "dropped"), (int(x) for x in o)))

    def debug_key_tables(self, which, first, count):
        """developer hook: the line tables on the device (which = 0: of the last key dedup, 1: registered) of keys first .. first + count - 1
        -> (words: count * 87 * 36 ints, rep or None, statuses, identity flags)"""
        words = (ctypes.c_int32 * (count * 87 * 36))()
        rep = (ctypes.c_uint32 * max(count, 1))()
        st, inf = ctypes.create_string_buffer(max(count, 1)), ctypes.create_string_buffer(max(count, 1))
        _check("bn254_debug_key_tables", self._lib.bn254_debug_key_tables(self._h, which, first, count, words, rep, st, inf))
        return list(words), (list(rep)[:count] if which == 0 else None), st.raw[:count], inf.raw[:count]

    def debug_key_fold_tables(self, first, count):
        """developer hook: the folded rows of the keys first .. first + count - 1 of the last key dedup (OPT_KEY_DEDUP_FOLD)
        -> count * 22 * 90 ints ([row][K0 .. K4][re, im][9 limbs])"""
        words = (ctypes.c_int32 * (count * 22 * 90))()
        _check("bn254_debug_key_fold_tables", self._lib.bn254_debug_key_fold_tables(self._h, first, count, words))
        return list(words)

    def debug_agg_tables_info(self):
        """developer hook: which tables the registered pools have -> dict(n_groups, groups4, wide2, wide1, t4_builder: 0 none, 1 pairs + quads,
        2 k_pool_subsets_g1)"""
        o = (ctypes.c_uint64 * 5)()
        _check("bn254_debug_agg_tables", self._lib.bn254_debug_agg_tables(self._h, -1, 0, 0, o, None))
        return dict(zip(("n_groups", "groups4", "wide2", "wide1", "t4_builder"), (int(v) for v in o)))

    def debug_agg_tables(self, which, first, count):
        """developer hook: entries first .. first + count - 1 of table `which` (the context's pool index, 0 .. 7) of the registered pools ->
        (points: canonical bytes, 128 per entry for which in (0, 3, 5) else 64, zeros under an identity flag; flags: the raw status bytes)"""
        size = 128 if which in (0, 3, 5) else 64
        pts, fl = ctypes.create_string_buffer(max(count * size, 1)), ctypes.create_string_buffer(max(count, 1))
        _check("bn254_debug_agg_tables", self._lib.bn254_debug_agg_tables(self._h, which, first, count, pts, fl))
        return pts.raw[:count * size], fl.raw[:count]

    def debug_agg_rand_last(self):
        """what the last batch_aggregate_verify_distinct_keyed_randomized[_device] did: dict(ran, groups, table_pairs, failed_groups, rechecked,
        single_groups)"""
        o = (ctypes.c_uint64 * 6)()
        _check("bn254_debug_agg_rand_last", self._lib.bn254_debug_agg_rand_last(self._h, o))
        return dict(zip(("ran", "groups", "table_pairs", "failed_groups", "rechecked", "single_groups"), (int(x) for x in o)))

    def debug_agg_rand_sums(self):
        """the G1 side of that call's group checks as it left them (include/bn254_hip.h: bn254_debug_agg_rand_sums): a list with one
        dict(nagg, verdict, s, pairs=[(key index, 64-byte bucket sum), ...]) per group, the groups without an aggregate included; [] when
        the call took the exact route.  Read it directly after that call: ANY later call on the engine (a sign, a sum, a registration)
        may reuse the workspace, and the hook then returns whatever lies there"""
        return self._debug_rand_sums("bn254_debug_agg_rand_sums")

    def _debug_rand_sums(self, name):
        f = getattr(self._lib, name)
        dims = (ctypes.c_uint64 * 2)()
        _check(name, f(self._h, dims, 0, 0, None, None, None, None, None, None))
        ng, ntp = int(dims[0]), int(dims[1])
        if ng == 0:
            return []
        nagg, verdict, s = (ctypes.c_uint32 * ng)(), ctypes.create_string_buffer(ng), ctypes.create_string_buffer(64 * ng)
        first, keys, pts = (ctypes.c_uint64 * (ng + 1))(), (ctypes.c_uint32 * max(ntp, 1))(), ctypes.create_string_buffer(64 * max(ntp, 1))
        _check(name, f(self._h, dims, ng, ntp, nagg, verdict, s, first, keys, pts))
        assert (int(dims[0]), int(dims[1])) == (ng, ntp)
        return [dict(nagg=int(nagg[g]), verdict=verdict.raw[g], s=s.raw[64 * g:64 * g + 64],
                     pairs=[(int(keys[t]), pts.raw[64 * t:64 * t + 64]) for t in range(int(first[g]), int(first[g + 1]))]) for g in range(ng)]

    def debug_bitmap_rand_last(self):
        """what the last batch_verify_keyed_bitmap_randomized[_device] did: dict(ran, groups, table_pairs, failed_groups, rechecked, single_groups)"""
        o = (ctypes.c_uint64 * 6)()
        _check("bn254_debug_bitmap_rand_last", self._lib.bn254_debug_bitmap_rand_last(self._h, o))
        return dict(zip(("ran", "groups", "table_pairs", "failed_groups", "rechecked", "single_groups"), (int(x) for x in o)))

    def debug_collect_rand_last(self):
        """what the last batch_collect_keyed_bitmap_randomized[_device] did, summed over its slices: dict(slices, groups, failed_groups,
        rechecked); all 0 when it took the exact route"""
        o = (ctypes.c_uint64 * 4)()
        _check("bn254_debug_collect_rand_last", self._lib.bn254_debug_collect_rand_last(self._h, o))
        return dict(zip(("slices", "groups", "failed_groups", "rechecked"), (int(x) for x in o)))

    def debug_collect_opt_last(self):
        """what the last batch_collect_keyed_bitmap_optimistic[_device] did, counted on the device: dict(checked, passed, exact_tuples,
        exact_shares) — tuples whose sum was verified, those that passed, tuples sent the exact way (failed, a duplicate, below the
        per-tuple minimum), shares verified one by one; all 0 when the call took the exact route as a whole"""
        o = (ctypes.c_uint64 * 4)()
        _check("bn254_debug_collect_opt_last", self._lib.bn254_debug_collect_opt_last(self._h, o))
        return dict(zip(("checked", "passed", "exact_tuples", "exact_shares"), (int(x) for x in o)))

    def debug_threshold_opt_last(self):
        """what the last batch_threshold_combine_keyed_optimistic[_device] did, counted on the device: dict(checked, passed, exact_tuples,
        exact_shares) — tuples checked under the group key, those that passed, tuples sent the exact way (failed, a duplicate, fewer
        candidates than the threshold), shares verified one by one; all 0 after any call that did not take the route"""
        o = (ctypes.c_uint64 * 4)()
        _check("bn254_debug_threshold_opt_last", self._lib.bn254_debug_threshold_opt_last(self._h, o))
        return dict(zip(("checked", "passed", "exact_tuples", "exact_shares"), (int(x) for x in o)))

    def debug_merge_opt_last(self):
        """what the last merge_keyed_bitmap_optimistic[_device] did, counted on the device: dict(checked, passed, exact_tuples, exact_parts) —
        tuples whose sum was verified, those that passed, tuples sent the exact way (failed, or an overlap), partials verified one by one;
        all 0 after any call that did not take the route"""
        o = (ctypes.c_uint64 * 4)()
        _check("bn254_debug_merge_opt_last", self._lib.bn254_debug_merge_opt_last(self._h, o))
        return dict(zip(("checked", "passed", "exact_tuples", "exact_parts"), (int(x) for x in o)))

    def debug_bitmap_rand_sums(self):
        """the G1 side of that call's group checks as it left them (include/bn254_hip.h: bn254_debug_bitmap_rand_sums), in the format of
        debug_agg_rand_sums: one dict(nagg, verdict, s, pairs=[(key index, 64-byte T_{g,j}), ...]) per group; [] when the call took the exact
        route.  Read it directly after that call"""
        return self._debug_rand_sums("bn254_debug_bitmap_rand_sums")

    def last_kernel_ms(self):
        ms = (ctypes.c_float * 4)()
        _check("bn254_ctx_last_kernel_ms", self._lib.bn254_ctx_last_kernel_ms(self._h, ms))
        return {"decode": ms[0], "hash_to_g1": ms[1], "miller_loop": ms[2], "final_exp": ms[3]}

    def probe_leaf_floor(self, n, mode=0):
        """ms of the kernel that runs only the product leaves of a verify's Miller loop (mode 0) / final exponentiation (mode 1), n lane
        pairs (include/bn254_hip.h)"""
        ms = ctypes.c_float()
        _check("bn254_probe_leaf_floor", self._lib.bn254_probe_leaf_floor(self._h, n, mode, ctypes.byref(ms)))
        return ms.value

    def probe_fe_program(self, n, steps):
        """ms of the final exponentiation's accumulator machine on the program `steps` = [(opcode, arg), ...] (include/bn254_hip.h)"""
        prog = bytes(b for st in steps for b in st)
        ms = ctypes.c_float()
        _check("bn254_probe_fe_program", self._lib.bn254_probe_fe_program(self._h, n, prog, len(steps), ctypes.byref(ms)))
        return ms.value

    def last_clocks(self):
        """OPT_CLOCK_PROBE on: achieved shader clock (MHz) of the last lane-pair Miller kernel, final exponentiation and issue probe"""
        mhz = (ctypes.c_double * 3)()
        _check("bn254_ctx_last_clocks", self._lib.bn254_ctx_last_clocks(self._h, mhz))
        return {"miller_loop": mhz[0], "final_exp": mhz[1], "issue_probe": mhz[2]}

    # ---- host-pointer entry points ------------------------------------------------------
    def batch_verify(self, messages, sigs, pks, flags=0):
        n = len(messages)
        assert len(sigs) == n * G1_BYTES and len(pks) == n * G2_BYTES
        msgs, off = pack_messages(messages)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_verify", self._lib.bn254_batch_verify(self._h, msgs, off, bytes(sigs), bytes(pks), n, flags, status))
        return status.raw[:n]

    def batch_verify_compressed(self, messages, sigs33, pks65):
        """verify from the compressed encodings (33-byte signatures, 65-byte public keys)"""
        n = len(messages)
        assert len(sigs33) == n * 33 and len(pks65) == n * 65
        msgs, off = pack_messages(messages)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_verify_compressed",
               self._lib.bn254_batch_verify_compressed(self._h, msgs, off, bytes(sigs33), bytes(pks65), n, status))
        return status.raw[:n]

    def batch_verify_randomized(self, messages, sigs, pks, seed32, flags=0):
        """opt-in randomised batch verification (include/bn254_hip.h) -> (status bytes, group_ok bytes)"""
        n = len(messages)
        assert len(sigs) == n * G1_BYTES and len(pks) == n * G2_BYTES and len(seed32) == 32
        msgs, off = pack_messages(messages)
        status = ctypes.create_string_buffer(max(n, 1))
        ng = (n + 63) // 64
        groups = ctypes.create_string_buffer(max(ng, 1))
        _check("bn254_batch_verify_randomized",
               self._lib.bn254_batch_verify_randomized(self._h, msgs, off, bytes(sigs), bytes(pks), n, flags, bytes(seed32), status, groups))
        return status.raw[:n], groups.raw[:ng]

    def batch_hash_to_g1(self, messages):
        n = len(messages)
        msgs, off = pack_messages(messages)
        pts = ctypes.create_string_buffer(max(n, 1) * G1_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        tries = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_hash_to_g1", self._lib.bn254_batch_hash_to_g1(self._h, msgs, off, n, pts, status, tries))
        return pts.raw[:n * G1_BYTES], status.raw[:n], tries.raw[:n]

    def batch_pairing_check(self, g1s, g2s, n, k, flags=0):
        assert len(g1s) == n * k * G1_BYTES and len(g2s) == n * k * G2_BYTES
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_pairing_check", self._lib.bn254_batch_pairing_check(self._h, bytes(g1s), bytes(g2s), n, k, flags, status))
        return status.raw[:n]

    def batch_pairing(self, g1s, g2s, n, k=1, flags=0):
        assert len(g1s) == n * k * G1_BYTES and len(g2s) == n * k * G2_BYTES
        gt = ctypes.create_string_buffer(max(n, 1) * GT_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_pairing", self._lib.bn254_batch_pairing(self._h, bytes(g1s), bytes(g2s), n, k, flags, gt, status))
        return gt.raw[:n * GT_BYTES], status.raw[:n]

    def batch_check_public_keys(self, pk_g2, pk_g1, n, flags=0):
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_check_public_keys", self._lib.bn254_batch_check_public_keys(self._h, bytes(pk_g2), bytes(pk_g1), n, flags, status))
        return status.raw[:n]

    def _binop(self, name, a, b, n, size):
        out = ctypes.create_string_buffer(max(n, 1) * size)
        status = ctypes.create_string_buffer(max(n, 1))
        _check(name, getattr(self._lib, name)(self._h, bytes(a), bytes(b), n, out, status))
        return out.raw[:n * size], status.raw[:n]

    def batch_g1_add(self, a, b, n):
        return self._binop("bn254_batch_g1_add", a, b, n, G1_BYTES)

    def batch_g2_add(self, a, b, n):
        return self._binop("bn254_batch_g2_add", a, b, n, G2_BYTES)

    def batch_g1_mul(self, points, scalars, n, reduce_scalar=False):
        """points=None multiplies the G1 generator (PublicKeyG1::from_private_key)."""
        out = ctypes.create_string_buffer(max(n, 1) * G1_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_g1_mul", self._lib.bn254_batch_g1_mul(self._h, None if points is None else bytes(points), bytes(scalars), n,
                                                               int(reduce_scalar), out, status))
        return out.raw[:n * G1_BYTES], status.raw[:n]

    def batch_g2_mul(self, points, scalars, n, reduce_scalar=False):
        """points=None multiplies the G2 generator (PublicKey::from_private_key)."""
        out = ctypes.create_string_buffer(max(n, 1) * G2_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_g2_mul", self._lib.bn254_batch_g2_mul(self._h, None if points is None else bytes(points), bytes(scalars), n,
                                                               int(reduce_scalar), out, status))
        return out.raw[:n * G2_BYTES], status.raw[:n]

    def batch_sign(self, messages, sks):
        n = len(messages)
        msgs, off = pack_messages(messages)
        sigs = ctypes.create_string_buffer(max(n, 1) * G1_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_sign", self._lib.bn254_batch_sign(self._h, msgs, off, bytes(sks), n, sigs, status))
        return sigs.raw[:n * G1_BYTES], status.raw[:n]

    def _sum(self, name, points, seg_off, size):
        n = len(seg_off) - 1
        off = (ctypes.c_uint64 * (n + 1))(*seg_off)
        out = ctypes.create_string_buffer(max(n, 1) * size)
        status = ctypes.create_string_buffer(max(n, 1))
        _check(name, getattr(self._lib, name)(self._h, bytes(points), off, n, out, status))
        return out.raw[:n * size], status.raw[:n]

    def batch_g1_sum(self, points, seg_off):
        return self._sum("bn254_batch_g1_sum", points, seg_off, G1_BYTES)

    def batch_g2_sum(self, points, seg_off):
        return self._sum("bn254_batch_g2_sum", points, seg_off, G2_BYTES)

    def batch_g1_msm(self, points, scalars, seg_off, reduce_scalar=False):
        """segmented scalar-weighted sums in G1 (include/bn254_hip.h: bn254_batch_g1_msm): out[i] = sum of scalars[s] * points[s] over the
        terms seg_off[i] .. seg_off[i+1]; returns (the n sums, the n status bytes)"""
        n = len(seg_off) - 1
        m = int(seg_off[n]) if n >= 0 else 0
        assert len(points) == m * G1_BYTES and len(scalars) == m * SCALAR_BYTES
        off = (ctypes.c_uint64 * (n + 1))(*seg_off)
        out = ctypes.create_string_buffer(max(n, 1) * G1_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_g1_msm", self._lib.bn254_batch_g1_msm(self._h, bytes(points), bytes(scalars), off, n, int(reduce_scalar), out, status))
        return out.raw[:n * G1_BYTES], status.raw[:n]

    def batch_g1_msm_device(self, d_points, d_scalars, d_seg_off, n, d_out, d_status, reduce_scalar=False, stream=None):
        _check("bn254_batch_g1_msm_device",
               self._lib.bn254_batch_g1_msm_device(self._h, d_points, d_scalars, d_seg_off, n, int(reduce_scalar), d_out, d_status, stream))

    def batch_g2_msm(self, points, scalars, seg_off, reduce_scalar=False):
        """segmented scalar-weighted sums in G2 (include/bn254_hip.h: bn254_batch_g2_msm): out[i] = sum of scalars[s] * points[s] over the
        terms seg_off[i] .. seg_off[i+1], 128-byte points; returns (the n sums, the n status bytes)"""
        n = len(seg_off) - 1
        m = int(seg_off[n]) if n >= 0 else 0
        assert len(points) == m * G2_BYTES and len(scalars) == m * SCALAR_BYTES
        off = (ctypes.c_uint64 * (n + 1))(*seg_off)
        out = ctypes.create_string_buffer(max(n, 1) * G2_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_g2_msm", self._lib.bn254_batch_g2_msm(self._h, bytes(points), bytes(scalars), off, n, int(reduce_scalar), out, status))
        return out.raw[:n * G2_BYTES], status.raw[:n]

    def batch_g2_msm_device(self, d_points, d_scalars, d_seg_off, n, d_out, d_status, reduce_scalar=False, stream=None):
        _check("bn254_batch_g2_msm_device",
               self._lib.bn254_batch_g2_msm_device(self._h, d_points, d_scalars, d_seg_off, n, int(reduce_scalar), d_out, d_status, stream))

    def batch_g2_poly_eval(self, coeffs, poly_off, eval_poly, eval_x):
        """polynomials with G2 coefficients at small integer points (include/bn254_hip.h: bn254_batch_g2_poly_eval): polynomial i is the
        coefficients poly_off[i] .. poly_off[i+1] of `coeffs` (128 B each, lowest degree first); evaluation e is (eval_poly[e], eval_x[e]),
        x any uint32.  Returns (the q values sum x^k C_k, the q status bytes)."""
        p = len(poly_off) - 1
        m = int(poly_off[p]) if p >= 0 else 0
        q = len(eval_poly)
        assert p >= 0 and len(coeffs) == m * G2_BYTES and len(eval_x) == q
        off = (ctypes.c_uint64 * (p + 1))(*poly_off)
        polys = (ctypes.c_uint32 * max(q, 1))(*eval_poly)
        xs = (ctypes.c_uint32 * max(q, 1))(*eval_x)
        out = ctypes.create_string_buffer(max(q, 1) * G2_BYTES)
        status = ctypes.create_string_buffer(max(q, 1))
        _check("bn254_batch_g2_poly_eval", self._lib.bn254_batch_g2_poly_eval(self._h, bytes(coeffs), off, p, polys, xs, q, out, status))
        return out.raw[:q * G2_BYTES], status.raw[:q]

    def batch_g2_poly_eval_device(self, d_coeffs, d_poly_off, p, d_eval_poly, d_eval_x, q, d_out, d_status, stream=None):
        _check("bn254_batch_g2_poly_eval_device",
               self._lib.bn254_batch_g2_poly_eval_device(self._h, d_coeffs, d_poly_off, p, d_eval_poly, d_eval_x, q, d_out, d_status, stream))

    def batch_g2_vector_combine(self, vectors, scalars, d, length, reduce_scalar=False):
        """d vectors of `length` G2 points (vector-major, 128 B each) combined column by column under one 32-byte scalar per vector
        (include/bn254_hip.h: bn254_batch_g2_vector_combine): out[k] = sum_i scalars[i] * vectors[i][k].  Returns (the `length` sums, the
        `length` status bytes)."""
        assert len(vectors) == d * length * G2_BYTES and len(scalars) == d * SCALAR_BYTES
        out = ctypes.create_string_buffer(max(length, 1) * G2_BYTES)
        status = ctypes.create_string_buffer(max(length, 1))
        _check("bn254_batch_g2_vector_combine",
               self._lib.bn254_batch_g2_vector_combine(self._h, bytes(vectors), bytes(scalars), d, length, int(reduce_scalar), out, status))
        return out.raw[:length * G2_BYTES], status.raw[:length]

    def batch_g2_vector_combine_device(self, d_vectors, d_scalars, d, length, d_out, d_status, reduce_scalar=False, stream=None):
        _check("bn254_batch_g2_vector_combine_device",
               self._lib.bn254_batch_g2_vector_combine_device(self._h, d_vectors, d_scalars, d, length, int(reduce_scalar), d_out, d_status, stream))

    def reshare_commitments(self, vectors, dealer_keys, t_new, threshold, bm_words=None):
        """the commitments of the next committee's polynomial from the sub-dealings of old members (include/bn254_hip.h:
        bn254_ctx_reshare_commitments): vectors = len(dealer_keys) * t_new commitments, dealer-major; dealer_keys strictly increasing indices
        into the registered set (the OLD committee).  Returns (the t_new commitments — zero bytes unless the status is 0 —, the call's status,
        the per-dealer status bytes, the used row as bm_words integers: S on success, else the qualified dealers)."""
        d = len(dealer_keys)
        assert len(vectors) == d * t_new * G2_BYTES
        if bm_words is None:
            bm_words = max(1, (self.n_registered_keys + 31) // 32)
        keys = (ctypes.c_uint32 * max(d, 1))(*dealer_keys)
        dealer_st = ctypes.create_string_buffer(max(d, 1))
        row = (ctypes.c_uint32 * max(bm_words, 1))()
        out = ctypes.create_string_buffer(max(t_new, 1) * G2_BYTES)
        st = ctypes.create_string_buffer(1)
        _check("bn254_ctx_reshare_commitments",
               self._lib.bn254_ctx_reshare_commitments(self._h, bytes(vectors), keys, d, int(t_new), int(threshold), 0, dealer_st, row, bm_words, out, st))
        return out.raw[:t_new * G2_BYTES], st.raw[0], dealer_st.raw[:d], list(row)[:bm_words]

    def register_keys_commitments(self, commitments, n_keys, flags=0):
        """register pk_j = f(j + 1) * G2, j < n_keys, from the t Feldman commitments of f (include/bn254_hip.h:
        bn254_ctx_register_keys_commitments).  Returns (the per-key status bytes, the call's status): a commitment that does not decode gives
        (None, its decode status) and leaves the context without keys.  Does not install the group key: set_group_key(commitments[:128]) does."""
        t = len(commitments) // G2_BYTES
        assert len(commitments) == t * G2_BYTES
        key_st = ctypes.create_string_buffer(max(n_keys, 1))
        st = ctypes.create_string_buffer(1)
        self.group_key_set = False
        self.n_registered_keys = 0
        _check("bn254_ctx_register_keys_commitments",
               self._lib.bn254_ctx_register_keys_commitments(self._h, bytes(commitments), t, n_keys, flags, key_st, st))
        if st.raw[0] != 0:
            return None, st.raw[0]
        self.n_registered_keys = n_keys
        return key_st.raw[:n_keys], 0

    def check_dealing(self, threshold, seed32):
        """are the registered keys a `threshold`-of-n dealing, and which group key do they interpolate to (include/bn254_hip.h:
        bn254_ctx_check_dealing): returns (group key: 128 bytes, zeroed unless the status is 0; status; bad_key: the lowest key with a
        non-zero registration status, or 0xFFFFFFFF).  Does not install the group key: set_group_key does."""
        assert len(seed32) == 32
        pk = ctypes.create_string_buffer(G2_BYTES)
        st = ctypes.create_string_buffer(1)
        bad = ctypes.c_uint32(0)
        _check("bn254_ctx_check_dealing", self._lib.bn254_ctx_check_dealing(self._h, int(threshold), bytes(seed32), 0, pk, st, ctypes.byref(bad)))
        return pk.raw, st.raw[0], bad.value

    def debug_dealing_coefficients(self, n_keys, threshold, seed32):
        """the coefficients c_0 .. c_n-1 of check_dealing's degree check -> n_keys * 32 bytes, big-endian, reduced"""
        assert len(seed32) == 32
        out = ctypes.create_string_buffer(max(n_keys, 1) * 32)
        _check("bn254_debug_dealing_coefficients", self._lib.bn254_debug_dealing_coefficients(self._h, n_keys, int(threshold), bytes(seed32), out))
        return out.raw[:n_keys * 32]

    def batch_aggregate_verify(self, messages, pk_pool, sig_pool, tuple_msg, signer_lists, flags=0):
        """messages: M byte strings; pk_pool: S*128 B; sig_pool: M*S*64 B (signer s on message m at m*S+s);
        tuple i verifies messages[tuple_msg[i]] against the aggregate of signer_lists[i]."""
        n, n_msgs = len(tuple_msg), len(messages)
        n_signers = len(pk_pool) // G2_BYTES
        assert len(sig_pool) == n_msgs * n_signers * G1_BYTES and len(signer_lists) == n
        msgs, off = pack_messages(messages)
        t_off = (ctypes.c_uint64 * (n + 1))()
        flat = []
        for i, lst in enumerate(signer_lists):
            t_off[i] = len(flat)
            flat.extend(lst)
        t_off[n] = len(flat)
        idx = (ctypes.c_uint32 * max(len(flat), 1))(*flat)
        tm = (ctypes.c_uint32 * max(n, 1))(*tuple_msg)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_aggregate_verify",
               self._lib.bn254_batch_aggregate_verify(self._h, msgs, off, n_msgs, bytes(pk_pool), n_signers, bytes(sig_pool), tm, t_off, idx, n, flags, status))
        return status.raw[:n]

    def batch_aggregate_verify_distinct(self, messages, pks, agg_sigs, agg_sizes, flags=0):
        """Aggregates over distinct messages: aggregate i owns the next agg_sizes[i] of the (messages[j], pks[j*128:]) pairs and is
        checked against agg_sigs[i*64:] (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct).  Returns n status bytes."""
        m, n = len(messages), len(agg_sizes)
        assert len(pks) == m * G2_BYTES and len(agg_sigs) == n * G1_BYTES and sum(agg_sizes) == m
        msgs, off = pack_messages(messages)
        a_off = (ctypes.c_uint64 * (n + 1))()
        pos = 0
        for i, k in enumerate(agg_sizes):
            a_off[i] = pos
            pos += int(k)
        a_off[n] = pos
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_aggregate_verify_distinct",
               self._lib.bn254_batch_aggregate_verify_distinct(self._h, msgs, off, bytes(pks), m, bytes(agg_sigs), a_off, n, flags, status))
        return status.raw[:n]

    def batch_aggregate_verify_distinct_keyed(self, messages, key_idx, agg_sigs, agg_sizes, flags=0):
        """batch_aggregate_verify_distinct against the registered keys: pk_j = registered[key_idx[j]]
        (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct_keyed).  Returns n status bytes."""
        m, n = len(messages), len(agg_sizes)
        assert len(key_idx) == m and len(agg_sigs) == n * G1_BYTES and sum(agg_sizes) == m
        msgs, off = pack_messages(messages)
        idx = (ctypes.c_uint32 * max(m, 1))(*key_idx)
        a_off = (ctypes.c_uint64 * (n + 1))()
        pos = 0
        for i, k in enumerate(agg_sizes):
            a_off[i] = pos
            pos += int(k)
        a_off[n] = pos
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_aggregate_verify_distinct_keyed",
               self._lib.bn254_batch_aggregate_verify_distinct_keyed(self._h, msgs, off, idx, m, bytes(agg_sigs), a_off, n, flags, status))
        return status.raw[:n]

    def batch_aggregate_verify_distinct_keyed_randomized(self, messages, key_idx, agg_sigs, agg_sizes, seed32, flags=0):
        """batch_aggregate_verify_distinct_keyed with the pairing checks of whole groups of aggregates combined under random weights from seed32
        (include/bn254_hip.h: bn254_batch_aggregate_verify_distinct_keyed_randomized).  Returns n status bytes."""
        m, n = len(messages), len(agg_sizes)
        assert len(key_idx) == m and len(agg_sigs) == n * G1_BYTES and sum(agg_sizes) == m and len(seed32) == 32
        msgs, off = pack_messages(messages)
        idx = (ctypes.c_uint32 * max(m, 1))(*key_idx)
        a_off = (ctypes.c_uint64 * (n + 1))()
        pos = 0
        for i, k in enumerate(agg_sizes):
            a_off[i] = pos
            pos += int(k)
        a_off[n] = pos
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_aggregate_verify_distinct_keyed_randomized",
               self._lib.bn254_batch_aggregate_verify_distinct_keyed_randomized(self._h, msgs, off, idx, m, bytes(agg_sigs), a_off, n, flags, bytes(seed32),
                                                                                status))
        return status.raw[:n]

    def register_pools(self, messages, pk_pool, sig_pool, expect_tuples, flags=0):
        """the pools of an aggregate verify decoded, hashed and tabulated ONCE (bn254_ctx_register_pools): for a fixed validator set / message
        set whose tuples keep arriving; `expect_tuples` = the batch size the subset-sum tables are chosen for"""
        n_msgs = len(messages)
        n_signers = len(pk_pool) // G2_BYTES
        assert len(sig_pool) == n_msgs * n_signers * G1_BYTES
        msgs, off = pack_messages(messages)
        _check("bn254_ctx_register_pools",
               self._lib.bn254_ctx_register_pools(self._h, msgs, off, n_msgs, bytes(pk_pool), n_signers, bytes(sig_pool), flags, expect_tuples))

    def batch_aggregate_verify_registered(self, tuple_msg, signer_lists):
        """as batch_aggregate_verify on the registered pools: only the tuples cross the boundary"""
        n = len(tuple_msg)
        assert len(signer_lists) == n
        t_off = (ctypes.c_uint64 * (n + 1))()
        flat = []
        for i, lst in enumerate(signer_lists):
            t_off[i] = len(flat)
            flat.extend(lst)
        t_off[n] = len(flat)
        idx = (ctypes.c_uint32 * max(len(flat), 1))(*flat)
        tm = (ctypes.c_uint32 * max(n, 1))(*tuple_msg)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_aggregate_verify_registered", self._lib.bn254_batch_aggregate_verify_registered(self._h, tm, t_off, idx, n, status))
        return status.raw[:n]

    def register_pools_device(self, d_msgs, d_msg_off, n_msgs, d_pk_pool, n_signers, d_sig_pool, expect_tuples, flags=0, stream=None):
        _check("bn254_ctx_register_pools_device",
               self._lib.bn254_ctx_register_pools_device(self._h, d_msgs, d_msg_off, n_msgs, d_pk_pool, n_signers, d_sig_pool, flags, expect_tuples, stream))

    def batch_aggregate_verify_registered_device(self, d_tuple_msg, d_tuple_off, d_signer_idx, n, d_status, stream=None):
        _check("bn254_batch_aggregate_verify_registered_device",
               self._lib.bn254_batch_aggregate_verify_registered_device(self._h, d_tuple_msg, d_tuple_off, d_signer_idx, n, d_status, stream))

    def batch_g1_decompress(self, data, n):
        out = ctypes.create_string_buffer(max(n, 1) * G1_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_g1_decompress", self._lib.bn254_batch_g1_decompress(self._h, bytes(data), n, out, status))
        return out.raw[:n * G1_BYTES], status.raw[:n]

    def batch_g1_decompress_device(self, d_in33, n, d_out64, d_status, stream=None):
        """the device-pointer form: enqueues only; d_in33 needs no alignment (include/bn254_hip.h: bn254_batch_g1_decompress_device)"""
        _check("bn254_batch_g1_decompress_device", self._lib.bn254_batch_g1_decompress_device(self._h, d_in33, n, d_out64, d_status, stream))

    def batch_g2_decompress(self, data, n):
        out = ctypes.create_string_buffer(max(n, 1) * G2_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_g2_decompress", self._lib.bn254_batch_g2_decompress(self._h, bytes(data), n, out, status))
        return out.raw[:n * G2_BYTES], status.raw[:n]

    # ---- test hooks -----------------------------------------------------------------------
    def debug_fp_op(self, op, a, b, n):
        out = ctypes.create_string_buffer(max(n, 1) * 32)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_debug_fp_op", self._lib.bn254_debug_fp_op(self._h, op, bytes(a), None if b is None else bytes(b), n, out, status))
        return out.raw[:n * 32], status.raw[:n]

    def debug_fr_op(self, op, a, b, n):
        """Fr on n 32-byte big-endian operands (include/bn254_hip.h: bn254_debug_fr_op) -> n * 32 bytes"""
        out = ctypes.create_string_buffer(max(n, 1) * 32)
        _check("bn254_debug_fr_op", self._lib.bn254_debug_fr_op(self._h, op, bytes(a), None if b is None else bytes(b), n, out))
        return out.raw[:n * 32]

    def debug_lagrange_at_zero(self, xs, seg_off):
        """the Lagrange coefficients at zero of the points xs (uint32) within their segments -> len(xs) * 32 bytes"""
        n, m = len(seg_off) - 1, len(xs)
        assert seg_off[n] == m
        x = (ctypes.c_uint32 * max(m, 1))(*xs)
        off = (ctypes.c_uint64 * (n + 1))(*seg_off)
        out = ctypes.create_string_buffer(max(m, 1) * 32)
        _check("bn254_debug_lagrange_at_zero", self._lib.bn254_debug_lagrange_at_zero(self._h, x, off, n, out))
        return out.raw[:m * 32]

    def debug_fp12_op(self, op, a, b, n):
        out = ctypes.create_string_buffer(max(n, 1) * GT_BYTES)
        _check("bn254_debug_fp12_op", self._lib.bn254_debug_fp12_op(self._h, op, bytes(a), None if b is None else bytes(b), n, out))
        return out.raw[:n * GT_BYTES]

    def debug_final_exp_limbs(self, layout, limbs, n, want_gt=False):
        """final exponentiation of layout 0..6 on n x 108 int32 limbs (include/bn254_hip.h) -> (Gt bytes or None, status bytes)"""
        assert len(limbs) == n * 108
        arr = (ctypes.c_int32 * max(len(limbs), 1))(*limbs)
        gt = ctypes.create_string_buffer(max(n, 1) * GT_BYTES) if want_gt else None
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_debug_final_exp_limbs", self._lib.bn254_debug_final_exp_limbs(self._h, layout, arr, n, gt, status))
        return (gt.raw[:n * GT_BYTES] if want_gt else None), status.raw[:n]

    def debug_miller_loop(self, g1s, g2s, n):
        out = ctypes.create_string_buffer(max(n, 1) * GT_BYTES)
        _check("bn254_debug_miller_loop", self._lib.bn254_debug_miller_loop(self._h, bytes(g1s), bytes(g2s), n, out))
        return out.raw[:n * GT_BYTES]

    def debug_hash_candidate(self, h, n):
        out = ctypes.create_string_buffer(max(n, 1) * G1_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_debug_hash_candidate", self._lib.bn254_debug_hash_candidate(self._h, bytes(h), n, out, status))
        return out.raw[:n * G1_BYTES], status.raw[:n]

    def debug_jacobi(self, mode, a, b, n):
        """the hash filter's Jacobi symbol on n 32-byte big-endian integers (include/bn254_hip.h: bn254_debug_jacobi; mode 0 a value below q,
        1 a candidate x, 2 the symbol (a / b)) -> (n * 32 bytes handed to the passes, n flag bytes)"""
        value = ctypes.create_string_buffer(max(n, 1) * 32)
        flags = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_debug_jacobi", self._lib.bn254_debug_jacobi(self._h, mode, bytes(a), None if b is None else bytes(b), n, value, flags))
        return value.raw[:n * 32], flags.raw[:n]

    def debug_fq2_limbs(self, layout, op, operands, coef, n):
        """one Fq2 primitive per item on raw limbs (include/bn254_hip.h: bn254_debug_fq2_limbs; layout 0 one lane, 1 a lane pair per item).
        operands: n x 4 x 18 int32, coef: n x 4 int32 — as bytes in native order or as sequences of ints -> (n x 18 int32 as bytes, n flag bytes)"""
        def words(x, count):
            if isinstance(x, (bytes, bytearray, memoryview)):
                x = bytes(x)
                assert len(x) == 4 * count, (len(x), count)
                return x
            assert len(x) == count, (len(x), count)
            return bytes((ctypes.c_int32 * max(count, 1))(*x))[:4 * count]
        ops_b, coef_b = words(operands, n * 72), words(coef, n * 4)
        out = ctypes.create_string_buffer(max(n, 1) * 72)
        flags = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_debug_fq2_limbs", self._lib.bn254_debug_fq2_limbs(self._h, layout, op, ops_b, coef_b, n, out, flags))
        return out.raw[:n * 72], flags.raw[:n]

    # ---- device-pointer entry points (inputs resident in HBM; enqueue only) ---------------
    def register_keys(self, pks, flags=0):
        """replace the context's registered key set (uncompressed G2, 128 B each); returns the per-key status bytes
        (what PublicKey::from_uncompressed reports, subgroup check included)"""
        n = len(pks) // G2_BYTES
        assert len(pks) == n * G2_BYTES
        st = ctypes.create_string_buffer(max(n, 1))
        self.group_key_set = False
        _check("bn254_ctx_register_keys", self._lib.bn254_ctx_register_keys(self._h, bytes(pks), n, flags, st))
        self.n_registered_keys = n
        return st.raw[:n]

    def set_group_key(self, group_pk, flags=0):
        """the group key f(0) * G2 of batch_threshold_combine_keyed_optimistic (include/bn254_hip.h: bn254_ctx_set_group_key): 128 bytes, or
        None to forget it.  Returns the key's decode status (registration's codes); a non-zero status leaves no group key set.  A
        registration (register_keys, register_keys_pop) forgets the group key."""
        assert group_pk is None or len(group_pk) == G2_BYTES
        st = ctypes.create_string_buffer(1)
        self.group_key_set = False
        _check("bn254_ctx_set_group_key", self._lib.bn254_ctx_set_group_key(self._h, None if group_pk is None else bytes(group_pk), flags, st))
        self.group_key_set = group_pk is not None and st.raw[0] == 0
        return st.raw[0]

    def register_keys_pop(self, pks, pops, flags=0):
        """register_keys with every key's proof of possession checked (include/bn254_hip.h: bn254_ctx_register_keys_pop): pops = one 64-byte
        proof per key.  Returns the per-key status bytes — the plain registration's if non-zero, else the proof's under
        flags & FLAG_REJECT_IDENTITY — which ARE the keys' registration statuses: every keyed call refuses an unproven key with 9.
        If the call fails the context is left without keys."""
        n = len(pks) // G2_BYTES
        assert len(pks) == n * G2_BYTES and len(pops) == n * G1_BYTES
        st = ctypes.create_string_buffer(max(n, 1))
        self.n_registered_keys = 0
        self.group_key_set = False
        _check("bn254_ctx_register_keys_pop", self._lib.bn254_ctx_register_keys_pop(self._h, bytes(pks), bytes(pops), n, flags, st))
        self.n_registered_keys = n
        return st.raw[:n]

    def batch_pop_prove(self, sks):
        """n private keys (32 B each) -> (public keys, proofs of possession, status bytes): pk = sk * G2 as batch_g2_mul(None, sks,
        reduce_scalar=True) gives it, pop = sk * H(POP_TAG || pk) as batch_sign gives it"""
        n = len(sks) // SCALAR_BYTES
        assert len(sks) == n * SCALAR_BYTES
        pks = ctypes.create_string_buffer(max(n, 1) * G2_BYTES)
        pops = ctypes.create_string_buffer(max(n, 1) * G1_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_pop_prove", self._lib.bn254_batch_pop_prove(self._h, bytes(sks), n, pks, pops, status))
        return pks.raw[:n * G2_BYTES], pops.raw[:n * G1_BYTES], status.raw[:n]

    def batch_pop_verify(self, pks, pops, flags=0):
        """status bytes of the proofs: batch_verify of message POP_TAG || pk_i, signature pop_i, key pk_i under
        flags | FLAG_G2_SUBGROUP_CHECK.  Pass FLAG_REJECT_IDENTITY: the identity key with the identity proof verifies without it."""
        n = len(pks) // G2_BYTES
        assert len(pks) == n * G2_BYTES and len(pops) == n * G1_BYTES
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_pop_verify", self._lib.bn254_batch_pop_verify(self._h, bytes(pks), bytes(pops), n, flags, status))
        return status.raw[:n]

    def batch_pop_prove_device(self, d_sks, n, d_pks, d_pops, d_status, stream=None):
        _check("bn254_batch_pop_prove_device", self._lib.bn254_batch_pop_prove_device(self._h, d_sks, n, d_pks, d_pops, d_status, stream))

    def batch_pop_verify_device(self, d_pks, d_pops, n, d_status, flags=0, stream=None):
        _check("bn254_batch_pop_verify_device", self._lib.bn254_batch_pop_verify_device(self._h, d_pks, d_pops, n, flags, d_status, stream))

    def batch_verify_keyed(self, messages, sigs, key_idx, flags=0):
        n = len(messages)
        assert len(sigs) == n * g1_item_bytes(flags) and len(key_idx) == n
        msgs, off = pack_messages(messages)
        idx = (ctypes.c_uint32 * max(n, 1))(*key_idx)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_verify_keyed", self._lib.bn254_batch_verify_keyed(self._h, msgs, off, bytes(sigs), idx, n, flags, status))
        return status.raw[:n]

    def batch_verify_keyed_bitmap(self, messages, sigs, bitmaps, bm_words, flags=0):
        """same-message aggregates as signer bitmaps over the registered keys: bitmaps = n * bm_words uint32 words (signer j of tuple i = bit
        j % 32 of bitmaps[i * bm_words + j // 32]); returns the status bytes (include/bn254_hip.h: bn254_batch_verify_keyed_bitmap)"""
        n = len(messages)
        assert len(sigs) == n * g1_item_bytes(flags) and len(bitmaps) == n * bm_words
        msgs, off = pack_messages(messages)
        bits = (ctypes.c_uint32 * max(len(bitmaps), 1))(*bitmaps)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_verify_keyed_bitmap",
               self._lib.bn254_batch_verify_keyed_bitmap(self._h, msgs, off, bytes(sigs), bits, bm_words, n, flags, status))
        return status.raw[:n]

    def batch_verify_keyed_bitmap_device(self, d_msgs, d_off, d_sigs, d_signer_bits, bm_words, n, d_status, flags=0, stream=None):
        _check("bn254_batch_verify_keyed_bitmap_device",
               self._lib.bn254_batch_verify_keyed_bitmap_device(self._h, d_msgs, d_off, d_sigs, d_signer_bits, bm_words, n, flags, d_status, stream))

    # ---- what a bitmap call knows besides a status byte (include/bn254_hip.h: aggregate keys, H(m), voting weight) ----
    def batch_aggregate_keys_bitmap(self, bitmaps, bm_words, n, flags=0):
        """(aggregate keys, status bytes) of n bitmap rows: 128 bytes per row — the uncompressed sum of the set registered keys, zeros for the
        identity and where the status (rule 2 of the bitmap verify) is non-zero"""
        assert len(bitmaps) == n * bm_words
        bits = (ctypes.c_uint32 * max(len(bitmaps), 1))(*bitmaps)
        keys = ctypes.create_string_buffer(max(n, 1) * G2_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_aggregate_keys_bitmap", self._lib.bn254_batch_aggregate_keys_bitmap(self._h, bits, bm_words, n, flags, keys, status))
        return keys.raw[:n * G2_BYTES], status.raw[:n]

    def batch_aggregate_keys_bitmap_device(self, d_signer_bits, bm_words, n, d_agg_keys, d_status, flags=0, stream=None):
        _check("bn254_batch_aggregate_keys_bitmap_device",
               self._lib.bn254_batch_aggregate_keys_bitmap_device(self._h, d_signer_bits, bm_words, n, flags, d_agg_keys, d_status, stream))

    def batch_verify_keyed_bitmap_export(self, messages, sigs, bitmaps, bm_words, flags=0, want_hashes=True, want_keys=True):
        """batch_verify_keyed_bitmap that also returns what it computed: (status bytes, H(m) 64 B each or None, aggregate keys 128 B each or
        None); the outputs of a tuple whose status is neither 0 nor 9 are zero bytes"""
        n = len(messages)
        assert len(sigs) == n * g1_item_bytes(flags) and len(bitmaps) == n * bm_words
        msgs, off = pack_messages(messages)
        bits = (ctypes.c_uint32 * max(len(bitmaps), 1))(*bitmaps)
        status = ctypes.create_string_buffer(max(n, 1))
        hashes = ctypes.create_string_buffer(max(n, 1) * G1_BYTES) if want_hashes else None
        keys = ctypes.create_string_buffer(max(n, 1) * G2_BYTES) if want_keys else None
        _check("bn254_batch_verify_keyed_bitmap_export",
               self._lib.bn254_batch_verify_keyed_bitmap_export(self._h, msgs, off, bytes(sigs), bits, bm_words, n, flags, status, hashes, keys))
        return status.raw[:n], hashes.raw[:n * G1_BYTES] if want_hashes else None, keys.raw[:n * G2_BYTES] if want_keys else None

    def batch_verify_keyed_bitmap_export_device(self, d_msgs, d_off, d_sigs, d_signer_bits, bm_words, n, d_status, d_hashes, d_agg_keys, flags=0, stream=None):
        _check("bn254_batch_verify_keyed_bitmap_export_device",
               self._lib.bn254_batch_verify_keyed_bitmap_export_device(self._h, d_msgs, d_off, d_sigs, d_signer_bits, bm_words, n, flags, d_status, d_hashes,
                                                                       d_agg_keys, stream))

    def set_key_weights(self, weights):
        """voting weights of the registered keys (one unsigned 64-bit integer per key, total below 2^64), or None to forget them; every
        registration forgets them"""
        if weights is None:
            _check("bn254_ctx_set_key_weights", self._lib.bn254_ctx_set_key_weights(self._h, None, 0))
            return
        n = len(weights)
        if any(w < 0 or w >> 64 for w in weights):
            raise ValueError("a weight does not fit 64 bits")
        arr = (ctypes.c_uint64 * max(n, 1))(*weights)
        _check("bn254_ctx_set_key_weights", self._lib.bn254_ctx_set_key_weights(self._h, arr, n))

    def batch_bitmap_weights(self, bitmaps, bm_words, n):
        """(weights, status bytes) of n bitmap rows: the sum of the set keys' weights where rule 2 of the bitmap verify gives 0, else 0"""
        assert len(bitmaps) == n * bm_words
        bits = (ctypes.c_uint32 * max(len(bitmaps), 1))(*bitmaps)
        weight = (ctypes.c_uint64 * max(n, 1))()
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_bitmap_weights", self._lib.bn254_batch_bitmap_weights(self._h, bits, bm_words, n, weight, status))
        return list(weight[:n]), status.raw[:n]

    def batch_bitmap_weights_device(self, d_signer_bits, bm_words, n, d_weight, d_status, stream=None):
        _check("bn254_batch_bitmap_weights_device", self._lib.bn254_batch_bitmap_weights_device(self._h, d_signer_bits, bm_words, n, d_weight, d_status, stream))

    @staticmethod
    def _collect_buffers(messages, shares, share_keys, sizes, bm_words, flags=0):
        """what the collect and the threshold call marshal alike: the C arguments behind the context (msgs .. bm_words) and the five output
        buffers (share statuses, tuple statuses, one G1 point per tuple, the bitmap rows, one count per tuple)"""
        n, n_shares = len(messages), len(share_keys)
        assert len(sizes) == n and all(k >= 0 for k in sizes) and sum(sizes) == n_shares and len(shares) == n_shares * g1_item_bytes(flags)
        msgs, off = pack_messages(messages)
        ends = [0]
        for k in sizes:
            ends.append(ends[-1] + int(k))
        share_off = (ctypes.c_uint64 * (n + 1))(*ends)
        keys = (ctypes.c_uint32 * max(n_shares, 1))(*share_keys)
        outs = (ctypes.create_string_buffer(max(n_shares, 1)), ctypes.create_string_buffer(max(n, 1)), ctypes.create_string_buffer(max(n, 1) * G1_BYTES),
                (ctypes.c_uint32 * max(n * bm_words, 1))(), (ctypes.c_uint32 * max(n, 1))())
        return (msgs, off, bytes(shares), keys, share_off, n_shares, n, bm_words), outs

    def batch_collect_keyed_bitmap(self, messages, shares, share_keys, sizes, bm_words, flags=0, want_counts=False, seed32=None, optimistic=False):
        """build signer-bitmap aggregates from individual signatures (include/bn254_hip.h: bn254_batch_collect_keyed_bitmap): tuple i is
        messages[i] with the next sizes[i] shares (64 B each, 33 B under FLAG_G1_COMPRESSED; share s said to be by registered key share_keys[s]).  Returns (share status
        bytes, tuple status bytes, the n aggregates, the n * bm_words bitmap words) — and the signer counts with want_counts.
        seed32: see batch_collect_keyed_bitmap_randomized; optimistic: see batch_collect_keyed_bitmap_optimistic."""
        n, n_shares = len(messages), len(share_keys)
        args, (share_st, tuple_st, agg, bits, counts) = Engine._collect_buffers(messages, shares, share_keys, sizes, bm_words, flags)
        head = (self._h,) + args + (flags,)
        tail = (share_st, tuple_st, agg, bits, counts if want_counts else None)
        if optimistic:
            _check("bn254_batch_collect_keyed_bitmap_optimistic", self._lib.bn254_batch_collect_keyed_bitmap_optimistic(*head, *tail))
        elif seed32 is not None:
            _check("bn254_batch_collect_keyed_bitmap_randomized", self._lib.bn254_batch_collect_keyed_bitmap_randomized(*head, bytes(seed32), *tail))
        else:
            _check("bn254_batch_collect_keyed_bitmap", self._lib.bn254_batch_collect_keyed_bitmap(*head, *tail))
        out = (share_st.raw[:n_shares], tuple_st.raw[:n], agg.raw[:n * G1_BYTES], list(bits)[:n * bm_words])
        return out + (list(counts)[:n],) if want_counts else out

    def batch_threshold_combine_keyed(self, messages, shares, share_keys, sizes, bm_words, threshold, flags=0):
        """t-of-n threshold signatures over the registered keys (include/bn254_hip.h: bn254_batch_threshold_combine_keyed): the arguments of
        batch_collect_keyed_bitmap and the threshold.  Returns (share status bytes, tuple status bytes, the n group signatures, the
        n * bm_words words of the rows — the keys used, or of a failed tuple the keys that were there —, the counts of keys with a valid share)."""
        n, n_shares = len(messages), len(share_keys)
        args, (share_st, tuple_st, sigs, bits, counts) = Engine._collect_buffers(messages, shares, share_keys, sizes, bm_words, flags)
        assert 0 < int(threshold) < 1 << 32, "threshold must be at least 1"
        _check("bn254_batch_threshold_combine_keyed",
               self._lib.bn254_batch_threshold_combine_keyed(self._h, *args, int(threshold), flags, share_st, tuple_st, sigs, bits, counts))
        return share_st.raw[:n_shares], tuple_st.raw[:n], sigs.raw[:n * G1_BYTES], list(bits)[:n * bm_words], list(counts)[:n]

    def batch_threshold_combine_keyed_optimistic(self, messages, shares, share_keys, sizes, bm_words, threshold, flags=0):
        """batch_threshold_combine_keyed by interpolating first and verifying each tuple's result once under the group key (set_group_key;
        include/bn254_hip.h: bn254_batch_threshold_combine_keyed_optimistic).  Same arguments, same five results; in a tuple that passes its
        check the shares outside the kept keys read their pre-check status and the count is of candidates."""
        n, n_shares = len(messages), len(share_keys)
        args, (share_st, tuple_st, sigs, bits, counts) = Engine._collect_buffers(messages, shares, share_keys, sizes, bm_words, flags)
        assert 0 < int(threshold) < 1 << 32, "threshold must be at least 1"
        _check("bn254_batch_threshold_combine_keyed_optimistic",
               self._lib.bn254_batch_threshold_combine_keyed_optimistic(self._h, *args, int(threshold), flags, share_st, tuple_st, sigs, bits, counts))
        return share_st.raw[:n_shares], tuple_st.raw[:n], sigs.raw[:n * G1_BYTES], list(bits)[:n * bm_words], list(counts)[:n]

    def batch_threshold_combine_keyed_optimistic_device(self, d_msgs, d_msg_off, d_shares, d_share_key, d_share_off, n_shares, n, bm_words, threshold,
                                                        d_share_status, d_tuple_status, d_group_sigs, d_used_bits, d_n_valid=None, flags=0, stream=None):
        _check("bn254_batch_threshold_combine_keyed_optimistic_device",
               self._lib.bn254_batch_threshold_combine_keyed_optimistic_device(self._h, d_msgs, d_msg_off, d_shares, d_share_key, d_share_off, n_shares, n,
                                                                               bm_words, threshold, flags, d_share_status, d_tuple_status, d_group_sigs,
                                                                               d_used_bits, d_n_valid, stream))

    def batch_threshold_combine_keyed_device(self, d_msgs, d_msg_off, d_shares, d_share_key, d_share_off, n_shares, n, bm_words, threshold,
                                             d_share_status, d_tuple_status, d_group_sigs, d_used_bits, d_n_valid=None, flags=0, stream=None):
        _check("bn254_batch_threshold_combine_keyed_device",
               self._lib.bn254_batch_threshold_combine_keyed_device(self._h, d_msgs, d_msg_off, d_shares, d_share_key, d_share_off, n_shares, n, bm_words,
                                                                    threshold, flags, d_share_status, d_tuple_status, d_group_sigs, d_used_bits, d_n_valid,
                                                                    stream))

    def batch_collect_keyed_bitmap_device(self, d_msgs, d_msg_off, d_shares, d_share_key, d_share_off, n_shares, n, bm_words, d_share_status,
                                          d_tuple_status, d_agg_sigs, d_signer_bits, d_n_signers=None, flags=0, stream=None):
        _check("bn254_batch_collect_keyed_bitmap_device",
               self._lib.bn254_batch_collect_keyed_bitmap_device(self._h, d_msgs, d_msg_off, d_shares, d_share_key, d_share_off, n_shares, n, bm_words,
                                                                 flags, d_share_status, d_tuple_status, d_agg_sigs, d_signer_bits, d_n_signers, stream))

    def merge_keyed_bitmap(self, messages, parts, part_bitmaps, sizes, bm_words, flags=0, want_counts=False, optimistic=False):
        """merge partial signer-bitmap aggregates into one aggregate per message (include/bn254_hip.h: bn254_batch_merge_keyed_bitmap):
        tuple i is messages[i] with the next sizes[i] partials (64 B each, 33 B under FLAG_G1_COMPRESSED; partial p has the bm_words bitmap words part_bitmaps[p * bm_words
        ..]).  Returns (partial status bytes, taken bytes, tuple status bytes, the n aggregates, the n * bm_words bitmap words) — and the
        signer counts with want_counts.  optimistic: see merge_keyed_bitmap_optimistic."""
        n = len(messages)
        assert len(sizes) == n and all(k >= 0 for k in sizes)
        n_parts = sum(int(k) for k in sizes)
        assert len(parts) == n_parts * g1_item_bytes(flags) and len(part_bitmaps) == n_parts * bm_words
        name = "bn254_batch_merge_keyed_bitmap_optimistic" if optimistic else "bn254_batch_merge_keyed_bitmap"
        msgs, off = pack_messages(messages)
        ends = [0]
        for k in sizes:
            ends.append(ends[-1] + int(k))
        part_off = (ctypes.c_uint64 * (n + 1))(*ends)
        rows = (ctypes.c_uint32 * max(n_parts * bm_words, 1))(*part_bitmaps)
        part_st = ctypes.create_string_buffer(max(n_parts, 1))
        taken = ctypes.create_string_buffer(max(n_parts, 1))
        tuple_st = ctypes.create_string_buffer(max(n, 1))
        agg = ctypes.create_string_buffer(max(n, 1) * G1_BYTES)
        bits = (ctypes.c_uint32 * max(n * bm_words, 1))()
        counts = (ctypes.c_uint32 * max(n, 1))()
        _check(name, getattr(self._lib, name)(self._h, msgs, off, bytes(parts), rows, part_off, n_parts, n, bm_words, flags, part_st, taken, tuple_st, agg, bits,
                                              counts if want_counts else None))
        out = (part_st.raw[:n_parts], taken.raw[:n_parts], tuple_st.raw[:n], agg.raw[:n * G1_BYTES], list(bits)[:n * bm_words])
        return out + (list(counts)[:n],) if want_counts else out

    def merge_keyed_bitmap_device(self, d_msgs, d_msg_off, d_parts, d_part_bits, d_part_off, n_parts, n, bm_words, d_part_status, d_part_taken,
                                  d_tuple_status, d_agg_sigs, d_signer_bits, d_n_signers=None, flags=0, stream=None):
        """the device-pointer form: enqueues only (include/bn254_hip.h: bn254_batch_merge_keyed_bitmap_device)"""
        _check("bn254_batch_merge_keyed_bitmap_device",
               self._lib.bn254_batch_merge_keyed_bitmap_device(self._h, d_msgs, d_msg_off, d_parts, d_part_bits, d_part_off, n_parts, n, bm_words, flags,
                                                               d_part_status, d_part_taken, d_tuple_status, d_agg_sigs, d_signer_bits, d_n_signers, stream))

    def merge_keyed_bitmap_optimistic(self, messages, parts, part_bitmaps, sizes, bm_words, flags=0, want_counts=False):
        """merge_keyed_bitmap with ONE verify per tuple — the sum of its candidate partials against the keys of their union row — and the
        partials checked one by one only where that fails or two candidates overlap (include/bn254_hip.h:
        bn254_batch_merge_keyed_bitmap_optimistic).  The same six outputs, except that partials whose errors cancel within a passing tuple
        read 0 and are taken."""
        return Engine.merge_keyed_bitmap(self, messages, parts, part_bitmaps, sizes, bm_words, flags, want_counts, optimistic=True)

    def merge_keyed_bitmap_optimistic_device(self, d_msgs, d_msg_off, d_parts, d_part_bits, d_part_off, n_parts, n, bm_words, d_part_status, d_part_taken,
                                             d_tuple_status, d_agg_sigs, d_signer_bits, d_n_signers=None, flags=0, stream=None):
        """the device-pointer form: enqueues only (include/bn254_hip.h: bn254_batch_merge_keyed_bitmap_optimistic_device)"""
        _check("bn254_batch_merge_keyed_bitmap_optimistic_device",
               self._lib.bn254_batch_merge_keyed_bitmap_optimistic_device(self._h, d_msgs, d_msg_off, d_parts, d_part_bits, d_part_off, n_parts, n, bm_words,
                                                                          flags, d_part_status, d_part_taken, d_tuple_status, d_agg_sigs, d_signer_bits,
                                                                          d_n_signers, stream))

    def batch_collect_keyed_bitmap_optimistic(self, messages, shares, share_keys, sizes, bm_words, flags=0, want_counts=False):
        """batch_collect_keyed_bitmap with ONE verify per tuple — the sum of its candidate shares against the sum of their keys — and the
        shares checked one by one only where that fails (include/bn254_hip.h: bn254_batch_collect_keyed_bitmap_optimistic).  The same five
        outputs, except that shares whose errors cancel within a passing tuple read 0."""
        return Engine.batch_collect_keyed_bitmap(self, messages, shares, share_keys, sizes, bm_words, flags, want_counts, optimistic=True)

    def batch_collect_keyed_bitmap_optimistic_device(self, d_msgs, d_msg_off, d_shares, d_share_key, d_share_off, n_shares, n, bm_words, d_share_status,
                                                     d_tuple_status, d_agg_sigs, d_signer_bits, d_n_signers=None, flags=0, stream=None):
        _check("bn254_batch_collect_keyed_bitmap_optimistic_device",
               self._lib.bn254_batch_collect_keyed_bitmap_optimistic_device(self._h, d_msgs, d_msg_off, d_shares, d_share_key, d_share_off, n_shares, n,
                                                                            bm_words, flags, d_share_status, d_tuple_status, d_agg_sigs, d_signer_bits,
                                                                            d_n_signers, stream))

    def batch_collect_keyed_bitmap_randomized(self, messages, shares, share_keys, sizes, bm_words, seed32, flags=0, want_counts=False):
        """batch_collect_keyed_bitmap with the pairing checks of the shares combined, 64 shares of one key at a time, under random weights
        from seed32 (include/bn254_hip.h: bn254_batch_collect_keyed_bitmap_randomized; flags: FLAG_RAND64 / FLAG_RAND_GLV and the decode
        flags).  The same outputs, byte for byte."""
        assert len(seed32) == 32
        return Engine.batch_collect_keyed_bitmap(self, messages, shares, share_keys, sizes, bm_words, flags, want_counts, seed32=seed32)

    def batch_collect_keyed_bitmap_randomized_device(self, d_msgs, d_msg_off, d_shares, d_share_key, d_share_off, n_shares, n, bm_words, seed32,
                                                     d_share_status, d_tuple_status, d_agg_sigs, d_signer_bits, d_n_signers=None, flags=0, stream=None):
        assert len(seed32) == 32
        _check("bn254_batch_collect_keyed_bitmap_randomized_device",
               self._lib.bn254_batch_collect_keyed_bitmap_randomized_device(self._h, d_msgs, d_msg_off, d_shares, d_share_key, d_share_off, n_shares, n,
                                                                            bm_words, flags, bytes(seed32), d_share_status, d_tuple_status, d_agg_sigs,
                                                                            d_signer_bits, d_n_signers, stream))

    def batch_verify_keyed_bitmap_randomized(self, messages, sigs, bitmaps, bm_words, seed32, flags=0):
        """batch_verify_keyed_bitmap with the pairing checks of whole groups of tuples combined under random weights from seed32
        (include/bn254_hip.h: bn254_batch_verify_keyed_bitmap_randomized).  Returns the status bytes."""
        n = len(messages)
        assert len(sigs) == n * g1_item_bytes(flags) and len(bitmaps) == n * bm_words and len(seed32) == 32
        msgs, off = pack_messages(messages)
        bits = (ctypes.c_uint32 * max(len(bitmaps), 1))(*bitmaps)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_verify_keyed_bitmap_randomized",
               self._lib.bn254_batch_verify_keyed_bitmap_randomized(self._h, msgs, off, bytes(sigs), bits, bm_words, n, flags, bytes(seed32), status))
        return status.raw[:n]

    def batch_verify_keyed_bitmap_randomized_device(self, d_msgs, d_off, d_sigs, d_signer_bits, bm_words, n, seed32, d_status, flags=0, stream=None):
        assert len(seed32) == 32
        _check("bn254_batch_verify_keyed_bitmap_randomized_device",
               self._lib.bn254_batch_verify_keyed_bitmap_randomized_device(self._h, d_msgs, d_off, d_sigs, d_signer_bits, bm_words, n, flags,
                                                                           bytes(seed32), d_status, stream))

    def batch_verify_keyed_randomized(self, messages, sigs, key_idx, seed32, flags=0):
        n = len(messages)
        assert len(sigs) == n * g1_item_bytes(flags) and len(key_idx) == n and len(seed32) == 32
        msgs, off = pack_messages(messages)
        idx = (ctypes.c_uint32 * max(n, 1))(*key_idx)
        status = ctypes.create_string_buffer(max(n, 1))
        _check("bn254_batch_verify_keyed_randomized",
               self._lib.bn254_batch_verify_keyed_randomized(self._h, msgs, off, bytes(sigs), idx, n, flags, bytes(seed32), status))
        return status.raw[:n]

    def batch_verify_keyed_randomized_device(self, d_msgs, d_off, d_sigs, d_key_idx, n, seed32, d_status, flags=0, stream=None):
        assert len(seed32) == 32
        _check("bn254_batch_verify_keyed_randomized_device",
               self._lib.bn254_batch_verify_keyed_randomized_device(self._h, d_msgs, d_off, d_sigs, d_key_idx, n, flags, bytes(seed32), d_status, stream))

    def batch_verify_keyed_device(self, d_msgs, d_off, d_sigs, d_key_idx, n, d_status, flags=0, stream=None):
        _check("bn254_batch_verify_keyed_device",
               self._lib.bn254_batch_verify_keyed_device(self._h, d_msgs, d_off, d_sigs, d_key_idx, n, flags, d_status, stream))

    def batch_verify_device(self, d_msgs, d_off, d_sigs, d_pks, n, d_status, flags=0, stream=None):
        _check("bn254_batch_verify_device",
               self._lib.bn254_batch_verify_device(self._h, d_msgs, d_off, d_sigs, d_pks, n, flags, d_status, stream))

    def batch_verify_compressed_device(self, d_msgs, d_off, d_sigs33, d_pks65, n, d_status, stream=None):
        """batch_verify_device from the compressed encodings (33-byte signatures, 65-byte public keys, any byte alignment)"""
        _check("bn254_batch_verify_compressed_device",
               self._lib.bn254_batch_verify_compressed_device(self._h, d_msgs, d_off, d_sigs33, d_pks65, n, d_status, stream))

    def batch_verify_randomized_device(self, d_msgs, d_off, d_sigs, d_pks, n, seed32, d_status, d_group_ok=None, flags=0, stream=None):
        assert len(seed32) == 32
        _check("bn254_batch_verify_randomized_device",
               self._lib.bn254_batch_verify_randomized_device(self._h, d_msgs, d_off, d_sigs, d_pks, n, flags, bytes(seed32), d_status, d_group_ok, stream))

    def batch_hash_to_g1_device(self, d_msgs, d_off, n, d_points, d_status, d_tries=None, stream=None):
        _check("bn254_batch_hash_to_g1_device",
               self._lib.bn254_batch_hash_to_g1_device(self._h, d_msgs, d_off, n, d_points, d_status, d_tries, stream))

    def batch_pairing_device(self, d_g1, d_g2, n, k, d_gt, d_status, flags=0, stream=None):
        _check("bn254_batch_pairing_device", self._lib.bn254_batch_pairing_device(self._h, d_g1, d_g2, n, k, flags, d_gt, d_status, stream))

    def batch_aggregate_verify_device(self, d_msgs, d_msg_off, n_msgs, d_pk_pool, n_signers, d_sig_pool, d_tuple_msg, d_tuple_off, d_signer_idx, n,
                                      d_status, flags=0, stream=None):
        _check("bn254_batch_aggregate_verify_device",
               self._lib.bn254_batch_aggregate_verify_device(self._h, d_msgs, d_msg_off, n_msgs, d_pk_pool, n_signers, d_sig_pool, d_tuple_msg,
                                                             d_tuple_off, d_signer_idx, n, flags, d_status, stream))

    def batch_aggregate_verify_distinct_device(self, d_msgs, d_msg_off, d_pks, m, d_agg_sigs, d_agg_off, n, d_status, flags=0, stream=None):
        _check("bn254_batch_aggregate_verify_distinct_device",
               self._lib.bn254_batch_aggregate_verify_distinct_device(self._h, d_msgs, d_msg_off, d_pks, m, d_agg_sigs, d_agg_off, n, flags, d_status,
                                                                      stream))

    def batch_aggregate_verify_distinct_keyed_randomized_device(self, d_msgs, d_msg_off, d_key_idx, m, d_agg_sigs, d_agg_off, n, seed32, d_status, flags=0,
                                                                stream=None):
        assert len(seed32) == 32
        _check("bn254_batch_aggregate_verify_distinct_keyed_randomized_device",
               self._lib.bn254_batch_aggregate_verify_distinct_keyed_randomized_device(self._h, d_msgs, d_msg_off, d_key_idx, m, d_agg_sigs, d_agg_off, n,
                                                                                       flags, bytes(seed32), d_status, stream))

    def batch_aggregate_verify_distinct_keyed_device(self, d_msgs, d_msg_off, d_key_idx, m, d_agg_sigs, d_agg_off, n, d_status, flags=0, stream=None):
        _check("bn254_batch_aggregate_verify_distinct_keyed_device",
               self._lib.bn254_batch_aggregate_verify_distinct_keyed_device(self._h, d_msgs, d_msg_off, d_key_idx, m, d_agg_sigs, d_agg_off, n, flags,
                                                                            d_status, stream))

    def batch_sign_device(self, d_msgs, d_off, d_sks, n, d_sigs, d_status, stream=None):
        _check("bn254_batch_sign_device", self._lib.bn254_batch_sign_device(self._h, d_msgs, d_off, d_sks, n, d_sigs, d_status, stream))

    def batch_g2_mul_device(self, d_points, d_scalars, n, d_out, d_status, reduce_scalar=False, stream=None):
        _check("bn254_batch_g2_mul_device",
               self._lib.bn254_batch_g2_mul_device(self._h, d_points, d_scalars, n, int(reduce_scalar), d_out, d_status, stream))

    def batch_g1_mul_device(self, d_points, d_scalars, n, d_out, d_status, reduce_scalar=False, stream=None):
        _check("bn254_batch_g1_mul_device",
               self._lib.bn254_batch_g1_mul_device(self._h, d_points, d_scalars, n, int(reduce_scalar), d_out, d_status, stream))


MGPU_OPT_GATHER = 1
MGPU_OPT_TIMING = 2
MGPU_GATHER_AUTO, MGPU_GATHER_RCCL, MGPU_GATHER_COPY = 0, 1, 2


def shard_range(n_total, g, n_dev):
    """contiguous slice [lo, hi) of ceil(n_total / n_dev) items owned by entry g — the arithmetic of bn254_mgpu_shard_range
    (include/bn254_hip.h), restated here so that it can be checked without a GPU"""
    per = (n_total + n_dev - 1) // n_dev
    lo = min(n_total, g * per)
    return lo, min(n_total, lo + per)


class _EngineView(Engine):
    """an Engine over a context OWNED by a MultiEngine (options, reserve, register_keys per device); never destroys it"""

    def __init__(self, lib, handle, device):
        self._lib, self._h, self.device = lib, handle, device

    def close(self):
        self._h = None


class MultiEngine:
    """The batch sharded over the GPUs of one node from ONE process (include/bn254_hip.h, section "Multi-GPU"): one context, one
    stream and one parked worker thread per entry of `devices`; the only exchange between devices is the gather of the status bytes
    (RCCL's C API; peer copies when a device is listed twice)."""

    def __init__(self, devices):
        self._lib = _native.load()
        self.devices = list(devices)
        arr = (ctypes.c_int * len(self.devices))(*self.devices)
        h = ctypes.c_void_p()
        _check("bn254_mgpu_create", self._lib.bn254_mgpu_create(arr, len(self.devices), ctypes.byref(h)))
        self._h = h
        self.n_dev = len(self.devices)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bn254_mgpu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, fn, rc):
        if rc == -10004:
            raise NativeError(fn + " [" + self._lib.bn254_mgpu_last_error(self._h).decode(errors="replace") + "]", rc)
        _check(fn, rc)

    def engine(self, g):
        return _EngineView(self._lib, ctypes.c_void_p(self._lib.bn254_mgpu_ctx(self._h, g)), self.devices[g])

    def shard_len(self, n):
        return self._lib.bn254_mgpu_shard_len(self._h, n)

    def gathered_len(self, n):
        return self._lib.bn254_mgpu_gathered_len(self._h, n)

    def shard_range(self, n, g):
        lo, hi = ctypes.c_size_t(), ctypes.c_size_t()
        _check("bn254_mgpu_shard_range", self._lib.bn254_mgpu_shard_range(self._h, n, g, ctypes.byref(lo), ctypes.byref(hi)))
        return lo.value, hi.value

    def reserve(self, n_total, init_collectives=False):
        self._check("bn254_mgpu_reserve", self._lib.bn254_mgpu_reserve(self._h, n_total, int(init_collectives)))

    def synchronize(self):
        _check("bn254_mgpu_synchronize", self._lib.bn254_mgpu_synchronize(self._h))

    def set_option(self, option, value):
        _check("bn254_mgpu_set_option", self._lib.bn254_mgpu_set_option(self._h, option, value))

    def last_timing(self):
        """per device: (compute ms, collective ms) of the last call (MGPU_OPT_TIMING on)"""
        a, b = (ctypes.c_float * self.n_dev)(), (ctypes.c_float * self.n_dev)()
        _check("bn254_mgpu_last_timing", self._lib.bn254_mgpu_last_timing(self._h, a, b))
        return list(a), list(b)

    # ---- host-pointer entry points: the whole batch in, the whole result out ---------------------------------------------
    def batch_verify(self, messages, sigs, pks, flags=0):
        n = len(messages)
        assert len(sigs) == n * G1_BYTES and len(pks) == n * G2_BYTES
        msgs, off = pack_messages(messages)
        status = ctypes.create_string_buffer(max(n, 1))
        self._check("bn254_mgpu_batch_verify", self._lib.bn254_mgpu_batch_verify(self._h, msgs, off, bytes(sigs), bytes(pks), n, flags, status))
        return status.raw[:n]

    def batch_hash_to_g1(self, messages):
        n = len(messages)
        msgs, off = pack_messages(messages)
        pts = ctypes.create_string_buffer(max(n, 1) * G1_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        tries = ctypes.create_string_buffer(max(n, 1))
        self._check("bn254_mgpu_batch_hash_to_g1", self._lib.bn254_mgpu_batch_hash_to_g1(self._h, msgs, off, n, pts, status, tries))
        return pts.raw[:n * G1_BYTES], status.raw[:n], tries.raw[:n]

    def batch_verify_compressed(self, messages, sigs33, pks65):
        n = len(messages)
        assert len(sigs33) == n * 33 and len(pks65) == n * 65
        msgs, off = pack_messages(messages)
        status = ctypes.create_string_buffer(max(n, 1))
        self._check("bn254_mgpu_batch_verify_compressed",
                    self._lib.bn254_mgpu_batch_verify_compressed(self._h, msgs, off, bytes(sigs33), bytes(pks65), n, status))
        return status.raw[:n]

    def register_keys(self, pks, flags=0):
        """the whole key set on every device -> per-key status bytes"""
        n = len(pks) // G2_BYTES
        st = ctypes.create_string_buffer(max(n, 1))
        self._check("bn254_mgpu_register_keys", self._lib.bn254_mgpu_register_keys(self._h, bytes(pks), n, flags, st))
        return st.raw[:n]

    def register_keys_pop(self, pks, pops, flags=0):
        """... with every key's proof of possession (64 B each) checked on every device -> per-key status bytes (Engine.register_keys_pop)"""
        n = len(pks) // G2_BYTES
        assert len(pks) == n * G2_BYTES and len(pops) == n * G1_BYTES
        st = ctypes.create_string_buffer(max(n, 1))
        self._check("bn254_mgpu_register_keys_pop", self._lib.bn254_mgpu_register_keys_pop(self._h, bytes(pks), bytes(pops), n, flags, st))
        return st.raw[:n]

    def batch_verify_keyed(self, messages, sigs, key_idx, flags=0):
        n = len(messages)
        assert len(sigs) == n * G1_BYTES and len(key_idx) == n
        msgs, off = pack_messages(messages)
        idx = (ctypes.c_uint32 * max(n, 1))(*key_idx)
        status = ctypes.create_string_buffer(max(n, 1))
        self._check("bn254_mgpu_batch_verify_keyed", self._lib.bn254_mgpu_batch_verify_keyed(self._h, msgs, off, bytes(sigs), idx, n, flags, status))
        return status.raw[:n]

    def batch_aggregate_verify(self, messages, pk_pool, sig_pool, tuple_msg, signer_lists, flags=0):
        """as Engine.batch_aggregate_verify, the tuples sharded over the devices"""
        n, n_msgs = len(tuple_msg), len(messages)
        n_signers = len(pk_pool) // G2_BYTES
        assert len(sig_pool) == n_msgs * n_signers * G1_BYTES and len(signer_lists) == n
        msgs, off = pack_messages(messages)
        t_off = (ctypes.c_uint64 * (n + 1))()
        flat = []
        for i, lst in enumerate(signer_lists):
            t_off[i] = len(flat)
            flat.extend(lst)
        t_off[n] = len(flat)
        idx = (ctypes.c_uint32 * max(len(flat), 1))(*flat)
        tm = (ctypes.c_uint32 * max(n, 1))(*tuple_msg)
        status = ctypes.create_string_buffer(max(n, 1))
        self._check("bn254_mgpu_batch_aggregate_verify",
                    self._lib.bn254_mgpu_batch_aggregate_verify(self._h, msgs, off, n_msgs, bytes(pk_pool), n_signers, bytes(sig_pool), tm, t_off, idx, n,
                                                                flags, status))
        return status.raw[:n]

    def batch_pairing(self, g1s, g2s, n, k=1, flags=0):
        """-> (Gt bytes, status bytes, checksum = sum mod 2^64 of the little-endian 64-bit words of all Gt bytes)"""
        assert len(g1s) == n * k * G1_BYTES and len(g2s) == n * k * G2_BYTES
        gt = ctypes.create_string_buffer(max(n, 1) * GT_BYTES)
        status = ctypes.create_string_buffer(max(n, 1))
        cs = ctypes.c_uint64(0)
        self._check("bn254_mgpu_batch_pairing",
                    self._lib.bn254_mgpu_batch_pairing(self._h, bytes(g1s), bytes(g2s), n, k, flags, gt, status, ctypes.byref(cs)))
        return gt.raw[:n * GT_BYTES], status.raw[:n], cs.value

    # ---- device-pointer entry points: per-device lists of raw device pointers (ints), enqueue only ---------------------
    def _ptrs(self, seq):
        if seq is None:
            return None
        assert len(seq) == self.n_dev
        return (ctypes.c_void_p * self.n_dev)(*[ctypes.c_void_p(p) if p else None for p in seq])

    def batch_verify_device(self, d_msgs, d_off, d_sigs, d_pks, n, d_status_all, flags=0, streams=None):
        self._check("bn254_mgpu_batch_verify_device",
                    self._lib.bn254_mgpu_batch_verify_device(self._h, self._ptrs(d_msgs), self._ptrs(d_off), self._ptrs(d_sigs), self._ptrs(d_pks),
                                                             n, flags, self._ptrs(d_status_all), self._ptrs(streams)))

    def batch_pairing_device(self, d_g1, d_g2, n, k, d_gt, d_status_all, d_checksum=None, flags=0, streams=None):
        self._check("bn254_mgpu_batch_pairing_device",
                    self._lib.bn254_mgpu_batch_pairing_device(self._h, self._ptrs(d_g1), self._ptrs(d_g2), n, k, flags, self._ptrs(d_gt),
                                                              self._ptrs(d_status_all), self._ptrs(d_checksum), self._ptrs(streams)))


_default = {}


def default_engine(device=0):
    if device not in _default:
        _default[device] = Engine(device)
    return _default[device]
