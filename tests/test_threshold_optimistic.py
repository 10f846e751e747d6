"""The optimistic threshold call (include/bn254_hip.h: bn254_ctx_set_group_key, bn254_batch_threshold_combine_keyed_optimistic[_device],
bn254_debug_threshold_opt_last, BN254_OPT_THRESHOLD_OPT_MIN_SHARES) without a GPU: declared with the exact call's arity, exported with
matching argtypes, the option numbered in the header and in the Python mirror, bound in INTEGRATION.md's extern block, mirrored in bn254.hpp
(which compiles, with its example, against the library); the header states the contract; the Python mirrors refuse malformed items and a
missing group key before they touch a device; the model restates the rules on a tuple of each kind."""
import os
import re
import subprocess

import pytest

from bn254_amd import _native
from tests import threshold_opt_model as OM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ["bn254_batch_threshold_combine_keyed", "bn254_batch_threshold_combine_keyed_device"]
NAMES = ["bn254_batch_threshold_combine_keyed_optimistic", "bn254_batch_threshold_combine_keyed_optimistic_device"]
OTHERS = {"bn254_ctx_set_group_key": 4, "bn254_debug_threshold_opt_last": 2}


def _arity(decl):
    return len([a for a in decl.split(",") if a.strip()])


def _header():
    return open(os.path.join(ROOT, "include", "bn254_hip.h")).read()


def _header_decls(names):
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    return {name: re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr) for name in names}


def _types(decl):
    """the argument types of a declaration, names dropped"""
    return [re.sub(r"\s*\b\w+$", "", a.strip()) for a in decl.split(",")]


def test_declared_with_the_exact_calls_arguments():
    decls = _header_decls(EXACT + NAMES + list(OTHERS))
    for name in NAMES + list(OTHERS):
        assert decls[name], name
        assert name in _native.EXPORTED_SYMBOLS
    for exact, opt, arity in zip(EXACT, NAMES, (16, 17)):
        assert _arity(decls[opt].group(1)) == arity == _arity(decls[exact].group(1))
        assert _types(decls[opt].group(1)) == _types(decls[exact].group(1)), opt          # the same arguments in the same order
    for name, arity in OTHERS.items():
        assert _arity(decls[name].group(1)) == arity, name
    assert "const uint8_t *group_pk" in decls["bn254_ctx_set_group_key"].group(1) and "uint8_t *status" in decls["bn254_ctx_set_group_key"].group(1)
    assert "uint64_t out[4]" in decls["bn254_debug_threshold_opt_last"].group(1)


def test_option_number_in_header_and_mirror():
    from bn254_amd import engine
    hdr = _header()
    numbers = {name: int(v) for name, v in re.findall(r"#define (BN254_OPT_\w+) (\d+)", hdr)}
    assert numbers["BN254_OPT_THRESHOLD_OPT_MIN_SHARES"] == 46 == engine.OPT_THRESHOLD_OPT_MIN_SHARES
    assert max(numbers.values()) == 46 and list(numbers.values()).count(46) == 1       # the next free number after 45, used once
    ws = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    default = int(re.search(r"#define THRESHOLD_OPT_MIN_SHARES_DEFAULT (\d+)", ws).group(1))
    assert default == engine.THRESHOLD_OPT_MIN_SHARES_DEFAULT
    text = re.search(r"#define BN254_OPT_THRESHOLD_OPT_MIN_SHARES 46 /\*(.*?)\*/", hdr, flags=re.S).group(1)
    assert ("Default %d" % default) in text and "0 = no lower bound" in text


def test_header_states_the_contract():
    hdr = _header()
    body = hdr[hdr.index("OPTIMISTIC THRESHOLD COMBINE"):hdr.index("int bn254_batch_threshold_combine_keyed_optimistic(")]
    for phrase in ("WHAT IS PROVED", "IDENTITY A", "IDENTITY B", "DEVIATION 1", "DEVIATION 2", "WHOLE-CALL ROUTING", "No seed, no randomness",
                   "no group key set returns BN254_E_BAD_ARGUMENT", "never synchronises with the host", "ms[3] exact fallback"):
        assert phrase in body, phrase
    key = hdr[hdr.index("THE GROUP KEY of the optimistic threshold call"):hdr.index("int bn254_ctx_set_group_key(")]
    for phrase in ("leaves NO group key set", "forget the group key", "does NOT check that the registered keys interpolate"):
        assert phrase in key, phrase
    units = _native.translation_units()
    assert os.path.join(ROOT, "bn254_amd", "csrc", "bn254_threshold.hip") in units


def test_exported_by_the_library():
    _native.build()
    lib = _native.load()
    decls = _header_decls(NAMES + list(OTHERS))
    for name in NAMES + list(OTHERS):
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == _arity(decls[name].group(1)), name


def test_integration_extern_block_matches_header():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    decls = _header_decls(NAMES + ["bn254_ctx_set_group_key"])
    for name in NAMES + ["bn254_ctx_set_group_key"]:
        m = re.search(r"\bfn\s+%s\s*\(([^)]*)\)\s*->\s*c_int;" % name, doc)
        assert m, name
        assert _arity(re.sub(r"/\*.*?\*/", "", m.group(1))) == _arity(decls[name].group(1)), name
    assert "interpolate to the group key" in doc and "forgets the group key" in doc


def test_cpp_mirror_and_example_compile(tmp_path):
    _native.build()
    host = os.path.join(ROOT, "bn254_amd", "host")
    hpp = open(os.path.join(host, "bn254.hpp")).read()
    assert "bn254_batch_threshold_combine_keyed_optimistic(e.raw()" in hpp and "bn254_ctx_set_group_key(e.raw()" in hpp
    assert "register_group_key(" in hpp and "threshold_combine_keyed_optimistic(" in hpp
    example = open(os.path.join(host, "threshold_example.cpp")).read()
    assert "threshold_combine_keyed_optimistic" in example and "register_group_key" in example
    common = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", host]
    link = [_native.LIB_PATH, "-Wl,-rpath," + os.path.dirname(_native.LIB_PATH)]
    subprocess.check_call(common + [os.path.join(host, "threshold_example.cpp"), "-o", str(tmp_path / "threshold_example")] + link)


def test_api_rejects_malformed_items_and_a_missing_group_key_before_the_device(monkeypatch):
    from bn254_amd import api, engine

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(engine, "default_engine", no_device)
    sig = api.Signature(bytes(64))
    for items in ([(b"a", [sig], [0]), (b"b", [sig])], [(b"a", [sig], [0], [1])], [(b"a", [sig, sig], [0])], [(b"a", [], [3])]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.batch_threshold_combine_keyed_optimistic(items, 1)
        assert e.value.kind == api.ErrorKind.InvalidLength
    for idx in ([0, -1], [1 << 32, 0]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.threshold_combine_keyed_optimistic(b"a", [sig, sig], idx, 1)
        assert e.value.kind == api.ErrorKind.IndexOutOfBounds
    for t in (0, -3, 1 << 32):
        with pytest.raises(ValueError):
            api.ECDSA.threshold_combine_keyed_optimistic(b"a", [sig], [0], t)

    class Keyless:                                      # knows its key count, has no group key, and must not be called
        n_registered_keys = 3

        def batch_threshold_combine_keyed_optimistic(self, *a, **k):
            raise AssertionError("a device was touched")
    with pytest.raises(ValueError) as e:
        api.ECDSA.threshold_combine_keyed_optimistic(b"a", [sig], [0], 1, engine=Keyless())
    assert "group key" in str(e.value)

    class Keyed(Keyless):                               # ... and with one, the call reaches the engine with the exact call's arguments
        group_key_set = True

        def batch_threshold_combine_keyed_optimistic(self, messages, shares, share_keys, sizes, bm_words, threshold):
            assert (messages, shares, share_keys, sizes, bm_words, threshold) == ([b"a"], bytes(64), [2], [1], 1, 1)
            return b"\0", b"\0", bytes(64), [4], [1]
    r = api.ECDSA.threshold_combine_keyed_optimistic(b"a", [sig], [2], 1, engine=Keyed())
    assert r[0].raw == bytes(64) and r[1] == [2] and r[2] == [None]
    # the engine mirrors: sizes must add up, the threshold must be positive, a group key is 128 bytes
    with pytest.raises(AssertionError):
        engine.Engine.batch_threshold_combine_keyed_optimistic(None, [b"a", b"b"], bytes(128), [0, 1], [1, 2], 1, 1)
    with pytest.raises(AssertionError):
        engine.Engine.batch_threshold_combine_keyed_optimistic(None, [b"a"], bytes(64), [0], [1], 1, 0)
    with pytest.raises(AssertionError):
        engine.Engine.set_group_key(None, bytes(64))


def test_model_on_one_tuple_of_each_kind():
    """tests/threshold_opt_model.py itself, threshold 3 over 6 keys: a passing tuple (deviation 1: the bad share of key 5 is never looked
    at), a failing one (the exact call's answer), a duplicate, too few candidates, a refused tuple"""
    keys = [0, 1, 2, 5] + [0, 1, 2, 3] + [0, 0, 1, 2] + [4, 5] + [0, 1, 2]
    sizes = [4, 4, 4, 2, 3]
    tuple_st = [0, 0, 0, 0, 2]
    dec = [0] * 17
    dec[5] = 4                                          # tuple 1, key 1: off the curve — not a candidate
    pre = OM.precheck(dec, keys, [0] * 6, sizes, tuple_st)
    assert pre == [0] * 5 + [4] + [0] * 8 + [2] * 3
    exact = list(pre)
    exact[3] = 9                                        # tuple 0, key 5: invalid, outside S'
    exact[4] = 9                                        # tuple 1, key 0: invalid, inside S'
    asked = []

    def tuple_check(i, chosen):
        asked.append((i, chosen))
        return 0 if i == 0 else 9
    m = OM.combine(keys, pre, sizes, tuple_st, 1, 3, tuple_check, lambda s: exact[s])
    assert asked == [(0, [(0, 0), (1, 1), (2, 2)]), (1, [(0, 4), (2, 6), (3, 7)])]
    assert m["flags"] == [OM.CHECK, OM.CHECK, OM.EXACT, OM.EXACT, OM.FINAL] and m["verdicts"] == [0, 9, None, None, None]
    assert m["hook"] == dict(checked=2, passed=1, exact_tuples=3, exact_shares=3 + 4 + 2) and m["queue"] == [4, 6, 7, 8, 9, 10, 11, 12, 13]
    assert m["share_status"] == [0, 0, 0, 0] + [9, 4, 0, 0] + [0] * 6 + [2] * 3          # share 3 reads 0: deviation 1
    assert m["tuple_status"] == [0, 9, 0, 9, 2] and m["counts"] == [4, 2, 3, 2, 0]
    assert m["rows"] == [[0b111], [0b1100], [0b111], [0b110000], [0]]
    assert m["chosen"] == [[(0, 0), (1, 1), (2, 2)], [], [(0, 8), (1, 10), (2, 11)], [], []]
