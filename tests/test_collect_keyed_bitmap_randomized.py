"""bn254_batch_collect_keyed_bitmap_randomized[_device] (include/bn254_hip.h), without a GPU:
- the two entry points are declared with the exact call's arity + 1 (seed32 in front of the first output array), exported with matching
  argtypes and bound in INTEGRATION.md's extern block; so is the debug hook;
- options 38 and 39 have numbers of their own and are mirrored in engine.py;
- the Python mirrors refuse malformed items and a seed that is not 32 bytes before they touch a device."""
import os
import re

import pytest

from bn254_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = ["bn254_batch_collect_keyed_bitmap", "bn254_batch_collect_keyed_bitmap_device"]
NAMES = ["bn254_batch_collect_keyed_bitmap_randomized", "bn254_batch_collect_keyed_bitmap_randomized_device"]
HOOK = "bn254_debug_collect_rand_last"


def _args(decl):
    return [a.strip() for a in decl.split(",") if a.strip()]


def _header():
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)


def _decl(name, text=None):
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, text or _header())
    assert m, name
    return _args(m.group(1))


def test_declared_with_the_exact_arity_plus_the_seed():
    for exact, rand in zip(EXACT, NAMES):
        a, b = _decl(exact), _decl(rand)
        assert len(b) == len(a) + 1, rand
        at = next(i for i, x in enumerate(a) if "share_status" in x)        # the first output array
        assert b[at] == "const uint8_t *seed32", b[at]
        assert b[:at] == a[:at] and b[at + 1:] == a[at:], rand
        assert rand in _native.EXPORTED_SYMBOLS
    assert HOOK in _native.EXPORTED_SYMBOLS
    assert _decl(HOOK) == ["bn254_ctx *ctx", "uint64_t out[4]"]
    # the hook is a developer hook: hidden with the others
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    assert hdr.index("#ifndef BN254_NO_DEV_HOOKS") < hdr.index("int %s(" % HOOK) < hdr.index("#endif /* BN254_NO_DEV_HOOKS */")
    assert all(hdr.index("int %s(" % n) < hdr.index("#ifndef BN254_NO_DEV_HOOKS") for n in NAMES)


def test_options_have_numbers_of_their_own():
    from bn254_amd import engine
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    assert re.search(r"#define BN254_OPT_COLLECT_RAND_MIN_SHARES 38\b", hdr) and engine.OPT_COLLECT_RAND_MIN_SHARES == 38
    assert re.search(r"#define BN254_OPT_COLLECT_RAND_MIN_PER_KEY 39\b", hdr) and engine.OPT_COLLECT_RAND_MIN_PER_KEY == 39
    numbers = [int(x) for x in re.findall(r"#define BN254_OPT_\w+ (\d+)\b", hdr)]
    assert numbers.count(38) == 1 and numbers.count(39) == 1 and len(numbers) == len(set(numbers))
    mirrored = [v for k, v in vars(engine).items() if k.startswith("OPT_")]
    assert mirrored.count(38) == 1 and mirrored.count(39) == 1
    # ... and so are their defaults
    ws = open(os.path.join(ROOT, "bn254_amd", "csrc", "bn254_ws.h")).read()
    assert int(re.search(r"#define COLLECT_RAND_MIN_SHARES_DEFAULT (\d+)", ws).group(1)) == engine.COLLECT_RAND_MIN_SHARES_DEFAULT
    assert int(re.search(r"#define COLLECT_RAND_MIN_PER_KEY_DEFAULT (\d+)", ws).group(1)) == engine.COLLECT_RAND_MIN_PER_KEY_DEFAULT


def test_exported_by_the_library():
    _native.build()
    lib = _native.load()
    for name in NAMES + [HOOK]:
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == len(_decl(name)), name


def test_integration_extern_block_matches_header():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NAMES:
        m = re.search(r"\bfn\s+%s\s*\(([^)]*)\)\s*->\s*c_int;" % name, doc)
        assert m, name
        args = _args(m.group(1))
        assert len(args) == len(_decl(name)), name
        assert [a.split(":")[0] for a in args].index("seed32") == next(i for i, x in enumerate(_decl(name)) if "seed32" in x)


def test_cpp_mirror_declares_the_randomised_forms():
    hpp = open(os.path.join(ROOT, "bn254_amd", "host", "bn254.hpp")).read()
    assert "batch_aggregate_keyed_signers_randomized(" in hpp and "aggregate_keyed_signers_randomized(" in hpp
    assert "bn254_batch_collect_keyed_bitmap_randomized(" in hpp


def test_api_rejects_malformed_items_and_seeds_before_the_device(monkeypatch):
    from bn254_amd import api, engine

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(engine, "default_engine", no_device)
    sig = api.Signature(bytes(64))
    for items in ([(b"a", [sig], [0]), (b"b", [sig])], [(b"a", [sig], [0], [1])], [(b"a", [sig, sig], [0])], [(b"a", [], [3])]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.batch_aggregate_keyed_signers_randomized(items, seed=bytes(32))
        assert e.value.kind == api.ErrorKind.InvalidLength
    for idx in ([0, -1], [1 << 32, 0]):
        with pytest.raises(api.Error) as e:
            api.ECDSA.aggregate_keyed_signers_randomized(b"a", [sig, sig], idx)
        assert e.value.kind == api.ErrorKind.IndexOutOfBounds
    for seed in (b"", bytes(31), bytes(33)):
        with pytest.raises(ValueError):
            api.ECDSA.batch_aggregate_keyed_signers_randomized([(b"a", [sig], [0])], seed=seed)
        with pytest.raises(ValueError):
            api.ECDSA.aggregate_keyed_signers_randomized(b"a", [sig], [0], seed=seed)

    class Blind:
        pass
    with pytest.raises(ValueError):
        api.ECDSA.aggregate_keyed_signers_randomized(b"a", [sig], [0], engine=Blind())
    # the engine mirror: a 32-byte seed, sizes that add up to the shares
    with pytest.raises(AssertionError):
        engine.Engine.batch_collect_keyed_bitmap_randomized(None, [b"a"], bytes(64), [0], [1], 1, bytes(31))
    with pytest.raises(AssertionError):
        engine.Engine.batch_collect_keyed_bitmap_randomized(None, [b"a", b"b"], bytes(128), [0, 1], [1, 2], 1, bytes(32))
    with pytest.raises(AssertionError):
        engine.Engine.batch_collect_keyed_bitmap_randomized_device(None, 0, 0, 0, 0, 0, 1, 1, 1, bytes(5), 0, 0, 0, 0)
