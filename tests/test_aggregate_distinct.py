"""Aggregate verification over distinct messages, the parts that need no GPU: the two entry points are declared, exported and bound in
INTEGRATION.md's extern block with the header's arity; the Python mirror refuses mismatched lengths before it touches a device."""
import os
import re

import pytest

from bn254_amd import _native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["bn254_batch_aggregate_verify_distinct", "bn254_batch_aggregate_verify_distinct_device"]


def _arity(decl):
    return len([a for a in decl.split(",") if a.strip()])


def _header_decls():
    hdr = open(os.path.join(ROOT, "include", "bn254_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return {name: re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, hdr) for name in NAMES}


def test_declared_and_registered():
    decls = _header_decls()
    for name in NAMES:
        assert decls[name], name
        assert name in _native.EXPORTED_SYMBOLS
    assert _arity(decls[NAMES[0]].group(1)) == 10 and _arity(decls[NAMES[1]].group(1)) == 11


def test_exported_by_the_library():
    _native.build()
    lib = _native.load()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == _arity(_header_decls()[name].group(1))


def test_integration_extern_block_matches_header():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    decls = _header_decls()
    for name in NAMES:
        m = re.search(r"\bfn\s+%s\s*\(([^)]*)\)\s*->\s*c_int;" % name, doc)
        assert m, name
        assert _arity(m.group(1)) == _arity(decls[name].group(1)), name


def test_api_rejects_mismatched_lengths_before_the_device(monkeypatch):
    from bn254_amd import api, engine

    def no_device(*a, **k):
        raise AssertionError("a device was touched")
    monkeypatch.setattr(engine, "default_engine", no_device)
    sig = api.Signature(bytes(64))
    pk = api.PublicKey(bytes(128))
    with pytest.raises(api.Error) as e:
        api.ECDSA.aggregate_verify([b"a", b"b"], sig, [pk])
    assert e.value.kind == api.ErrorKind.InvalidLength
    with pytest.raises(api.Error) as e:
        api.ECDSA.batch_aggregate_verify_distinct([([b"a"], sig, [pk]), ([b"a", b"b"], sig, [pk])])
    assert e.value.kind == api.ErrorKind.InvalidLength
