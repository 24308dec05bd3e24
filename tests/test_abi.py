"""The C-ABI library loads and exports every symbol include/afm.h declares (no GPU needed)."""
import ctypes
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "afm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(afm_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_header_symbols():
    from afm import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = header_functions()
    assert len(names) >= 7
    for n in names:
        assert hasattr(L, n), n
    assert set(names) == set(_lib.SIGNATURES), set(names) ^ set(_lib.SIGNATURES)


def header_prototypes():
    """name -> (return, [parameter]) of every prototype of include/afm.h, in the vocabulary of
    _lib.SIGNATURES (an int return is "int": the header does not say status or value)."""
    src = open(os.path.join(ROOT, "include", "afm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    scalar = {"int": "int", "int64_t": "i64", "double": "f64"}
    element = {"double": "f64*", "int32_t": "i32*", "int64_t": "i64*", "uint64_t": "i64*",
               "char": "str", "afm_ctx": "ctx"}
    protos = {}
    for ret, name, params in re.findall(r"^(const char\*|int64_t|int)\s+(afm_\w+)\s*\(([^)]*)\)\s*;",
                                        src, flags=re.M):
        kinds = []
        for prm in (params.split(",") if params.strip() != "void" else []):
            base, stars, _ = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\**)\s*(\w+)\s*", prm).groups()
            # a single-star double / int32 / (u)int64 / char / afm_ctx is typed; the rest (void*,
            # afm_ctx**, void**, the host uint32_t mask) is an opaque pointer
            kinds.append(scalar[base] if not stars else
                         element.get(base, "ptr") if stars == "*" else "ptr")
        protos[name] = ({"const char*": "str", "int64_t": "i64", "int": "int"}[ret], kinds)
    return protos


def test_signature_table_matches_header_prototypes():
    from afm import _lib
    protos = header_prototypes()
    assert sorted(protos) == header_functions() and len(protos) == 59
    for name, (ret, kinds) in protos.items():
        tret, tparams = _lib.SIGNATURES[name]
        assert {"status": "int"}.get(tret, tret) == ret, name
        assert [t.removeprefix("host:") for t in tparams.split()] == kinds, name


class RecordingLib:
    """Stand-in for libafm: records every lookup and call; ``rc``: name -> return value."""

    def __init__(self, rc=None):
        self.rc, self.lookups, self.calls = rc or {}, [], []

    def __getattr__(self, name):
        self.lookups.append(name)

        def fn(*args):
            if name == "afm_last_error":
                return b"stand-in message"
            self.calls.append((name, args))
            return self.rc.get(name, 0)
        return fn


def _standin_context(monkeypatch, rc=None):
    from afm import _lib
    fake = RecordingLib(rc)
    monkeypatch.setattr(_lib, "lib", lambda: fake)
    ctx = _lib.Context(0)                     # afm_ctx_create "succeeds" on the stand-in
    ctx.handle = ctypes.c_void_p(0x1234)
    fake.calls.clear()
    return ctx, fake


def test_call_marshals_by_the_table(monkeypatch):
    ctx, fake = _standin_context(monkeypatch)
    assert ctx.call("afm_vec_add_f64", 3, None, None) == 0
    assert fake.calls == [("afm_vec_add_f64", (ctx.handle, 3, None, None))]
    assert fake.calls[0][1][0] is ctx.handle                 # the same c_void_p object
    ctx.call("afm_ols_solve_f64", None, None, 2, 1, 1, None, None, None)   # tol: an int
    tol = fake.calls[1][1][5]                               # (handle, gram, shift, p, nseg, tol, ..)
    assert type(tol) is float and tol == 1.0
    assert ctx.call("afm_zgram_part_bytes", 5) == 0          # no context parameter
    assert fake.calls[2] == ("afm_zgram_part_bytes", (5,))


def test_call_rejects_bad_arguments_before_the_library(monkeypatch):
    import torch
    from afm import _lib
    ctx, fake = _standin_context(monkeypatch)
    with pytest.raises(TypeError):
        ctx.call("afm_vec_add_f64", 3.0, None, None)         # a float for int64_t n
    with pytest.raises(TypeError):
        ctx.call("afm_vec_add_f64", 3, None)                 # one argument short
    with pytest.raises(TypeError):
        ctx.call("afm_vec_add_f64", 3, None, None, None)
    x = torch.zeros(64, dtype=torch.float64)
    with pytest.raises(_lib.AfmError, match="afm_vec_add_f64 argument 2"):
        ctx.call("afm_vec_add_f64", 64, x, None)             # a CPU tensor
    with pytest.raises(_lib.AfmError):
        ctx.call("afm_vec_add_f64", 64, ctypes.c_void_p(8), None)   # not a tensor
    assert fake.calls == []


def test_call_checks_the_return_value(monkeypatch):
    from afm import _lib
    ctx, fake = _standin_context(monkeypatch, {"afm_vec_add_f64": -1, "afm_factors_state_bytes": -1,
                                               "afm_factors_part_words": 4096})
    with pytest.raises(_lib.AfmError, match=r"afm_vec_add_f64 failed \(-1\): stand-in message"):
        ctx.call("afm_vec_add_f64", 3, None, None)
    with pytest.raises(_lib.AfmError, match="afm_factors_state_bytes"):
        ctx.call("afm_factors_state_bytes", 100)
    assert ctx.call("afm_factors_part_words", 100, 128, 0, 64) == 4096


def test_call_looks_the_function_up_per_call(monkeypatch):
    from afm import _lib
    ctx, fake = _standin_context(monkeypatch)
    ctx.call("afm_vec_add_f64", 3, None, None)
    ctx.call("afm_vec_add_f64", 3, None, None)
    assert fake.lookups.count("afm_vec_add_f64") == 2
    other = RecordingLib()
    monkeypatch.setattr(_lib, "lib", lambda: other)
    ctx.call("afm_vec_add_f64", 3, None, None)
    assert len(fake.calls) == 2 and len(other.calls) == 1


def test_factor_names_match_reference_order():
    import oracle
    from afm import FACTOR_NAMES, _lib
    assert _lib.factor_names() == FACTOR_NAMES == oracle.FACTOR_NAMES
    g = np.load(os.path.join(ROOT, "tests", "golden", "factors_edge.npz"))
    assert list(g["all_cols"]) == FACTOR_NAMES


def test_errors_do_not_throw_without_gpu():
    from afm import _lib
    L = _lib.lib()
    h = ctypes.c_void_p()
    rc = L.afm_ctx_create(123456, ctypes.byref(h))
    assert rc != 0 and len(L.afm_last_error()) > 0
    assert L.afm_ctx_destroy(None) != 0
    assert L.afm_version() >= 1


def test_bit_packing_roundtrip():
    import torch
    from afm import pack_bits, unpack_bits
    from afm.synthetic import unpack_bits as np_unpack, valid_bits
    rng = np.random.default_rng(0)
    v = rng.random((197, 128)) < 0.7
    b = pack_bits(torch.from_numpy(v))
    assert np.array_equal(unpack_bits(b, 197).numpy(), v)
    assert np.array_equal(b.numpy().view(np.uint64), valid_bits(v))
    assert np.array_equal(np_unpack(valid_bits(v), 197), v)
