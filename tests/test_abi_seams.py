"""The library exports every symbol include/afm_seams.h declares, with the signatures of the fifth
table of afm/_lib.py (no GPU needed) -- what tests/test_abi_rankic.py checks for
include/afm_rankic.h."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_source():
    src = open(os.path.join(ROOT, "include", "afm_seams.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def header_functions():
    return sorted(set(re.findall(r"\b(afm_[a-z0-9_]+)\s*\(", header_source())))


def header_prototypes():
    """name -> (return, [parameter]) in the vocabulary of _lib.SIGNATURES_SEAMS."""
    scalar = {"int": "int", "int64_t": "i64", "double": "f64"}
    element = {"double": "f64*", "int32_t": "i32*", "int64_t": "i64*", "uint64_t": "i64*",
               "char": "str", "afm_ctx": "ctx"}
    protos = {}
    for ret, name, params in re.findall(r"^(const char\*|int64_t|int)\s+(afm_\w+)\s*\(([^)]*)\)\s*;",
                                        header_source(), flags=re.M):
        kinds = []
        for prm in (params.split(",") if params.strip() != "void" else []):
            base, stars, _ = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s*(\**)\s*(\w+)\s*", prm).groups()
            kinds.append(scalar[base] if not stars else
                         element.get(base, "ptr") if stars == "*" else "ptr")
        protos[name] = ({"const char*": "str", "int64_t": "i64", "int": "int"}[ret], kinds)
    return protos


def test_library_exports_seams_header_symbols():
    from afm import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = header_functions()
    assert names == ["afm_factors_rows_f64", "afm_gram_final_f64", "afm_gram_tree3_f64",
                     "afm_ols_solve_parts_f64", "afm_zstats_rows_f64"]
    for n in names:
        assert hasattr(L, n), n
    assert set(names) == set(_lib.SIGNATURES_SEAMS)


def test_seams_table_is_disjoint_and_loaded():
    from afm import _lib
    assert _lib.LOADED_TABLES == _lib.ALL_TABLES + (_lib.SIGNATURES_SEAMS,)
    for table in _lib.ALL_TABLES:
        assert not set(_lib.SIGNATURES_SEAMS) & set(table)
    f = _lib.lib().afm_gram_tree3_f64
    assert f.restype is ctypes.c_int and len(f.argtypes) == 9
    assert f.argtypes[1] is ctypes.c_int and f.argtypes[2] is ctypes.c_void_p


def test_seams_table_matches_header_prototypes():
    from afm import _lib
    protos = header_prototypes()
    assert sorted(protos) == header_functions()
    for name, (ret, kinds) in protos.items():
        tret, tparams = _lib.SIGNATURES_SEAMS[name]
        assert {"status": "int"}.get(tret, tret) == ret, name
        assert [t.removeprefix("host:") for t in tparams.split()] == kinds, name


def test_call_plans_cover_the_seams_table(monkeypatch):
    from afm import _lib
    calls = []

    class Fake:
        def __getattr__(self, name):
            def fn(*args):
                calls.append((name, args))
                return 0
            return fn
    monkeypatch.setattr(_lib, "lib", lambda: Fake())
    ctx = _lib.Context(0)
    ctx.handle = ctypes.c_void_p(0x1234)
    calls.clear()
    ctx.call("afm_gram_final_f64", 30, None, 8, None, 0, None, None)
    ctx.call("afm_vec_add_f64", 3, None, None)              # the earlier tables still resolve
    assert [c[0] for c in calls] == ["afm_gram_final_f64", "afm_vec_add_f64"]
    assert calls[0][1][0] is ctx.handle and calls[0][1][1] == 30 and calls[0][1][3] == 8
