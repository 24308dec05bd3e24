"""The library exports every symbol include/afm_rankic.h declares, with the signatures of the fourth
table of afm/_lib.py (no GPU needed) -- what tests/test_abi_screen.py checks for
include/afm_screen.h."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_source():
    src = open(os.path.join(ROOT, "include", "afm_rankic.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def header_functions():
    return sorted(set(re.findall(r"\b(afm_[a-z0-9_]+)\s*\(", header_source())))


def header_prototypes():
    """name -> (return, [parameter]) in the vocabulary of _lib.SIGNATURES_RANK."""
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


def test_library_exports_rank_header_symbols():
    from afm import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = header_functions()
    assert names == ["afm_rank_returns_f64", "afm_rank_scratch_words", "afm_screen_rank_ic_f64"]
    for n in names:
        assert hasattr(L, n), n
    assert set(names) == set(_lib.SIGNATURES_RANK)


def test_rank_table_is_disjoint_from_the_other_three():
    from afm import _lib
    assert _lib.ALL_TABLES == _lib.TABLES + (_lib.SIGNATURES_RANK,) and len(_lib.TABLES) == 3
    for table in _lib.TABLES:
        assert not set(_lib.SIGNATURES_RANK) & set(table)


def test_rank_table_matches_header_prototypes():
    from afm import _lib
    protos = header_prototypes()
    assert sorted(protos) == header_functions()
    for name, (ret, kinds) in protos.items():
        tret, tparams = _lib.SIGNATURES_RANK[name]
        assert {"status": "int"}.get(tret, tret) == ret, name
        assert [t.removeprefix("host:") for t in tparams.split()] == kinds, name


def test_scratch_words_needs_no_gpu():
    """The scratch-size query is plain host code: nothing at or below the LDS capacity, a slot per
    workgroup in flight past it, an error for a shape the kernels do not take."""
    import rank_ref
    from afm import _lib
    L = _lib.lib()
    cap = rank_ref.kernel_constant("kRankLdsRows")
    assert L.afm_rank_scratch_words(64) == 0 and L.afm_rank_scratch_words(cap) == 0
    assert L.afm_rank_scratch_words(cap + 64) == rank_ref.kernel_constant("kRankSlots") * (cap + 64)
    for bad in (0, 100, rank_ref.MAX_ROWS + 64):
        assert L.afm_rank_scratch_words(bad) < 0
    assert b"lda" in L.afm_last_error()


def test_lib_and_call_plans_cover_all_four_tables(monkeypatch):
    from afm import _lib
    L = _lib.lib()
    f = L.afm_screen_rank_ic_f64
    assert f.restype is ctypes.c_int and len(f.argtypes) == 18
    assert f.argtypes[2] is ctypes.c_int64 and f.argtypes[6] is ctypes.c_int
    assert f.argtypes[1] is ctypes.c_void_p and f.argtypes[17] is ctypes.c_void_p
    assert L.afm_rank_scratch_words.restype is ctypes.c_int64
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
    ctx.call("afm_rank_returns_f64", 7, 64, None, 5, None, None, None, None, None)
    (name, args), = calls
    assert name == "afm_rank_returns_f64" and args[0] is ctx.handle and args[1:3] == (7, 64)
    assert ctx.call("afm_rank_scratch_words", 128) == 0 and calls[-1] == ("afm_rank_scratch_words",
                                                                           (128,))
    ctx.call("afm_screen_summary_f64", None, 10, 4, None, 2, 2001, None, None, None)
    ctx.call("afm_mean_variance_weights_f64", None, 10, 4, 4, None, 1, 0, 0.1, None, None, None)
    ctx.call("afm_vec_add_f64", 3, None, None)              # the three old tables still resolve
    assert [c[0] for c in calls[2:]] == ["afm_screen_summary_f64", "afm_mean_variance_weights_f64",
                                         "afm_vec_add_f64"]
