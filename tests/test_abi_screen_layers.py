"""The library exports every symbol include/afm_screen_layers.h declares, with the signatures of
afm/_lib.py's SIGNATURES_LAYERS table (no GPU needed) -- what tests/test_abi_rankic.py checks for
include/afm_rankic.h."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_source():
    src = open(os.path.join(ROOT, "include", "afm_screen_layers.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def header_functions():
    return sorted(set(re.findall(r"\b(afm_[a-z0-9_]+)\s*\(", header_source())))


def header_prototypes():
    """name -> (return, [parameter]) in the vocabulary of _lib.SIGNATURES_LAYERS."""
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


def test_library_exports_layers_header_symbols():
    from afm import _lib
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = header_functions()
    assert names == ["afm_screen_layer_series_f64", "afm_screen_layers_f64"]
    for n in names:
        assert hasattr(L, n), n
    assert set(names) == set(_lib.SIGNATURES_LAYERS)


def test_layers_table_is_disjoint_and_bound_beside_the_loaded_tables():
    from afm import _lib
    assert _lib.BOUND_TABLES == _lib.LOADED_TABLES + (_lib.SIGNATURES_LAYERS,)
    assert len(_lib.LOADED_TABLES) == 5
    for table in _lib.LOADED_TABLES:
        assert not set(_lib.SIGNATURES_LAYERS) & set(table)


def test_layers_table_matches_header_prototypes():
    from afm import _lib
    protos = header_prototypes()
    assert sorted(protos) == header_functions()
    for name, (ret, kinds) in protos.items():
        tret, tparams = _lib.SIGNATURES_LAYERS[name]
        assert {"status": "int"}.get(tret, tret) == ret, name
        assert [t.removeprefix("host:") for t in tparams.split()] == kinds, name


def test_layers_arguments_follow_the_ic_entry_point():
    """afm_screen_layers_f64 takes afm_screen_ic_f64's arguments up to nrows, then its outputs."""
    from afm import _lib
    ic = _lib.SIGNATURES_SCREEN["afm_screen_ic_f64"][1].split()
    ly = _lib.SIGNATURES_LAYERS["afm_screen_layers_f64"][1].split()
    assert ly[:len(ic) - 1] == ic[:-1]
    assert ly[len(ic) - 1:] == ["f64*", "i32*", "f64*", "f64*"]


def test_lib_and_call_plans_cover_the_new_table_and_the_old_ones(monkeypatch):
    from afm import _lib
    L = _lib.lib()
    f = L.afm_screen_layers_f64
    assert f.restype is ctypes.c_int and len(f.argtypes) == 18
    assert f.argtypes[2] is ctypes.c_int64 and f.argtypes[6] is ctypes.c_int
    assert f.argtypes[1] is ctypes.c_void_p and f.argtypes[17] is ctypes.c_void_p
    g = L.afm_screen_layer_series_f64
    assert g.restype is ctypes.c_int and len(g.argtypes) == 8
    assert g.argtypes[1] is ctypes.c_int64 and g.argtypes[2] is ctypes.c_int
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
    ctx.call("afm_screen_layer_series_f64", 7, 3, None, None, None, None, None)
    (name, args), = calls
    assert name == "afm_screen_layer_series_f64" and args[0] is ctx.handle and args[1:3] == (7, 3)
    ctx.call("afm_screen_layers_f64", None, 640, 10, 64, None, 2, None, None, None, 5, None, None,
             None, None, None, None, None)
    assert calls[-1][0] == "afm_screen_layers_f64" and calls[-1][1][2:5] == (640, 10, 64)
    ctx.call("afm_screen_summary_f64", None, 10, 4, None, 2, 2001, None, None, None)
    ctx.call("afm_rank_returns_f64", 7, 64, None, 5, None, None, None, None, None)
    ctx.call("afm_gram_tree3_f64", 4, None, 1, 1, 1, 1, 1, None)
    ctx.call("afm_mean_variance_weights_f64", None, 10, 4, 4, None, 1, 0, 0.1, None, None, None)
    ctx.call("afm_vec_add_f64", 3, None, None)              # the five old tables still resolve
    assert [c[0] for c in calls[2:]] == ["afm_screen_summary_f64", "afm_rank_returns_f64",
                                         "afm_gram_tree3_f64", "afm_mean_variance_weights_f64",
                                         "afm_vec_add_f64"]
