"""The library exports the two symbols include/afm_xcorr.h declares, with the signatures of
afm/_lib.py's SIGNATURES_XCORR table (no GPU needed) -- what tests/test_abi_screen_layers.py checks
for include/afm_screen_layers.h, with its parser."""
import ctypes
import os
import re

import test_abi_screen_layers as A

ROOT = A.ROOT


def xcorr_header(monkeypatch):
    """The parser of test_abi_screen_layers.py on include/afm_xcorr.h."""
    src = open(os.path.join(ROOT, "include", "afm_xcorr.h")).read()
    monkeypatch.setattr(A, "header_source", lambda: re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return A.header_functions(), A.header_prototypes()


def test_library_exports_xcorr_header_symbols(monkeypatch):
    from afm import _lib
    names, _ = xcorr_header(monkeypatch)
    assert names == ["afm_screen_xcorr_f64", "afm_screen_xcorr_summary_f64"]
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(L, n), n
    assert set(names) == set(_lib.SIGNATURES_XCORR)


def test_xcorr_table_matches_header_prototypes(monkeypatch):
    from afm import _lib
    names, protos = xcorr_header(monkeypatch)
    assert sorted(protos) == names
    for name, (ret, kinds) in protos.items():
        tret, tparams = _lib.SIGNATURES_XCORR[name]
        assert {"status": "int"}.get(tret, tret) == ret, name
        assert [t.removeprefix("host:") for t in tparams.split()] == kinds, name


def test_xcorr_table_is_disjoint_and_layered_on_the_bound_tables():
    from afm import _lib
    assert _lib.CALL_TABLES == _lib.BOUND_TABLES + (_lib.SIGNATURES_XCORR,)
    assert _lib.BOUND_TABLES == _lib.LOADED_TABLES + (_lib.SIGNATURES_LAYERS,)
    assert len(_lib.BOUND_TABLES) == 6
    for table in _lib.BOUND_TABLES:
        assert not set(_lib.SIGNATURES_XCORR) & set(table)


def test_xcorr_arguments_follow_the_ic_entry_point():
    """afm_screen_xcorr_f64 takes afm_screen_ic_f64's arguments up to nrows, then its output."""
    from afm import _lib
    ic = _lib.SIGNATURES_SCREEN["afm_screen_ic_f64"][1].split()
    xc = _lib.SIGNATURES_XCORR["afm_screen_xcorr_f64"][1].split()
    assert xc[:len(ic) - 1] == ic[:-1]
    assert xc[len(ic) - 1:] == ["f64*"]
    assert _lib.SIGNATURES_XCORR["afm_screen_xcorr_summary_f64"][1].split() == \
        ["ctx", "f64*", "i64", "int", "f64*"]


def test_lib_and_call_plans_cover_the_new_table_and_the_old_ones(monkeypatch):
    from afm import _lib
    L = _lib.lib()
    f = L.afm_screen_xcorr_f64
    assert f.restype is ctypes.c_int and len(f.argtypes) == 15
    assert f.argtypes[2] is ctypes.c_int64 and f.argtypes[6] is ctypes.c_int
    assert f.argtypes[1] is ctypes.c_void_p and f.argtypes[14] is ctypes.c_void_p
    g = L.afm_screen_xcorr_summary_f64
    assert g.restype is ctypes.c_int and len(g.argtypes) == 5
    assert g.argtypes[2] is ctypes.c_int64 and g.argtypes[3] is ctypes.c_int
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
    ctx.call("afm_screen_xcorr_summary_f64", None, 7, 3, None)
    (name, args), = calls
    assert name == "afm_screen_xcorr_summary_f64" and args[0] is ctx.handle and args[2:4] == (7, 3)
    ctx.call("afm_screen_xcorr_f64", None, 640, 10, 64, None, 2, None, None, None, 5, None, None,
             None, None)
    assert calls[-1][0] == "afm_screen_xcorr_f64" and calls[-1][1][2:5] == (640, 10, 64)
    ctx.call("afm_screen_layer_series_f64", 7, 3, None, None, None, None, None)
    ctx.call("afm_screen_summary_f64", None, 10, 4, None, 2, 2001, None, None, None)
    ctx.call("afm_rank_returns_f64", 7, 64, None, 5, None, None, None, None, None)
    ctx.call("afm_gram_tree3_f64", 4, None, 1, 1, 1, 1, 1, None)
    ctx.call("afm_mean_variance_weights_f64", None, 10, 4, 4, None, 1, 0, 0.1, None, None, None)
    ctx.call("afm_vec_add_f64", 3, None, None)              # the six old tables still resolve
    assert [c[0] for c in calls[2:]] == ["afm_screen_layer_series_f64", "afm_screen_summary_f64",
                                         "afm_rank_returns_f64", "afm_gram_tree3_f64",
                                         "afm_mean_variance_weights_f64", "afm_vec_add_f64"]
