"""The library exports the symbol include/afm_xsprep.h declares, with the signature of
afm/_lib.py's SIGNATURES_XSPREP table (no GPU needed) -- what tests/test_abi_xcorr.py checks for
include/afm_xcorr.h, with the parser of tests/test_abi_screen_layers.py."""
import ctypes
import os
import re

import pytest

import test_abi_screen_layers as A

ROOT = A.ROOT
NAME = "afm_xs_preprocess_f64"


def xsprep_header(monkeypatch):
    src = open(os.path.join(ROOT, "include", "afm_xsprep.h")).read()
    monkeypatch.setattr(A, "header_source", lambda: re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return A.header_functions(), A.header_prototypes()


def test_library_exports_xsprep_header_symbol(monkeypatch):
    from afm import _lib
    names, _ = xsprep_header(monkeypatch)
    assert names == [NAME]
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME)
    assert set(names) == set(_lib.SIGNATURES_XSPREP)


def test_xsprep_table_matches_header_prototype(monkeypatch):
    from afm import _lib
    names, protos = xsprep_header(monkeypatch)
    assert sorted(protos) == names
    ret, kinds = protos[NAME]
    tret, tparams = _lib.SIGNATURES_XSPREP[NAME]
    assert {"status": "int"}.get(tret, tret) == ret
    assert tparams.split() == kinds and len(kinds) == 23


def test_xsprep_table_is_disjoint_and_layered_on_the_call_tables():
    from afm import _lib
    assert _lib.PREP_TABLES == _lib.CALL_TABLES + (_lib.SIGNATURES_XSPREP,)
    assert _lib.CALL_TABLES == _lib.BOUND_TABLES + (_lib.SIGNATURES_XCORR,)
    assert len(_lib.CALL_TABLES) == 7
    for table in _lib.CALL_TABLES:
        assert not set(_lib.SIGNATURES_XSPREP) & set(table)


def test_xsprep_arguments_follow_the_ic_entry_point():
    """afm_xs_preprocess_f64 takes afm_screen_ic_f64's arguments up to nd, then the row sets
    without the unused `rows`, the groups, the parameters and its outputs."""
    from afm import _lib
    ic = _lib.SIGNATURES_SCREEN["afm_screen_ic_f64"][1].split()
    xp = _lib.SIGNATURES_XSPREP[NAME][1].split()
    assert xp[:11] == ic[:11]                               # ctx .. nd
    assert ic[11:14] == ["f64*", "i32*", "i32*"] and xp[11:13] == ic[12:14]
    assert xp[13:] == ["i32*", "i64", "int", "int", "f64", "f64", "int", "f64*", "i64", "f64*"]


def test_lib_and_call_plans_cover_the_new_table_and_the_old_ones(monkeypatch):
    from afm import _lib
    f = getattr(_lib.lib(), NAME)
    assert f.restype is ctypes.c_int and len(f.argtypes) == 23
    assert f.argtypes[2] is ctypes.c_int64 and f.argtypes[6] is ctypes.c_int
    assert f.argtypes[17] is ctypes.c_double and f.argtypes[18] is ctypes.c_double
    assert f.argtypes[1] is ctypes.c_void_p and f.argtypes[22] is ctypes.c_void_p
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
    ctx.call(NAME, None, 640, 10, 64, None, 2, None, None, None, 5, None, None, None, 0, 7, 1,
             4.4478, 4.4478, 3, None, 640, None)
    (name, args), = calls
    assert name == NAME and args[0] is ctx.handle and args[2:5] == (640, 10, 64)
    assert args[14:20] == (0, 7, 1, 4.4478, 4.4478, 3)
    with pytest.raises(TypeError):
        ctx.call(NAME, None, 640)
    ctx.call("afm_screen_xcorr_summary_f64", None, 7, 3, None)
    ctx.call("afm_screen_layer_series_f64", 7, 3, None, None, None, None, None)
    ctx.call("afm_screen_summary_f64", None, 10, 4, None, 2, 2001, None, None, None)
    ctx.call("afm_rank_returns_f64", 7, 64, None, 5, None, None, None, None, None)
    ctx.call("afm_gram_tree3_f64", 4, None, 1, 1, 1, 1, 1, None)
    ctx.call("afm_mean_variance_weights_f64", None, 10, 4, 4, None, 1, 0, 0.1, None, None, None)
    ctx.call("afm_vec_add_f64", 3, None, None)              # the seven old tables still resolve
    assert [c[0] for c in calls[1:]] == [
        "afm_screen_xcorr_summary_f64", "afm_screen_layer_series_f64", "afm_screen_summary_f64",
        "afm_rank_returns_f64", "afm_gram_tree3_f64", "afm_mean_variance_weights_f64",
        "afm_vec_add_f64"]


def test_python_surface():
    import dataclasses

    import afm
    from afm.xsprep import XsPrep
    assert afm.XsPrep is XsPrep and callable(afm.preprocess_factors) and callable(afm.preprocess_grid)
    p = XsPrep()
    assert (p.winsor, p.n_mad, p.quantiles, p.neutralize, p.standardize) == \
        (None, 3.0, (0.01, 0.99), False, True)
    assert (p.mode, p.flags, p.params) == (0, 2, (0.0, 0.0))
    q = XsPrep("mad", neutralize=True)
    assert (q.mode, q.flags) == (1, 3) and q.params == (3.0 * 1.4826, 3.0 * 1.4826)
    assert XsPrep("quantile", quantiles=(0, 1), standardize=False).params == (0.0, 1.0)
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.winsor = "mad"
    for bad in (dict(winsor="sigma"), dict(n_mad=0), dict(n_mad=float("inf")),
                dict(quantiles=(0.5, 0.5)), dict(quantiles=(-0.1, 0.9)), dict(quantiles=(0.1, 1.1)),
                dict(quantiles=0.5)):
        with pytest.raises(ValueError):
            XsPrep(**bad)
    fields = [f.name for f in dataclasses.fields(afm.PanelGrid)]
    assert fields[-1] == "group" and afm.PanelGrid.__dataclass_fields__["group"].default is None
