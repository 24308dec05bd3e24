"""The library exports the symbols include/afm_combine.h declares, with the signatures of
afm/_lib.py's SIGNATURES_COMBINE table (no GPU needed) -- what tests/test_abi_xsprep.py checks for
include/afm_xsprep.h, with the parser of tests/test_abi_screen_layers.py."""
import ctypes
import os
import re

import pytest

import test_abi_screen_layers as A

ROOT = A.ROOT
NAMES = ["afm_combine_f64", "afm_ic_weights_f64"]


def combine_header(monkeypatch):
    src = open(os.path.join(ROOT, "include", "afm_combine.h")).read()
    monkeypatch.setattr(A, "header_source", lambda: re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return A.header_functions(), A.header_prototypes()


def test_library_exports_combine_header_symbols(monkeypatch):
    from afm import _lib
    names, _ = combine_header(monkeypatch)
    assert sorted(names) == NAMES
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(L, n)
    assert set(names) == set(_lib.SIGNATURES_COMBINE)


def test_combine_table_matches_header_prototypes(monkeypatch):
    from afm import _lib
    names, protos = combine_header(monkeypatch)
    assert sorted(protos) == sorted(names)
    for n, nargs in zip(NAMES, (17, 12)):
        ret, kinds = protos[n]
        tret, tparams = _lib.SIGNATURES_COMBINE[n]
        assert {"status": "int"}.get(tret, tret) == ret
        assert tparams.split() == kinds and len(kinds) == nargs


def test_header_limits():
    src = open(os.path.join(ROOT, "include", "afm_combine.h")).read()
    defs = dict(re.findall(r"#define (AFM_COMBINE_\w+) (\d+)", src))
    assert defs == {"AFM_COMBINE_EQUAL": "0", "AFM_COMBINE_IC": "1", "AFM_COMBINE_ICIR": "2",
                    "AFM_COMBINE_MAXIR": "3", "AFM_COMBINE_MAX_K": "128",
                    "AFM_COMBINE_MAX_WINDOW": "1024"}
    from afm import combine
    assert combine.METHODS == {"equal": 0, "ic": 1, "icir": 2, "maxir": 3}
    assert (combine.MAX_K, combine.MAX_WINDOW) == (128, 1024)


def test_combine_table_is_disjoint_and_layered_on_the_prep_tables():
    from afm import _lib
    assert _lib.COMBINE_TABLES == _lib.PREP_TABLES + (_lib.SIGNATURES_COMBINE,)
    assert _lib.PREP_TABLES == _lib.CALL_TABLES + (_lib.SIGNATURES_XSPREP,)
    assert len(_lib.PREP_TABLES) == 8
    for table in _lib.PREP_TABLES:
        assert not set(_lib.SIGNATURES_COMBINE) & set(table)


def test_combine_arguments_follow_the_preprocess_entry_point():
    """afm_combine_f64 takes afm_xs_preprocess_f64's arguments up to nrows, then the weights, their
    stride and its two outputs."""
    from afm import _lib
    xp = _lib.SIGNATURES_XSPREP["afm_xs_preprocess_f64"][1].split()
    cb = _lib.SIGNATURES_COMBINE["afm_combine_f64"][1].split()
    assert cb[:13] == xp[:13]                               # ctx .. nrows
    assert cb[13:] == ["f64*", "i64", "f64*", "i32*"]
    assert _lib.SIGNATURES_COMBINE["afm_ic_weights_f64"][1].split() == \
        ["ctx", "f64*", "i64"] + ["int"] * 6 + ["f64", "f64*", "f64*"]


def test_lib_and_call_plans_cover_the_new_table_and_the_old_ones(monkeypatch):
    from afm import _lib
    f = getattr(_lib.lib(), "afm_combine_f64")
    assert f.restype is ctypes.c_int and len(f.argtypes) == 17
    assert f.argtypes[2] is ctypes.c_int64 and f.argtypes[6] is ctypes.c_int
    assert f.argtypes[14] is ctypes.c_int64 and f.argtypes[16] is ctypes.c_void_p
    f = getattr(_lib.lib(), "afm_ic_weights_f64")
    assert f.restype is ctypes.c_int and len(f.argtypes) == 12
    assert f.argtypes[2] is ctypes.c_int64 and f.argtypes[3:9] == [ctypes.c_int] * 6
    assert f.argtypes[9] is ctypes.c_double and f.argtypes[11] is ctypes.c_void_p
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
    ctx.call("afm_ic_weights_f64", None, 40, 17, 2, 3, 20, 5, 10, 0.25, None, None)
    ctx.call("afm_combine_f64", None, 640, 10, 64, None, 2, None, None, None, 5, None, None, None,
             2, None, None)
    (n0, a0), (n1, a1) = calls
    assert n0 == "afm_ic_weights_f64" and a0[0] is ctx.handle and a0[2:10] == (40, 17, 2, 3, 20, 5,
                                                                               10, 0.25)
    assert n1 == "afm_combine_f64" and a1[2:5] == (640, 10, 64) and a1[14] == 2
    with pytest.raises(TypeError):
        ctx.call("afm_combine_f64", None, 640)
    ctx.call("afm_xs_preprocess_f64", None, 640, 10, 64, None, 2, None, None, None, 5, None, None,
             None, 0, 7, 1, 4.4478, 4.4478, 3, None, 640, None)
    ctx.call("afm_screen_xcorr_summary_f64", None, 7, 3, None)
    ctx.call("afm_screen_summary_f64", None, 10, 4, None, 2, 2001, None, None, None)
    ctx.call("afm_vec_add_f64", 3, None, None)              # the old tables still resolve
    assert [c[0] for c in calls[2:]] == ["afm_xs_preprocess_f64", "afm_screen_xcorr_summary_f64",
                                         "afm_screen_summary_f64", "afm_vec_add_f64"]


def test_python_surface():
    import dataclasses

    import afm
    from afm.combine import ICWeights
    assert afm.ICWeights is ICWeights
    assert callable(afm.ic_weights) and callable(afm.combine_grid) and callable(afm.combine_factors)
    p = ICWeights()
    assert (p.method, p.window, p.embargo, p.min_periods, p.shrink, p.return_type) == \
        ("icir", 60, 1, 30, 0.5, "return_1")
    assert (p.code, p.q) == (2, 0)
    r = ICWeights("maxir", window=5, return_type="return_5")
    assert (r.code, r.q, r.embargo, r.min_periods) == (3, 2, 5, 2)
    assert ICWeights("ic", return_type="return_2").embargo == 2
    assert ICWeights("ic", window=1).min_periods == 1
    assert ICWeights("equal", embargo=0, min_periods=1).embargo == 0
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.window = 5
    for bad in (dict(method="sharpe"), dict(window=0), dict(window=1025), dict(embargo=-1),
                dict(min_periods=0), dict(window=10, min_periods=11),
                dict(method="icir", min_periods=1), dict(method="maxir", min_periods=1),
                dict(method="icir", window=1), dict(shrink=0.0), dict(shrink=1.5),
                dict(shrink=float("nan")), dict(return_type="return_3")):
        with pytest.raises(ValueError):
            ICWeights(**bad)
    with pytest.raises(TypeError):
        afm.combine._check_spec("icir")
