"""The library exports the symbols include/afm_turnover.h declares, with the signatures of
afm/_lib.py's SIGNATURES_TURNOVER table (no GPU needed) -- what tests/test_abi_combine.py checks
for include/afm_combine.h, with the parser of tests/test_abi_screen_layers.py."""
import ctypes
import os
import re

import pytest

import test_abi_screen_layers as A

ROOT = A.ROOT
NAMES = ["afm_screen_turnover_f64", "afm_screen_turnover_scratch_bytes",
         "afm_screen_turnover_summary_f64"]


def turnover_header(monkeypatch):
    src = open(os.path.join(ROOT, "include", "afm_turnover.h")).read()
    monkeypatch.setattr(A, "header_source", lambda: re.sub(r"/\*.*?\*/", "", src, flags=re.S))
    return A.header_functions(), A.header_prototypes()


def test_library_exports_turnover_header_symbols(monkeypatch):
    from afm import _lib
    names, _ = turnover_header(monkeypatch)
    assert sorted(names) == NAMES
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(L, n)
    assert set(names) == set(_lib.SIGNATURES_TURNOVER)


def test_turnover_table_matches_header_prototypes(monkeypatch):
    from afm import _lib
    names, protos = turnover_header(monkeypatch)
    assert sorted(protos) == sorted(names)
    for n, nargs in zip(NAMES, (19, 3, 8)):
        ret, kinds = protos[n]
        tret, tparams = _lib.SIGNATURES_TURNOVER[n]
        assert {"status": "int"}.get(tret, tret) == ret
        assert [t.removeprefix("host:") for t in tparams.split()] == kinds and len(kinds) == nargs
    # the lags are a host array; the scratch query returns int64_t and takes no context
    assert _lib.SIGNATURES_TURNOVER["afm_screen_turnover_f64"][1].split()[13] == "host:i32*"
    assert _lib.SIGNATURES_TURNOVER["afm_screen_turnover_scratch_bytes"] == ("i64", "i64 int i64")
    assert protos["afm_screen_turnover_scratch_bytes"][0] == "i64"


def test_header_limit_and_guard():
    src = open(os.path.join(ROOT, "include", "afm_turnover.h")).read()
    assert dict(re.findall(r"#define (AFM_TURNOVER_\w+) (\d+)", src)) == \
        {"AFM_TURNOVER_MAX_LAGS": "8"}
    assert "#ifndef AFM_TURNOVER_H" in src and "#define AFM_TURNOVER_H" in src
    from afm import turnover
    assert turnover.MAX_LAGS == 8


def test_turnover_table_is_disjoint_and_layered_on_the_combine_tables():
    from afm import _lib
    assert _lib.TURNOVER_TABLES == _lib.COMBINE_TABLES + (_lib.SIGNATURES_TURNOVER,)
    assert _lib.COMBINE_TABLES == _lib.PREP_TABLES + (_lib.SIGNATURES_COMBINE,)
    assert len(_lib.COMBINE_TABLES) == 9
    for table in _lib.COMBINE_TABLES:
        assert not set(_lib.SIGNATURES_TURNOVER) & set(table)


def test_turnover_arguments_follow_the_combine_entry_point():
    """afm_screen_turnover_f64 takes afm_combine_f64's arguments up to nrows, then the lags, their
    count, its three outputs and the scratch."""
    from afm import _lib
    cb = _lib.SIGNATURES_COMBINE["afm_combine_f64"][1].split()
    tv = _lib.SIGNATURES_TURNOVER["afm_screen_turnover_f64"][1].split()
    assert tv[:13] == cb[:13]                               # ctx .. nrows
    assert tv[13:] == ["host:i32*", "int", "f64*", "i32*", "f64*", "i64*"]


def test_scratch_query_needs_no_context_and_rejects_a_bad_lda():
    from afm import _lib
    f = _lib.lib().afm_screen_turnover_scratch_bytes
    assert f.restype is ctypes.c_int64 and f.argtypes == [ctypes.c_int64, ctypes.c_int,
                                                          ctypes.c_int64]
    small = f(12, 3, 64)
    assert small > 0 and small % 8 == 0
    assert f(12, 6, 64) == 2 * small                        # the marks of every date and column
    assert f(2, 1, 32768) > f(2, 1, 16384) > 0              # the sort's scratch past 16384 rows
    # bounded: never the 4.9 GB of all dates at once
    assert 0 < f(4112, 97, 2816) <= (160 << 20)
    for nd, K, lda in ((12, 3, 96), (12, 3, 0), (12, 3, 32832), (-1, 3, 64), (12, 0, 64)):
        assert f(nd, K, lda) < 0
        assert b"afm_screen_turnover_scratch_bytes" in _lib.lib().afm_last_error()


def test_lib_and_call_plans_cover_the_new_table_and_the_old_ones(monkeypatch):
    from afm import _lib
    f = getattr(_lib.lib(), "afm_screen_turnover_f64")
    assert f.restype is ctypes.c_int and len(f.argtypes) == 19
    assert f.argtypes[2] is ctypes.c_int64 and f.argtypes[6] is ctypes.c_int
    assert f.argtypes[13] is ctypes.c_void_p and f.argtypes[14] is ctypes.c_int
    f = getattr(_lib.lib(), "afm_screen_turnover_summary_f64")
    assert f.restype is ctypes.c_int and len(f.argtypes) == 8
    assert f.argtypes[4] is ctypes.c_int64 and f.argtypes[5:7] == [ctypes.c_int] * 2
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
    lags = (ctypes.c_int32 * 2)(1, 5)
    ctx.call("afm_screen_turnover_f64", None, 640, 10, 64, None, 2, None, None, None, 5, None,
             None, lags, 2, None, None, None, None)
    ctx.call("afm_screen_turnover_summary_f64", None, None, None, 5, 2, 2, None)
    ctx.call("afm_screen_turnover_scratch_bytes", 5, 2, 64)
    (n0, a0), (n1, a1), (n2, a2) = calls
    assert n0 == "afm_screen_turnover_f64" and a0[0] is ctx.handle and a0[2:5] == (640, 10, 64)
    assert a0[13] is lags and a0[14] == 2
    assert n1 == "afm_screen_turnover_summary_f64" and a1[0] is ctx.handle and a1[4:7] == (5, 2, 2)
    assert n2 == "afm_screen_turnover_scratch_bytes" and a2 == (5, 2, 64)   # no context
    with pytest.raises(TypeError):
        ctx.call("afm_screen_turnover_f64", None, 640)
    ctx.call("afm_combine_f64", None, 640, 10, 64, None, 2, None, None, None, 5, None, None, None,
             2, None, None)
    ctx.call("afm_vec_add_f64", 3, None, None)              # the old tables still resolve
    assert [c[0] for c in calls[3:]] == ["afm_combine_f64", "afm_vec_add_f64"]


def test_python_surface_and_lag_validation():
    import dataclasses

    import afm
    from afm.turnover import Turnover
    assert afm.Turnover is Turnover
    assert callable(afm.turnover_grid) and callable(afm.factor_turnover)
    assert Turnover().lags == (1, 5, 21)
    assert Turnover([2, 3]).lags == (2, 3)
    assert Turnover(tuple(range(1, 9))).lags == tuple(range(1, 9))
    with pytest.raises(dataclasses.FrozenInstanceError):
        Turnover().lags = (1,)
    for bad in ((), (0,), (-1, 2), (5, 1), (1, 1), tuple(range(1, 10)), (1.5,), ("1",), 3):
        with pytest.raises(ValueError):
            Turnover(bad)
    with pytest.raises(TypeError):
        afm.turnover._check_spec((1, 5))
