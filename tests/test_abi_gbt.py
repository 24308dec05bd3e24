"""The library exports the symbols include/afm_gbt.h declares, with the signatures of
afm/_lib.py's SIGNATURES_GBT table (no GPU needed) -- what tests/test_abi_turnover.py checks for
include/afm_turnover.h, with the parser of tests/test_abi_screen_layers.py (uint8_t* added)."""
import ctypes
import dataclasses
import os
import re

import numpy as np
import pytest

import test_abi_screen_layers as A

ROOT = A.ROOT
NAMES = ["afm_gbt_bin_f64", "afm_gbt_fit_f64", "afm_gbt_hist_i64", "afm_gbt_predict_f64",
         "afm_gbt_scratch_bytes", "afm_gbt_values_f64"]
NARGS = dict(zip(NAMES, (16, 23, 11, 17, 4, 12)))


def gbt_header(monkeypatch):
    src = open(os.path.join(ROOT, "include", "afm_gbt.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    # the shared parser knows double / int32_t / int64_t / uint64_t elements: a uint8_t buffer is
    # parsed under a name of its own and mapped to the table's "u8*" below
    monkeypatch.setattr(A, "header_source", lambda: src)
    protos = A.header_prototypes()
    for name, params in re.findall(r"^(?:int64_t|int)\s+(afm_\w+)\s*\(([^)]*)\)\s*;", src,
                                   flags=re.M):
        for i, prm in enumerate(params.split(",")):
            if re.search(r"\buint8_t\s*\*", prm):
                assert protos[name][1][i] == "ptr"
                protos[name][1][i] = "u8*"
    return A.header_functions(), protos


def test_library_exports_gbt_header_symbols(monkeypatch):
    from afm import _lib
    names, _ = gbt_header(monkeypatch)
    assert sorted(names) == NAMES
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(L, n)
    assert set(names) == set(_lib.SIGNATURES_GBT)


def test_gbt_table_matches_header_prototypes(monkeypatch):
    from afm import _lib
    names, protos = gbt_header(monkeypatch)
    assert sorted(protos) == sorted(names)
    for n in NAMES:
        ret, kinds = protos[n]
        tret, tparams = _lib.SIGNATURES_GBT[n]
        assert {"status": "int"}.get(tret, tret) == ret, n
        assert tparams.split() == kinds and len(kinds) == NARGS[n], n
    assert _lib.SIGNATURES_GBT["afm_gbt_scratch_bytes"] == ("i64", "i64 int int int")
    assert _lib.SIGNATURES_GBT["afm_gbt_hist_i64"][1].split()[1] == "u8*"
    assert _lib.SIGNATURES_GBT["afm_gbt_bin_f64"][1].split()[-1] == "u8*"


def test_header_limits_and_guard():
    src = open(os.path.join(ROOT, "include", "afm_gbt.h")).read()
    assert dict(re.findall(r"#define (AFM_GBT_\w+) (\d+)", src)) == \
        {"AFM_GBT_MAX_DEPTH": "6", "AFM_GBT_MAX_BIN": "256", "AFM_GBT_MAX_COLS": "256",
         "AFM_GBT_MAX_WEIGHT": "4095"}
    assert "#ifndef AFM_GBT_H" in src and "#define AFM_GBT_H" in src
    from afm import gbt
    assert (gbt.MAX_DEPTH, gbt.MAX_BIN, gbt.MAX_COLS, gbt.MAX_WEIGHT) == (6, 256, 256, 4095)


def test_gbt_table_is_disjoint_and_layered_on_the_turnover_tables():
    from afm import _lib
    assert _lib.GBT_TABLES == _lib.TURNOVER_TABLES + (_lib.SIGNATURES_GBT,)
    assert len(_lib.TURNOVER_TABLES) == 10
    for table in _lib.TURNOVER_TABLES:
        assert not set(_lib.SIGNATURES_GBT) & set(table)


def test_predict_arguments_follow_zpredict():
    """afm_gbt_predict_f64 takes afm_zpredict_f64's arguments with the trees (and their depth,
    count and base score) in place of beta."""
    from afm import _lib
    zp = _lib.SIGNATURES["afm_zpredict_f64"][1].split()
    gp = _lib.SIGNATURES_GBT["afm_gbt_predict_f64"][1].split()
    assert gp[:9] == zp[:9]                                  # ctx .. zs
    assert gp[9:15] == ["i32*", "f64*", "f64*", "int", "int", "f64"]
    assert gp[15:] == zp[10:]                                # bits, pred


def test_scratch_query_needs_no_context_and_rejects_bad_shapes():
    from afm import _lib
    f = _lib.lib().afm_gbt_scratch_bytes
    assert f.restype is ctypes.c_int64
    assert f.argtypes == [ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    small = f(1000, 8, 3, 256)
    assert small > 0 and small % 256 == 0
    # the level histograms (4 nodes x 8 columns x 256 bins x 16 bytes) and 16 bytes a row
    assert small >= 4 * 8 * 256 * 16 + 16 * 1000
    assert f(1000, 8, 6, 256) > f(1000, 8, 3, 256) > f(1000, 8, 3, 16)
    assert 0 < f(41_000_000, 97, 3, 256) <= (1 << 30)        # the headline fit: under a GiB
    for n, p, D, B in ((0, 8, 3, 256), (1 << 31, 8, 3, 256), (10, 0, 3, 256), (10, 257, 3, 256),
                       (10, 8, 0, 256), (10, 8, 7, 256), (10, 8, 3, 1), (10, 8, 3, 257)):
        assert f(n, p, D, B) < 0
        assert b"afm_gbt_scratch_bytes" in _lib.lib().afm_last_error()


def test_lib_and_call_plans_cover_the_new_table_and_the_old_ones(monkeypatch):
    from afm import _lib
    L = _lib.lib()
    for n in NAMES:
        f = getattr(L, n)
        assert len(f.argtypes) == NARGS[n]
        assert f.restype is (ctypes.c_int64 if n == "afm_gbt_scratch_bytes" else ctypes.c_int)
    f = L.afm_gbt_fit_f64
    assert f.argtypes[1] is ctypes.c_void_p and f.argtypes[2] is ctypes.c_int64
    assert f.argtypes[9:12] == [ctypes.c_int] * 3 and f.argtypes[12:16] == [ctypes.c_double] * 4
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
    ctx.call("afm_gbt_hist_i64", None, 100, 128, 3, 16, None, None, None, 4, None)
    ctx.call("afm_gbt_scratch_bytes", 100, 3, 3, 16)
    ctx.call("afm_screen_turnover_summary_f64", None, None, None, 5, 2, 2, None)
    (n0, a0), (n1, a1), (n2, _) = calls
    assert n0 == "afm_gbt_hist_i64" and a0[0] is ctx.handle and a0[2:6] == (100, 128, 3, 16)
    assert n1 == "afm_gbt_scratch_bytes" and a1 == (100, 3, 3, 16)          # no context
    assert n2 == "afm_screen_turnover_summary_f64"                           # the old tables resolve
    with pytest.raises(TypeError):
        ctx.call("afm_gbt_hist_i64", None, 100)


def test_u8_buffers_are_checked():
    """A u8* parameter takes a contiguous torch.uint8 tensor on the context's device or None."""
    import torch
    from afm import _lib
    conv = _lib._device_buffer(torch.uint8, 0, "bins")
    assert conv(None) is None
    with pytest.raises(_lib.AfmError):
        conv(torch.zeros(4, dtype=torch.uint8))              # on the host
    with pytest.raises(_lib.AfmError):
        conv(np.zeros(4, dtype=np.uint8))
    plans = _lib._plans(0)
    assert len(plans["afm_gbt_hist_i64"][1]) == 10
    with pytest.raises(_lib.AfmError):
        plans["afm_gbt_hist_i64"][1][0](torch.zeros(4, dtype=torch.int32))


def test_option_is_listed():
    from afm import _lib
    assert _lib.options.DEFAULTS["gbt_rows_per_wg"] == 0
    src = open(os.path.join(ROOT, "include", "afm.h")).read()
    assert '"gbt_rows_per_wg"' in src
    abi = open(os.path.join(ROOT, "alpha-multi-factor-models_amd", "csrc", "abi.cpp")).read()
    assert abi.count('"gbt_rows_per_wg"') == 2               # set and get


def test_python_surface_and_parameter_validation():
    import afm
    from afm.gbt import GBTModel, GBTParams, GBTRegressor
    assert afm.GBTParams is GBTParams and afm.GBTModel is GBTModel
    assert afm.GBTRegressor is GBTRegressor
    d = GBTParams()
    assert (d.n_rounds, d.max_depth, d.eta) == (400, 3, 0.025)
    assert (d.reg_lambda, d.gamma, d.min_child_weight, d.max_bin, d.base_score) == \
        (1.0, 0.0, 1.0, 256, 0.0)
    assert d.n_nodes == 15 and GBTParams(max_depth=6).n_nodes == 127
    assert "excess return" in GBTParams.__doc__
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.eta = 0.1
    for bad in (dict(n_rounds=0), dict(max_depth=0), dict(max_depth=7), dict(max_bin=1),
                dict(max_bin=257), dict(reg_lambda=-1.0), dict(gamma=-0.5),
                dict(min_child_weight=0.5), dict(eta=float("nan")), dict(base_score=float("inf")),
                dict(max_depth=2.5), dict(eta="0.1"), dict(n_rounds="3")):
        with pytest.raises(ValueError):
            GBTParams(**bad)
    assert GBTRegressor(max_depth=2, n_rounds=5).params == GBTParams(max_depth=2, n_rounds=5)
    with pytest.raises(TypeError):
        GBTRegressor(depth=2)
    with pytest.raises(TypeError):
        afm.gbt._check_params({"max_depth": 3})


def test_model_importance_top_features_and_npz_round_trip(tmp_path):
    from afm.gbt import GBTModel, GBTParams
    prm = GBTParams(n_rounds=2, max_depth=2, eta=0.5, base_score=0.25)
    feat = np.array([[2, 0, -1, -1, -1, -2, -2], [0, -1, 2, -2, -2, -1, -1]], np.int32)
    sbin = np.where(feat >= 0, 1, -1).astype(np.int32)
    thr = np.where(feat >= 0, 0.5, 0.0)
    val = np.arange(14, dtype=np.float64).reshape(2, 7) / 8
    ev = np.zeros((2, 2, 6))
    ev[:, :, 0] = 10
    ev[:, 1] = [[10, 1, 2, 5, 6, 5.0], [10, 1, 2, 5, 6, 4.0]]           # valid IC: round 1 higher
    m = GBTModel(prm, ["a", "b", "c"], feat, sbin, thr, val, np.zeros((3, 255)),
                 np.zeros(3, np.int32), ev)
    assert m.importance("weight").tolist() == [2.0, 0.0, 2.0]
    assert m.top_features(10) == ["a", "c"]                   # ties by column order, "b" never split
    assert m.top_features(1) == ["a"]
    assert m.importance("gain")[1] == 0.0 and m.importance("gain")[0] > 0
    with pytest.raises(ValueError):
        m.importance("cover")
    assert m.best_round == 1 and m.n_trees == 2
    assert list(m.evals.columns) == ["train_rmse", "train_ic", "valid_rmse", "valid_ic",
                                     "n_train", "n_valid"]
    path = tmp_path / "model.npz"
    m.save(path)
    m2 = GBTModel.load(path)
    assert m2.params == prm and m2.features == m.features and m2.best_round == 1
    for k in ("feat", "bin", "thr", "val", "cuts", "ncuts", "evals_raw"):
        assert getattr(m2, k).tobytes() == getattr(m, k).tobytes() and \
            getattr(m2, k).dtype == getattr(m, k).dtype


def test_pipeline_gbt_methods_are_one_gpu_only():
    from types import SimpleNamespace
    from afm.pipeline import Pipeline
    for call in (lambda s: Pipeline.gbt_fit(s), lambda s: Pipeline.gbt_predict(s, None),
                 lambda s: Pipeline.selected_features(s, None)):
        with pytest.raises(NotImplementedError):
            call(SimpleNamespace(W=2))


def test_regressor_rejects_non_finite_input_on_the_host():
    from afm.gbt import GBTRegressor
    X = np.zeros((8, 2))
    y = np.zeros(8)
    X[3, 1] = np.nan
    with pytest.raises(ValueError, match="NaN or inf"):
        GBTRegressor(n_rounds=1).fit(X, y)
    X[3, 1] = 0.0
    y[2] = np.inf
    with pytest.raises(ValueError, match="NaN or inf"):
        GBTRegressor(n_rounds=1).fit(X, y)
    y[2] = 0.0
    for sw in (np.full(8, 0.5), np.full(8, -1.0), np.full(8, 4096.0)):
        with pytest.raises(ValueError, match="sample_weight"):
            GBTRegressor(n_rounds=1).fit(X, y, sample_weight=sw)
    with pytest.raises(ValueError, match="positive weight"):
        GBTRegressor(n_rounds=1).fit(X, y, sample_weight=np.zeros(8))
