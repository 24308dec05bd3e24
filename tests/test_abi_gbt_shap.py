"""The library exports the symbols include/afm_gbt_shap.h declares, with the signatures of
afm/_lib.py's SIGNATURES_GBT_SHAP table (no GPU needed) -- what tests/test_abi_mlp.py checks for
include/afm_mlp.h, with the parser of tests/test_abi_screen_layers.py (uint8_t* as in
tests/test_abi_gbt.py) -- and the host side of the attribution: GBTModel's cover, its importance
kinds and the npz round trip."""
import ctypes
import os
import re

import numpy as np
import pytest

import test_abi_screen_layers as A

ROOT = A.ROOT
NAMES = ["afm_gbt_cover_i64", "afm_gbt_shap_f64", "afm_gbt_shap_scratch_bytes"]
NARGS = dict(zip(NAMES, (11, 21, 5)))


def shap_header(monkeypatch):
    src = open(os.path.join(ROOT, "include", "afm_gbt_shap.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    monkeypatch.setattr(A, "header_source", lambda: src)
    protos = A.header_prototypes()
    for name, params in re.findall(r"^(?:int64_t|int)\s+(afm_\w+)\s*\(([^)]*)\)\s*;", src,
                                   flags=re.M):
        for i, prm in enumerate(params.split(",")):
            if re.search(r"\buint8_t\s*\*", prm):
                assert protos[name][1][i] == "ptr"
                protos[name][1][i] = "u8*"
    return A.header_functions(), protos


def test_library_exports_shap_header_symbols(monkeypatch):
    from afm import _lib
    names, _ = shap_header(monkeypatch)
    assert sorted(names) == NAMES
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert hasattr(L, n)
    assert set(names) == set(_lib.SIGNATURES_GBT_SHAP)


def test_shap_table_matches_header_prototypes(monkeypatch):
    from afm import _lib
    names, protos = shap_header(monkeypatch)
    assert sorted(protos) == sorted(names)
    for n in NAMES:
        ret, kinds = protos[n]
        tret, tparams = _lib.SIGNATURES_GBT_SHAP[n]
        assert {"status": "int"}.get(tret, tret) == ret, n
        assert tparams.split() == kinds and len(kinds) == NARGS[n], n
    # addressing, zs and bits are afm_gbt_predict_f64's; cover follows the trees
    gp = _lib.SIGNATURES_GBT["afm_gbt_predict_f64"][1].split()
    sh = _lib.SIGNATURES_GBT_SHAP["afm_gbt_shap_f64"][1].split()
    assert sh[:12] == gp[:12] and sh[12] == "i64*" and sh[13:17] == gp[12:16]
    assert sh[17:] == ["i64*", "f64*", "f64*", "i64*"]           # scratch, contrib, agg, cnt
    assert _lib.SIGNATURES_GBT_SHAP["afm_gbt_cover_i64"][1].split()[1] == "u8*"


def test_header_guard_and_limit_and_the_gbt_header_is_untouched():
    src = open(os.path.join(ROOT, "include", "afm_gbt_shap.h")).read()
    assert "#ifndef AFM_GBT_SHAP_H" in src and "#define AFM_GBT_SHAP_H" in src
    assert '#include "afm_gbt.h"' in src
    assert dict(re.findall(r"#define (AFM_GBT_SHAP_\w+) (\d+)", src)) == \
        {"AFM_GBT_SHAP_MAX_TREES": "1048576"}
    gbt = open(os.path.join(ROOT, "include", "afm_gbt.h")).read()
    assert "shap" not in gbt and "cover" not in gbt
    mk = open(os.path.join(ROOT, "alpha-multi-factor-models_amd", "Makefile")).read()
    # the two object rules and the prof rule depend on every public header, this one included
    assert mk.count("$(wildcard $(INC)/*.h)") == 3 and "INC := $(HERE)../include" in mk
    assert not re.search(r"\$\(INC\)/afm\w*\.h", mk)


def test_shap_table_is_disjoint_and_layered_on_the_mlp_tables():
    from afm import _lib
    assert _lib.SHAP_TABLES == _lib.MLP_TABLES + (_lib.SIGNATURES_GBT_SHAP,)
    assert _lib.MLP_TABLES == _lib.GBT_TABLES + (_lib.SIGNATURES_MLP,)
    assert len(_lib.MLP_TABLES) == 12
    for table in _lib.MLP_TABLES:
        assert not set(_lib.SIGNATURES_GBT_SHAP) & set(table)
    assert not any(n.startswith(("afm_gbt_shap", "afm_gbt_cover")) for n in _lib.SIGNATURES_GBT)


def test_scratch_query_needs_no_context_and_rejects_bad_shapes():
    from afm import _lib
    f = _lib.lib().afm_gbt_shap_scratch_bytes
    assert f.restype is ctypes.c_int64
    assert f.argtypes == [ctypes.c_int64, ctypes.c_int64] + [ctypes.c_int] * 3
    small = f(128, 4, 8, 3, 25)
    assert small > 0 and small % 256 == 0
    # a path record per possible leaf, and {sum, sum |.|} per (date, block, column) + a count
    assert small >= 25 * 8 * 100 + 4 * 2 * 9 * 16 + 4 * 2 * 8
    assert f(128, 4, 8, 6, 25) > small > f(128, 4, 8, 3, 0) > 0
    assert f(128, 8, 8, 3, 25) > small and f(128, 4, 97, 3, 25) > small
    assert f(64, 0, 1, 1, 0) >= 0
    assert 0 < f(10048, 1300, 97, 3, 400) < (1 << 30)        # the headline test dates: under a GiB
    for lda, nt, p, D, R in ((0, 4, 8, 3, 25), (100, 4, 8, 3, 25), (128, -1, 8, 3, 25),
                             (128, 4, 0, 3, 25), (128, 4, 257, 3, 25), (128, 4, 8, 0, 25),
                             (128, 4, 8, 7, 25), (128, 4, 8, 3, -1), (128, 4, 8, 3, (1 << 20) + 1),
                             (128, 1 << 30, 8, 3, 25)):
        assert f(lda, nt, p, D, R) < 0, (lda, nt, p, D, R)
        assert b"afm_gbt_shap_scratch_bytes" in _lib.lib().afm_last_error()


def test_lib_and_call_plans_cover_the_new_table_and_the_old_ones(monkeypatch):
    from afm import _lib
    L = _lib.lib()
    for n in NAMES:
        f = getattr(L, n)
        assert len(f.argtypes) == NARGS[n]
        assert f.restype is (ctypes.c_int64 if n.endswith("_bytes") else ctypes.c_int)
    f = L.afm_gbt_shap_f64
    assert f.argtypes[1] is ctypes.c_void_p and f.argtypes[2:6] == [ctypes.c_int64] * 4
    assert f.argtypes[13:15] == [ctypes.c_int] * 2 and f.argtypes[15] is ctypes.c_double
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
    ctx.call("afm_gbt_cover_i64", None, 100, 128, 3, None, None, None, 3, 25, None)
    ctx.call("afm_gbt_shap_scratch_bytes", 128, 4, 8, 3, 25)
    ctx.call("afm_mlp_param_count", 5, 16, 16)
    (n0, a0), (n1, a1), (n2, _) = calls
    assert n0 == "afm_gbt_cover_i64" and a0[0] is ctx.handle and a0[2:5] == (100, 128, 3)
    assert n1 == "afm_gbt_shap_scratch_bytes" and a1 == (128, 4, 8, 3, 25)   # no context
    assert n2 == "afm_mlp_param_count"                                       # the old tables resolve
    with pytest.raises(TypeError):
        ctx.call("afm_gbt_shap_f64", None, 64)


def _model(cover="yes"):
    from afm.gbt import GBTModel, GBTParams
    prm = GBTParams(n_rounds=2, max_depth=2, eta=0.5, base_score=0.25)
    feat = np.array([[2, 0, -1, -1, -1, -2, -2], [0, -1, 2, -2, -2, -1, -1]], np.int32)
    sbin = np.where(feat >= 0, 1, -1).astype(np.int32)
    thr = np.where(feat >= 0, 0.5, 0.0)
    val = np.arange(14, dtype=np.float64).reshape(2, 7) / 8
    cov = np.array([[20, 12, 8, 5, 7, 0, 0], [20, 6, 14, 0, 0, 4, 10]], np.int64)
    ev = np.zeros((2, 2, 6))
    ev[:, :, 0] = 10
    args = (prm, ["a", "b", "c"], feat, sbin, thr, val, np.zeros((3, 255)), np.zeros(3, np.int32),
            ev)
    return GBTModel(*args, cover=cov) if cover else GBTModel(*args), cov


def test_model_cover_keyword_importance_and_npz_round_trip(tmp_path):
    import inspect
    from afm.gbt import GBTModel, check_cover
    prm = list(inspect.signature(GBTModel.__init__).parameters.values())
    assert [q.name for q in prm[1:10]] == ["params", "features", "feat", "bin", "thr", "val",
                                           "cuts", "ncuts", "evals_raw"]
    assert prm[10].name == "cover" and prm[10].default is None and len(prm) == 11
    m, cov = _model()
    assert m.cover.dtype == np.int64 and np.array_equal(m.cover, cov)
    # column a splits nodes (0,1) and (1,0): covers 12 and 20; column c splits (0,0) and (1,2)
    assert m.importance("total_cover").tolist() == [32.0, 0.0, 34.0]
    assert m.importance("cover").tolist() == [16.0, 0.0, 17.0]
    assert m.importance("weight").tolist() == [2.0, 0.0, 2.0]            # as before
    with pytest.raises(ValueError):
        m.importance("shap")
    check_cover(m)
    check_cover(m, 1)
    bare, _ = _model(cover=None)
    assert bare.cover is None
    for kind in ("cover", "total_cover"):
        with pytest.raises(ValueError, match="cover"):
            bare.importance(kind)
    with pytest.raises(ValueError, match="cover"):
        check_cover(bare)
    with pytest.raises(ValueError, match="cover"):
        bare.device_cover(None)
    for mod in (m, bare):
        path = tmp_path / "model.npz"
        mod.save(path)
        back = GBTModel.load(path)
        assert (back.cover is None) == (mod.cover is None)
        if mod.cover is not None:
            assert back.cover.tobytes() == mod.cover.tobytes() and back.cover.dtype == np.int64
        for k in ("feat", "bin", "thr", "val"):
            assert getattr(back, k).tobytes() == getattr(mod, k).tobytes()
    with np.load(path) as z:
        assert "cover" not in z.files
    with pytest.raises(ValueError):
        GBTModel(m.params, m.features, m.feat, m.bin, m.thr, m.val, m.cuts, m.ncuts, m.evals_raw,
                 cover=cov[:1])


def test_cover_is_validated_on_the_host_before_any_launch():
    from afm.gbt import check_cover, contribs_dense
    m, cov = _model()
    X = np.zeros((4, 3))
    bare, _ = _model(cover=None)
    with pytest.raises(ValueError, match="cover"):
        contribs_dense(bare, X)
    m.cover = cov.copy()
    m.cover[0, 3] = 0                                     # a present leaf nobody reaches
    with pytest.raises(ValueError, match="cover"):
        contribs_dense(m, X)
    check_cover(m, 0)                                     # no tree, nothing to check
    m.cover = cov.copy()
    m.cover[1, 2] = 15                                    # 15 != 4 + 10
    with pytest.raises(ValueError, match="cover"):
        contribs_dense(m, X)
    with pytest.raises(ValueError, match="cover"):
        check_cover(m)
    check_cover(m, 1)                                     # the first tree alone is fine
    with pytest.raises(ValueError):
        contribs_dense(_model()[0], np.zeros((4, 2)))     # other features


def test_pipeline_attribution_methods_are_one_gpu_only_and_validate():
    from types import SimpleNamespace
    from afm.pipeline import Pipeline
    with pytest.raises(NotImplementedError):
        Pipeline.gbt_contribs(SimpleNamespace(W=2), None)
    with pytest.raises(NotImplementedError):
        Pipeline.selected_features(SimpleNamespace(W=2), None, by="shap")
    with pytest.raises(TypeError):
        Pipeline.gbt_contribs(SimpleNamespace(W=1), object())
    m, _ = _model()
    with pytest.raises(ValueError, match="split"):
        Pipeline.gbt_contribs(SimpleNamespace(W=1), m, split="all")
    with pytest.raises(ValueError, match="by="):
        Pipeline.selected_features(SimpleNamespace(W=1), m, by="gain")
    doc = Pipeline.gbt_contribs.__doc__
    assert "nt * (p + 1) * lda * 8" in doc and "4.8 GB" in doc and "8 GB per 1,000" in doc
    assert 605 * 98 * 10048 * 8 == 4765967360                 # that configuration's planes
