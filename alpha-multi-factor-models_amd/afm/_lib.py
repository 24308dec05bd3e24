"""ctypes binding of libafm.so (the C-ABI declared in include/afm.h, include/afm_mv.h,
include/afm_screen.h, include/afm_rankic.h, include/afm_seams.h, include/afm_screen_layers.h,
include/afm_xcorr.h, include/afm_xsprep.h, include/afm_combine.h, include/afm_turnover.h,
include/afm_gbt.h, include/afm_mlp.h, include/afm_gbt_shap.h, include/afm_risk.h and
include/afm_lstm.h).

The product path has no CPU fallback: if the library is missing or no GPU is visible, every
call raises.  ``make -C alpha-multi-factor-models_amd`` (or ``__graft_entry__.build()``) builds
the library in-tree.
"""
from __future__ import annotations

import contextlib
import ctypes
import operator
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
# AFM_LIB: an alternative build of the same library (A/B kernel variants, profiling builds)
LIB_PATH = os.environ.get("AFM_LIB") or os.path.join(HERE, "libafm.so")

P = ctypes.c_void_p
I64 = ctypes.c_int64
I32 = ctypes.c_int
DBL = ctypes.c_double

# name -> (return, parameters) as include/afm.h declares them (tests/test_abi.py compares every
# prototype with this table).  Return: "status" (int: 0 or an AFM_E* code), "int" / "i64" (a value,
# negative on failure), "str".  Parameters: ctx (afm_ctx*), int, i64, f64, str (const char*);
# device buffers by element type -- f64*, i32*, i64* (int64_t / uint64_t: torch.int64 words);
# ptr: opaque (void*, afm_ctx**, a host array); host:i64*: a host int64_t.
SIGNATURES = {
    "afm_ctx_create": ("status", "int ptr"),
    "afm_ctx_set_stream": ("status", "ctx ptr"),
    "afm_ctx_set_option": ("status", "ctx str i64"),
    "afm_ctx_get_option": ("status", "ctx str host:i64*"),
    "afm_stream_create_cu_mask": ("status", "int ptr int ptr"),
    "afm_stream_destroy": ("status", "ptr"),
    "afm_ctx_destroy": ("status", "ctx"),
    "afm_last_error": ("str", ""),
    "afm_version": ("int", ""),
    "afm_factor_name": ("str", "int"),
    "afm_factors_f64": ("status", "ctx i64 i64 i64 f64* f64* f64* f64* i64* f64* i64* i64*"),
    "afm_factors_state_bytes": ("i64", "ctx i64"),
    "afm_factors_slab_f64": ("status", "ctx i64 i64 i64 i64 i64 f64* f64* f64* f64* i64* f64* i64* "
                                       "i64* f64*"),
    "afm_factors_range_f64": ("status", "ctx i64 i64 i64 i64 i64 f64* f64* f64* f64* i64* f64* "
                                        "i64* i64* f64*"),
    "afm_xs_gram_f64": ("status", "ctx f64* i64 i64 i64 i64 i32* int int i64* i64 i64 f64* f64*"),
    "afm_ols_solve_f64": ("status", "ctx f64* f64* int i64 f64 f64* f64* i32*"),
    "afm_pool_moments_f64": ("status", "ctx f64* f64* int i64 f64* f64*"),
    "afm_pool_tree_f64": ("status", "ctx f64* f64* int i64 int f64* f64*"),
    "afm_pool_segments_f64": ("status", "ctx f64* f64* int i64 i64 f64* f64*"),
    "afm_labels_f64": ("status", "ctx i64 i64 i64 i64 f64* f64* i64* f64* f64*"),
    "afm_drop_last_obs_bits": ("status", "ctx i64 i64 i64* i64* i64*"),
    "afm_drop_last_obs_bits_range": ("status", "ctx i64 i64 i64* i64* i64* i64 i64"),
    "afm_factors_part_words": ("i64", "ctx i64 i64 i64 i64"),
    "afm_factors_range_part_f64": ("status", "ctx i64 i64 i64 i64 i64 f64* f64* i64* f64* f64* "
                                             "i64*"),
    "afm_factor_masks_f64": ("status", "ctx i64 i64 i64 i64 i64 i64* i64* i64* i64*"),
    "afm_predict_f64": ("status", "ctx f64* i64 i64 i64 i64 i32* int f64* i64 i64* int f64*"),
    "afm_fama_macbeth_f64": ("status", "ctx f64* i32* i64 int f64* f64*"),
    "afm_ols_residual_f64": ("status", "ctx f64* i64 int int f64* f64* f64*"),
    "afm_vec_add_f64": ("status", "ctx i64 f64* f64*"),
    "afm_ols_intercept_f64": ("status", "ctx int f64* f64*"),
    "afm_lasso_cd_f64": ("status", "ctx f64* int f64 f64 int f64 int f64* f64*"),
    "afm_talib_factors_f64": ("status", "ctx i64 i64 i64 f64* f64* i64* f64*"),
    "afm_ffill_f64": ("status", "ctx i64 i64 i64 f64* i64*"),
    "afm_date_mean_fill_f64": ("status", "ctx i64 i64 i64 i64 f64* i64* f64*"),
    "afm_group_demean_f64": ("status", "ctx i64 i64* i64 f64* f64* f64*"),
    "afm_rebalance_f64": ("status", "ctx i64 i64 i64 i32* i64 f64* i64* f64* i64* i64 i64 i64 f64* "
                                    "f64* int f64 f64 i32* i32* f64* f64* i32* i64* i32*"),
    "afm_pnl_scan_f64": ("status", "ctx i64 i32* i32* f64* i32* i64* f64 f64 f64* f64* f64* f64*"),
    "afm_bootstrap_pnl_f64": ("status", "ctx i64 i32* i64 f64* i32* i32* f64* i64 i64 i32* f64 f64 "
                                        "f64* f64* f64* f64*"),
    "afm_min_variance_weights_f64": ("status", "ctx f64* i64 i64 int f64 f64 f64* f64* i32*"),
    "afm_fwd_returns_f64": ("status", "ctx i64 i64 f64* i64* f64*"),
    "afm_xs_prepare_f64": ("status", "ctx i64 i64 i64 f64* f64* f64* f64* i32* i32*"),
    "afm_xs_prepare_range_f64": ("status", "ctx i64 i64 i64 i64 i64 f64* f64* f64* f64* i32* i32*"),
    "afm_xs_rank_f64": ("status", "ctx i64 i64 f64* i32* i64* i32* i32* i32*"),
    "afm_xs_layers_f64": ("status", "ctx i64 i64 f64* i32* i64* i32* i32* i32*"),
    "afm_xs_stats_f64": ("status", "ctx i64 i64 i32* i64 f64* i32* i32* i32* int f64* f64* i32* "
                                   "f64*"),
    "afm_xs_series_f64": ("status", "ctx i64 f64* f64* f64* i32* int int f64* f64* f64* f64* f64*"),
    "afm_zscore_stats_f64": ("status", "ctx f64* i64 i64 i64 i32* int i64* i64 i64 f64* f64*"),
    "afm_zscore_stats_slab_f64": ("status", "ctx f64* i64 i64 i64 i32* int i64* i64 i64 f64* int "
                                            "int f64* f64*"),
    "afm_zscore_apply_f64": ("status", "ctx f64* i64 i64 i64 i32* int i64* i64 i64 f64* f64* f64* "
                                       "i64 i32* i64*"),
    "afm_zgram_part_bytes": ("int", "int"),
    "afm_zstats_finalize_f64": ("status", "ctx f64* f64* int i64 f64* i32*"),
    "afm_row_bits": ("status", "ctx i64 i64 i64* i64* i32* i64 i64 i64*"),
    "afm_zgram_f64": ("status", "ctx f64* i64 i64 i32* i32* int int f64* int i64* i64 i64 int i64 "
                                "i64 i64 f64* int"),
    "afm_zpool_f64": ("status", "ctx f64* i64 i64 i32* i32* int int f64* int i64* i64 i64 i64 int "
                                "i64 int f64* int"),
    "afm_gram_tree_f64": ("status", "ctx int f64* i64 int int f64*"),
    "afm_zpredict_f64": ("status", "ctx f64* i64 i64 i64 i64 i32* int f64* f64* i64* f64*"),
    "afm_lasso_fit_f64": ("status", "ctx f64* f64* int f64 int f64 int f64* f64*"),
    "afm_lasso_batch_f64": ("status", "ctx f64* i64 f64* i64 int f64* int i64 int int f64 int f64* "
                                      "f64*"),
    "afm_gram_score_f64": ("status", "ctx f64* i64 f64* i64 int f64* int i64 f64*"),
}
# the same for include/afm_mv.h, the mean-variance entry points (tests/test_abi_mv.py)
SIGNATURES_MV = {
    "afm_rebalance_mv_f64": ("status", "ctx i64 i64 i64 i32* i64 f64* i64* f64* i64* i64 i64 i64 "
                                       "f64* f64* int f64 f64 f64* f64 i32* i32* f64* f64* i32* "
                                       "i64* i32*"),
    "afm_mean_variance_weights_f64": ("status", "ctx f64* i64 i64 int f64* f64 f64 f64 f64* f64* "
                                                "i32*"),
}
# ... and for include/afm_screen.h, the factor-screening entry points (tests/test_abi_screen.py)
SIGNATURES_SCREEN = {
    "afm_screen_ic_f64": ("status", "ctx f64* i64 i64 i64 i32* int f64* i32* i32* i64 f64* i32* "
                                    "i32* f64*"),
    "afm_screen_summary_f64": ("status", "ctx f64* i64 int i32* int int f64* f64* f64*"),
}
TABLES = (SIGNATURES, SIGNATURES_MV, SIGNATURES_SCREEN)
# ... and for include/afm_rankic.h, the rank (Spearman) IC entry points (tests/test_abi_rankic.py)
SIGNATURES_RANK = {
    "afm_rank_scratch_words": ("i64", "i64"),
    "afm_rank_returns_f64": ("status", "ctx i64 i64 i32* i64 f64* i32* i32* i64* i64*"),
    "afm_screen_rank_ic_f64": ("status", "ctx f64* i64 i64 i64 i32* int f64* i32* i32* i64 f64* "
                                         "i32* i32* i32* i64* i64* f64*"),
}
ALL_TABLES = TABLES + (SIGNATURES_RANK,)
# ... and for include/afm_seams.h, the fused launches of the step's seams (tests/test_abi_seams.py)
SIGNATURES_SEAMS = {
    "afm_gram_tree3_f64": ("status", "ctx int f64* int int int int int f64*"),
    "afm_gram_final_f64": ("status", "ctx int f64* int f64* int f64* f64*"),
    "afm_ols_solve_parts_f64": ("status", "ctx f64* int f64* int i64 f64 f64* f64* i32*"),
    "afm_factors_rows_f64": ("status", "ctx i64 i64 i64 f64* f64* f64* f64* i64* f64* i64* i64* "
                                       "i64* i64*"),
    "afm_zstats_rows_f64": ("status", "ctx f64* f64* int i64 f64* i32* i64 i64* i64 i64 i64*"),
}
LOADED_TABLES = ALL_TABLES + (SIGNATURES_SEAMS,)
# ... and for include/afm_screen_layers.h, the layers / long-short / top-k of the factor screen
# (tests/test_abi_screen_layers.py)
SIGNATURES_LAYERS = {
    "afm_screen_layers_f64": ("status", "ctx f64* i64 i64 i64 i32* int f64* i32* i32* i64 f64* i32* "
                                        "i32* f64* i32* f64* f64*"),
    "afm_screen_layer_series_f64": ("status", "ctx i64 int f64* f64* f64* f64* f64*"),
}
BOUND_TABLES = LOADED_TABLES + (SIGNATURES_LAYERS,)
# ... and for include/afm_xcorr.h, the cross-factor correlation of the screen (tests/test_abi_xcorr.py)
SIGNATURES_XCORR = {
    "afm_screen_xcorr_f64": ("status", "ctx f64* i64 i64 i64 i32* int f64* i32* i32* i64 f64* i32* "
                                       "i32* f64*"),
    "afm_screen_xcorr_summary_f64": ("status", "ctx f64* i64 int f64*"),
}
CALL_TABLES = BOUND_TABLES + (SIGNATURES_XCORR,)
# ... and for include/afm_xsprep.h, the per-date winsorise / neutralise / standardise in front of
# the screen (tests/test_abi_xsprep.py)
SIGNATURES_XSPREP = {
    "afm_xs_preprocess_f64": ("status", "ctx f64* i64 i64 i64 i32* int f64* i32* i32* i64 i32* i32* "
                                        "i32* i64 int int f64 f64 int f64* i64 f64*"),
}
PREP_TABLES = CALL_TABLES + (SIGNATURES_XSPREP,)
# ... and for include/afm_combine.h, the rolling IC weights and the weighted composite of the
# screened columns (tests/test_abi_combine.py)
SIGNATURES_COMBINE = {
    "afm_ic_weights_f64": ("status", "ctx f64* i64 int int int int int int f64 f64* f64*"),
    "afm_combine_f64": ("status", "ctx f64* i64 i64 i64 i32* int f64* i32* i32* i64 i32* i32* f64* "
                                  "i64 f64* i32*"),
}
COMBINE_TABLES = PREP_TABLES + (SIGNATURES_COMBINE,)
# ... and for include/afm_turnover.h, the rank autocorrelation and turnover of the screened columns
# (tests/test_abi_turnover.py); host:i32*: a host int32_t array
SIGNATURES_TURNOVER = {
    "afm_screen_turnover_scratch_bytes": ("i64", "i64 int i64"),
    "afm_screen_turnover_f64": ("status", "ctx f64* i64 i64 i64 i32* int f64* i32* i32* i64 i32* "
                                          "i32* host:i32* int f64* i32* f64* i64*"),
    "afm_screen_turnover_summary_f64": ("status", "ctx f64* i32* f64* i64 int int f64*"),
}
TURNOVER_TABLES = COMBINE_TABLES + (SIGNATURES_TURNOVER,)
# ... and for include/afm_gbt.h, the gradient-boosted trees (tests/test_abi_gbt.py); u8*: a device
# buffer of bytes (torch.uint8), the bin matrix
SIGNATURES_GBT = {
    "afm_gbt_scratch_bytes": ("i64", "i64 int int int"),
    "afm_gbt_values_f64": ("status", "ctx f64* i64 i64 i64 i32* int f64* i32* i32* i64 f64*"),
    "afm_gbt_bin_f64": ("status", "ctx f64* i64 i64 i64 i32* int f64* i32* i32* i64 i64 f64* i32* "
                                  "int u8*"),
    "afm_gbt_hist_i64": ("status", "ctx u8* i64 i64 int int i32* i64* i32* int i64*"),
    "afm_gbt_fit_f64": ("status", "ctx u8* i64 i64 int f64* i32* f64* i32* int int int f64 f64 f64 "
                                  "f64 i32* i32* f64* f64* f64* f64* i64*"),
    "afm_gbt_predict_f64": ("status", "ctx f64* i64 i64 i64 i64 i32* int f64* i32* f64* f64* int "
                                      "int f64 i64* f64*"),
}
GBT_TABLES = TURNOVER_TABLES + (SIGNATURES_GBT,)
# ... and for include/afm_mlp.h, the ensembles of dense networks (tests/test_abi_mlp.py);
# host:f64*: a host array of doubles (the learning rates)
SIGNATURES_MLP = {
    "afm_mlp_param_count": ("i64", "int int int"),
    "afm_mlp_scratch_bytes": ("i64", "int int int int int"),
    "afm_mlp_fit_f64": ("status", "ctx f64* f64* i64 i64 i64 int int int int f64* host:f64* f64 f64 "
                                  "f64 int int f64* f64* f64*"),
    "afm_mlp_forward_f64": ("status", "ctx f64* i64 i64 i64 int int int int f64* f64*"),
}
MLP_TABLES = GBT_TABLES + (SIGNATURES_MLP,)
# ... and for include/afm_gbt_shap.h, the cover and the TreeSHAP contributions of the boosted trees
# (tests/test_abi_gbt_shap.py)
SIGNATURES_GBT_SHAP = {
    "afm_gbt_cover_i64": ("status", "ctx u8* i64 i64 int i32* i32* i32* int int i64*"),
    "afm_gbt_shap_scratch_bytes": ("i64", "i64 i64 int int int"),
    "afm_gbt_shap_f64": ("status", "ctx f64* i64 i64 i64 i64 i32* int f64* i32* f64* f64* i64* int "
                                   "int f64 i64* i64* f64* f64* i64*"),
}
SHAP_TABLES = MLP_TABLES + (SIGNATURES_GBT_SHAP,)
# ... and for include/afm_risk.h, the factor risk model and the weight solve from a supplied
# covariance (tests/test_abi_risk.py)
SIGNATURES_RISK = {
    "afm_risk_resid_f64": ("status", "ctx f64* i64 i64 i64 i64 i32* int int f64* i32* i64* f64*"),
    "afm_risk_factor_cov_f64": ("status", "ctx f64* i32* i64 int f64 int int f64* i32*"),
    "afm_risk_specific_f64": ("status", "ctx f64* i64 i64 i64 f64 int int f64* f64*"),
    "afm_risk_book_f64": ("status", "ctx f64* i64 i64 i64 i32* int i32* i64 i32* i32* f64* f64* f64* "
                                    "f64* int f64* f64* f64* i32*"),
    "afm_cov_weights_f64": ("status", "ctx f64* int f64* f64 f64 f64 f64* i32*"),
    "afm_rebalance_cov_f64": ("status", "ctx i64 i64 i32* i64 i32* i32* f64* int i32* f64* f64 f64 "
                                        "f64 f64* f64* f64* f64* i32*"),
}
RISK_TABLES = SHAP_TABLES + (SIGNATURES_RISK,)
# ... and for include/afm_lstm.h, the ensembles of stacked LSTMs (tests/test_abi_lstm.py)
SIGNATURES_LSTM = {
    "afm_lstm_param_count": ("i64", "int int int"),
    "afm_lstm_scratch_bytes": ("i64", "int int int int int int"),
    "afm_lstm_fit_f64": ("status", "ctx f64* f64* i64 i64 i64 int int int int int f64* host:f64* f64 "
                                   "f64 f64 int int f64* f64* f64*"),
    "afm_lstm_grad_f64": ("status", "ctx f64* f64* i64 i64 int int int int int int f64* f64* f64* "
                                    "f64*"),
    "afm_lstm_forward_f64": ("status", "ctx f64* i64 i64 i64 int int int int int f64* f64*"),
    "afm_lstm_act_f64": ("status", "ctx int f64* i64 f64*"),
}
LSTM_TABLES = RISK_TABLES + (SIGNATURES_LSTM,)      # what lib() declares and Context.call resolves
_RESTYPE = {"status": I32, "int": I32, "i64": I64, "str": ctypes.c_char_p}
_ARGTYPE = {"int": I32, "i64": I64, "f64": DBL, "str": ctypes.c_char_p}    # every pointer: void*


class AfmError(RuntimeError):
    pass


_lib = None
_lock = threading.Lock()


def lib():
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise ImportError(f"{LIB_PATH} is not built: run `make -C "
                                      f"{os.path.dirname(HERE)}` (hipcc, gfx950)")
                L = ctypes.CDLL(LIB_PATH)
                for table in LSTM_TABLES:
                    for name, (res, params) in table.items():
                        f = getattr(L, name)
                        f.restype = _RESTYPE[res]
                        f.argtypes = [_ARGTYPE.get(t, P) for t in params.split()]
                _lib = L
    return _lib


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().afm_last_error().decode(errors="replace")
        raise AfmError(f"{what or 'afm'} failed ({rc}): {msg}")


def _as_given(a):
    return a


def _device_buffer(dtype, device: int, where: str):
    """Converter of one f64* / i32* / i64* / u8* parameter: None -> NULL, a contiguous ``dtype`` tensor
    on cuda:``device`` -> its address; anything else is rejected before the library is entered."""
    import torch

    def conv(t):
        if t is None:
            return None
        if not isinstance(t, torch.Tensor):
            raise AfmError(f"{where}: expected a {dtype} tensor or None, got {type(t).__name__}")
        if t.get_device() != device or t.dtype is not dtype or not t.is_contiguous():
            raise AfmError(f"{where}: expected a contiguous {dtype} tensor on cuda:{device}, got "
                           f"{t.dtype} on {t.device}, contiguous={t.is_contiguous()}")
        return t.data_ptr()
    return conv


def _plans(device: int) -> dict:
    """name -> (takes the context, one converter per further parameter, failed(return value)):
    how Context.call marshals each entry point of the signature tables for the context of
    ``device``."""
    import torch
    scalar = {"int": operator.index, "i64": operator.index, "f64": float}
    buffer = {"f64*": torch.float64, "i32*": torch.int32, "i64*": torch.int64,
              "u8*": torch.uint8}
    negative = (0).__gt__
    failed = {"status": bool, "int": negative, "i64": negative, "str": lambda s: s is None}
    plans = {}
    for name, (res, params) in (item for table in LSTM_TABLES for item in table.items()):
        toks = params.split()
        takes_ctx = toks[:1] == ["ctx"]
        convs = tuple(_device_buffer(buffer[t], device, f"{name} argument {i}") if t in buffer
                      else scalar.get(t, _as_given)
                      for i, t in enumerate(toks[takes_ctx:], 1))
        plans[name] = (takes_ctx, convs, failed[res])
    return plans


class Context:
    """One afm_ctx per device; calls are issued on torch's current stream of that device."""

    _by_device: dict = {}

    def __init__(self, device: int):
        self.device = device
        h = P()
        check(lib().afm_ctx_create(device, ctypes.byref(h)), "afm_ctx_create")
        self.handle = h
        self._plans = _plans(device)

    def call(self, name: str, *args):
        """The entry point ``name`` of the library (looked up at call time) with this context's
        handle first where it takes one, ``args`` marshalled by its SIGNATURES entry: a device
        buffer parameter takes a tensor (checked: device, dtype, contiguity) or None, an integer
        parameter anything with ``__index__``, a double anything ``float()`` takes, an opaque
        pointer a c_void_p / ctypes array / int.  Raises AfmError on a failure return (a status
        that is not 0, a negative count), else returns the value.  The stream is the caller's
        business: ``on`` inside a pipeline, ``run`` for a stand-alone launch."""
        takes_ctx, convs, failed = self._plans[name]
        if len(args) != len(convs):
            raise TypeError(f"{name} takes {len(convs)} arguments ({len(args)} given)")
        cargs = [cv(a) for cv, a in zip(convs, args)]
        fn = getattr(lib(), name)
        rc = fn(self.handle, *cargs) if takes_ctx else fn(*cargs)
        if failed(rc):
            raise AfmError(f"{name} failed ({rc}): "
                           f"{lib().afm_last_error().decode(errors='replace')}")
        return rc

    @classmethod
    def get(cls, device: int | None = None) -> "Context":
        import torch
        if not torch.cuda.is_available():
            raise AfmError("no GPU visible: the afm engine runs on MI355X only (no CPU fallback)")
        if device is None:
            device = torch.cuda.current_device()
        ctx = cls._by_device.get(device)
        if ctx is None:
            ctx = cls._by_device[device] = Context(device)
        return ctx

    def set_option(self, name: str, value: int):
        """afm_ctx_set_option: an execution option of this context (include/afm.h)."""
        self.call("afm_ctx_set_option", name.encode(), int(value))

    def get_option(self, name: str) -> int:
        """afm_ctx_get_option: the current value of an execution option."""
        v = I64()
        self.call("afm_ctx_get_option", name.encode(), ctypes.byref(v))
        return int(v.value)

    def bind_stream(self):
        import torch
        s = torch.cuda.current_stream(self.device).cuda_stream
        check(lib().afm_ctx_set_stream(self.handle, P(s)), "afm_ctx_set_stream")
        return self.handle

    @contextlib.contextmanager
    def on(self, stream):
        """``with ctx.on(stream) as h:`` -- the block's launches go to ``stream``: torch's current
        stream and this context are switched together, and on the way out (also when the block
        raises) the context is bound again to the stream that is current once more."""
        import torch
        try:
            with torch.cuda.stream(stream):
                yield self.bind_stream()
        finally:
            self.bind_stream()


def ptr(t) -> P:
    """Device pointer of a contiguous torch tensor."""
    if not t.is_contiguous():
        raise AfmError("tensor must be contiguous")
    return P(t.data_ptr())


def run(name: str, *args, device: int | None = None):
    """A stand-alone launch: ``Context.call`` on the context of ``device`` (default: the device of
    the first tensor among ``args``), bound to torch's current stream of that device."""
    if device is None:
        device = next((a.device.index for a in args if hasattr(a, "data_ptr")), None)
    ctx = Context.get(device)
    ctx.bind_stream()
    return ctx.call(name, *args)


def factor_names() -> list:
    L = lib()
    return [L.afm_factor_name(i).decode() for i in range(98)]


class options:
    """Context manager: execution options of the device's context (afm_ctx_set_option) for the
    duration of a block, restored after it to the values they had before (nesting-safe) -- the
    invariance tests' work splits."""

    DEFAULTS = {"factor_split": 0, "factor_pair": 1, "factor_fast": 1, "gram_checked": 0,
                "gbt_rows_per_wg": 0, "mlp_steps_per_launch": 0, "lstm_rows_per_wg": 0}

    def __init__(self, device: int | None = None, **opts):
        self.device, self.opts = device, opts

    def __enter__(self):
        self.ctx = Context.get(self.device)
        self.saved = {k: self.ctx.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.ctx.set_option(k, v)
        return self.ctx

    def __exit__(self, *exc):
        for k, v in self.saved.items():
            self.ctx.set_option(k, v)
        return False


def cu_mask_stream(device: int, exclude: int):
    """A torch stream on ``device`` whose kernels avoid ``exclude`` compute units (spread evenly
    over the logical CU mask), made by afm_stream_create_cu_mask; the pipeline's FM side stream
    (PipelineConfig.fm_free_cus).  The stream lives as long as the returned object."""
    import torch
    n = torch.cuda.get_device_properties(device).multi_processor_count
    if not 0 < exclude < n:
        raise AfmError(f"exclude must be in 1..{n - 1} compute units")
    keep = [True] * n
    for i in range(exclude):                       # every (n / exclude)-th CU left free
        keep[(i * n) // exclude] = False
    words = (ctypes.c_uint32 * ((n + 31) // 32))()
    for i, k in enumerate(keep):
        if k:
            words[i // 32] |= 1 << (i % 32)
    h = P()
    check(lib().afm_stream_create_cu_mask(device, words, len(words), ctypes.byref(h)),
          "afm_stream_create_cu_mask")
    return _MaskedStream(device, h)


class _MaskedStream:
    def __init__(self, device, handle):
        import torch
        self.handle = handle
        self.stream = torch.cuda.ExternalStream(handle.value, device=torch.device("cuda", device))

    def __del__(self):
        try:
            lib().afm_stream_destroy(self.handle)
        except Exception:
            pass
