"""afm -- MI355X-native engine for the factor-research hot path of
Yuliang-Eliott/Alpha-Multi-factor-models.

Drop-in Python surface (same names, arguments and results as the reference):

* ``compute_factors(data)``                      -- No-talib.py:1-93
* ``AlphaSignalAnalyzer(df, name, prices).run()`` -- KKT Yuliang Jiang.py:280-375
* ``LinearRegression().fit/predict``              -- KKT:582-598 (pooled OLS)
* ``Lasso(alpha, max_iter).fit/predict``           -- KKT:605-607 (coordinate descent)
* ``lasso_path(X, y)`` / ``LassoCV(cv).fit``       -- scikit-learn's path and CV alpha selection
                                                    (the choice of alpha KKT:605 hard-codes)
* ``FactorScreen(df, prices).run()``               -- KKT:465, 472 for every column at once
                                                    (per-date IC, per-year IR, summary)
* ``preprocess_factors(df, groups=..., prep=XsPrep(...))`` -- the per-date winsorise / sector-
                                                    neutralise / standardise of every column
                                                    (``groupby('date').transform``)
* ``combine_factors(df, prices, weights=ICWeights(...))`` -- the rolling IC-weighted composite
                                                    of the columns (``rolling`` over the ICs)
* ``factor_turnover(df, prices, lags=(1, 5, 21))``  -- the rank autocorrelation and the layer /
                                                    top-10 turnover of every column
* ``GBTRegressor(**params).fit/predict``           -- KKT:481-576 (XGBoost: boosted regression
                                                    trees, bit-reproducible histograms);
                                                    ``predict(X, pred_contribs=True)``: the exact
                                                    TreeSHAP contributions, the bias last
* ``PortfolioManager(...)``                       -- KKT:795-970
* ``RiskParams`` / ``RiskModel`` (``Pipeline.risk_fit``) -- the multi-factor risk model behind the
                                                    reference's sample covariance (KKT:858-859):
                                                    EWMA factor and specific risk, book risk,
                                                    weights from B F B' + D
* ``split_zscore(all_df)``                       -- KKT:424-458 (z-score + split)

All compute runs in hand-written HIP kernels (libafm.so, C-ABI in include/afm.h); there is no
CPU fallback.
"""
from .factors import FACTOR_NAMES, compute_factors, factor_panel  # noqa: F401
from .grid import PanelGrid, pack_bits, unpack_bits  # noqa: F401
from . import regression  # noqa: F401
from .regression import (Lasso, LassoCV, LinearRegression, cross_sectional_ols,  # noqa: F401
                         lasso_path)
from .analyzer import AlphaSignalAnalyzer  # noqa: F401
from .screen import FactorScreen, screen_grid, select_factors  # noqa: F401
from .xsprep import XsPrep, preprocess_factors, preprocess_grid  # noqa: F401
from .combine import ICWeights, combine_factors, combine_grid, ic_weights  # noqa: F401
from .turnover import Turnover, factor_turnover, turnover_grid  # noqa: F401
from .gbt import GBTModel, GBTParams, GBTRegressor  # noqa: F401
from .mlp import MLPModel, MLPParams, MLPRegressor  # noqa: F401
from .lstm import LSTMModel, LSTMParams, LSTMRegressor  # noqa: F401
from .portfolio import PortfolioManager, mean_variance_weights  # noqa: F401
from .risk import RiskModel, RiskParams, bias_statistic, cov_weights  # noqa: F401
from .zscore import split_zscore, zscore_grid  # noqa: F401

__all__ = ["compute_factors", "factor_panel", "FACTOR_NAMES", "PanelGrid", "pack_bits",
           "unpack_bits", "LinearRegression", "Lasso", "LassoCV", "lasso_path",
           "cross_sectional_ols", "AlphaSignalAnalyzer", "FactorScreen", "screen_grid",
           "select_factors", "PortfolioManager", "split_zscore", "zscore_grid", "XsPrep",
           "preprocess_factors", "preprocess_grid", "ICWeights", "ic_weights", "combine_grid",
           "combine_factors", "Turnover", "turnover_grid", "factor_turnover", "GBTParams",
           "GBTModel", "GBTRegressor", "MLPParams", "MLPModel", "MLPRegressor", "RiskParams",
           "RiskModel", "bias_statistic", "cov_weights", "LSTMParams", "LSTMModel",
           "LSTMRegressor"]
