"""numpy restatement of Quantities::accumulate / write_out (source/quantities.template.h), the yardstick of
tests/test_gpu_quantities.py; itself pinned in tests/test_quantities_cpu.py by the reference's own
tests/golden/euler_check-mass-conservation_01.output and by the exactness of the trapezoid rule.

Written from the formulas. A manifold is (index [n], weight [n]). The value of a point is (V, V o V),
V = to_primitive_state(U_i) (helpers_postprocessor.primitive_state). Per accumulate(U, t):
    swap(t_old, t_new);  new = values of U
    if t_old == 0 and t_new == 0:   t_old = t - 1;  t_new = t                      (first call: nothing is added)
    else:  t_new = t;  tau = t_new - t_old;  sum += 0.5 tau old;  sum += 0.5 tau new  (in this order);  t_sum += tau
    series.append((t, sum_p w_p x_p / sum_p w_p))
The means are formed with math.fsum (exactly rounded sums of the rounded products), so that the yardstick carries no
summation error of its own. time_averaged = sum * (1 / t_sum), from t_new - t_sum to t_new.

Tolerances (derived, not tuned). FUNCTION_LEVEL = 1e-13 is the project's function-level figure
(tests/helpers_postprocessor.py): a primitive state is a few operations on U.
  * a point, component c:            FUNCTION_LEVEL |V_c|;  second moment: 2 FUNCTION_LEVEL V_c^2  (d(V^2) = 2 V dV)
  * a mean over n points:            (FUNCTION_LEVEL + D eps) S_c,  S_c = sum w |x_c| / sum w.
    Every term carries its point's error (FUNCTION_LEVEL |x_c|) and then
    passes through a chain of D floating-point additions of the device's FIXED reduction, each of which adds at most
    eps times the magnitude of the partial sum, itself bounded by the sum of the magnitudes. D is computed from the
    launch shape kernels_quantities.hpp documents (chain_length()): the terms a lane adds, 6 shuffle levels, the waves
    of a block, the block partials a lane of the final wave adds, 6 shuffle levels, the ranks. The mean is judged
    against S_c and not against itself: the mean v_2 ~ 1e-18 of the golden run is a cancellation of terms ~ 1e-3.
  * a time-averaged value after N accumulations:  (FUNCTION_LEVEL + 2 N eps) max over the history of |x_c| (twice that
    for a second moment): a weighted mean of the history (the weights 0.5 tau / t_sum sum to 1), 2 additions per call
    in the reference's order; 2 N eps covers their roundings and those of the products."""
from __future__ import annotations

import math

import numpy as np

import helpers_postprocessor as hp
from ryujin_amd import capi

EPS = hp.EPS
FUNCTION_LEVEL = hp.FUNCTION_LEVEL

# launch shape of k_quantities_sweep / k_quantities_final (ryujin_amd/csrc/kernels_quantities.hpp)
BLOCK, WAVE, MAX_BLOCKS = 256, 64, 1024


def chain_length(points_per_rank) -> int:
    """D: the longest chain of additions a term passes through; points_per_rank: the manifold's points on every rank"""
    longest = 0
    for n in points_per_rank:
        if n == 0:
            continue
        blocks = min(MAX_BLOCKS, -(-n // BLOCK))
        per_lane = -(-n // (blocks * BLOCK))
        longest = max(longest, per_lane + 6 + BLOCK // WAVE + -(-blocks // WAVE) + 6)
    return longest + len(points_per_rank)


def point_values(equation, dim, params, U, index) -> np.ndarray:
    """[n, 2k]: (V, V o V) of the points"""
    V = hp.primitive_state(equation, dim, np.asarray(U, dtype=np.float64)[np.asarray(index, dtype=np.int64)], params)
    return np.concatenate([V, V * V], axis=1)


def point_tolerance(values: np.ndarray) -> np.ndarray:
    k = values.shape[1] // 2
    return np.concatenate([FUNCTION_LEVEL * np.abs(values[:, :k]), 2.0 * FUNCTION_LEVEL * values[:, k:]], axis=1)


def weighted_mean(weight, values) -> np.ndarray:
    """sum_p w_p x_p / sum_p w_p per column, NaN (0/0) without points as in the reference"""
    weight = np.asarray(weight, dtype=np.float64)
    mass = math.fsum(weight)
    if mass == 0.0:
        return np.full(values.shape[1], np.nan)
    return np.array([math.fsum(weight * values[:, c]) / mass for c in range(values.shape[1])])


def mean_tolerance(weight, values, D: int) -> np.ndarray:
    return (FUNCTION_LEVEL + D * EPS) * weighted_mean(weight, np.abs(values))


class Statistics:
    """val_old, val_new, val_sum, t_old, t_new, t_sum and the time series of ONE manifold (:516-549)"""

    def __init__(self, equation, dim, params, index, weight):
        self.equation, self.dim, self.params = equation, dim, params
        self.index = np.asarray(index, dtype=np.int64)
        self.weight = np.asarray(weight, dtype=np.float64)
        self.width = 2 * len(capi.component_names(equation, dim)[1])
        self.clear()

    def clear(self):
        n = len(self.index)
        self.val_old = np.zeros((n, self.width))
        self.val_new = np.zeros((n, self.width))
        self.val_sum = np.zeros((n, self.width))
        self.t_old = self.t_new = self.t_sum = 0.0
        self.series = []
        self.history_max = np.zeros((n, self.width))  # per point, max over the history of |x_c|
        self.n_accumulations = 0

    def values(self, U):
        return point_values(self.equation, self.dim, self.params, U, self.index)

    def accumulate(self, U, t: float):
        self.t_old, self.t_new = self.t_new, self.t_old
        self.val_old, self.val_new = self.val_new, self.val_old
        self.val_new = self.values(U)
        if self.t_old == 0.0 and self.t_new == 0.0:
            self.t_old = t - 1.0
            self.t_new = t
        else:
            self.t_new = t
            tau = self.t_new - self.t_old
            self.val_sum = self.val_sum + 0.5 * tau * self.val_old
            self.val_sum = self.val_sum + 0.5 * tau * self.val_new
            self.t_sum += tau
        self.n_accumulations += 1
        self.history_max = np.maximum(self.history_max, np.abs(self.val_new))
        self.series.append(np.concatenate([[t], weighted_mean(self.weight, self.val_new)]))

    def time_averaged(self):
        """(values, t_begin, t_end) or None while t_sum == 0 (:636-643)"""
        if self.t_sum == 0.0:
            return None
        return self.val_sum * (1.0 / self.t_sum), self.t_new - self.t_sum, self.t_new

    def time_averaged_tolerance(self) -> np.ndarray:
        k = self.width // 2
        factor = np.concatenate([np.ones(k), 2.0 * np.ones(k)])
        return factor * (FUNCTION_LEVEL + 2.0 * self.n_accumulations * EPS) * self.history_max

    def series_array(self) -> np.ndarray:
        return np.array(self.series).reshape(len(self.series), 1 + self.width)
