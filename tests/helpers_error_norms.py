"""numpy restatement of the norms of TimeLoop::compute_error() (source/time_loop.template.h:692-833) as
ryujin_hip_error_norms_compute defines them (include/ryujin_hip.h), the yardstick of tests/test_gpu_error_norms.py.

Written from the formulas, over the same tables the device is given: cells [n_cells, dofs_per_cell], shape
[n_q, dofs_per_cell], JxW [n_cells, n_q] (in the per-cell form the products weights[q] * measure[cell], the one
rounding the device makes too). Per component, with x = e = U - A or x = A:
    Linf = max_i |x_i| over the owned rows                (the same IEEE subtraction as the device: equal bit for bit)
    x_q  = sum_v N_qv x_v                                  (float64 einsum)
    L1   = fsum_{cells, q} |x_q| JxW_q,   L2 = sqrt(fsum_{cells, q} x_q^2 JxW_q)
math.fsum returns the exactly rounded sum of the rounded terms: the yardstick carries no summation error of its own.
The consolidated numbers are formed as the reference forms them (:797-805), with numpy's division: x / 0 = inf,
0 / 0 = NaN.

Tolerances (derived, not tuned). With X_q = sum_v |N_qv| |x_v| >= |x_q|, the terms are bounded by T1 = X_q JxW_q and
T2 = X_q^2 JxW_q. A sum of dofs_per_cell products carries at most dofs_per_cell eps X_q whatever the order (device:
left to right; einsum: its own), so
  * a term |x_q| JxW_q is off by at most (dofs_per_cell + HANDFUL) eps T1 on either side -- HANDFUL = 4 covers the
    products with JxW_q, weights[q] * measure and the final rounding of the term --,
  * a term x_q^2 JxW_q by at most (2 dofs_per_cell + HANDFUL) eps T2 (d(x^2) = 2 |x| dx),
  * and on the device every term then passes through a chain of D additions of the FIXED reduction, each of which adds
    at most eps times the magnitude of the partial sum, itself bounded by the sum of the magnitudes. D comes from the
    launch shape kernels_error_norms.hpp documents (chain_length()): the n_q terms of a cell, the cells a lane adds, 6
    shuffle levels, the waves of a block, the block partials a lane of the final wave adds, 6 shuffle levels, the ranks.
Both sides together: |device - yardstick| <= (D + 2 (2 dofs_per_cell + HANDFUL)) eps sum T for either integral (the
L1 factor is taken as large as the L2 one: one formula). A root: |sqrt a - sqrt b| = |a - b| / (sqrt a + sqrt b)
<= |a - b| / sqrt b, plus eps sqrt b for the roundings of the two roots. A ratio E / A: tol_E / A + E tol_A / A^2 + eps
E / A, and their sum over n components n eps sum more."""
from __future__ import annotations

import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)
HANDFUL = 4

# launch shape of k_error_norms_cells / k_error_norms_final (ryujin_amd/csrc/kernels_error_norms.hpp)
BLOCK, WAVE, MAX_BLOCKS = 256, 64, 1024


def chain_length(cells_per_rank, n_q: int) -> int:
    """D: the longest chain of additions a term passes through; cells_per_rank: the number of cells of every rank"""
    longest = 0
    for n in cells_per_rank:
        if n == 0:
            continue
        blocks = min(MAX_BLOCKS, -(-n // BLOCK))
        per_lane = -(-n // (blocks * BLOCK))
        longest = max(longest, n_q + per_lane + 6 + BLOCK // WAVE + -(-blocks // WAVE) + 6)
    return longest + len(cells_per_rank)


def full_jxw(jxw, weights, n_q):
    """[n_cells, n_q]: JxW as the device uses it, from either form"""
    jxw = np.asarray(jxw, dtype=np.float64)
    if jxw.ndim == 1:
        return np.asarray(weights, dtype=np.float64)[None, :] * jxw[:, None]
    return jxw.reshape(-1, n_q)


def integrals(x, cells, shape, jxw):
    """(L1, L2^2, sum T1, sum T2) of the nodal values x [n] over the cells"""
    xv = np.asarray(x, dtype=np.float64)[np.asarray(cells, dtype=np.int64)]          # [cells, v]
    xq = np.einsum("qv,cv->cq", shape, xv)
    Xq = np.einsum("qv,cv->cq", np.abs(shape), np.abs(xv))
    return (math.fsum((np.abs(xq) * jxw).ravel()), math.fsum((xq * xq * jxw).ravel()),
            math.fsum((Xq * jxw).ravel()), math.fsum((Xq * Xq * jxw).ravel()))


def restatement(U, A, n_owned, cells, shape, jxw, components, normalize, weights=None, D=0):
    """U, A [n, k]; the cells of ALL ranks in one list (indices into U and A). Returns a dict:
    out [3], detail [n_components, 6], tol_detail [n_components, 6] (0 for the Linf columns), tol_out [3]."""
    shape = np.asarray(shape, dtype=np.float64)
    n_q, dpc = shape.shape
    jxw = full_jxw(jxw, weights, n_q)
    factor = (D + 2 * (2 * dpc + HANDFUL)) * EPS
    detail = np.zeros((len(components), 6))
    tol = np.zeros((len(components), 6))
    for row, c in enumerate(components):
        a = np.asarray(A, dtype=np.float64)[:, c]
        e = np.asarray(U, dtype=np.float64)[:, c] - a
        for offset, x in ((0, e), (3, a)):
            l1, s2, t1, t2 = integrals(x, cells, shape, jxw)
            l2 = math.sqrt(s2)
            detail[row, offset:offset + 3] = (np.abs(x[:n_owned]).max(), l1, l2)
            tol[row, offset + 1] = factor * t1
            tol[row, offset + 2] = (factor * t2 / l2 + EPS * l2) if l2 > 0.0 else 0.0
    out = np.zeros(3)
    tol_out = np.zeros(3)
    with np.errstate(divide="ignore", invalid="ignore"):
        for q in range(3):
            total, magnitude, t = 0.0, 0.0, 0.0
            for row in range(len(components)):
                E, An = detail[row, q], detail[row, 3 + q]
                tE, tA = tol[row, q], tol[row, 3 + q]
                if normalize:
                    r = np.float64(E) / np.float64(An)
                    t += (tE / An + E * tA / (An * An) + EPS * r) if An > 0.0 else 0.0
                else:
                    r, t = E, t + tE
                total = total + r
                magnitude += abs(r)
            out[q] = total
            tol_out[q] = t + len(components) * EPS * magnitude if q > 0 and np.isfinite(magnitude) else 0.0
    return dict(out=out, detail=detail, tol_detail=tol, tol_out=tol_out)


def compare(label, got_out, got_detail, ref):
    """Linf columns equal bit for bit, every integral within its derived bound; prints each figure first"""
    detail, tol = ref["detail"], ref["tol_detail"]
    got_detail = np.asarray(got_detail)
    assert got_detail.shape == detail.shape, (label, got_detail.shape, detail.shape)
    for col, name in enumerate(("Linf e", "L1 e", "L2 e", "Linf A", "L1 A", "L2 A")):
        err = np.abs(got_detail[:, col] - detail[:, col])
        if col % 3 == 0:
            print(f"{label} {name}: device {got_detail[:, col]}, yardstick {detail[:, col]}")
        else:
            print(f"{label} {name}: max err / tol {(err / np.maximum(tol[:, col], 1e-300)).max():.3e}")
    for col in (0, 3):
        assert np.array_equal(got_detail[:, col], detail[:, col]), (label, "Linf", col, got_detail[:, col],
                                                                    detail[:, col])
    for col in (1, 2, 4, 5):
        err = np.abs(got_detail[:, col] - detail[:, col])
        assert np.isfinite(got_detail[:, col]).all() and (err <= tol[:, col]).all(), (label, col, err, tol[:, col])
    out = np.asarray(got_out)
    print(f"{label} consolidated: device {out}, yardstick {ref['out']}, tol {ref['tol_out']}")
    if np.isfinite(ref["out"]).all():
        assert out[0] == ref["out"][0], (label, "consolidated Linf", out[0], ref["out"][0])
        assert (np.abs(out[1:] - ref["out"][1:]) <= ref["tol_out"][1:]).all(), (label, out, ref["out"], ref["tol_out"])
    else:
        assert np.array_equal(out, ref["out"], equal_nan=True), (label, out, ref["out"])


def lexicographic_quads(quads):
    """counter-clockwise quadrilaterals (tests/helpers_q1_quads.annulus_mesh) -> vertices v = ix + 2 iy"""
    return np.asarray(quads)[:, [0, 1, 3, 2]]


def nodal_scatter(n, cells, shape, jxw):
    """m_i = sum_cells sum_q JxW_q N_qv scattered to the nodes: the lumped mass of the cell list"""
    m = np.zeros(n)
    np.add.at(m, np.asarray(cells, dtype=np.int64), np.einsum("cq,qv->cv", jxw, shape))
    return m


def random_vectors(n, k, seed, positive=True):
    """a random state and a random "analytic" vector, every component bounded away from zero"""
    rng = np.random.default_rng(seed)
    A = rng.uniform(0.5, 2.0, size=(n, k)) * (1.0 if positive else rng.choice([-1.0, 1.0], size=(1, k)))
    U = A * (1.0 + rng.uniform(-0.1, 0.1, size=(n, k)))
    return U, A
