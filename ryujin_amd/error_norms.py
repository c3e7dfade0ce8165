"""Host-side parts of the device-resident TimeLoop::compute_error() (ryujin_hip_error_norms_*,
source/time_loop.template.h:692-833): the Q1 tables of QGauss<dim>(3) that the reference integrates with, JxW of
multilinear cells, and the writer of the reference's log block."""
from __future__ import annotations

import numpy as np


def gauss3():
    """points and weights of QGauss<1>(3) on [0, 1]"""
    x = np.array([-np.sqrt(3.0 / 5.0), 0.0, np.sqrt(3.0 / 5.0)]) * 0.5 + 0.5
    return x, np.array([5.0, 8.0, 5.0]) / 18.0


def _q1_reference(dim: int):
    """(points [n_q, dim], weights [n_q], bits [2^dim, dim]): the tensorised QGauss(3), x running fastest as in
    deal.II, and the corner (ix, iy, iz) of vertex v = ix + 2 iy + 4 iz"""
    if dim not in (1, 2, 3):
        raise ValueError(f"dim = {dim}")
    x, w = gauss3()
    grids = np.meshgrid(*([np.arange(3)] * dim), indexing="ij")
    idx = np.stack([g.T.reshape(-1) for g in grids], axis=1)  # x fastest
    points = x[idx]
    weights = np.prod(w[idx], axis=1)
    bits = np.array([[(v >> d) & 1 for d in range(dim)] for v in range(1 << dim)])
    return points, weights, bits


def q1_tables(dim: int):
    """(shape [3^dim, 2^dim], weights [3^dim]): phi_v(x_q) of the multilinear shape functions, vertices in deal.II's
    lexicographic order v = ix + 2 iy + 4 iz, at the points of QGauss<dim>(3) on the unit cell, and their weights"""
    points, weights, bits = _q1_reference(dim)
    factors = np.where(bits[None, :, :] == 1, points[:, None, :], 1.0 - points[:, None, :])  # [q, v, d]
    return np.ascontiguousarray(np.prod(factors, axis=2)), weights


def q1_jxw(positions, cells):
    """[n_cells, 3^dim]: |det J(x_q)| w_q of the multilinear map of every cell (cells [n_cells, 2^dim] indices into
    positions [n, dim], lexicographic vertices), 1-D to 3-D -- FEValues::JxW with MappingQ1 and QGauss<dim>(3)"""
    x = np.asarray(positions, dtype=np.float64)
    dim = x.shape[1]
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 1 << dim)
    points, weights, bits = _q1_reference(dim)
    factors = np.where(bits[None, :, :] == 1, points[:, None, :], 1.0 - points[:, None, :])  # [q, v, d]
    sign = np.where(bits == 1, 1.0, -1.0)                                                       # d phi_v / d x_d factor
    grad = np.empty((len(points), 1 << dim, dim))
    for d in range(dim):
        others = np.prod(np.delete(factors, d, axis=2), axis=2) if dim > 1 else np.ones(factors.shape[:2])
        grad[:, :, d] = sign[None, :, d] * others
    J = np.einsum("cva,qvb->cqab", x[cells], grad)  # J[a, b] = d x_a / d xi_b
    return np.abs(np.linalg.det(J)) * weights[None, :]


def format_error_block(n_dofs: int, t: float, linf: float, l1: float, l2: float, normalize: bool = True) -> str:
    """the block TimeLoop::compute_error() writes to the log file (:811-823), 16 significant digits"""
    description = "Normalized consolidated" if normalize else "Consolidated"
    g = lambda v: f"{v:.16g}"  # noqa: E731  (std::setprecision(16), default float format)
    return ("\nComputed errors:\n\n"
            f"{description} Linf, L1, and L2 errors at final time \n"
            f"#dofs = {int(n_dofs)}\n"
            f"t     = {g(t)}\n"
            f"Linf  = {g(linf)}\n"
            f"L1    = {g(l1)}\n"
            f"L2    = {g(l2)}\n")


def write_error_block(path: str, n_dofs: int, t: float, linf: float, l1: float, l2: float,
                      normalize: bool = True) -> None:
    with open(path, "a") as f:
        f.write(format_error_block(n_dofs, t, linf, l1, l2, normalize))
