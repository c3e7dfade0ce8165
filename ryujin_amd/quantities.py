"""Host-side mirror of ryujin::Quantities (source/quantities.template.h) over ryujin_hip_quantities_*.

The statistics live on the device (HyperbolicModule.quantities_*); this class selects the points as prepare() does and
writes the reference's files. The text formatting is kept in functions that take arrays (format_* below), so that it
can be checked without a device.

A manifold is (name, level_set, options): level_set a callable positions[n, dim] -> values[n] or a number (the
reference's "0."), options a string of the reference's keywords ("instantaneous", "time_averaged", "space_averaged")
or a combination of capi.Q_*. There is no expression parser.
"""
from __future__ import annotations

import numpy as np

from . import capi

_KEYWORDS = (("instantaneous", capi.Q_INSTANTANEOUS), ("time_averaged", capi.Q_TIME_AVERAGED),
             ("space_averaged", capi.Q_SPACE_AVERAGED))


def parse_options(options) -> int:
    """the reference looks for its keywords with std::string::find (:260-261, :512-513)"""
    if isinstance(options, str):
        return sum(flag for word, flag in _KEYWORDS if word in options)
    return int(options)


def _num(x: float) -> str:
    return "%.14e" % x  # std::scientific << std::setprecision(14)


def _vec(v) -> str:
    return " ".join(_num(x) for x in np.atleast_1d(v))  # operator<< of dealii::Tensor<1, n>


def header(equation: int, dim: int) -> str:
    """header_ (:235-245), from the Description's primitive component names"""
    return "primitive state (" + ", ".join(capi.component_names(equation, dim)[1]) + ")\t and 2nd moments\n"


def evaluate_level_set(level_set, positions: np.ndarray) -> np.ndarray:
    positions = np.asarray(positions, dtype=np.float64)
    if callable(level_set):
        return np.asarray(level_set(positions), dtype=np.float64).reshape(len(positions))
    return np.full(len(positions), float(level_set))


def select_interior_points(level_set, positions, row_lengths, n_owned: int) -> np.ndarray:
    """prepare() (:135-183): owned, |f(x_i)| <= 1e-12, row length > 1, ascending local index"""
    f = evaluate_level_set(level_set, positions[:n_owned])
    keep = ~(np.abs(f) > 1.0e-12) & (np.asarray(row_lengths[:n_owned]) != 1)
    return np.flatnonzero(keep).astype(np.uint32)


def select_boundary_entries(level_set, b_i, b_positions, n_owned: int) -> np.ndarray:
    """prepare() (:208-224): entries of the boundary map in their order, owned, |f(x)| < 1e-12"""
    f = evaluate_level_set(level_set, b_positions)
    return np.flatnonzero((np.asarray(b_i) < n_owned) & (np.abs(f) < 1.0e-12))


def format_interior_points(per_rank) -> str:
    """<base>-<name>-R<cycle>-points.dat of an interior map (:275-291); per_rank: [(positions [n, dim], mass [n])]"""
    out = ["#\n# position\tinterior mass\n"]
    for rank, (positions, mass) in enumerate(per_rank):
        out.append(f"# rank {rank}\n")
        out.extend(_vec(x) + "\t" + _num(m) + "\n" for x, m in zip(positions, mass))
    return "".join(out)


def format_boundary_points(per_rank) -> str:
    """... of a boundary map (:317-334); per_rank: [(positions, normals, normal mass, boundary mass)]"""
    out = ["#\n# position\tnormal\tnormal mass\tboundary mass\n"]
    for rank, (positions, normals, normal_mass, boundary_mass) in enumerate(per_rank):
        out.append(f"# rank {rank}\n")
        out.extend(_vec(x) + "\t" + _vec(n) + "\t" + _num(nm) + "\t" + _num(bm) + "\n"
                   for x, n, nm, bm in zip(positions, normals, normal_mass, boundary_mass))
    return "".join(out)


def format_values(time_stamp: str, head: str, per_rank, scale: float = 1.0) -> str:
    """internal_write_out (:445-458); per_rank: [values [n, 2k]] -- (state, state o state) per point"""
    out = [time_stamp, "# ", head]
    for rank, values in enumerate(per_rank):
        values = np.asarray(values, dtype=np.float64)
        k = values.shape[1] // 2 if values.ndim == 2 else 0
        out.append(f"# rank {rank}\n")
        out.extend(_vec(scale * row[:k]) + "\t" + _vec(scale * row[k:]) + "\n" for row in values)
    return "".join(out)


def instantaneous_stamp(t: float) -> str:
    return "# at t = " + _num(t) + "\n"  # (:611)


def time_averaged_stamp(t_begin: float, t_end: float) -> str:
    return "# averaged from t = " + _num(t_begin) + " to t = " + _num(t_end) + "\n"  # (:639-640)


def format_time_series(head: str, rows, append: bool) -> str:
    """internal_write_out_time_series (:470-490); rows [n, 1 + 2k]"""
    out = [] if append else ["# time t\t" + head]
    for row in np.asarray(rows, dtype=np.float64):
        k = (len(row) - 1) // 2
        out.append(_num(row[0]) + "\t" + _vec(row[1:1 + k]) + "\t" + _vec(row[1 + k:]) + "\n")
    return "".join(out)


class Quantities:
    """prepare(name), accumulate(state, t), write_out(state, t, cycle), clear_statistics() as the reference's class.

    gather(obj) -> list of every rank's obj on rank 0 and None elsewhere (Utilities::MPI::gather); the default serves
    one rank. Files are written where gather() returns a list."""

    def __init__(self, module, interior_manifolds=(), boundary_manifolds=(), clear_statistics_on_writeout: bool = True,
                 gather=None):
        self.m = module
        # std::map: the maps are visited in the order of their names
        self.interior_manifolds = sorted(((n, f, parse_options(o)) for n, f, o in interior_manifolds),
                                         key=lambda e: e[0])
        self.boundary_manifolds = sorted(((n, f, parse_options(o)) for n, f, o in boundary_manifolds),
                                         key=lambda e: e[0])
        self.clear_statistics_on_writeout = clear_statistics_on_writeout
        self.gather = gather if gather is not None else (lambda obj: [obj])
        self.base_name = None
        self.maps = []  # (name, options, manifold id, "interior" | "boundary", point data)

    def prepare(self, name: str) -> None:
        m, off = self.m, self.m.offline
        self.base_name = name
        self.time_series_cycle = None
        self.header = header(m.equation, m.dim)
        m.quantities_reset()
        self.maps = []
        n_owned = off.n_owned
        if self.interior_manifolds:
            positions, mass = off.positions, off.mi
            lengths = np.diff(off.row_starts.astype(np.int64))
        for mname, level_set, options in self.interior_manifolds:
            idx = select_interior_points(level_set, positions, lengths, n_owned)
            mid = m.quantities_add_manifold(idx, mass[idx], options)
            self.maps.append((mname, options, mid, "interior", (positions[idx], mass[idx])))
        if self.boundary_manifolds:
            b_i, b_pos, b_normal, b_mass = off.b_i, off.b_positions, off.b_normal, off.b_mass
            # the merged normal's length; not kept by the offline data of this project
            b_normal_mass = getattr(off, "b_normal_mass", np.full(len(b_i), np.nan))
        for mname, level_set, options in self.boundary_manifolds:
            e = select_boundary_entries(level_set, b_i, b_pos, n_owned)
            mid = m.quantities_add_manifold(b_i[e], b_mass[e], options)
            self.maps.append((mname, options, mid, "boundary", (b_pos[e], b_normal[e], b_normal_mass[e], b_mass[e])))
        self.clear_statistics()
        self.mesh_files_have_been_written = False

    def clear_statistics(self) -> None:
        self.m.quantities_clear_statistics()

    def accumulate(self, state, t: float) -> None:
        self.m.quantities_accumulate(state, t)

    def _write(self, path: str, text: str, append: bool = False) -> None:
        with open(path, "a" if append else "w") as f:
            f.write(text)

    def write_mesh_files(self, cycle: int) -> None:
        for mname, options, _, kind, points in self.maps:
            if not options & (capi.Q_INSTANTANEOUS | capi.Q_TIME_AVERAGED):
                continue  # (:260-262)
            received = self.gather(points)
            if received is not None:
                text = format_interior_points(received) if kind == "interior" else format_boundary_points(received)
                self._write(f"{self.base_name}-{mname}-R{cycle:04d}-points.dat", text)

    def write_out(self, state, t: float, cycle: int) -> None:
        if not self.mesh_files_have_been_written:
            self.write_mesh_files(cycle)
            self.mesh_files_have_been_written = True
        for mname, options, mid, _, _ in self.maps:
            prefix = f"{self.base_name}-{mname}-R{cycle:04d}"
            if options & capi.Q_INSTANTANEOUS:
                received = self.gather(self.m.quantities_instantaneous(mid, state, t))
                if received is not None:
                    self._write(prefix + "-instantaneous.dat",
                                format_values(instantaneous_stamp(t), self.header, received))
            if options & capi.Q_TIME_AVERAGED:
                result = self.m.quantities_time_averaged(mid)
                if result is not None:  # (:636; t_sum is the same on every rank)
                    values, t_begin, t_end = result
                    received = self.gather(values)  # (scaled by 1 / t_sum in the library)
                    if received is not None:
                        self._write(prefix + "-time_averaged.dat",
                                    format_values(time_averaged_stamp(t_begin, t_end), self.header, received))
            if options & capi.Q_SPACE_AVERAGED:
                append = self.time_series_cycle is not None
                if not append:
                    self.time_series_cycle = cycle
                rows = self.m.quantities_time_series(mid, clear=True)
                if self.gather(None) is not None:  # rank 0 (every rank holds the same series)
                    self._write(f"{self.base_name}-{mname}-R{self.time_series_cycle:04d}-space_averaged_time_series.dat",
                                format_time_series(self.header, rows, append), append)
        if self.clear_statistics_on_writeout:
            self.clear_statistics()
