"""VTUOutput of the reference (source/vtu_output.template.h) on top of the device-resident extraction
(ryujin_hip_output_*): the values of "vtu output quantities" are formed and gathered on the device -- at all locally
relevant nodes, or at the nodes of the cells a level set of "manifolds" cuts -- and this module writes them as VTK XML
UnstructuredGrid files, the form of DataOut::write_vtu_with_pvtu_record: one .vtu piece per rank and, on several
ranks, a .pvtu record naming the pieces (the MPI-IO single-file form has no counterpart). deal.II is not available to
this project, so there is no reference file to compare with: the contract is the VTK XML format itself -- Float32 point
data and points, Int32 connectivity and offsets, UInt8 types, binary arrays as base64 of a zlib stream behind the
block header of vtkZLibDataCompressor, and the fields TIME and CYCLE of DataOutBase::VtkFlags(t, cycle). Standard
library and numpy only."""
from __future__ import annotations

import base64
import math
import os
import struct
import zlib

import numpy as np

from . import capi

# VTK cell types and the lexicographic -> VTK vertex order of a cell (deal.II numbers the vertices of a cell
# lexicographically, x fastest; VTK walks a quadrilateral and each face of a hexahedron counter-clockwise)
VTK_LINE, VTK_QUAD, VTK_HEXAHEDRON = 3, 9, 12
VTK_CELL = {1: (VTK_LINE, (0, 1)), 2: (VTK_QUAD, (0, 1, 3, 2)), 3: (VTK_HEXAHEDRON, (0, 1, 3, 2, 4, 5, 7, 6))}


def file_names(name: str, cycle: int, rank: int = 0, n_ranks: int = 1, levelsets: bool = False):
    """(piece, record): name_000123.vtu on one rank; name_000123.<rank>.vtu and name_000123.pvtu on several
    (write_vtu_with_pvtu_record("", name, cycle, comm, 6)); the level-set output as name-levelsets_000123..."""
    base = f"{name}{'-levelsets' if levelsets else ''}_{int(cycle):06d}"
    if n_ranks <= 1:
        return base + ".vtu", None
    digits = max(1, int(math.ceil(math.log10(n_ranks))))
    return f"{base}.{int(rank):0{digits}d}.vtu", base + ".pvtu"


def encode_array(a: np.ndarray) -> str:
    """A binary DataArray body: base64 of the header (number of blocks, block size, size of the last block, compressed
    size of every block; UInt32) followed by base64 of the zlib stream -- one block; an empty array is no block."""
    raw = np.ascontiguousarray(a).astype(a.dtype.newbyteorder("<"), copy=False).tobytes()
    if not raw:
        return base64.b64encode(struct.pack("<3I", 0, 0, 0)).decode()
    packed = zlib.compress(raw, 1)  # DataOutBase::CompressionLevel::best_speed
    header = struct.pack("<4I", 1, len(raw), len(raw), len(packed))
    return base64.b64encode(header).decode() + base64.b64encode(packed).decode()


_VTK_TYPE = {np.dtype(np.float32): "Float32", np.dtype(np.float64): "Float64", np.dtype(np.int32): "Int32",
             np.dtype(np.uint8): "UInt8"}


def _data_array(a: np.ndarray, name: str | None = None, components: int | None = None) -> str:
    attributes = f'type="{_VTK_TYPE[a.dtype]}"'
    if name is not None:
        attributes += f' Name="{name}"'
    if components is not None:
        attributes += f' NumberOfComponents="{components}"'
    return f'<DataArray {attributes} format="binary">\n{encode_array(a)}\n</DataArray>\n'


def write_vtu(path: str, points, cells, point_data: dict, t: float | None = None, cycle: int | None = None) -> None:
    """One piece: points [n, dim], cells [n_cells, 2^dim] of LEXICOGRAPHICALLY ordered vertices (indices into points),
    point_data name -> [n] values (stored as Float32). Zero cells and zero points are a valid file."""
    points = np.asarray(points, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] not in VTK_CELL:
        raise ValueError("points is [n, dim], dim = 1, 2 or 3")
    dim = points.shape[1]
    vtk_type, order = VTK_CELL[dim]
    cells = np.asarray(cells, dtype=np.int64).reshape(-1, 2 ** dim)
    n_points, n_cells = len(points), len(cells)
    xyz = np.zeros((n_points, 3), dtype=np.float32)
    xyz[:, :dim] = points
    connectivity = cells[:, list(order)].astype(np.int32).reshape(-1)
    offsets = (np.arange(1, n_cells + 1, dtype=np.int64) * 2 ** dim).astype(np.int32)
    types = np.full(n_cells, vtk_type, dtype=np.uint8)
    out = ['<?xml version="1.0" ?>\n',
           '<VTKFile type="UnstructuredGrid" version="0.1" compressor="vtkZLibDataCompressor" '
           'byte_order="LittleEndian">\n', '<UnstructuredGrid>\n']
    if t is not None or cycle is not None:
        out.append("<FieldData>\n")
        if cycle is not None:
            out.append(f'<DataArray type="Float32" Name="CYCLE" NumberOfTuples="1" format="ascii">{int(cycle)}'
                       '</DataArray>\n')
        if t is not None:
            out.append(f'<DataArray type="Float32" Name="TIME" NumberOfTuples="1" format="ascii">{float(t)!r}'
                       '</DataArray>\n')
        out.append("</FieldData>\n")
    out.append(f'<Piece NumberOfPoints="{n_points}" NumberOfCells="{n_cells}">\n')
    out.append("<Points>\n" + _data_array(xyz, components=3) + "</Points>\n")
    out.append("<Cells>\n" + _data_array(connectivity, "connectivity") + _data_array(offsets, "offsets") +
               _data_array(types, "types") + "</Cells>\n")
    out.append('<PointData Scalars="scalars">\n')
    for name, values in point_data.items():
        values = np.asarray(values, dtype=np.float32).reshape(-1)
        if values.size != n_points:
            raise ValueError(f"\"{name}\" holds {values.size} values for {n_points} points")
        out.append(_data_array(values, name))
    out.append("</PointData>\n</Piece>\n</UnstructuredGrid>\n</VTKFile>\n")
    with open(path, "w") as f:
        f.write("".join(out))


def write_pvtu(path: str, pieces, names) -> None:
    """The record of DataOutInterface::write_pvtu_record: the point data names and every piece's file name"""
    out = ['<?xml version="1.0" ?>\n', '<VTKFile type="PUnstructuredGrid" version="0.1" byte_order="LittleEndian">\n',
           '<PUnstructuredGrid GhostLevel="0">\n', '<PPointData Scalars="scalars">\n']
    out += [f'<PDataArray type="Float32" Name="{name}" format="ascii"/>\n' for name in names]
    out += ["</PPointData>\n", '<PPoints>\n<PDataArray type="Float32" NumberOfComponents="3"/>\n</PPoints>\n']
    out += [f'<Piece Source="{os.path.basename(piece)}"/>\n' for piece in pieces]
    out += ["</PUnstructuredGrid>\n", "</VTKFile>\n"]
    with open(path, "w") as f:
        f.write("".join(out))


class VTUOutput:
    """VTUOutput<Description, dim, Number> (source/vtu_output.h): quantities = "vtu output quantities" (default, as
    the reference's: the conserved and the initial-precomputed names, vtu_output.template.h:52-58), manifolds =
    "manifolds". The postprocessed fields the module holds a configuration for may be named too ("schlieren_rho");
    the caller runs postprocess_compute before the output. rank / n_ranks name the piece of a partitioned run."""

    def __init__(self, module, quantities=None, manifolds=(), cells=None, directory: str = ".", rank: int = 0,
                 n_ranks: int = 1):
        self.m = module
        if quantities is None:
            tables = capi.output_names(module.equation, module.dim)
            quantities = (*tables["conserved"], *tables["initial_precomputed"])
        self.quantities = list(quantities)
        self.manifolds = [manifolds] if isinstance(manifolds, str) else list(manifolds)
        self.cells = np.ascontiguousarray(module.offline.cells if cells is None else cells,
                                          dtype=np.uint32).reshape(-1, 2 ** module.dim)
        self.directory, self.rank, self.n_ranks = directory, rank, n_ranks
        self.positions = np.ascontiguousarray(module.offline.positions, dtype=np.float64).reshape(-1, module.dim)
        self.prepare()

    def prepare(self) -> None:
        """SelectedComponentsExtractor::check and the level-set selection, once (ryujin_hip_output_configure)"""
        self.m.output_configure(self.quantities, self.cells, self.manifolds, self.positions)
        self.cell_ids, self.node_ids, self.connectivity = self.m.output_selection()

    def _write(self, name, cycle, t, levelsets, points, cells, values):
        piece, record = file_names(name, cycle, self.rank, self.n_ranks, levelsets)
        written = [os.path.join(self.directory, piece)]
        write_vtu(written[0], points, cells, dict(zip(self.quantities, values)), t, cycle)
        if record is not None and self.rank == 0:
            pieces = [file_names(name, cycle, r, self.n_ranks, levelsets)[0] for r in range(self.n_ranks)]
            written.append(os.path.join(self.directory, record))
            write_pvtu(written[1], pieces, self.quantities)
        return written

    def schedule_output(self, state, name: str, t: float, cycle: int, output_full: bool = True,
                        output_levelsets: bool = False) -> list:
        """schedule_output (vtu_output.template.h:80-205): name_<cycle>.vtu with every locally relevant node and
        every cell of this rank, name-levelsets_<cycle>.vtu with the selected cells and their nodes (only with
        manifolds, :156). Collective over the ranks. Returns the paths written."""
        written = []
        if output_full:
            values = self.m.output_extract(state, levelsets=False, precision="float32")
            written += self._write(name, cycle, t, False, self.positions, self.cells, values)
        if output_levelsets and self.manifolds:
            values = self.m.output_extract(state, levelsets=True, precision="float32")
            written += self._write(name, cycle, t, True, self.positions[self.node_ids], self.connectivity, values)
        return written
