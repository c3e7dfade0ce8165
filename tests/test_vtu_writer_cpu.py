"""The VTK XML writer of ryujin_amd/vtu_output.py on the CPU. There is no reference file to compare with (deal.II is
not available): the contract is the format itself, so the files are read back here with xml.etree and a decoder of the
binary arrays written independently of the writer (base64 -> block header -> zlib)."""
import base64
import os
import struct
import xml.etree.ElementTree as ET
import zlib

import numpy as np
import pytest

from ryujin_amd import vtu_output as vo

DTYPES = {"Float32": "<f4", "Float64": "<f8", "Int32": "<i4", "UInt8": "u1"}


def decode(element):
    """A binary DataArray of a file with compressor="vtkZLibDataCompressor" and UInt32 headers: base64 of
    (n_blocks, block_size, last_block_size, compressed sizes ...), then base64 of the concatenated zlib streams"""
    assert element.get("format") == "binary"
    text = "".join(element.text.split())
    n_blocks = struct.unpack("<I", base64.b64decode(text[:8])[:4])[0]
    header_bytes = 4 * (3 + n_blocks)
    header_chars = 4 * ((header_bytes + 2) // 3)
    header = struct.unpack(f"<{3 + n_blocks}I", base64.b64decode(text[:header_chars])[:header_bytes])
    raw = b""
    if n_blocks:
        body = base64.b64decode(text[header_chars:])
        at = 0
        for size in header[3:]:
            raw += zlib.decompress(body[at:at + size])
            at += size
        assert at == len(body)
        assert len(raw) == header[1] * (n_blocks - 1) + header[2]
    return np.frombuffer(raw, dtype=DTYPES[element.get("type")])


def read(path):
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.get("type") == "UnstructuredGrid"
    assert root.get("byte_order") == "LittleEndian" and root.get("compressor") == "vtkZLibDataCompressor"
    piece = root.find("UnstructuredGrid/Piece")
    out = dict(n_points=int(piece.get("NumberOfPoints")), n_cells=int(piece.get("NumberOfCells")))
    points = piece.find("Points/DataArray")
    assert points.get("NumberOfComponents") == "3" and points.get("type") == "Float32"
    out["points"] = decode(points).reshape(-1, 3)
    for a in piece.findall("Cells/DataArray"):
        out[a.get("Name")] = decode(a)
    out["point_data"] = {a.get("Name"): decode(a) for a in piece.findall("PointData/DataArray")}
    out["types_of"] = {a.get("Name"): a.get("type") for a in piece.findall("PointData/DataArray")}
    out["field"] = {a.get("Name"): a.text for a in root.findall("UnstructuredGrid/FieldData/DataArray")}
    return out


def lattice(dim, n):
    """points of an (n + 1)^dim lattice, x fastest, stretched per direction; cells with lexicographic vertices"""
    axes = [np.linspace(0.0, 1.0 + 0.5 * d, n + 1) for d in range(dim)]
    grid = np.meshgrid(*axes, indexing="ij")
    points = np.stack([g.reshape(-1, order="F") for g in grid], axis=1)
    stride = [(n + 1) ** d for d in range(dim)]
    cells = []
    for c in np.ndindex(*([n] * dim)):
        c = c[::-1]  # x fastest
        base = sum(c[d] * stride[d] for d in range(dim))
        cells.append([base + sum(((v >> d) & 1) * stride[d] for d in range(dim)) for v in range(2 ** dim)])
    return points, np.array(cells)


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_a_file_reads_back_to_the_same_bits(tmp_path, dim):
    points, cells = lattice(dim, 3)
    rng = np.random.default_rng(dim)
    data = {"rho": rng.normal(size=len(points)).astype(np.float32),
            "schlieren_rho": rng.random(len(points)).astype(np.float32)}
    data["rho"][:4] = [np.inf, -np.inf, 1e-42, -0.0]   # inf, a Float32 denormal, the signed zero
    path = str(tmp_path / "a.vtu")
    vo.write_vtu(path, points, cells, data, t=0.125, cycle=7)
    got = read(path)
    assert got["n_points"] == len(points) and got["n_cells"] == len(cells)
    assert got["points"].dtype == np.float32
    assert np.array_equal(got["points"][:, :dim], points.astype(np.float32)) and (got["points"][:, dim:] == 0).all()
    assert list(got["point_data"]) == ["rho", "schlieren_rho"] and set(got["types_of"].values()) == {"Float32"}
    for name, values in data.items():
        assert got["point_data"][name].tobytes() == values.tobytes()
    # offsets and types: line 3, quadrilateral 9, hexahedron 12
    per_cell = 2 ** dim
    assert np.array_equal(got["offsets"], per_cell * np.arange(1, len(cells) + 1))
    assert (got["types"] == {1: 3, 2: 9, 3: 12}[dim]).all() and got["types"].dtype == np.uint8
    assert got["connectivity"].dtype == np.int32 and got["offsets"].dtype == np.int32
    order = {1: [0, 1], 2: [0, 1, 3, 2], 3: [0, 1, 3, 2, 4, 5, 7, 6]}[dim]
    assert np.array_equal(got["connectivity"].reshape(-1, per_cell), cells[:, order])
    # TIME and CYCLE as DataOutBase::VtkFlags(t, cycle) writes them
    assert float(got["field"]["TIME"]) == 0.125 and int(got["field"]["CYCLE"]) == 7


def test_quad_and_hex_orderings_give_positive_volume(tmp_path):
    """VTK's quadrilateral is walked counter-clockwise (positive shoelace area); its hexahedron has the top face above
    the bottom face in the same sense (positive triple product of the edges at vertex 0, and vertex 6 opposite 0)"""
    points, cells = lattice(2, 3)
    vo.write_vtu(str(tmp_path / "q.vtu"), points, cells, {})
    got = read(str(tmp_path / "q.vtu"))
    for quad in got["connectivity"].reshape(-1, 4):
        x, y = got["points"][quad, 0].astype(float), got["points"][quad, 1].astype(float)
        area = 0.5 * sum(x[i] * y[(i + 1) % 4] - x[(i + 1) % 4] * y[i] for i in range(4))
        assert area > 0.0 and np.isclose(area, (1.0 / 3) * (1.5 / 3))
    points, cells = lattice(3, 2)
    vo.write_vtu(str(tmp_path / "h.vtu"), points, cells, {})
    got = read(str(tmp_path / "h.vtu"))
    for hexa in got["connectivity"].reshape(-1, 8):
        p = got["points"][hexa].astype(float)
        volume = np.dot(np.cross(p[1] - p[0], p[3] - p[0]), p[4] - p[0])
        assert volume > 0.0 and np.isclose(volume, (1.0 / 2) * (1.5 / 2) * (2.0 / 2))
        # the bottom face 0-1-2-3 and the top face 4-5-6-7 are walked in the same sense, 4 above 0 ... 7 above 3
        for v in range(4):
            assert np.allclose((p[4 + v] - p[v])[:2], 0.0) and p[4 + v][2] > p[v][2]
        assert np.allclose(p[2] - p[1], p[3] - p[0]) and np.allclose(p[6] - p[0], p.max(axis=0) - p.min(axis=0))


@pytest.mark.parametrize("dim", [1, 2, 3])
def test_a_piece_without_cells_is_a_valid_file(tmp_path, dim):
    path = str(tmp_path / "empty.vtu")
    vo.write_vtu(path, np.zeros((0, dim)), np.zeros((0, 2 ** dim), dtype=np.uint32), {"rho": np.zeros(0)}, t=1.0,
                 cycle=0)
    got = read(path)
    assert got["n_points"] == 0 and got["n_cells"] == 0
    assert got["points"].size == 0 and got["connectivity"].size == 0 and got["offsets"].size == 0
    assert got["types"].size == 0 and got["point_data"]["rho"].size == 0
    assert int(got["field"]["CYCLE"]) == 0


def test_point_data_of_the_wrong_length_is_refused(tmp_path):
    points, cells = lattice(2, 2)
    with pytest.raises(ValueError):
        vo.write_vtu(str(tmp_path / "x.vtu"), points, cells, {"rho": np.zeros(len(points) + 1)})


def test_file_names_are_the_references():
    assert vo.file_names("solution", 123) == ("solution_000123.vtu", None)
    assert vo.file_names("solution", 123, levelsets=True) == ("solution-levelsets_000123.vtu", None)
    assert vo.file_names("out/run", 0, rank=2, n_ranks=3) == ("out/run_000000.2.vtu", "out/run_000000.pvtu")
    assert vo.file_names("s", 7, rank=3, n_ranks=12, levelsets=True) == ("s-levelsets_000007.03.vtu",
                                                                        "s-levelsets_000007.pvtu")


def test_the_pvtu_record_names_every_piece(tmp_path):
    pieces = [vo.file_names("solution", 5, r, 3)[0] for r in range(3)]
    path = str(tmp_path / vo.file_names("solution", 5, 0, 3)[1])
    vo.write_pvtu(path, [os.path.join(str(tmp_path), p) for p in pieces], ["rho", "alpha"])
    root = ET.parse(path).getroot()
    assert root.tag == "VTKFile" and root.get("type") == "PUnstructuredGrid"
    assert [p.get("Source") for p in root.findall("PUnstructuredGrid/Piece")] == pieces
    assert [a.get("Name") for a in root.findall("PUnstructuredGrid/PPointData/PDataArray")] == ["rho", "alpha"]
    assert root.find("PUnstructuredGrid/PPoints/PDataArray").get("NumberOfComponents") == "3"
