"""The stencil classes on the CPU (ryujin_amd/csrc/host_layout.hpp: SellLayout::build_stencil_classes): every slice
marked uniform reproduces the explicit arrays from its class entry -- the bits of c_ij and m_ij, row + delta == cols --
lane by lane, has no padding, and shares its class only with slices of the same key; and how many slices of the meshes
the GPU tests and the bench line run on are uniform. Host logic only: no GPU, no HIP runtime. The checker is a
stand-alone program and is built with the address and undefined-behaviour sanitizers."""
import json
import os
import subprocess

import pytest

from ryujin_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "stencil_classes")


@pytest.fixture(scope="module")
def checker():
    synth = _build.build_synth()
    src = os.path.join(ROOT, "tests", "cpp", "stencil_classes.cc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ryujin_amd", "csrc"), src, synth,
                    "-Wl,-rpath," + os.path.dirname(synth), "-o", BIN], check=True)
    return BIN


def _run(checker, *args):
    out = subprocess.run([checker, *map(str, args)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr, out.stderr  # (the undefined-behaviour sanitizer reports and goes on)
    return json.loads(out.stdout)


@pytest.mark.parametrize("mesh", [("mach3", 60, 1, 0), ("box", 2, 200, 24, 1), ("box", 1, 500, 1, 1),
                                  ("box", 3, 120, 12, 12), ("box", 3, 20, 20, 20)],
                         ids=["mach3_step_2d(60)", "rectangle_2d(200,ny=24)", "1d(500)", "box_3d(120x12x12)", "box_3d(20)"])
def test_uniform_slices_reproduce_the_explicit_arrays(checker, mesh):
    r = _run(checker, *mesh)
    assert r["violations"] == 0 and r["padded_rows"] == 0, r
    assert r["n_uniform_slices"] <= r["n_full_slices"] and r["n_uniform_tiles"] <= r["n_tiles"], r
    assert (r["n_classes"] == 0) == (r["n_uniform_slices"] == 0), r
    if mesh[:2] != ("box", 3) or mesh[2] > 64:  # (lattice rows of 21 nodes: no slice lies inside one)
        assert r["n_uniform_slices"] > 0, r


def test_counts_on_the_small_step_mesh(checker):
    """mach3_step_2d(60): 89 of its 145 whole slices in 3 classes; a middle rank of three (export rows first) has none,
    and then there is no table at all."""
    r = _run(checker, "mach3", 60, 1, 0)
    assert (r["n_full_slices"], r["n_uniform_slices"], r["n_classes"]) == (145, 89, 3), r
    r = _run(checker, "mach3", 60, 3, 1)
    assert (r["n_uniform_slices"], r["n_uniform_tiles"], r["n_classes"], r["violations"]) == (0, 0, 0, 0), r


def test_counts_on_the_bench_mesh(checker):
    """mach3_step_2d(995), 2 498 844 gridpoints: 38 016 of 39 044 whole slices (97.4 % of the entries) in 6 classes."""
    r = _run(checker, "mach3", 995, 1, 0)
    assert (r["n_full_slices"], r["n_uniform_slices"], r["n_classes"]) == (39044, 38016, 6), r
    assert r["violations"] == 0 and r["padded_rows"] == 0, r
    assert abs(r["n_uniform_tiles"] / r["n_tiles"] - 0.974) < 0.0005, r
