"""The table of norms next to the stencil classes on the CPU (ryujin_amd/csrc/host_layout.hpp: SellLayout::class_norms):
every entry holds |c_ij| = sqrt(c_0 c_0 + c_1 c_1) and its reciprocal bit for bit as recomputed from the explicit c_ij
array, and the table is empty exactly where the class table is. Host logic only: no GPU, no HIP runtime. The checker is a
stand-alone program and is built with the address and undefined-behaviour sanitizers."""
import json
import os
import subprocess

import pytest

from ryujin_amd import _build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "class_norms")


@pytest.fixture(scope="module")
def checker():
    synth = _build.build_synth()
    src = os.path.join(ROOT, "tests", "cpp", "class_norms.cc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "ryujin_amd", "csrc"), src, synth,
                    "-Wl,-rpath," + os.path.dirname(synth), "-o", BIN], check=True)
    return BIN


def _run(checker, *args):
    out = subprocess.run([checker, *map(str, args)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr, out.stderr  # (the undefined-behaviour sanitizer reports and goes on)
    return json.loads(out.stdout)


@pytest.mark.parametrize("mesh", [("mach3", 60, 1, 0), ("mach3", 995, 1, 0), ("box", 2, 200, 24, 1), ("box", 1, 500, 1, 1)],
                         ids=["mach3_step_2d(60)", "mach3_step_2d(995)", "rectangle_2d(200,ny=24)", "1d(500)"])
def test_norms_are_what_step_2_would_compute(checker, mesh):
    r = _run(checker, *mesh)
    assert r["violations"] == 0 and r["not_finite"] == 0, r
    # every entry of the class table has its pair of norms, and a slice of its class checked it (at least a class of
    # three columns: these meshes all have uniform slices, tests/test_stencil_classes.py)
    assert r["n_entries"] == r["n_norms"] == r["n_checked"] >= 3, r


def test_no_class_table_no_norms(checker):
    """a middle rank of three (export rows first) has no uniform slice: both tables are empty"""
    r = _run(checker, "mach3", 60, 3, 1)
    assert r == dict(n_entries=0, n_norms=0, n_checked=0, not_finite=0, violations=0), r
