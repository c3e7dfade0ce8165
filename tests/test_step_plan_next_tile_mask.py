"""StepPlan::next_tile_mask on the CPU (ryujin_amd/csrc/step_plan.hpp): step 6 hands its mask of limited tiles to step 7
exactly where every launch of step 6 is the single-launch cached kernel with one wave per slice, step 7 is the cached
kernel and the run is not checked -- over the case table of tests/helpers_plan_cases.py, whose literals say which
launches share slices -- and the plan refuses every other combination. Host logic only: no GPU, no HIP runtime."""
import json
import os
import subprocess

import pytest

import helpers_plan_cases as plan_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "next_tile_mask_plan")


@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "cpp", "next_tile_mask_plan.cc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ryujin_amd", "csrc"), src,
                    "-o", BIN], check=True)
    return BIN


def _run(checker, *args):
    out = subprocess.run([checker, *map(str, args)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads(out.stdout)


def _expected(dim, plan, step6_launches):
    """from the table's literals alone"""
    return (plan["step6"] == "cached" and plan["step7"] == "last_cached" and not plan["checked"] and dim <= 2 and
            not any(q["shares_slices"] for q in step6_launches))


@pytest.mark.parametrize("name", sorted(plan_cases.CASES) + ["erk33"])
def test_the_boolean_over_the_case_table_of_the_gpu_variants(checker, name):
    case = plan_cases.ERK33_CASE if name == "erk33" else plan_cases.CASES[name]
    off = case["mesh"]()
    width = int(plan_cases.widths_of(off).max())
    n_slices = (off.n_owned + 63) // 64
    for update in (case, case["second_update"]):
        if update is None:
            continue
        assert [q["n_slices"] for q in update["step6_launches"]] == [n_slices]
        args = ("plan", case["equation"], off.dim, width, n_slices, 0, update["limited_fraction"], case["stages"])
        r = _run(checker, *args)
        assert r["step6_cached"] == (update["plan"]["step6"] == "cached")
        assert r["step7_last_cached"] == (update["plan"]["step7"] == "last_cached")
        assert r["interior_shares_slices"] == update["step6_launches"][0]["shares_slices"] and not r["export_shares_slices"]
        assert r["next_tile_mask"] == _expected(off.dim, update["plan"], update["step6_launches"]), (name, r)
        assert r["next_tiles_elided"] == r["next_tile_mask"]  # the default: step 6 does not store the zeros either
        stored = _run(checker, *args, "mask=1")
        assert stored["next_tile_mask"] == r["next_tile_mask"] and not stored["next_tiles_elided"]
        # the switch, a checked run
        assert not _run(checker, *args, "mask=-1")["next_tile_mask"]
        assert not _run(checker, *args, "checked=1")["next_tile_mask"]
        # the kernels of the large meshes on every mesh: nothing shares a slice any more
        large = _run(checker, *args, "no_split=1")
        assert not large["interior_shares_slices"]
        assert large["next_tile_mask"] == (large["step6_cached"] and large["step7_last_cached"] and off.dim <= 2)


def test_the_table_reaches_both_values():
    """(otherwise the test above compares False with False)"""
    # (the dimension from the width of the unrolled step 3: the Q2 lattices, 27, run the generic sweeps in 2-D)
    values = {name: _expected({3: 1, 9: 2, 27: 3}[c["plan"]["diag_width"]], c["plan"], c["step6_launches"])
              for name, c in plan_cases.CASES.items()}
    on = sorted(k for k, v in values.items() if v)
    assert on == ["aeos_1d_1025", "aeos_2d_step_1588", "euler_1d_1025", "euler_2d_box_4096", "euler_2d_box_4097", "euler_2d_step_1588", "scalar_2d_1148",
                  "sw_2d_1148"], on
    assert len(values) - len(on) >= 10


def test_a_split_sweep_carries_the_mask_only_if_neither_launch_shares_slices(checker):
    """shallow water on two ranks (the table's TWO_RANK_CASE): the export part of a few slices shares them in step 6 and
    writes no mask, so the update runs without one; with P_ij per tile (Euler) no launch ever shares"""
    case = plan_cases.TWO_RANK_CASE
    for expected in case["ranks"]:
        (n_export, _, export_shares), (n_interior, _, interior_shares) = expected["launches"]
        r = _run(checker, "plan", case["equation"], 2, 9, n_export + n_interior, n_export, 1.0, 0)
        assert (r["export_shares_slices"], r["interior_shares_slices"]) == (export_shares, interior_shares) == (True, False)
        assert not r["next_tile_mask"]
        r = _run(checker, "plan", case["equation"], 2, 9, n_export + n_interior, n_export, 1.0, 0, "no_split=1")
        assert r["next_tile_mask"] and not r["export_shares_slices"]
        r = _run(checker, "plan", "euler", 2, 9, n_export + n_interior, n_export, 1.0, 0)
        assert r["next_tile_mask"] and not r["export_shares_slices"]
    # an export part above the sharing limit as well
    assert _run(checker, "plan", "shallow_water", 2, 9, 2100, 1025, 1.0, 0)["next_tile_mask"]
    assert not _run(checker, "plan", "shallow_water", 2, 9, 2100, 1076, 1.0, 0)["next_tile_mask"]  # interior: 1024


def test_the_boolean_is_its_definition_over_the_input_lattice(checker):
    r = _run(checker, "lattice")
    assert r["violations"] == 0, r
    for key in ("on", "on_split_sweep", "off_by_switch", "off_by_sharing"):
        assert r[key] > 0, (key, r)
    # the switch is the only difference between the three thirds of the lattice: on and eliding, on, off
    assert r["on"] == 2 * r["off_by_switch"] == 2 * r["elided"]


def test_violated_fires_when_the_boolean_is_forced_on(checker):
    """SPLIT (in the only launch, and in the export launch alone), P_ij per slice (2-D by the switch, 3-D), the generic
    step 7, a checked run"""
    r = _run(checker, "forced")
    for name in ("split", "split_export_part", "per_slice", "per_slice_3d", "generic_step7", "checked"):
        assert r[name]["off_in_the_plan"] and r[name]["refused"].startswith("step plan: "), (name, r)
    assert "one wave per slice" in r["split"]["refused"] and "one wave per slice" in r["split_export_part"]["refused"]
    assert "single-launch cached step 6" in r["per_slice"]["refused"]
    assert "single-launch cached step 6" in r["per_slice_3d"]["refused"]
    assert r["accepted"] is True
    assert "cached step 7" in r["accepted_with_generic_step7"]
    assert "checked" in r["accepted_but_checked"]
