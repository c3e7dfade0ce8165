"""The step plan on the CPU (ryujin_amd/csrc/step_plan.hpp): which kernels an update runs. The stored-P_ij variants give
the same bits by design, so a change that silently moves a configuration to another variant passes every parity test;
here the invariants the kernels rely on are checked over the whole input lattice, and the kernel paths of the benchmark
configurations are pinned to what the kernel traces of record show (profiles/r07_kernel_trace*.md; C1:
profiles/r04p_kernel_trace_c1.md with the template arguments of today's k_lij_stage0). Host logic only: no GPU, no HIP
runtime."""
import json
import os
import subprocess

import pytest

from ryujin_amd.workloads import benchmark_workload

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "tests", "cpp", "step_plan_cases")


@pytest.fixture(scope="module")
def checker():
    src = os.path.join(ROOT, "tests", "cpp", "step_plan_cases.cc")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "ryujin_amd", "csrc"), src,
                    "-o", BIN], check=True)
    return BIN


def _run(checker, *args):
    out = subprocess.run([checker, *map(str, args)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads(out.stdout)


def test_invariants_over_the_input_lattice(checker):
    """Per tile implies V_i, one wave per slice and dim <= 2; per slice implies V_i; the checked build stores P_ij
    everywhere; the two selective modes exclude each other and imply the stage-0 kernel; step 4 stores its part of P_ij
    exactly when step 5 neither recomputes nor forms it; step 6 gets V_i only where it exists and never shares slices
    with per-tile storage; EulerAEOS with rows of more than 32 entries is refused. And the lattice reaches every
    variant: all three storage modes, one to four waves per slice, both sides of the fold limit."""
    r = _run(checker, "lattice")
    assert r["violations"] == 0, r
    # 11 (equation, dim) x 3 stages x 3 iterations x 2 dG x 5 widths x 11 meshes x 4 storages x 2 checked x 4 fractions
    # x 2 pending x 2 Riemann paths / friction
    assert r["plans"] == 11 * 3 * 3 * 2 * 5 * 11 * 4 * 2 * 4 * 2 * 2
    assert r["refused"] == r["plans"] // 11 * 3 * 2 // 5  # EulerAEOS (3 of 11) with 33 or 65 entries (2 of 5)
    for key in ("pij_stored_1", "pij_stored_2", "pij_stored_3", "stage0_groups_1", "stage0_groups_2", "stage0_groups_3",
                "stage0_groups_4", "step6_shares_slices", "fuse_precompute", "has_V", "step5_0", "step5_1", "step5_2",
                "step5_3", "step5_4", "step5_5", "step6_0", "step6_1", "step6_2", "step6_3"):
        assert r.get(key, 0) > 0, (key, r)


def _step_points(cells_per_unit):
    """Gridpoints of the Mach-3 step mesh, [0,3]x[0,1] minus the step [0.6,3]x[0,0.2] (the nodes strictly inside it and
    on its lower and right edge do not exist)."""
    n = cells_per_unit
    nx0, ny0 = round(0.6 * n), round(0.2 * n)
    return (3 * n + 1) * (n + 1) - (3 * n - nx0) * ny0


def _slices(points):
    return (points + 63) // 64


E2, E3, A2, S2 = "Euler<2>", "Euler<3>", "EulerAeos<2>", "ShallowWater<2>"

# (equation, dim, widest row, gridpoints) and the kernels of steps 2 - 7, first update of a context (limited fraction 1)
# and developed flow (the fraction the bench line of record reports; C3 44 %, the others do not depend on it)
PINS = {
    "step2d": (("euler", 2, 9, _step_points(benchmark_workload("step2d").resolution)), 0.9, [
        f"k_dij_alpha_records<{E2}, false>", "k_dij_diag_unrolled<9>", "k_low_order<2, false, false, false>",
        f"k_lij_stage0<{E2}, 1, false, true>", f"k_high_order_next_cached<{E2}, 9, 9, false, 0>",
        f"k_high_order_last_cached<{E2}, 9, 3>"], None),
    "step2d_aeos": (("euler_aeos", 2, 9, _step_points(benchmark_workload("step2d_aeos").resolution)), 0.9, [
        "k_alpha_aeos<2>", "k_dij_aeos<2>", "k_dij_diag_unrolled<9>", "k_low_order_aeos<2, false, false, false>",
        f"k_lij_stage0<{A2}, 1, false, true>", f"k_high_order_next_cached<{A2}, 9, 9, false, 0>",
        f"k_high_order_last_cached<{A2}, 9, 3>"], None),
    "sw2d": (("shallow_water", 2, 9, (benchmark_workload("sw2d").resolution + 1) ** 2), 0.67, [
        f"k_dij_alpha_records<{S2}, false>", "k_dij_diag_unrolled<9>", "k_low_order_sw_single_walk<2, false, 9, false>",
        f"k_pij_lij<{S2}, false, false>", f"k_high_order_next_cached<{S2}, 9, 9, false, 0>",
        f"k_high_order_last_cached<{S2}, 9, 3>"], None),
    "cylinder3d": (("euler", 3, 27, 4176134), 1.0, [  # h = 1/96: the gridpoints of record (DESIGN_HISTORY.md)
        f"k_dij_alpha_records<{E3}, false>", "k_dij_diag_unrolled<27>", "k_low_order<3, false, false, false>",
        f"k_lij_stage0<{E3}, 1, false, false>", f"k_high_order_next_cached<{E3}, 27, 2, false, 0>",
        f"k_high_order_last_cached<{E3}, 27, 3>"], None),
    # first update: P_ij everywhere, the plain kernels; developed: per slice, step 6 as light, repair, heavy
    "sedov3d": (("euler", 3, 27, (benchmark_workload("sedov3d").resolution + 1) ** 3), 0.44, [
        f"k_dij_alpha_records<{E3}, false>", "k_dij_diag_unrolled<27>", "k_low_order<3, false, false, false>",
        f"k_lij_stage0<{E3}, 1, true, false>", f"k_high_order_next_cached<{E3}, 27, 2, false, 1>",
        f"k_pij_repair<{E3} >", f"k_high_order_next_cached<{E3}, 27, 2, false, 2>",
        f"k_high_order_last_cached<{E3}, 27, 3>"], [
        f"k_dij_alpha_records<{E3}, false>", "k_dij_diag_unrolled<27>", "k_low_order<3, false, false, false>",
        f"k_lij_stage0<{E3}, 1, false, false>", f"k_high_order_next_cached<{E3}, 27, 2, false, 0>",
        f"k_high_order_last_cached<{E3}, 27, 3>"]),
    # C1, bench.py --cells-per-unit 130: 43 109 gridpoints, 674 slices: three waves per slice in step 5 (no V_i), the
    # four waves of a block share a slice in step 6
    "c1": (("euler", 2, 9, _step_points(130)), 1.0, [
        f"k_dij_alpha_records<{E2}, false>", "k_dij_diag_unrolled<9>", "k_low_order<2, false, false, false>",
        f"k_lij_stage0<{E2}, 3, false, false>", f"k_high_order_next_cached<{E2}, 9, 9, true, 0>",
        f"k_high_order_last_cached<{E2}, 9, 3>"], None),
}
STORED = {"step2d": 3, "step2d_aeos": 3, "sw2d": 1, "cylinder3d": 1, "sedov3d": 2, "c1": 1}


def test_gridpoints_of_record():
    assert _step_points(995) == 2498844 and _step_points(130) == 43109  # DESIGN_HISTORY.md


@pytest.mark.parametrize("key", sorted(PINS))
def test_kernel_path_of_the_benchmark_configurations(checker, key):
    """The full kernel path, by the names rocprofv3 prints (bench.py's KERNEL_OF_SWEEP matches their prefixes), for the
    first update of a context and for the developed flow."""
    (equation, dim, width, points), fraction, developed, first = PINS[key]
    r = _run(checker, "path", equation, dim, width, _slices(points), fraction)
    assert r["kernels"] == developed, r
    assert r["pij_stored"] == STORED[key]
    r = _run(checker, "path", equation, dim, width, _slices(points), 1.0)
    assert r["kernels"] == (developed if first is None else first), r
    assert r["pij_stored"] == (STORED[key] if first is None else 1)
    # the last sweep carries the next pre-pass on the large Euler and shallow-water meshes, never on C1 or EulerAEOS
    assert r["fuse_precompute"] == (key in ("step2d", "sw2d", "cylinder3d", "sedov3d"))


# ---- the case table of tests/test_gpu_plan_variants.py against plan_step()

import helpers_plan_cases as plan_cases  # noqa: E402


def _checked_plan(checker, equation, off_dim, widths, n_owned, limited_fraction, stages, launch_sizes, options=()):
    """launch_sizes may end in options ("key=value") as well"""
    n_slices = (n_owned + 63) // 64  # host_layout.hpp: n_slices = ceil(n_owned / 64)
    r = _run(checker, "plan", equation, off_dim, int(widths.max()), n_slices, limited_fraction, stages, *launch_sizes,
             *options)
    return n_slices, r


def _assert_table_entry(r, n_slices, plan, step5_launches, step6_launches):
    launches = r.pop("launches")
    assert r == plan, {k: (r[k], plan.get(k)) for k in r if r[k] != plan.get(k)}
    assert [dict(n_slices=q["n_slices"], grid_y=q["step5_grid_y"]) for q in launches] == step5_launches
    assert [dict(n_slices=q["n_slices"], grid_y=1, shares_slices=q["step6_shares_slices"])
            for q in launches] == step6_launches
    assert sum(q["n_slices"] for q in launches) == n_slices


@pytest.mark.parametrize("name", sorted(plan_cases.CASES) + sorted(plan_cases.ERK33_CASES))
def test_case_table_of_the_gpu_variants_is_what_plan_step_decides(checker, name):
    """Every entry of tests/helpers_plan_cases.py: the mesh of the case is built, n_owned and the widest row are taken
    from it, and the plan and the per-launch decisions plan_step() makes of them must equal the table's literals -- the
    table the GPU test holds HyperbolicModule.last_plan() against."""
    case = plan_cases.ERK33_CASES[name] if name in plan_cases.ERK33_CASES else plan_cases.CASES[name]
    off = case["mesh"]()
    assert off.n_owned == case["n_points"]
    widths = plan_cases.widths_of(off)
    for update in (case, case["second_update"]):
        if update is None:
            continue
        sizes = [q["n_slices"] for q in update["step5_launches"]]
        n_slices, r = _checked_plan(checker, case["equation"], off.dim, widths, off.n_owned, update["limited_fraction"],
                                    case["stages"], sizes, case["options"])
        _assert_table_entry(r, n_slices, update["plan"], update["step5_launches"], update["step6_launches"])


def test_limited_fraction_of_the_second_update_is_the_oracles(oracle):
    """aeos_3d_box_1424: the fraction the second update's plan literal carries is the share of slices in which the
    oracle's first-pass l_ij of the FIRST compared update is below 1, and it lies below the 0.8 up to which P_ij is
    stored per slice"""
    from ryujin_amd import HyperbolicModule
    case = plan_cases.CASES["aeos_3d_box_1424"]
    off, U0, dirichlet, after_warm = plan_cases.build(case)
    U_start = plan_cases.warm_up(case, oracle, off, U0, dirichlet, after_warm)
    m = HyperbolicModule(off, plan_cases.params_of(case, oracle, off.dim), backend=oracle.backend())
    old, new = m.new_state_vector(U_start), m.new_state_vector()
    m.prepare_state_vector(old, 0.0, dirichlet)
    m.step(old, [], [], new)
    fraction = plan_cases.limited_slice_fraction(off, m.debug_fetch("lij_next"))
    m.close()
    assert fraction == case["second_update"]["limited_fraction"] == 719 / 1424 < 0.8


def test_case_table_two_ranks(checker):
    from ryujin_amd import offline
    case = plan_cases.TWO_RANK_CASE
    for rank, expected in enumerate(case["ranks"]):
        off = offline.SyntheticOffline(offline.rectangle_2d(case["n"], case["lower"], case["upper"], n_ranks=2, rank=rank))
        assert off.n_owned == expected["n_owned"]
        sizes = [s for s, _, _ in expected["launches"]]
        assert sizes[0] == (off.n_export + 63) // 64  # the export part: ceil(n_export / 64) slices
        n_slices, r = _checked_plan(checker, case["equation"], 2, plan_cases.widths_of(off), off.n_owned, 1.0, 0, sizes)
        _assert_table_entry(r, n_slices, case["plan"], [dict(n_slices=s, grid_y=y) for s, y, _ in expected["launches"]],
                            [dict(n_slices=s, grid_y=1, shares_slices=b) for s, _, b in expected["launches"]])


def test_sparse_q2_lattice_is_the_dense_one():
    """helpers_q2.q2_periodic_offline_sparse (the lattices of the k_pij_lij_recompute cases) entry by entry against the
    dense assembly"""
    import numpy as np
    from helpers_q2 import q2_periodic_offline, q2_periodic_offline_sparse
    a, xa = q2_periodic_offline(2, 5)
    b, xb = q2_periodic_offline_sparse(2, 5)
    assert np.array_equal(a.row_starts, b.row_starts) and np.array_equal(a.columns, b.columns)
    assert np.array_equal(a._keep["cij"], b._keep["cij"]) and np.array_equal(a._keep["mij"], b._keep["mij"])
    assert np.array_equal(xa, xb) and a.max_row_len == b.max_row_len
    np.testing.assert_allclose(a.mi, b.mi, rtol=4e-16)  # (row sums in another order)


# ---- the case table of tests/test_gpu_row_widths.py against plan_step()

import helpers_row_width_cases as width_cases  # noqa: E402


@pytest.mark.parametrize("name", sorted(width_cases.CASES))
def test_case_table_of_the_row_widths_is_what_plan_step_decides(checker, name):
    """Every entry of tests/helpers_row_width_cases.py: the lattice of the case is built, n_owned and the widest row are
    taken from it, and the plan and the launches plan_step() makes of them -- with the case's parameter edits, and once
    more with debug_no_small_mesh_split where the case runs twice -- must equal the table's literals."""
    case = width_cases.CASES[name]
    off = case["mesh"]()
    assert off.n_owned == case["n_points"]
    widths = plan_cases.widths_of(off)
    assert widths.max() == case["width"]
    for run, launches in enumerate(case["runs"]):
        sizes = [q["n_slices"] for q in launches["step5_launches"]]
        options = case["options"] + (("no_split=1",) if run == 1 else ())
        n_slices, r = _checked_plan(checker, case["equation"], off.dim, widths, off.n_owned, 1.0, case["stages"],
                                    sizes + list(options))
        _assert_table_entry(r, n_slices, case["plan"], launches["step5_launches"], launches["step6_launches"])
    assert len(case["runs"]) == (2 if case["plan"]["step5"] == "recompute" and off.dim == 2 and
                                 case["plan"]["fast_riemann"] else 1)


def test_euler_aeos_with_33_entries_is_refused_and_32_is_not(checker):
    refused = width_cases.AEOS_REFUSED
    out = subprocess.run([checker, "plan", "euler_aeos", "2", str(refused["width"]), "15", "1.0", "0", "15"],
                         capture_output=True, text=True)
    assert out.returncode == 1 and out.stderr.strip() == refused["message"]
    off = width_cases._lattice(refused["shape"], refused["width"])()
    assert plan_cases.widths_of(off).max() == 33 and refused["accepted"]["width"] == 32


@pytest.mark.parametrize("key", sorted(width_cases.AEOS_REFUSED_DIMENSIONS))
def test_euler_aeos_with_33_entries_is_refused_in_one_and_three_dimensions(checker, key):
    refused = width_cases.AEOS_REFUSED_DIMENSIONS[key]
    off = refused["mesh"]()
    assert off.dim == refused["dim"] and plan_cases.widths_of(off).max() == 33 == refused["width"]
    assert (off.n_owned + 63) // 64 == refused["n_slices"]
    n_slices = str(refused["n_slices"])
    out = subprocess.run([checker, "plan", "euler_aeos", str(off.dim), "33", n_slices, "1.0", "0", n_slices],
                         capture_output=True, text=True)
    assert out.returncode == 1 and out.stderr.strip() == refused["message"]
    accepted = width_cases.CASES[refused["accepted"]]
    assert accepted["equation"] == "euler_aeos" and 30 < accepted["width"] <= 32


def test_wide_rows_never_take_the_recompute_kernel(checker):
    """k_pij_lij_recompute keeps the undecided pairs of a row in one 64-bit mask indexed by the column: Euler up to two
    dimensions leaves it at 65 entries for k_pij_lij<WIDE> (found by euler_2d_65 of tests/test_gpu_row_widths.py)"""
    for dim in (1, 2):
        assert _run(checker, "plan", "euler", dim, 64, 15, 1.0, 0, 15)["step5"] == "recompute"
        r = _run(checker, "plan", "euler", dim, 65, 15, 1.0, 0, 15)
        assert r["step5"] == "pij_lij" and r["wide"] and r["step4_stores_p"] and r["has_V"]


def test_one_dimensional_rows_of_more_than_64_entries_take_the_wide_kernels(checker):
    """euler_1d_65, euler_1d_128 and sw_1d_65 of the table: `wide`, k_pij_lij<..<1>, false, true> and k_high_order, by
    the names rocprofv3 prints"""
    for name, E in (("euler_1d_65", "Euler<1>"), ("euler_1d_128", "Euler<1>"), ("sw_1d_65", "ShallowWater<1>")):
        case = width_cases.CASES[name]
        assert case["plan"]["wide"] and case["plan"]["step5"] == "pij_lij" and case["plan"]["step6"] == "high_order"
        r = _run(checker, "path", case["equation"], 1, case["width"], 10, 1.0)
        assert r["kernels"][-3:] == [f"k_pij_lij<{E}, false, true>", f"k_high_order<{E}, false, true>",
                                     f"k_high_order<{E}, true, false>"], r


# ---- the multi-rank case table of tests/test_gpu_row_widths_ranks.py against plan_step()

import helpers_row_width_ranks as rank_cases  # noqa: E402


@pytest.mark.parametrize("name", sorted(rank_cases.RANK_CASES))
def test_case_table_of_the_row_widths_on_ranks_is_what_plan_step_decides(checker, oracle, name):
    """Every rank of every entry of tests/helpers_row_width_ranks.py: the lattice is partitioned, the rank's widest
    owned row and slice count go to plan_step() with the case's parameter edits, and the plan and what the export and
    the interior launch make of it must equal the table's literals. The export part is ceil(n_export / 64) slices
    (ryujin_hip_ctx::sweep); a rank without an interior part has one launch."""
    built = rank_cases.built(name, oracle)
    case = built["case"]
    for view, expected in zip(built["views"], case["ranks"]):
        assert (view.n_owned, view.n_export) == (expected["n_owned"], expected["n_export"])
        sizes = [s for s, _, _ in expected["launches"]]
        n_all = (view.n_owned + 63) // 64
        assert sizes[0] == min(n_all, (view.n_export + 63) // 64) and len(sizes) == (2 if sizes[0] < n_all else 1)
        n_slices, r = _checked_plan(checker, case["equation"], built["off"].dim, plan_cases.widths_of(view), view.n_owned,
                                    1.0, 0, sizes + list(case["options"]))
        _assert_table_entry(r, n_slices, case["plan"], [dict(n_slices=s, grid_y=y) for s, y, _ in expected["launches"]],
                            [dict(n_slices=s, grid_y=1, shares_slices=b) for s, _, b in expected["launches"]])


# ---- the case table of tests/test_gpu_small_meshes.py against plan_step()

import helpers_small_meshes as small_cases  # noqa: E402


@pytest.mark.parametrize("name", sorted(small_cases.CASES))
def test_case_table_of_the_small_meshes_is_what_plan_step_decides(checker, name):
    """Every entry of tests/helpers_small_meshes.py: the mesh is built, n_owned and the widest row are taken from it, and
    the plan and the launches plan_step() makes of them -- as the mesh selects its kernels, and with
    debug_no_small_mesh_split -- must equal the table's literals; for the cases that also run ERK33 stages and the
    checked kernels, those plans as well. (debug_bc_fold_max_slices decides no field of the plan of a step() outside
    the device-resident driver.)"""
    case = small_cases.CASES[name]
    off = case["mesh"]()
    widths = plan_cases.widths_of(off)
    assert off.n_owned == case["n_points"] and widths.max() == case["width"]
    assert (off.n_owned + 63) // 64 == case["n_slices"]
    for run, options in enumerate(((), ("no_split=1",))):
        launches = case["launches"][run]
        sizes = [q["n_slices"] for q in launches["step5_launches"]]
        n_slices, r = _checked_plan(checker, case["equation"], off.dim, widths, off.n_owned, 1.0, 0, sizes + list(options))
        _assert_table_entry(r, n_slices, case["plans"][run], launches["step5_launches"], launches["step6_launches"])
        # the tile mask from step 6 to step 7, from the pinned literals (tests/test_step_plan_next_tile_mask.py holds
        # this expression against plan_step())
        plan = case["plans"][run]
        assert case["tile_mask"][run] == (plan["step6"] == "cached" and plan["step7"] == "last_cached" and off.dim <= 2
                                          and not plan["checked"]
                                          and not any(q["shares_slices"] for q in launches["step6_launches"]))
    if name in small_cases.SUBSET:
        for (plan, launches), stages, options in ((small_cases.stage_plan(name), 1, ()),
                                                  (small_cases.stage_plan(name), 2, ()),
                                                  (small_cases.checked_plan(name), 0, ("checked=1",))):
            n_slices, r = _checked_plan(checker, case["equation"], off.dim, widths, off.n_owned, 1.0, stages,
                                        [case["n_slices"]] + list(options))
            _assert_table_entry(r, n_slices, plan, launches["step5_launches"], launches["step6_launches"])


def test_case_table_of_the_small_meshes_covers_the_slice_counts_and_row_widths():
    """one, two and three slices; widest rows of 2, 3, 4, 8, 9, 18 and 27 entries; every case of the subset exists"""
    assert {c["n_slices"] for c in small_cases.CASES.values()} == {1, 2, 3}
    assert {c["width"] for c in small_cases.CASES.values()} == {2, 3, 4, 8, 9, 18, 27}
    assert {c["n_points"] for c in small_cases.CASES.values()} >= {2, 4, 8, 63, 64, 65}
    assert set(small_cases.SUBSET) <= set(small_cases.CASES) and len(small_cases.CASES) == 76


# ---- the dG case table of tests/test_gpu_dg_variants.py against plan_step()

import helpers_dg_cases as dg_cases  # noqa: E402


@pytest.mark.parametrize("name", sorted(dg_cases.CASES))
def test_case_table_of_the_dg_variants_is_what_plan_step_decides(checker, name):
    """Every entry of tests/helpers_dg_cases.py: the mesh is built, n_owned and the widest row are taken from it, and the
    plan and the launches plan_step() makes of them with dg=1 and the case's parameter edits must equal the literals"""
    case = dg_cases.CASES[name]
    off = case["mesh"]()
    assert off.n_owned == case["n_points"] and off.c.contents.discontinuous_ansatz == 1
    widths = plan_cases.widths_of(off)
    assert widths.max() == case["width"] and "dg=1" in case["options"]
    sizes = [q["n_slices"] for q in case["step5_launches"]]
    n_slices, r = _checked_plan(checker, case["equation"], off.dim, widths, off.n_owned, 1.0, case["stages"],
                                sizes + list(case["options"]))
    _assert_table_entry(r, n_slices, case["plan"], case["step5_launches"], case["step6_launches"])
    assert r["dg"] and r["step4_stores_p"] and r["step5"] == "pij_lij" and r["wide"] == (case["width"] > 64)


@pytest.mark.parametrize("name", sorted(dg_cases.RANK_CASES))
def test_case_table_of_the_dg_variants_on_ranks_is_what_plan_step_decides(checker, oracle, name):
    """per rank: the widest owned row and the slice count of the partition, the export and the interior launch"""
    b = dg_cases.built_ranks(name, oracle)
    case = b["case"]
    for view, (n_owned, n_export, launches) in zip(b["views"], b["entry"]["ranks"]):
        assert (view.n_owned, view.n_export) == (n_owned, n_export)
        sizes = [s for s, _, _ in launches]
        assert sizes[0] == (n_export + 63) // 64
        n_slices, r = _checked_plan(checker, case["equation"], b["off"].dim, plan_cases.widths_of(view), n_owned, 1.0, 0,
                                    sizes + list(case["options"]))
        _assert_table_entry(r, n_slices, case["plan"], [dict(n_slices=s, grid_y=y) for s, y, _ in launches],
                            [dict(n_slices=s, grid_y=1, shares_slices=x) for s, _, x in launches])


def test_the_plan_mode_takes_dg(checker):
    """dg=1 moves Euler 2-D with nine columns from the stage-0 kernel to step 4 storing P_ij and k_pij_lij<.., true, ..>;
    shallow water leaves the single walk; without the key the plan is the continuous one"""
    cg = _run(checker, "plan", "euler", 2, 9, 15, 1.0, 0, 15)
    dg = _run(checker, "plan", "euler", 2, 9, 15, 1.0, 0, 15, "dg=1")
    assert not cg["dg"] and cg["step5"] == "stage0_groups" and not cg["step4_stores_p"]
    assert dg["dg"] and dg["step5"] == "pij_lij" and dg["step4_stores_p"] and dg["has_V"] and dg["step6"] == "cached"
    assert _run(checker, "plan", "shallow_water", 2, 9, 15, 1.0, 0, 15)["step4_single_walk"]
    assert not _run(checker, "plan", "shallow_water", 2, 9, 15, 1.0, 0, 15, "dg=1")["step4_single_walk"]
    assert _run(checker, "path", "euler", 3, 189, 27, 1.0)["kernels"][-3] == "k_pij_lij<Euler<3>, false, true>"


def test_euler_aeos_on_wide_dg_stencils_is_refused(checker):
    refused = dg_cases.AEOS_REFUSED
    for key, (mesh, width) in refused["meshes"].items():
        off = mesh()
        out = subprocess.run([checker, "plan", "euler_aeos", str(off.dim), str(width), "1", "1.0", "0", "1", "dg=1"],
                             capture_output=True, text=True)
        assert out.returncode == 1 and out.stderr.strip() == refused["message"], key
    assert dg_cases.CASES[refused["accepted"]]["width"] == 20
