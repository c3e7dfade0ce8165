"""Stencil classes on the GPU (ryujin_amd/csrc/host_layout.hpp, kernels_euler.hpp): steps 2 and 4 take c_ij and the
column index of a uniform slice from its class entry instead of streaming 64 copies. The same bits into the same operations: U, alpha
and the fetched d_ij, l_ij, P_ij must be bit for bit what they are with the table switched off
(ryujin_hip_params::debug_stencil_classes = -1), alone and combined with the tile map switched off."""
import ctypes as C

import numpy as np
import pytest

from ryujin_amd import HyperbolicModule, capi, offline
from ryujin_amd.initial_states import euler_uniform, sw_circular_dam_break

pytestmark = pytest.mark.gpu


def _perturbed(U, seed=42, amp=1e-3):
    rng = np.random.default_rng(seed)
    return U * (1.0 + amp * rng.uniform(-1.0, 1.0, size=U.shape))


# case -> (equation, mesh recipe, (n_ranks, rank), params edit, (uniform slices, classes) with the table on)
CASES = {
    # 61 % of the slices uniform: both loops of every sweep run in one launch
    "euler_step_2d": (capi.EQ_EULER, lambda **kw: offline.mach3_step_2d(60, **kw), (1, 0), {}, (89, 3)),
    # ... and through the kernels of the large meshes (one wave per slice in step 5, P_ij per tile)
    "euler_step_2d_large_mesh_kernels": (capi.EQ_EULER, lambda **kw: offline.mach3_step_2d(60, **kw), (1, 0),
                                         {"debug_no_small_mesh_split": 1}, (89, 3)),
    # a middle rank of three (export rows first): no uniform slice, no table, and the info call says so
    "euler_step_2d_rank_1_of_3": (capi.EQ_EULER, lambda **kw: offline.mach3_step_2d(60, **kw), (3, 1), {}, (0, 0)),
    "shallow_water_2d": (capi.EQ_SHALLOW_WATER,
                         lambda **kw: offline.rectangle_2d(200, (-5.0, -5.0), (5.0, 5.0), ny=24, **kw), (1, 0), {}, (53, 3)),
    "euler_aeos_step_2d": (capi.EQ_EULER_AEOS, lambda **kw: offline.mach3_step_2d(60, **kw), (1, 0), {}, (89, 3)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_stencil_classes_give_the_same_bits_as_the_streamed_arrays(oracle, case):
    equation, recipe, (n_ranks, rank), edit, (n_uniform, n_classes) = CASES[case]
    off = offline.SyntheticOffline(recipe(n_ranks=n_ranks, rank=rank))
    if equation == capi.EQ_SHALLOW_WATER:
        U0, dirichlet = sw_circular_dam_break(off.positions), None
    else:
        U0 = _perturbed(euler_uniform(off.positions))
        dirichlet = euler_uniform(off.b_positions) if off.n_bdry else None
    results = []
    for classes, tile_map in ((0, 0), (-1, 0), (0, -1), (-1, -1)):
        p = oracle.default_params(equation, 2)
        p.cfl = 0.9
        p.debug_stencil_classes = classes
        p.debug_tile_map = tile_map
        for key, value in edit.items():
            setattr(p, key, value)
        comm = None
        if n_ranks > 1:  # a middle rank on its own: the loopback communicator stands in for its neighbours
            comm = C.c_void_p()
            assert capi.load_hip().ryujin_hip_comm_init_loopback(C.byref(comm), rank, n_ranks, 0) == 0
        m = HyperbolicModule(off, p, backend="hip", comm=comm)
        info = m.stencil_class_info()
        if classes == 0:
            assert (info["n_uniform_slices"], info["n_classes"]) == (n_uniform, n_classes), info
            assert (info["uniform_entry_fraction"] > 0.5) == (n_uniform > 0), info
        else:
            assert info == dict(n_uniform_slices=0, n_classes=0, uniform_entry_fraction=0.0), info
        a, b = m.new_state_vector(U0), m.new_state_vector()
        for _ in range(6):
            m.prepare_state_vector(a, 0.0, dirichlet)
            m.step(a, [], [], b)
            a, b = b, a
        temps = [b, m.new_state_vector(), m.new_state_vector()]
        for _ in range(2):
            m.time_step("ssprk 33", a, temps, dirichlet)
        results.append((a.download(), m.alpha().copy(), m.debug_fetch("dij"), m.debug_fetch("lij"), m.debug_fetch("pij")))
        m.close()
    assert np.isfinite(results[0][0]).all()
    for other in results[1:]:
        for x, y in zip(results[0], other):
            assert np.array_equal(x, y)
