"""The tile mask from step 6 to step 7 on the GPU (ryujin_amd/csrc/kernels_limiter.hpp, SliceFlags::next_tiles): the
first of the two limiter passes leaves, per 64-row slice, the columns in which some pair is limited, and does not store
the exact zeros of the other tiles; the last pass sets l = 0 in every other column without requesting the tile's
descriptor, l'_ij or l'_ji. lmin(0, x) = 0 for every x in [0, 1]: U, alpha, both limiter matrices and P_ij must be bit
for bit what they are with the mask switched off (ryujin_hip_params::debug_next_tile_mask = -1) and with the mask on
and every zero stored (= 1)."""
import ctypes as C

import numpy as np
import pytest

from ryujin_amd import HyperbolicModule, capi, offline
from ryujin_amd.initial_states import euler_from_primitive, euler_uniform, sw_circular_dam_break

pytestmark = pytest.mark.gpu


def _perturbed(U, seed=42, amp=1e-3, fraction=1.0):
    """multiplicative 1 + amp U(-1, 1) on the lowest-indexed `fraction` of the rows"""
    rng = np.random.default_rng(seed)
    out = U * (1.0 + amp * rng.uniform(-1.0, 1.0, size=U.shape))
    n = int(round(fraction * len(U)))
    out[n:] = U[n:]
    return out


def _step_mesh(**kw):
    return offline.mach3_step_2d(60, **kw)


def _interval(**kw):
    return offline.MeshSpec(1, (64 * 20,), (0.0,), (1.0,), (capi.BC_DIRICHLET, capi.BC_DO_NOTHING), **kw)


def _aeos_edit(p):
    p.eos = capi.EOS_POLYTROPIC_GAS
    p.compute_strict_bounds = 1


LARGE = {"debug_no_small_mesh_split": 1}  # the kernels of the large meshes: one wave per slice in steps 5 and 6

# case -> (equation, dim, mesh recipe, (n_ranks, rank), params edit, perturbed fraction of the rows,
#          the plan hands the mask on, tiles of both kinds required)
CASES = {
    # 145 slices through the large-mesh kernels (P_ij per tile): every slice limited ...
    "euler_step_2d_all_rows": (capi.EQ_EULER, 2, _step_mesh, (1, 0), LARGE, 1.0, True, False),
    # ... and limited and unlimited tiles inside the same slices
    "euler_step_2d_30_percent": (capi.EQ_EULER, 2, _step_mesh, (1, 0), LARGE, 0.3, True, True),
    # the default plan of this mesh: the four waves of a block share a slice in step 6, which writes no mask
    "euler_step_2d_default_plan": (capi.EQ_EULER, 2, _step_mesh, (1, 0), {}, 0.3, False, False),
    # shallow water: step 6 keeps the reference-order sum, P_ij stored everywhere
    "shallow_water_2d": (capi.EQ_SHALLOW_WATER, 2,
                         lambda **kw: offline.rectangle_2d(200, (-5.0, -5.0), (5.0, 5.0), ny=24, **kw), (1, 0), LARGE,
                         1.0, True, True),
    "euler_aeos_step_2d": (capi.EQ_EULER_AEOS, 2, _step_mesh, (1, 0), dict(LARGE, _edit=_aeos_edit), 0.3, True, True),
    # three columns, MAXW = 3
    "euler_1d": (capi.EQ_EULER, 1, _interval, (1, 0), LARGE, 1.0, True, True),
    # a middle rank of three on the loopback communicator, export rows first: two launches per sweep, packed exchange
    "euler_step_2d_rank_1_of_3": (capi.EQ_EULER, 2, _step_mesh, (3, 1), LARGE, 0.3, True, True),
    # the irregular-position path of transposed_positions under the mask
    "euler_step_2d_tile_map_off": (capi.EQ_EULER, 2, _step_mesh, (1, 0), dict(LARGE, debug_tile_map=-1), 0.3, True,
                                   True),
}


def _initial(equation, dim, off, fraction):
    if equation == capi.EQ_SHALLOW_WATER:
        return sw_circular_dam_break(off.positions), None
    if dim == 1:  # the shock tube of tests/test_gpu_parity.py
        x = off.positions[:, 0]
        U0 = euler_from_primitive(np.where(x < 0.5, 1.0, 0.125), np.zeros((len(x), 1)), np.where(x < 0.5, 1.0, 0.1))
        return _perturbed(U0, fraction=0.5), U0[off.b_i]
    U0 = _perturbed(euler_uniform(off.positions), fraction=fraction)
    return U0, (euler_uniform(off.b_positions) if off.n_bdry else None)


@pytest.mark.parametrize("case", sorted(CASES))
def test_the_mask_gives_the_same_bits_as_reading_every_tile(oracle, case):
    equation, dim, recipe, (n_ranks, rank), edit, fraction, active, both_kinds = CASES[case]
    off = offline.SyntheticOffline(recipe(n_ranks=n_ranks, rank=rank))
    U0, dirichlet = _initial(equation, dim, off, fraction)
    results, infos = [], []
    for mask in (0, 1, -1):
        p = oracle.default_params(equation, dim)
        p.cfl = 0.9
        p.debug_next_tile_mask = mask
        for key, value in edit.items():
            if key == "_edit":
                value(p)
            else:
                setattr(p, key, value)
        comm = None
        if n_ranks > 1:  # a middle rank on its own: the loopback communicator stands in for its neighbours
            comm = C.c_void_p()
            assert capi.load_hip().ryujin_hip_comm_init_loopback(C.byref(comm), rank, n_ranks, 0) == 0
        m = HyperbolicModule(off, p, backend="hip", comm=comm)
        a, b = m.new_state_vector(U0), m.new_state_vector()
        for _ in range(6):
            m.prepare_state_vector(a, 0.0, dirichlet)
            m.step(a, [], [], b)
            a, b = b, a
        info = m.next_tile_mask_info()
        stats = m.limiter_statistics()
        print(case, "mask", mask, info, stats)
        assert info["active"] == (active and mask >= 0), info
        assert info["n_tiles"] > 0 and (info["active"] or info["n_named"] == info["n_tiles"]), info
        infos.append((info, stats))
        temps = [b, m.new_state_vector(), m.new_state_vector()]
        for _ in range(2):
            m.time_step("ssprk 33", a, temps, dirichlet)
        assert m.next_tile_mask_info()["active"] == (active and mask >= 0)
        results.append((a.download(), m.alpha().copy(), m.debug_fetch("lij"), m.debug_fetch("lij_next"),
                        m.debug_fetch("pij")))
        m.close()
    assert np.isfinite(results[0][0]).all()
    (info, stats) = infos[0]
    assert infos[1] == infos[0]  # the mask does not depend on whether the zeros are stored
    if both_kinds:  # otherwise the case proves nothing: tiles step 7 reads AND tiles it skips
        assert 0 < info["n_named"] < info["n_tiles"], info
        if off.n_owned >= 100 * 64:  # (the statistics sample every 16th slice: too few on the smaller meshes)
            assert 0.0 < stats["limited_slice_fraction"], stats
            if "tiles_read_fraction" in stats:  # (P_ij per tile)
                assert 0.0 < stats["tiles_read_fraction"] < 1.0, stats
    elif active:
        # (six updates on, the noise is limited in every sampled slice and in about half of the tiles)
        assert 2 * info["n_named"] >= info["n_tiles"] and stats["limited_slice_fraction"] == 1.0, (info, stats)
    # the second-pass matrix holds exact zeros wherever the second pass limited nothing; some entry is not zero
    assert (results[0][2] != 0.0).any()
    for other in results[1:]:
        for x, y in zip(results[0], other):
            assert np.array_equal(x, y)


@pytest.mark.parametrize("stale", ["earlier_pass", "nan"])
def test_slots_step_6_does_not_store_are_never_looked_at(oracle, stale):
    """What step 6 leaves in the slot of an unlimited tile is stale: the first-pass l_ij of the update before, or -- after
    a restarted update -- a NaN. One update on the state with every slice limited fills both matrices with non-trivial
    values; then updates on a state perturbed in its lowest-indexed rows only, where most tiles are elided. `nan`:
    before each of them the buffer step 6 is about to write holds NaN in EVERY slot. The partner row of an elided slot
    takes l = 0 from its own exact zero; the fetched second-pass matrix has its zeros materialised -- a slot left
    behind would show as a NaN, and as a difference to the run that stores everything."""
    off = offline.SyntheticOffline(_step_mesh())
    U_limited = _perturbed(euler_uniform(off.positions))
    U_calm = _perturbed(euler_uniform(off.positions), seed=7, fraction=0.05)
    dirichlet = euler_uniform(off.b_positions)
    results = []
    for mask in (0, -1):
        p = oracle.default_params(capi.EQ_EULER, 2)
        p.cfl = 0.9
        p.debug_no_small_mesh_split = 1
        p.debug_next_tile_mask = mask
        m = HyperbolicModule(off, p, backend="hip")
        a, b = m.new_state_vector(U_limited), m.new_state_vector()
        m.prepare_state_vector(a, 0.0, dirichlet)
        m.step(a, [], [], b)
        named_limited = m.next_tile_mask_info()["n_named"]
        a.upload(U_calm)
        fetched = []
        for _ in range(3):
            if stale == "nan":
                m.debug_fill("lij_next", float("nan"))
            m.prepare_state_vector(a, 0.0, dirichlet)
            m.step(a, [], [], b)
            fetched.append(m.debug_fetch("lij"))
            a, b = b, a
        info = m.next_tile_mask_info()
        print(stale, "mask", mask, named_limited, info)
        if mask == 0:  # most tiles elided, where the update before had stored non-trivial values
            assert info["active"] and 0 < 4 * info["n_named"] < info["n_tiles"] < 2 * named_limited, (info, named_limited)
        results.append((a.download(), m.alpha().copy(), m.debug_fetch("lij_next"), *fetched))
        m.close()
    for x in results[0]:
        assert np.isfinite(x).all()
    assert (results[0][-1] != 0.0).any()
    for x, y in zip(results[0], results[1]):
        assert np.array_equal(x, y)
