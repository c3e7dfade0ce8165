"""The case table of tests/test_gpu_plan_variants.py: one entry per kernel variant that the launch-size splits of steps 5
and 6 select (ryujin_amd/csrc/step_plan.hpp), at the slice counts where the selection changes.

An entry holds a mesh recipe, the Description, the initial data, the warm-up (run on the ORACLE: the input of the
compared update does not depend on the code under test) and, as literals, the plan the update must run and what each
launch of steps 5 and 6 must have been given. tests/test_step_plan.py pins these literals against plan_step() on the CPU
(the checker's `plan` mode, fed with n_owned and the widest row of the case's mesh); the GPU test asserts them against
HyperbolicModule.last_plan(), which reports what was launched. Nothing here evaluates the thresholds.

The thresholds themselves (four waves per block; 2048 resident waves in step 5, 4096 in step 6; boundary conditions
folded into the pre-pass up to 4096 slices): step 5 takes 4 waves per slice up to 512 slices, 3 for 513 - 680, 2 for
681 - 1024, 1 above; step 6 shares a slice among the four waves of a block up to 1024 slices (dim <= 2, P_ij not per
tile)."""
from __future__ import annotations

import numpy as np

from ryujin_amd import HyperbolicModule, capi, offline
from ryujin_amd.initial_states import euler_from_primitive, euler_uniform


def perturbed(U, seed=42, amp=1e-3):
    """multiplicative 1 + amp U(-1,1) perturbation (initial_values.template.h:198-218), as tests/test_gpu_parity.py"""
    rng = np.random.default_rng(seed)
    return U * (1.0 + amp * rng.uniform(-1.0, 1.0, size=U.shape))


# ------------------------------------------------------------------ expected plans (literals; see the module docstring)

def _plan(step2, diag_width, step5, step5_groups, has_V, pij_stored, step6, step6_flags, step7="last_cached", *,
          step2_split=False, fast_riemann=False, step4_single_walk=False, step4_has_stages=False, step4_stores_p=True,
          tiles_predicted_from_history=False, wide=False, step4_friction=False, checked=False):
    return dict(step2=step2, step2_split=step2_split, fast_riemann=fast_riemann, diag_width=diag_width,
                step4_single_walk=step4_single_walk, step4_has_stages=step4_has_stages, step4_friction=step4_friction,
                step4_stores_p=step4_stores_p, dg=False, step5=step5, step5_groups=step5_groups, wide=wide,
                has_V=has_V, pij_stored=pij_stored, tiles_predicted_from_history=tiles_predicted_from_history,
                step6=step6, step6_flags=step6_flags, step7=step7, fuse_precompute=False, checked=checked)


def _euler_groups(width, groups):
    """Euler without stage vectors, Q1 rows: k_lij_stage0<Euler<dim>, groups> with P_ij everywhere; V_i only with one
    wave per slice"""
    return _plan("records", width, "stage0_groups", groups, groups == 1, 1, "cached", groups == 1, fast_riemann=True,
                 step4_stores_p=False)


def _euler_per_tile(width=9):
    """Euler 1-D, 2-D above 1024 slices: k_lij_stage0<Euler<dim>, 1, false, true>, tiles predicted from the history"""
    return _plan("records", width, "stage0_per_tile", 1, True, 3, "cached", True, fast_riemann=True, step4_stores_p=False,
                 tiles_predicted_from_history=True)


def _aeos_groups(groups, width=9):
    """EulerAEOS without stage vectors, Q1 rows: k_lij_stage0<EulerAeos<dim>, groups>; V_i only with one wave per slice"""
    return _plan("alpha_then_dij", width, "stage0_groups", groups, groups == 1, 1, "cached", groups == 1, step2_split=True,
                 step4_stores_p=False)


def _aeos_per_tile(width=9):
    """EulerAEOS 1-D, 2-D above 1024 slices: k_lij_stage0<EulerAeos<dim>, 1, false, true>"""
    return _plan("alpha_then_dij", width, "stage0_per_tile", 1, True, 3, "cached", True, step2_split=True,
                 step4_stores_p=False, tiles_predicted_from_history=True)


def _stored_everywhere(step2, **kw):
    """shallow water, scalar conservation, Euler with stage vectors: step 4 stores P_ij, step 5 is k_pij_lij (V_i)"""
    return _plan(step2, 9, "pij_lij", 1, True, 1, "cached", True, **kw)


def _recompute():
    """Euler 2-D, rows of up to 25 entries, no stage vectors: k_pij_lij_recompute<2, NY> (NY per launch), the generic
    high-order sweeps"""
    return _plan("records", 27, "recompute", 1, False, 1, "high_order", False, "high_order", fast_riemann=True,
                 step4_stores_p=False)


def _one(n_slices, grid_y, shares):
    return dict(step5_launches=[dict(n_slices=n_slices, grid_y=grid_y)],
                step6_launches=[dict(n_slices=n_slices, grid_y=1, shares_slices=shares)])


# ------------------------------------------------------------------ meshes and data

def _interval(n_points):
    return offline.MeshSpec(1, (n_points - 1,), (0.0,), (1.0,), (capi.BC_DIRICHLET, capi.BC_DO_NOTHING))


def _shock_tube(off):
    """the data of test_step_parity_1d"""
    x = off.positions[:, 0]
    U0 = euler_from_primitive(np.where(x < 0.5, 1.0, 0.125), np.zeros((len(x), 1)), np.where(x < 0.5, 1.0, 0.1))
    return dict(U0=perturbed(U0), dirichlet=U0[off.b_i])


def _front_through(off, center, corner):
    """|x - center| <= R with R a third of a cell short of `corner`: a front between that node and its neighbours, which
    also crosses the faces and edges that meet there -- the limiter acts in rows of every width"""
    x = off.positions
    h = np.abs(x[1] - x[0]).max()   # (lattice numbering: the first two nodes are neighbours)
    R = np.linalg.norm(np.asarray(corner) - np.asarray(center)) - 0.3 * h
    return np.linalg.norm(x - np.asarray(center), axis=1) <= R


def _mach3(off):
    """the uniform Mach-3 inflow of the step benchmark. The re-entrant corner of the step is the one row of eight
    entries, and the developing flow does not limit it: after the warm-up that node is compressed (a local extremum)"""
    def compress_corner(U):
        corner = np.flatnonzero(widths_of(off) == 8)
        U[corner] *= np.array([2.0, 2.0, 2.0, 4.0])   # twice the density and momentum, four times the energy
        return U
    return dict(U0=perturbed(euler_uniform(off.positions)), dirichlet=euler_uniform(off.b_positions),
                after_warm=compress_corner)


def _narrowest_compressed(data):
    """`data` with the rows of the fewest entries (1-D: the two ends; a box: its corners) compressed after the warm-up, as
    _mach3 compresses its corner: the later stages of a Runge-Kutta step do not limit them otherwise"""
    def recipe(off):
        out = data(off)

        def compress(U):
            narrowest = np.flatnonzero(widths_of(off) == widths_of(off).min())
            U[narrowest] *= np.array([2.0] * (off.dim + 1) + [4.0])   # twice the density and momentum, four times the energy
            return U
        return dict(out, after_warm=compress)
    return recipe


def _contrast_2d(off):
    """a slip box with a pressure and density contrast across a circle"""
    inside = _front_through(off, (0.6, 0.6), (1.0, 1.0))
    U0 = euler_from_primitive(np.where(inside, 1.0, 0.125), np.zeros((len(inside), 2)), np.where(inside, 10.0, 0.1))
    return dict(U0=perturbed(U0), dirichlet=None)


def _contrast_3d(off):
    inside = _front_through(off, (0.5, 0.5, 0.5), (1.0, 1.0, 1.0))
    U0 = euler_from_primitive(np.where(inside, 1.0, 0.125), np.zeros((len(inside), 3)), np.where(inside, 10.0, 0.1))
    return dict(U0=perturbed(U0), dirichlet=None)


def _contrast_3d_nasg(off):
    """the primitive state of _contrast_3d under the Noble-Abel stiffened gas of _nasg_edit"""
    import oracle_py
    from ryujin_amd.initial_states import aeos_from_primitive
    p = oracle_py.default_params(capi.EQ_EULER_AEOS, 3)
    _nasg_edit(p)
    inside = _front_through(off, (0.5, 0.5, 0.5), (1.0, 1.0, 1.0))
    U0 = aeos_from_primitive(p, np.where(inside, 1.0, 0.125), np.zeros((len(inside), 3)), np.where(inside, 10.0, 0.1))
    return dict(U0=perturbed(U0), dirichlet=None)


def _dam_break(off):
    U0 = np.zeros((off.n_relevant, 3))
    U0[:, 0] = np.where(_front_through(off, (2.5, 2.5), (5.0, 5.0)), 2.5, 0.5)
    return dict(U0=perturbed(U0), dirichlet=None)


def _kpp(off):
    """smooth and nowhere constant (in constant regions the Roe average of the reference amplifies last-bit differences
    of the transcendental flux, test_partitioned_other_descriptions_match_single_rank), steep enough for the limiter"""
    pos = off.positions
    u = np.pi * (1.9 + 1.5 * np.sin(0.9 * pos[:, 0]) * np.cos(1.1 * pos[:, 1] + 0.3))
    U0 = perturbed(u.reshape(-1, 1))
    return dict(U0=U0, dirichlet=U0[off.b_i])


def _kpp_edit(p):
    p.sc_flux = capi.FLUX_KPP


def _aeos_edit(p):
    p.eos = capi.EOS_POLYTROPIC_GAS
    p.compute_strict_bounds = 1


def _nasg_edit(p):
    """the Noble-Abel stiffened gas of test_aeos_step_parity_1d_and_3d: the surrogate gamma varies from node to node"""
    p.eos = capi.EOS_NOBLE_ABEL_STIFFENED_GAS
    p.compute_strict_bounds = 1
    p.eos_covolume_b, p.eos_pinf, p.eos_q = 0.1, 0.2, 0.05


def _q2_wave(off):
    """a uniform flow through random patches of 3 x 3 nodes with their own density and pressure (periodic Q2 lattice):
    jumps in every direction relative to the vertex, edge and cell nodes"""
    x = off.positions
    h = x[1, 1] - x[0, 1]
    block = np.floor(x / (3.0 * h) + 0.25).astype(np.int64)
    rng = np.random.default_rng(3)
    table = rng.uniform(0.0, 1.0, size=(int(block.max()) + 1, int(block.max()) + 1, 2))
    rho, p = 1.0 + 0.5 * table[block[:, 0], block[:, 1], 0], 1.0 + 2.0 * table[block[:, 0], block[:, 1], 1]
    v = np.zeros((off.n_owned, 2))
    v[:, 0], v[:, 1] = 0.5, -0.25
    return dict(U0=euler_from_primitive(rho, v, p), dirichlet=None)


def _q2_lattice(n_elements):
    from helpers_q2 import q2_periodic_offline_sparse
    return lambda: q2_periodic_offline_sparse(2, n_elements)[0]


def _synthetic(spec):
    return lambda: offline.SyntheticOffline(spec)


def _case(mesh, equation, data, n_points, plan, launches, *, warm, edit=None, cfl=0.9, limited_fraction=1.0, stages=0,
          second_update=None, options=()):
    """options: what the plan mode of the CPU checker is told besides the mesh (tests/test_step_plan.py)"""
    names = {"euler": capi.EQ_EULER, "euler_aeos": capi.EQ_EULER_AEOS, "scalar": capi.EQ_SCALAR_CONSERVATION,
             "shallow_water": capi.EQ_SHALLOW_WATER}
    return dict(mesh=mesh, equation=equation, eq=names[equation], data=data, n_points=n_points, plan=plan, warm=warm,
                edit=edit, cfl=cfl, limited_fraction=limited_fraction, stages=stages, second_update=second_update,
                options=tuple(options), **launches)


CASES = {}

# Euler 1-D shock tube: three columns over 4, 3, 2 and 1 waves; the last slice alternately full and holding one row
for _s, _full, _groups, _shares in ((512, True, 4, True), (513, False, 3, True), (680, True, 3, True),
                                    (681, False, 2, True), (1024, True, 2, True), (1025, False, 1, False)):
    _n = 64 * _s if _full else 64 * (_s - 1) + 1
    CASES[f"euler_1d_{_s}"] = _case(_synthetic(_interval(_n)), "euler", _shock_tube, _n,
                                    _euler_groups(3, _groups) if _groups > 1 else _euler_per_tile(3),
                                    _one(_s, _groups, _shares), warm=10)

# Euler 2-D: the Mach-3 step at 896 slices (two waves per slice, step 6 shares) and at 1588 (P_ij per tile, boundary
# conditions folded into the pre-pass); a slip box on both sides of the fold limit
CASES["euler_2d_step_896"] = _case(_synthetic(offline.mach3_step_2d(150)), "euler", _mach3, 57301,
                                   _euler_groups(9, 2), _one(896, 2, True), warm=12)
CASES["euler_2d_step_1588"] = _case(_synthetic(offline.mach3_step_2d(200)), "euler", _mach3, 101601,
                                    _euler_per_tile(), _one(1588, 1, False), warm=12)
CASES["euler_2d_box_4096"] = _case(_synthetic(offline.rectangle_2d(511)), "euler", _contrast_2d, 512 * 512,
                                   _euler_per_tile(), _one(4096, 1, False), warm=6)
CASES["euler_2d_box_4097"] = _case(_synthetic(offline.rectangle_2d(544, ny=480)), "euler", _contrast_2d, 545 * 481,
                                   _euler_per_tile(), _one(4097, 1, False), warm=6)

# EulerAEOS 2-D, polytropic gas: k_lij_stage0<EulerAeos<2>, 3 | 2>
CASES["aeos_2d_step_674"] = _case(_synthetic(offline.mach3_step_2d(130)), "euler_aeos", _mach3, 43109,
                                  _aeos_groups(3), _one(674, 3, True), warm=12, edit=_aeos_edit)
CASES["aeos_2d_step_896"] = _case(_synthetic(offline.mach3_step_2d(150)), "euler_aeos", _mach3, 57301,
                                  _aeos_groups(2), _one(896, 2, True), warm=12, edit=_aeos_edit)

# EulerAEOS in 1-D, on the per-tile side in 2-D and in 3-D: the meshes, data and warm-ups of the Euler cases above and
# below. 3-D at 1000 slices with the Noble-Abel stiffened gas (NASG); at 1424 the second update of the context stores
# P_ij per slice. Its limited fraction: the share of 64-row slices in which the ORACLE's first-pass l_ij of the first
# update has an off-diagonal entry below 1 (limited_slice_fraction; tests/test_step_plan.py evaluates it): 719 of 1424
# at a warm-up of one update, below the 0.8 up to which P_ij is stored per slice
for _s, _full, _groups, _shares in ((512, True, 4, True), (513, False, 3, True), (680, True, 3, True),
                                    (681, False, 2, True), (1024, True, 2, True), (1025, False, 1, False)):
    _n = 64 * _s if _full else 64 * (_s - 1) + 1
    CASES[f"aeos_1d_{_s}"] = _case(_synthetic(_interval(_n)), "euler_aeos", _shock_tube, _n,
                                   _aeos_groups(_groups, 3) if _groups > 1 else _aeos_per_tile(3),
                                   _one(_s, _groups, _shares), warm=10, edit=_aeos_edit)
CASES["aeos_2d_step_1588"] = _case(_synthetic(offline.mach3_step_2d(200)), "euler_aeos", _mach3, 101601,
                                   _aeos_per_tile(), _one(1588, 1, False), warm=12, edit=_aeos_edit)
CASES["aeos_3d_box_562"] = _case(_synthetic(offline.box_3d(32)), "euler_aeos", _contrast_3d, 33 ** 3,
                                 _aeos_groups(3, 27), _one(562, 3, False), warm=2, edit=_aeos_edit)
CASES["aeos_3d_box_1000"] = _case(_synthetic(offline.box_3d(39)), "euler_aeos", _contrast_3d_nasg, 40 ** 3,
                                  _aeos_groups(2, 27), _one(1000, 2, False), warm=2, edit=_nasg_edit)
CASES["aeos_3d_box_1424"] = _case(
    _synthetic(offline.box_3d(44)), "euler_aeos", _contrast_3d, 45 ** 3, _aeos_groups(1, 27),
    _one(1424, 1, False), warm=1, edit=_aeos_edit,
    second_update=dict(limited_fraction=719 / 1424,
                       plan=_plan("alpha_then_dij", 27, "stage0_per_slice", 1, True, 2, "per_slice", True,
                                  step2_split=True, step4_stores_p=False), **_one(1424, 1, False)))

# Euler 3-D radial contrast: 27 columns over 3, 2 and 1 waves; step 6 never shares slices in 3-D. The largest: the
# first update of a context stores P_ij everywhere, the second one per slice (few slices hold a limited pair)
CASES["euler_3d_box_562"] = _case(_synthetic(offline.box_3d(32)), "euler", _contrast_3d, 33 ** 3,
                                  _euler_groups(27, 3), _one(562, 3, False), warm=2)
CASES["euler_3d_box_1000"] = _case(_synthetic(offline.box_3d(39)), "euler", _contrast_3d, 40 ** 3,
                                   _euler_groups(27, 2), _one(1000, 2, False), warm=2)
CASES["euler_3d_box_1424"] = _case(
    _synthetic(offline.box_3d(44)), "euler", _contrast_3d, 45 ** 3, _euler_groups(27, 1),
    _one(1424, 1, False), warm=1,   # (the corner rows stay limited for the first three updates)
    second_update=dict(limited_fraction=0.5,
                       plan=_plan("records", 27, "stage0_per_slice", 1, True, 2, "per_slice", True, fast_riemann=True,
                                  step4_stores_p=False), **_one(1424, 1, False)))

# shallow water and scalar conservation store P_ij everywhere: only step 6 changes, at 1024 slices
for _name, _equation, _data, _step2, _kw, _edit in (
        ("sw", "shallow_water", _dam_break, "records", dict(step4_single_walk=True), None),
        ("scalar", "scalar", _kpp, "dij_alpha_sc", dict(step2_split=True), _kpp_edit)):
    for _n, _s, _shares in ((252, 1001, True), (270, 1148, False)):
        _bc = capi.BC_DIRICHLET if _equation == "scalar" else capi.BC_SLIP
        CASES[f"{_name}_2d_{_s}"] = _case(_synthetic(offline.rectangle_2d(_n, (-5.0, -5.0), (5.0, 5.0), bc=_bc)),
                                          _equation, _data, (_n + 1) ** 2, _stored_everywhere(_step2, **_kw),
                                          _one(_s, 1, _shares), warm=8, edit=_edit)

# Euler 2-D on a periodic Q2 lattice (rows of 9, 15 and 25 entries), no stage vectors: k_pij_lij_recompute<2, 3 | 2 | 1>
for _el, _s, _groups in ((100, 625, 3), (120, 900, 2), (140, 1225, 1)):
    CASES[f"euler_q2_{_s}"] = _case(_q2_lattice(_el), "euler", _q2_wave, 4 * _el * _el, _recompute(),
                                    _one(_s, _groups, False), warm=4, cfl=0.5)

del _s, _full, _groups, _shares, _n, _name, _equation, _data, _step2, _kw, _edit, _bc, _el

# step<1> and step<2> of ERK33 with stage vectors on the Mach-3 step at 896 slices: step 4 stores P_ij, step 5 is
# k_pij_lij, step 6 shares slices (tests/test_gpu_plan_variants.py runs the stages)
ERK33_CASE = _case(_synthetic(offline.mach3_step_2d(150)), "euler", _mach3, 57301,
                   _stored_everywhere("records", fast_riemann=True, step4_has_stages=True), _one(896, 1, True), warm=6,
                   stages=1)

# ... and on EulerAEOS (k_low_order_aeos<1 | 3, true, ...>, k_pij_lij<EulerAeos<1 | 3> >): the 1-D interval at 681 slices,
# where step 6 shares slices, and the 3-D box at 562
ERK33_CASES = {
    "erk33": ERK33_CASE,
    "erk33_aeos_1d_681": _case(
        _synthetic(_interval(64 * 680 + 1)), "euler_aeos", _narrowest_compressed(_shock_tube), 64 * 680 + 1,
        _plan("alpha_then_dij", 3, "pij_lij", 1, True, 1, "cached", True, step2_split=True, step4_has_stages=True),
        _one(681, 1, True), warm=10, edit=_aeos_edit, stages=1),
    "erk33_aeos_3d_box_562": _case(
        _synthetic(offline.box_3d(32)), "euler_aeos", _narrowest_compressed(_contrast_3d), 33 ** 3,
        _plan("alpha_then_dij", 27, "pij_lij", 1, True, 1, "cached", True, step2_split=True, step4_has_stages=True),
        _one(562, 1, False), warm=2, edit=_aeos_edit, stages=1),
}

# ... and on shallow water with Manning friction over an uneven, partly dry bed: the plain update of stage 0 runs
# k_low_order_sw_single_walk<1 | 2, false, 3 | 9, true>, step<1> and step<2> run <1 | 2, true, 3 | 9, true>. A Q1
# rectangle of 13 x 7 gridpoints (one full slice and 27 rows of a second one, boundary rows in both) and an interval
# of 100 gridpoints
def _uneven_bed(positions):
    """a bed that rises through the free surface of _over_uneven_bed towards the upper end of x: a dry shore"""
    x = positions[:, 0]
    Z = 0.15 * x + 0.1 * np.sin(2.0 * x)
    return Z + 0.1 * np.cos(1.5 * positions[:, 1]) if positions.shape[1] > 1 else Z


def _over_uneven_bed(spec):
    def mesh():
        off = offline.SyntheticOffline(spec)
        off.set_initial_precomputed(_uneven_bed(off.positions))
        return off
    return mesh


def _dam_break_over_uneven_bed(off):
    """water at rest with its surface at 1 left of x = 0 and at 0.6 right of it, dry where the bed is higher"""
    x = off.positions
    U0 = np.zeros((off.n_relevant, off.dim + 1))
    U0[:, 0] = np.maximum(np.where(x[:, 0] < 0.0, 1.0, 0.6) - _uneven_bed(x), 0.0)
    return dict(U0=U0, dirichlet=None)


def _manning_edit(p):
    p.manning_friction_coefficient = 0.03


ERK33_SW_FRICTION_CASES = {
    "erk33_sw_friction_2d_13x7": _case(
        _over_uneven_bed(offline.rectangle_2d(12, (-5.0, -2.5), (5.0, 2.5), ny=6, bc=capi.BC_SLIP)), "shallow_water",
        _dam_break_over_uneven_bed, 13 * 7,
        _stored_everywhere("records", step4_single_walk=True, step4_has_stages=True, step4_friction=True),
        _one(2, 1, True), warm=4, edit=_manning_edit, stages=1, options=("friction=1",)),
    "erk33_sw_friction_1d_100": _case(
        _over_uneven_bed(offline.MeshSpec(1, (99,), (-5.0,), (5.0,), (capi.BC_SLIP, capi.BC_SLIP))), "shallow_water",
        _dam_break_over_uneven_bed, 100,
        _plan("records", 3, "pij_lij", 1, True, 1, "cached", True, step4_single_walk=True, step4_has_stages=True,
              step4_friction=True),
        _one(2, 1, True), warm=4, edit=_manning_edit, stages=1, options=("friction=1",)),
}
ERK33_CASES.update(ERK33_SW_FRICTION_CASES)

# shallow water on two ranks (x slabs of a 381 x 381 point box): the export part of a rank is a few slices and shares
# them in step 6, the interior part has more than 1024 and does not
TWO_RANK_CASE = dict(
    n=380, lower=(-5.0, -5.0), upper=(5.0, 5.0), n_points=381 ** 2, warm=8, equation="shallow_water",
    plan=_stored_everywhere("records", step4_single_walk=True),
    # per rank: owned gridpoints, then (slices, gridDim.y of step 5, step 6 shares) of the export and the interior part
    ranks=[dict(n_owned=72390, launches=[(6, 1, True), (1126, 1, False)]),
           dict(n_owned=72771, launches=[(6, 1, True), (1132, 1, False)])])


# ------------------------------------------------------------------ running a case

def build(case):
    """(offline data, initial state, Dirichlet data, what is done to the state after the warm-up or None) of a case"""
    off = case["mesh"]()
    data = case["data"](off)
    return off, data["U0"], data["dirichlet"], data.get("after_warm")


def params_of(case, oracle, dim):
    p = oracle.default_params(case["eq"], dim)
    p.cfl = case["cfl"]
    if case["edit"]:
        case["edit"](p)
    return p


def widths_of(off):
    n = off.n_owned
    return np.diff(np.asarray(off.row_starts[: n + 1]).astype(np.int64))


def warm_up(case, oracle, off, U0, dirichlet, after_warm=None):
    """the state after case["warm"] updates ON THE ORACLE"""
    m = HyperbolicModule(off, params_of(case, oracle, off.dim), backend=oracle.backend())
    old, new = m.new_state_vector(U0), m.new_state_vector()
    for _ in range(case["warm"]):
        m.prepare_state_vector(old, 0.0, dirichlet)
        m.step(old, [], [], new)
        old, new = new, old
    U = old.download()
    m.close()
    return after_warm(U) if after_warm else U


def both_backends(case, oracle, off, U_start):
    """[(hip module, old, new), (oracle module, old, new)] holding the same state, as _both of tests/test_gpu_parity.py"""
    mods = []
    for backend in ("hip", oracle.backend()):
        m = HyperbolicModule(off, params_of(case, oracle, off.dim), backend=backend)
        mods.append((m, m.new_state_vector(U_start), m.new_state_vector()))
    return mods


def limiter_coverage(off, first_pass_lij):
    """What a case must show before it counts (the oracle's first-pass l_ij of the compared update): for every
    off-diagonal column position of the stencil, and for every row width that occurs, the number of entries below 1.
    A wave's share of the columns, and the rows that leave waves without a column, are otherwise compared on l = 1
    alone. Returns (per column position, per row width): dicts position / width -> count."""
    widths = widths_of(off)
    rs = np.concatenate([[0], np.cumsum(widths)])
    position = np.arange(rs[-1]) - np.repeat(rs[:-1], widths)
    width_of_entry = np.repeat(widths, widths)
    limited = (np.asarray(first_pass_lij)[: rs[-1]] < 1.0) & (position > 0)
    per_position = {int(q): int(limited[position == q].sum()) for q in range(1, int(widths.max()))}
    per_width = {int(w): int(limited[width_of_entry == w].sum()) for w in np.unique(widths) if w > 1}
    return per_position, per_width


def limited_slice_fraction(off, first_pass_lij):
    """the share of the 64-row slices in which some off-diagonal first-pass l_ij is below 1 -- what step 6 counts on the
    device (on every 16th slice) and plan_step() takes as `limited_fraction` in the next update"""
    widths = widths_of(off)
    rs = np.concatenate([[0], np.cumsum(widths)])
    limited = np.asarray(first_pass_lij)[: rs[-1]] < 1.0
    limited[rs[:-1]] = False   # (the diagonal entry holds no limiter value)
    rows = np.zeros(-(-off.n_owned // 64) * 64, dtype=bool)
    rows[: off.n_owned] = np.add.reduceat(limited.astype(np.int64), rs[:-1]) > 0
    return float(rows.reshape(-1, 64).any(axis=1).mean())
