"""The case table of tests/test_gpu_row_widths.py: one entry per value of the widest stencil row at which plan_step()
(ryujin_amd/csrc/step_plan.hpp) or a kernel changes behaviour, on both sides of every threshold:

  3 | 4 (1-D), 9 | 10 (2-D), 27 | 28 (3-D)   k_dij_diag_unrolled<3 | 9 | 27> -> k_dij_diag; steps 6 / 7 cached ->
                                             k_high_order; step 5 k_lij_stage0 -> k_pij_lij_recompute (Euler, dim <= 2)
                                             or k_pij_lij; shallow water leaves the single walk of step 4
  32 | 33                                    step 2: records / alpha_then_dij -> k_dij_alpha; EulerAEOS is refused (its
                                             cases stand at 4, 9 | 10, 31 in 1-D, 10, 32 in 2-D, 28, 32 in 3-D)
  64 | 65                                    `wide`: k_pij_lij / k_high_order walk the columns in blocks of 63; Euler up
                                             to two dimensions leaves k_pij_lij_recompute (one 64-bit mask per row)
  127 | 128                                  two full blocks | a third block of one column
  1023                                       the widest row the layout accepts; column 1022, lane 63 is the last entry
                                             the 16-bit queue of undecided pairs can hold

The meshes are lattices with a prescribed widest row (tests/helpers_row_width.py), open along the fastest axis so that
every slice pads narrow rows next to full ones (1-D: rings with widened rows in every slice). An entry holds, as helpers_plan_cases.py: mesh recipe, Description, data,
the warm-up (ON THE ORACLE), and as literals the plan and the launches the update must run; tests/test_step_plan.py pins
the literals against plan_step() on the CPU. `runs`: the launches per run of the case -- the k_pij_lij_recompute cases
run twice, as the mesh size selects the kernel (four waves per slice) and with debug_no_small_mesh_split (one).

The data: a uniform flow through random patches of 2^dim nodes with their own density and pressure (depth; value);
after the warm-up a handful of nodes -- rows of the widest width and one row of every other width -- are made local
extrema, alternately compressed and expanded: such a node is limited in about half of its columns whatever the width
(the pair count of a row scales its individual P_ij). coverage() states what the ORACLE's first-pass l_ij must show
before a case counts; tests/test_row_width_generator.py evaluates it on the CPU, the GPU test asserts it again."""
from __future__ import annotations

import numpy as np

import helpers_row_width as rw
from helpers_plan_cases import _case, _plan
from ryujin_amd import capi
from ryujin_amd.initial_states import euler_from_primitive

BLOCK = 63   # columns per block of the wide kernels (kernels_limiter.hpp: c_blk += 63)


# ------------------------------------------------------------------ meshes

def _lattice(shape, width, n_pairs=12):
    """open along axis 0; an even width: 12 pairs of full rows widened by the first offset beyond the stencil"""
    def make():
        base = width if width % 2 else width - 1
        pairs = None if width % 2 else rw.widening_pairs(shape, base, n_pairs)
        return rw.lattice_offline(shape, base, extra_pairs=pairs)
    return make


def _ring(n, width, two_partners=False):
    """1-D: a ring (the row sums of an open chain vanish only with c_ij of both signs that cancel across every cut).
    Rows of width - 2 or width - 3 entries, widened in every slice: the nodes a with 8 <= a mod 64 < 24 are paired with
    a + s, s the first offset beyond the stencil -- one or two more entries per row --, and for an even width the nodes
    14 and 14 + s + 1 mod 64 with each other.
    More than 64 entries (s >= 32: the run and its partners a + s no longer overlap, no row would get two more entries):
    every node of the run is paired with a + s AND a + s + 1, all indices modulo n -- the run has the full width, its
    partners one or two entries more than the other rows --, and for an even width the nodes 14 mod 64 with a + s + 2 as
    well; s is raised until s mod 64 lies in [17, 38], so that no partner is a node of another slice's run.
    two_partners: that recipe at any width (the first one reaches 31 entries at the most: a request of 32 or 33 gives
    rows of 31 or 32)."""
    def make():
        base = width - 2 if width % 2 else width - 3
        s = (base - 1) // 2 + 1
        a = np.arange(n)
        if base == 1:   # width 4: rows of three entries, a single pair per slice
            base, pairs = 3, np.stack([a[a % 64 == 10], a[a % 64 == 10] + 2], axis=1)
        elif width > 64 or two_partners:
            while not 17 <= s % 64 <= 38:   # the partners 8 + s ... 23 + s + 2 stay clear of the runs of other slices
                s += 1
            run, extra = a[(a % 64 >= 8) & (a % 64 < 24)], a[a % 64 == 14]
            pairs = np.concatenate([np.stack([run, (run + s) % n], axis=1), np.stack([run, (run + s + 1) % n], axis=1)])
            if width % 2 == 0:
                pairs = np.concatenate([pairs, np.stack([extra, (extra + s + 2) % n], axis=1)])
        else:
            run = a[(a % 64 >= 8) & (a % 64 < 24)]
            pairs = np.stack([run, run + s], axis=1)
            if width % 2 == 0:
                pairs = np.concatenate([pairs, np.stack([a[a % 64 == 14], a[a % 64 == 14] + s + 1], axis=1)])
        return rw.lattice_offline((n,), base, open_axes=(), extra_pairs=pairs)
    return make


LINE, PLANE, PLANE_1023, BOX = (640,), (40, 24), (40, 40), (16, 8, 8)


# ------------------------------------------------------------------ data

def _patch_table(off, n_fields, seed=3):
    """[n, n_fields] uniform random numbers, one set per patch of 2^dim lattice nodes"""
    shape = off.lattice_shape
    block = np.floor(off.positions * shape[0]).astype(np.int64) // 2
    patch = np.zeros(off.n_owned, dtype=np.int64)
    for a in reversed(range(off.dim)):
        patch = patch * ((shape[a] + 1) // 2) + block[:, a]
    table = np.random.default_rng(seed).uniform(0.0, 1.0, size=(int(patch.max()) + 1, n_fields))
    return table[patch]


def extremal_nodes(off):
    """the nodes made local extrema after the warm-up. Of up to 24 rows of the widest width, spread over the mesh: every
    other row itself, and of the rows between them the node of their LAST column (a row next to an extremum is pushed
    past its bounds in that column); the middle one of the rows of every other width."""
    widths = rw.widths_of(off)
    rs = np.asarray(off.row_starts).astype(np.int64)
    widest = np.flatnonzero(widths == widths.max())
    widest = widest[np.unique(np.linspace(0, len(widest) - 1, min(24, len(widest))).astype(np.int64))]
    nodes = list(widest[0::2]) + list(np.asarray(off.columns).astype(np.int64)[rs[widest[1::2] + 1] - 1])
    for w in np.unique(widths)[:-1]:
        rows = np.flatnonzero(widths == w)
        nodes.append(rows[len(rows) // 2])
    return np.unique(np.asarray(nodes, dtype=np.int64))


def _extrema(off, compress, expand, more=None):
    """`more`: further nodes, as a function of the offline data (the multi-rank cases place extrema next to a cut)"""
    def after_warm(U):
        nodes = extremal_nodes(off)
        if more is not None:
            nodes = np.unique(np.concatenate([nodes, np.asarray(more(off), dtype=np.int64)]))
        up = np.isin(np.arange(len(nodes)) % 4, (0, 3))   # (rows and their neighbours alternate in the list)
        U[nodes[up]] = compress(U[nodes[up]])
        U[nodes[~up]] = expand(U[nodes[~up]])
        return U
    return after_warm


def _euler_patches(off, more=None):
    t = _patch_table(off, 2)
    v = np.zeros((off.n_owned, off.dim))
    v[:, 0] = 0.5
    if off.dim > 1:
        v[:, 1] = -0.25
    f = np.array([2.0] * (off.dim + 1) + [4.0])   # twice the density and momentum, four times the energy
    return dict(U0=euler_from_primitive(1.0 + 0.5 * t[:, 0], v, 1.0 + 2.0 * t[:, 1]), dirichlet=None,
                after_warm=_extrema(off, lambda U: U * f, lambda U: U / f, more))


def _sw_patches(off, more=None):
    """water of depth 1 ... 1.5 over a smooth bathymetry (ryujin_hip_offline::initial_precomputed), a uniform discharge"""
    x = off.positions
    Z = 0.1 * np.cos(2.0 * np.pi * x[:, 0]) * (np.sin(2.0 * np.pi * x[:, 1] + 0.3) if off.dim > 1 else 1.0)
    off.set_initial_precomputed(Z)
    U0 = np.zeros((off.n_owned, off.dim + 1))
    U0[:, 0] = 1.0 + 0.5 * _patch_table(off, 1)[:, 0]
    U0[:, 1] = 0.3 * U0[:, 0]
    return dict(U0=U0, dirichlet=None, after_warm=_extrema(off, lambda U: 2.0 * U, lambda U: 0.5 * U, more))


def _scalar_patches(off, more=None):
    """values in (0.5, 2.5) around a smooth wave: nowhere constant (the KPP flux is transcendental; in constant regions
    the Roe average of the reference amplifies last-bit differences, helpers_plan_cases._kpp)"""
    x = off.positions
    u = 1.5 + 0.5 * np.sin(2.0 * np.pi * x[:, 0]) * np.cos(2.0 * np.pi * x[:, 1] + 0.3) + \
        0.5 * (_patch_table(off, 1)[:, 0] - 0.5)
    return dict(U0=u.reshape(-1, 1), dirichlet=None, after_warm=_extrema(off, lambda U: U + 1.0, lambda U: U - 1.0, more))


# ------------------------------------------------------------------ parameter edits

def _newton(p):
    p.riemann_newton_max_iterations = 2


def _checked(p):
    p.debug_expensive_bounds_check = 1


def _no_split(p):
    p.debug_no_small_mesh_split = 1


def _manning(p):
    p.manning_friction_coefficient = 0.03


def _kpp(p):
    p.sc_flux = capi.FLUX_KPP


def _burgers(p):
    p.sc_flux = capi.FLUX_BURGERS


def _aeos(p):
    p.eos = capi.EOS_POLYTROPIC_GAS
    p.compute_strict_bounds = 1


def _aeos_checked(p):
    _aeos(p)
    _checked(p)


# ------------------------------------------------------------------ expected plans (literals)

def _euler_recompute(step2, diag_width, **kw):
    """Euler up to two dimensions, no stage vectors, rows wider than Q1 and of at most 64 entries:
    k_pij_lij_recompute<dim, NY>, k_high_order twice"""
    kw.setdefault("fast_riemann", True)
    return _plan(step2, diag_width, "recompute", 1, False, 1, "high_order", False, "high_order", step4_stores_p=False,
                 **kw)


def _stored(step2, diag_width, wide, **kw):
    """step 4 stores P_ij, step 5 is k_pij_lij<E, false, wide> (V_i), k_high_order<E, false, wide> and <E, true, false>"""
    return _plan(step2, diag_width, "pij_lij", 1, True, 1, "high_order", False, "high_order", wide=wide, **kw)


def _runs(n_slices, *grid_y):
    """per run of the case (as the mesh size selects the kernels, then debug_no_small_mesh_split): the launches"""
    return [dict(step5_launches=[dict(n_slices=n_slices, grid_y=y)],
                 step6_launches=[dict(n_slices=n_slices, grid_y=1, shares_slices=False)]) for y in grid_y]


def _entry(name, shape, n_slices, width, equation, data, plan, grid_y=(1,), *, edit=None, options=(), stages=0,
           request=None):
    """width: the widest row the mesh has; request: the width asked of the recipe where the two differ"""
    runs = _runs(n_slices, *grid_y)
    request = width if request is None else request
    mesh = _ring(shape[0], request) if len(shape) == 1 else _lattice(shape, request)
    case = _case(mesh, equation, data, int(np.prod(shape)), plan, runs[0], warm=1, edit=edit, cfl=0.5, stages=stages)
    CASES[name] = dict(case, width=width, request=request, runs=runs, options=tuple(options))


CASES = {}
R, D, F, T = "records", "dij_alpha", False, True

# Euler, no stage vectors. 1-D (rings): k_pij_lij_recompute<1, 4> on 10 slices
_entry("euler_1d_4", LINE, 10, 4, "euler", _euler_patches, _euler_recompute(R, 9), (4,))
_entry("euler_1d_9", LINE, 10, 9, "euler", _euler_patches, _euler_recompute(R, 9), (4,))
_entry("euler_1d_10", LINE, 10, 10, "euler", _euler_patches, _euler_recompute(R, 27), (4,))
# ... and k_pij_lij<Euler<1>, false, true> above 64 entries: two blocks, and a third block of one column
for _w in (65, 128):
    _entry(f"euler_1d_{_w}", LINE, 10, _w, "euler", _euler_patches, _stored(D, 0, T, fast_riemann=True))
# 2-D: k_pij_lij_recompute up to 64 entries -- <2, 4> on these 15 slices, <2, 1> with debug_no_small_mesh_split --,
# k_pij_lij<Euler<2>, false, true> above
for _w, _step2, _diag in ((10, R, 27), (27, R, 27), (28, R, 0), (32, R, 0), (33, D, 0), (64, D, 0)):
    _entry(f"euler_2d_{_w}", PLANE, 15, _w, "euler", _euler_patches, _euler_recompute(_step2, _diag), (4, 1))
for _w in (65, 127, 128):
    _entry(f"euler_2d_{_w}", PLANE, 15, _w, "euler", _euler_patches, _stored(D, 0, T, fast_riemann=True))
_entry("euler_2d_1023", PLANE_1023, 25, 1023, "euler", _euler_patches, _stored(D, 0, T, fast_riemann=True))
# 3-D: k_pij_lij<Euler<3>, false, false | true>
for _w, _step2, _wide in ((28, R, F), (33, D, F), (65, D, T), (128, D, T)):
    _entry(f"euler_3d_{_w}", BOX, 16, _w, "euler", _euler_patches, _stored(_step2, 0, _wide, fast_riemann=True))

# Euler, further configurations: the general Riemann path, the checked build, step<2> of ERK33 with stage vectors
_entry("euler_2d_newton_32", PLANE, 15, 32, "euler", _euler_patches,
       _euler_recompute("alpha_then_dij", 0, fast_riemann=False, step2_split=True), (4,), edit=_newton,
       options=("newton=2",))
_entry("euler_2d_newton_33", PLANE, 15, 33, "euler", _euler_patches, _euler_recompute(D, 0, fast_riemann=False), (4,),
       edit=_newton, options=("newton=2",))
_entry("euler_2d_checked_65", PLANE, 15, 65, "euler", _euler_patches, _stored(D, 0, T, fast_riemann=True, checked=True),
       edit=_checked, options=("checked=1",))
_entry("euler_2d_erk33_10", PLANE, 15, 10, "euler", _euler_patches,
       _stored(R, 27, F, fast_riemann=True, step4_has_stages=True), stages=2)
_entry("euler_2d_erk33_128", PLANE, 15, 128, "euler", _euler_patches,
       _stored(D, 0, T, fast_riemann=True, step4_has_stages=True), stages=2)

# shallow water: bathymetry in the precomputed values, Manning friction in the 33 case; the two walks of step 4
_entry("sw_1d_4", LINE, 10, 4, "shallow_water", _sw_patches, _stored(R, 9, F))
_entry("sw_1d_65", LINE, 10, 65, "shallow_water", _sw_patches, _stored(D, 0, T))
for _w, _step2, _diag, _wide in ((10, R, 27, F), (32, R, 0, F), (64, D, 0, F), (65, D, 0, T), (128, D, 0, T)):
    _entry(f"sw_2d_{_w}", PLANE, 15, _w, "shallow_water", _sw_patches, _stored(_step2, _diag, _wide))
_entry("sw_2d_33", PLANE, 15, 33, "shallow_water", _sw_patches, _stored(D, 0, F, step4_friction=True), edit=_manning,
       options=("friction=1",))

# scalar conservation: KPP (10, 65), Burgers (28, 128)
for _w, _flux, _diag, _wide in ((10, _kpp, 27, F), (28, _burgers, 0, F), (65, _kpp, 0, T), (128, _burgers, 0, T)):
    _entry(f"scalar_2d_{_w}", PLANE, 15, _w, "scalar", _scalar_patches,
           _stored("dij_alpha_sc", _diag, _wide, step2_split=True), edit=_flux)

# EulerAEOS, polytropic gas, strict bounds
for _w, _diag in ((10, 27), (32, 0)):
    _entry(f"aeos_2d_{_w}", PLANE, 15, _w, "euler_aeos", _euler_patches,
           _stored("alpha_then_dij", _diag, F, step2_split=True), edit=_aeos)
# ... in 1-D (rings; the recipe reaches 31 entries at a request of 32) and 3-D, step<2> of ERK33 with stage vectors, the
# checked build: four bounds and four precomputed values per node throughout
_A = "alpha_then_dij"
for _w, _diag, _request in ((4, 9, 4), (9, 9, 9), (10, 27, 10), (31, 0, 32)):
    _entry(f"aeos_1d_{_w}", LINE, 10, _w, "euler_aeos", _euler_patches, _stored(_A, _diag, F, step2_split=True),
           edit=_aeos, request=_request)
for _w in (28, 32):
    _entry(f"aeos_3d_{_w}", BOX, 16, _w, "euler_aeos", _euler_patches, _stored(_A, 0, F, step2_split=True), edit=_aeos)
_entry("aeos_3d_erk33_28", BOX, 16, 28, "euler_aeos", _euler_patches,
       _stored(_A, 0, F, step2_split=True, step4_has_stages=True), edit=_aeos, stages=2)
_entry("aeos_2d_erk33_32", PLANE, 15, 32, "euler_aeos", _euler_patches,
       _stored(_A, 0, F, step2_split=True, step4_has_stages=True), edit=_aeos, stages=2)
_entry("aeos_3d_checked_28", BOX, 16, 28, "euler_aeos", _euler_patches,
       _stored(_A, 0, F, step2_split=True, checked=True), edit=_aeos_checked, options=("checked=1",))

del _w, _flux, _step2, _diag, _wide, _request, _A, R, D, F, T

# EulerAEOS with 33 entries: step() refuses on the host, before any launch, and the context runs on (step_plan.hpp)
AEOS_REFUSED = dict(shape=PLANE, width=33, accepted=CASES["aeos_2d_32"],
                    message="euler aeos: stencils of more than 32 entries")
# ... and in 1-D (a ring with two partners per widened node: rows of exactly 33 entries) and 3-D; `accepted`: the case
# run afterwards
AEOS_REFUSED_DIMENSIONS = {
    "1d": dict(mesh=_ring(LINE[0], 33, two_partners=True), dim=1, n_slices=10, width=33, accepted="aeos_1d_31",
               message=AEOS_REFUSED["message"]),
    "3d": dict(mesh=_lattice(BOX, 33), dim=3, n_slices=16, width=33, accepted="aeos_3d_32",
               message=AEOS_REFUSED["message"]),
}


# ------------------------------------------------------------------ what a case must show before it counts

def coverage(off, first_pass_lij, width):
    """The condition on the INPUTS (the oracle's first-pass l_ij of the compared update), as a dict of counts that must
    all be positive. Up to 65 entries: entries below 1 in every off-diagonal column position and in rows of every width
    (helpers_plan_cases.limiter_coverage). Wider rows: entries strictly between 0 and 1 -- pairs the fast path of the
    limiter did not decide -- in every block of 63 columns, in the first and the last column of every block (the last
    column of the last block is the last column of a widest row) and, in the 1023 case, in a column >= 512."""
    from helpers_plan_cases import limiter_coverage
    if width <= 65:
        per_position, per_width = limiter_coverage(off, first_pass_lij)
        out = {f"position {q}": v for q, v in per_position.items()}
        out.update({f"width {w}": v for w, v in per_width.items()})
        return out
    widths = rw.widths_of(off)
    rs = np.concatenate([[0], np.cumsum(widths)])
    position = np.arange(rs[-1]) - np.repeat(rs[:-1], widths)
    l = np.asarray(first_pass_lij)[: rs[-1]]
    per_position = np.bincount(position[(l > 0.0) & (l < 1.0) & (position > 0)], minlength=width)
    out = {}
    for first in range(1, width, BLOCK):
        last = min(first + BLOCK, width) - 1
        out[f"block {first}..{last}"] = int(per_position[first:last + 1].sum())
        out[f"column {first}"] = int(per_position[first])
        out[f"column {last}"] = int(per_position[last])
    out[f"last column {width - 1} of a widest row"] = int(per_position[width - 1])
    if width >= 1023:
        out["columns >= 512"] = int(per_position[512:].sum())
    return out


def summation_slack(off, equation):
    """row_slack of helpers_parity.compare_step for U_new: 2 W eps sum_j |term_j| of the row's limited update
    U_new = U_low + sum_j l_ij lambda P_ij over both passes, from the ORACLE's l_ij and P_ij (after the update "lij_next"
    holds the first pass's l_ij, "lij" the second pass's (1 - l) l'; both enter min-symmetrised). The terms of the low-order
    sum and of r_i are not among the fetched operands: no slack is claimed for them, nor for P_ij."""
    widths = rw.widths_of(off)
    rs = np.concatenate([[0], np.cumsum(widths)])
    tr = rw.transposed_entries(off)
    lam = np.repeat(1.0 / np.maximum(widths - 1, 1), widths)
    eps = np.finfo(np.float64).eps

    def row_slack(name, c):
        if name != "U":
            return None
        k = c["pij"].size // c["lij"].size
        first, second = c["lij_next"], c["lij"]
        l = np.minimum(first, first[tr]) + np.minimum(second, second[tr])
        terms = (l * lam)[:, None] * np.abs(c["pij"].reshape(-1, k))
        return 2.0 * widths[:, None] * eps * np.add.reduceat(terms, rs[:-1])
    return row_slack


# ------------------------------------------------------------------ running a case

ERK33_STEP2_WEIGHTS = (0.75, -2.0)   # step<2> of ERK33 (time_integrator.template.h:373-403)


def develop(case, oracle):
    """(offline data, Dirichlet data, states, stage weights, tau): the input of the compared update, developed ON THE
    ORACLE. states[-1] is the old state; with stage vectors (step<2> of ERK33, fed as
    test_erk33_stages_with_stage_vectors_share_slices_in_step_6) states[:-1] are the stage vectors -- stages 0 and 1
    run on the oracle -- and tau is the step size of stage 0."""
    import helpers_plan_cases as plan_cases
    from ryujin_amd import HyperbolicModule
    off, U0, dirichlet, after_warm = plan_cases.build(case)
    U_start = plan_cases.warm_up(case, oracle, off, U0, dirichlet, after_warm)
    if case["stages"] == 0:
        return off, dirichlet, [U_start], (), 0.0
    assert case["stages"] == 2
    m = HyperbolicModule(off, plan_cases.params_of(case, oracle, off.dim), backend=oracle.backend())
    v = [m.new_state_vector(U_start), m.new_state_vector(), m.new_state_vector()]
    m.prepare_state_vector(v[0], 0.0, dirichlet)
    tau = m.step(v[0], [], [], v[1])
    m.prepare_state_vector(v[0], 0.0, dirichlet)   # stage vectors are prepared state vectors
    m.prepare_state_vector(v[1], 0.0, dirichlet)
    m.step(v[1], [v[0]], [-1.0], v[2], tau)
    states = [x.download() for x in v]
    m.close()
    return off, dirichlet, states, ERK33_STEP2_WEIGHTS, tau


def modules(case, oracle, off, states, run=0):
    """[(hip module, old, new), (oracle module, old, new)] and the (hip, oracle) stage vectors, all holding `states`;
    run 1: with debug_no_small_mesh_split. The checked case switches the oracle to its checked control flow as well."""
    import helpers_plan_cases as plan_cases
    this = dict(case, edit=lambda p: ((case["edit"](p) if case["edit"] else None), _no_split(p))) if run == 1 else case
    mods = plan_cases.both_backends(this, oracle, off, states[-1])
    stage_vectors = tuple([m.new_state_vector(U) for U in states[:-1]] for m, _, _ in mods)
    if case["plan"]["checked"]:
        oracle.lib().ryujin_oracle_set_expensive_bounds_check(mods[1][0]._ctx, 1)
    return mods, stage_vectors, plan_cases.params_of(this, oracle, off.dim)


def oracle_first_pass(case, oracle, off, dirichlet, states, weights, tau):
    """the oracle's first-pass l_ij of the compared update (after a step with two limiter passes: "lij_next")"""
    import helpers_plan_cases as plan_cases
    from ryujin_amd import HyperbolicModule
    m = HyperbolicModule(off, plan_cases.params_of(case, oracle, off.dim), backend=oracle.backend())
    v = [m.new_state_vector(U) for U in states]
    new = m.new_state_vector()
    for x in v:
        m.prepare_state_vector(x, 0.0, dirichlet)
    m.step(v[-1], v[:-1], list(weights), new, tau)
    assert m.last_status == 0
    l = m.debug_fetch("lij_next")
    m.close()
    return l
