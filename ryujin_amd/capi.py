"""ctypes mirror of include/ryujin_hip.h and include/ryujin_synth.h.

Python is plumbing here (tests, bench.py); the product is libryujin_hip.so.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _build

c_double_p = C.POINTER(C.c_double)
c_u32_p = C.POINTER(C.c_uint32)
c_u64_p = C.POINTER(C.c_uint64)
c_u8_p = C.POINTER(C.c_uint8)
c_int_p = C.POINTER(C.c_int)

RYUJIN_OK, RYUJIN_WARN, RYUJIN_RESTART = 0, 1, 2
RYUJIN_ERR_TAU, RYUJIN_ERR_ARG, RYUJIN_ERR_HIP, RYUJIN_ERR_COMM, RYUJIN_ERR_UNSUPPORTED = -1, -2, -3, -4, -5
EQ_EULER, EQ_SHALLOW_WATER, EQ_EULER_AEOS, EQ_SCALAR_CONSERVATION = 0, 1, 2, 3
FLUX_BURGERS, FLUX_KPP, FLUX_POLYNOMIAL, FLUX_FUNCTION = 0, 1, 2, 3
EOS_POLYTROPIC_GAS, EOS_NOBLE_ABEL_STIFFENED_GAS, EOS_VAN_DER_WAALS, EOS_JONES_WILKINS_LEE = 0, 1, 2, 3
EOS_FUNCTION = 4  # four expressions (ryujin_hip_eos_configure_function)
# the programs of the function equation of state, the `which` of eos_function_evaluate
EOS_PRESSURE, EOS_SPECIFIC_INTERNAL_ENERGY, EOS_TEMPERATURE, EOS_SPEED_OF_SOUND = 0, 1, 2, 3
BC_DO_NOTHING, BC_PERIODIC, BC_SLIP, BC_NO_SLIP, BC_DIRICHLET, BC_DYNAMIC, BC_DIRICHLET_MOMENTUM = range(7)
IDV_WARN, IDV_RAISE_EXCEPTION = 0, 1
CUT_NONE, CUT_BOX, CUT_CYLINDER = 0, 1, 2
SCHEME_SSPRK_22, SCHEME_SSPRK_33, SCHEME_ERK_11, SCHEME_ERK_22, SCHEME_ERK_33, SCHEME_ERK_43, SCHEME_ERK_54 = range(7)
CFL_RECOVERY_NONE, CFL_RECOVERY_BANG_BANG = 0, 1
UNIQUE_ID_BYTES = 128
DEBUG_EULER_RIEMANN, DEBUG_EULER_LIMIT_1D, DEBUG_SW_RIEMANN, DEBUG_EULER_DIJ_2D, DEBUG_EULER_DIJ_3D = range(5)
DEBUG_EULER_DIJ_RECORDS_2D, DEBUG_EULER_DIJ_RECORDS_3D = 5, 6
DEBUG_SW_DIJ_2D, DEBUG_SW_DIJ_RECORDS_2D = 7, 8
DEBUG_EULER_RIEMANN_RECORDS, DEBUG_SW_RIEMANN_RECORDS = 9, 10
DEBUG_AEOS_RIEMANN, DEBUG_AEOS_LIMIT_1D = 11, 12
DEBUG_AEOS_DIJ_2D, DEBUG_AEOS_DIJ_RECORDS_2D = 13, 14
DEBUG_EULER_LIMIT_CHECKED_1D, DEBUG_EULER_LIMIT_2D = 15, 16
DEBUG_EULER_LIMIT_3D, DEBUG_AEOS_LIMIT_2D, DEBUG_AEOS_LIMIT_3D = 17, 18, 19
DEBUG_SW_LIMIT_1D, DEBUG_SW_LIMIT_2D, DEBUG_SCALAR_LIMIT = 20, 21, 22


DIRICHLET_FN = C.CFUNCTYPE(None, C.c_void_p, C.c_double, c_double_p)   # ryujin_hip_dirichlet_fn


class Params(C.Structure):
    _fields_ = [
        ("equation", C.c_int), ("dim", C.c_int),
        ("gamma", C.c_double), ("reference_density", C.c_double),
        ("vacuum_state_relaxation_small", C.c_double), ("vacuum_state_relaxation_large", C.c_double),
        ("gravity", C.c_double), ("manning_friction_coefficient", C.c_double),
        ("reference_water_depth", C.c_double), ("dry_state_relaxation_factor", C.c_double),
        ("dry_state_relaxation_small", C.c_double), ("dry_state_relaxation_large", C.c_double),
        ("cfl", C.c_double), ("id_violation_strategy", C.c_int),
        ("indicator_evc_factor", C.c_double),
        ("limiter_iterations", C.c_int), ("limiter_newton_tolerance", C.c_double),
        ("limiter_newton_max_iterations", C.c_int), ("limiter_relaxation_factor", C.c_double),
        ("limiter_limit_on_kinetic_energy", C.c_int), ("limiter_limit_on_square_velocity", C.c_int),
        ("riemann_newton_max_iterations", C.c_int), ("riemann_newton_tolerance", C.c_double),
        ("eos", C.c_int), ("compute_strict_bounds", C.c_int),
        ("eos_covolume_b", C.c_double), ("eos_q", C.c_double), ("eos_pinf", C.c_double),
        ("eos_vdw_a", C.c_double), ("eos_gas_constant_R", C.c_double),
        ("jwl_A", C.c_double), ("jwl_B", C.c_double), ("jwl_R1", C.c_double), ("jwl_R2", C.c_double),
        ("jwl_omega", C.c_double), ("jwl_rho_0", C.c_double), ("jwl_q_0", C.c_double),
        ("jwl_cv", C.c_double),
        ("sc_flux", C.c_int), ("sc_flux_polynomial", (C.c_double * 4) * 3),
        ("sc_derivative_approximation_delta", C.c_double), ("sc_use_greedy_wavespeed", C.c_int),
        ("sc_use_averaged_entropy", C.c_int), ("sc_random_entropies", C.c_int),
        # run-time switches of the library (no ParameterAcceptor counterpart; 0 = default)
        ("system_scope_events", C.c_int), ("debug_join_exchanges", C.c_int),
        ("debug_bc_fold_max_slices", C.c_int), ("debug_no_small_mesh_split", C.c_int),
        ("debug_pij_storage", C.c_int), ("debug_expensive_bounds_check", C.c_int),
        ("debug_tile_map", C.c_int), ("debug_band_stride", C.c_int),
        ("debug_xcd_chunk", C.c_int), ("debug_stencil_classes", C.c_int),
        ("debug_next_tile_mask", C.c_int),
    ]


class Offline(C.Structure):
    _fields_ = [
        ("n_export", C.c_uint32), ("n_internal", C.c_uint32), ("n_owned", C.c_uint32),
        ("n_relevant", C.c_uint32), ("simd_length", C.c_uint32),
        ("row_starts", c_u64_p), ("columns", c_u32_p), ("cij", c_double_p), ("mij", c_double_p),
        ("mi", c_double_p), ("mi_inv", c_double_p), ("measure_of_omega", C.c_double),
        ("n_bdry", C.c_uint32), ("b_i", c_u32_p), ("b_normal", c_double_p), ("b_id", c_u8_p),
        ("n_pairs", C.c_uint32), ("p_i", c_u32_p), ("p_col", c_u32_p), ("p_j", c_u32_p),
        ("initial_precomputed", c_double_p),
        ("n_nbr", C.c_int), ("nbr_rank", c_int_p), ("send_off", c_u32_p), ("send_idx", c_u32_p),
        ("recv_off", c_u32_p), ("row_send_off", c_u32_p), ("row_send_row", c_u32_p),
        ("row_send_col", c_u32_p),
        ("discontinuous_ansatz", C.c_int), ("incidence", c_double_p), ("mass_matrix_inverse", c_double_p),
    ]


class SynthSpec(C.Structure):
    _fields_ = [
        ("dim", C.c_int), ("n_cells", C.c_uint32 * 3), ("lower", C.c_double * 3),
        ("upper", C.c_double * 3), ("bc", C.c_int * 6), ("cut_kind", C.c_int),
        ("cut_lo", C.c_double * 3), ("cut_hi", C.c_double * 3), ("cyl_center", C.c_double * 2),
        ("cyl_radius", C.c_double), ("cut_bc", C.c_int), ("n_ranks", C.c_int), ("rank", C.c_int),
    ]


PP_SCHLIEREN, PP_VORTICITY = 0, 1
PP_MAX_QUANTITIES = 8
Q_INSTANTANEOUS, Q_TIME_AVERAGED, Q_SPACE_AVERAGED = 1, 2, 4
Q_MAX_MANIFOLDS = 16
Q_NONE_YET = 3
EN_MAX_DOFS_PER_CELL, EN_MAX_POINTS, EN_MAX_COMPONENTS = 27, 64, 5
OUT_MAX_QUANTITIES, OUT_MAX_MANIFOLDS = 32, 8
OUT_FLOAT32, OUT_FLOAT64 = 0, 1


class PostprocessQuantity(C.Structure):
    _fields_ = [("kind", C.c_int), ("is_primitive", C.c_int), ("component", C.c_int)]


# InitialValues (RYUJIN_IV_*): the analytic states of ryujin_hip_initial_values_configure
(IV_UNIFORM, IV_RADIAL_CONTRAST, IV_ISENTROPIC_VORTEX, IV_LEBLANC, IV_RAREFACTION, IV_CIRCULAR_DAM_BREAK,
 IV_PARABOLOID, IV_RITTER_DAM_BREAK, IV_SMOOTH_VORTEX, IV_SLOPING_FRICTION) = range(10)


class InitialValues(C.Structure):
    """ryujin_hip_initial_values"""
    _fields_ = [("state", C.c_int), ("params", C.c_double * 16), ("direction", C.c_double * 3),
                ("position", C.c_double * 3), ("perturbation", C.c_double)]


# configuration name (subsection "E - InitialValues") -> (RYUJIN_IV_*, shallow water?, parameters); a parameter is
# (the reference's name, first slot of ryujin_hip_initial_values::params, default -- a tuple fills consecutive
# slots). "gamma" is a parameter of the state for EulerAEOS only (Euler takes the system's).
IV_STATES = {
    "uniform": (IV_UNIFORM, False, (("primitive state", 0, (1.4, 3.0, 1.0)),)),
    "radial contrast": (IV_RADIAL_CONTRAST, False, (("primitive state inner", 0, (1.0, 0.0, 100.0)),
                                                    ("primitive state outer", 3, (1.0, 0.0, 0.1)),
                                                    ("radius", 6, 0.5))),
    "isentropic vortex": (IV_ISENTROPIC_VORTEX, False, (("mach number", 0, 2.0), ("beta", 1, 5.0),
                                                        ("gamma", 2, 1.4))),
    "leblanc": (IV_LEBLANC, False, ()),
    "rarefaction": (IV_RAREFACTION, False, (("gamma", 0, 1.4),)),
    "circular dam break": (IV_CIRCULAR_DAM_BREAK, True, (("still water depth", 0, 0.5), ("radius", 1, 2.5),
                                                         ("dam amplitude", 2, 2.5))),
    "paraboloid": (IV_PARABOLOID, True, (("free surface radius", 0, 1.0), ("water height", 1, 0.1),
                                         ("paraboloid length", 2, 10000.0), ("speed", 3, 2.0))),
    "ritter dam break": (IV_RITTER_DAM_BREAK, True, (("time initial", 0, 0.1), ("left water depth", 1, 0.005))),
    "smooth vortex": (IV_SMOOTH_VORTEX, True, (("reference depth", 0, 1.0), ("mach number", 1, 2.0),
                                               ("beta", 2, 0.1))),
    "sloping friction": (IV_SLOPING_FRICTION, True, (("ramp slope", 0, 1.0), ("initial discharge", 1, 0.1))),
}


# The Riemann-data, shock-front, ramp-up and Noh states (RYUJIN_IV_* from 11 on; 10 is the library's own id of the
# "function" state and refused by ryujin_hip_initial_values_configure). "contrast" and "uniform" exist in two
# Descriptions, so the key carries the family: ("euler", name) serves Euler and EulerAEOS, ("shallow water", name)
# shallow water. Value: (RYUJIN_IV_*, parameters) with the parameters as in IV_STATES.
(IV_CONTRAST, IV_THREE_STATE_CONTRAST, IV_FOUR_STATE_CONTRAST, IV_SHOCK_FRONT, IV_RAMP_UP, IV_NOH, IV_SMOOTH_WAVE,
 IV_ASTRO_JET, IV_SW_UNIFORM, IV_SW_CONTRAST) = range(11, 21)

IV_LIBRARY_STATES = {
    ("euler", "contrast"): (IV_CONTRAST, (("primitive state left", 0, (1.4, 0.0, 1.0)),
                                         ("primitive state right", 3, (1.4, 0.0, 1.0)))),
    ("euler", "three state contrast"): (IV_THREE_STATE_CONTRAST, (
        ("primitive state left", 0, (1.0, 0.0, 1.0e3)), ("left region length", 3, 0.1),
        ("primitive state middle", 4, (1.0, 0.0, 1.0e-2)), ("middle region length", 7, 0.8),
        ("primitive state right", 8, (1.0, 0.0, 1.0e2)))),
    ("euler", "four state contrast"): (IV_FOUR_STATE_CONTRAST, (
        ("primitive state bottom left", 0, (1.4, 0.0, 0.0, 1.0)), ("primitive state bottom right", 4, (1.4, 0.0, 0.0, 1.0)),
        ("primitive state top left", 8, (1.4, 0.0, 0.0, 1.0)), ("primitive state top right", 12, (1.4, 0.0, 0.0, 1.0)))),
    ("euler", "shock front"): (IV_SHOCK_FRONT, (("primitive state", 0, (1.4, 0.0, 1.0)), ("mach number", 3, 2.0),
                                               ("gamma", 4, 1.4))),
    ("euler", "ramp up"): (IV_RAMP_UP, (("primitive state initial", 0, (1.4, 0.0, 1.0)),
                                       ("primitive state final", 3, (1.4, 3.0, 1.0)),
                                       ("time initial", 6, 0.0), ("time final", 7, 1.0))),
    ("euler", "noh"): (IV_NOH, (("reference density", 0, 1.0), ("reference velocity magnitude", 1, 1.0),
                               ("reference pressure", 2, 1.0e-12), ("gamma", 3, 1.4))),
    ("euler", "smooth wave"): (IV_SMOOTH_WAVE, (("reference density", 0, 1.0), ("reference pressure", 1, 1.0),
                                               ("mach number", 2, 1.0))),
    ("euler", "astro jet"): (IV_ASTRO_JET, (("jet width", 0, 0.05), ("primitive jet state", 1, (5.0, 30.0, 0.4127)),
                                           ("primitive ambient right", 4, (5.0, 0.0, 0.4127)),
                                           ("gamma", 7, 5.0 / 3.0))),
    ("shallow water", "uniform"): (IV_SW_UNIFORM, (("primitive state", 0, (1.0, 1.0)),)),
    ("shallow water", "contrast"): (IV_SW_CONTRAST, (("primitive state left", 0, (1.0, 0.0)),
                                                    ("primitive state right", 2, (1.0, 0.0)))),
}


# The shallow-water states that bring their own bathymetry (RYUJIN_IV_* from 21 on), keyed like IV_LIBRARY_STATES. A
# selector parameter -- a string or a boolean of the reference -- has a fourth entry: its values in slot order, the
# slot holds the index; the fifth is the reference's message for any other string.
(IV_SW_FLOW_OVER_BUMP, IV_SW_THREE_BUMPS_DAM_BREAK, IV_SW_HOU_TEST, IV_SW_TRANSIENT, IV_SW_SOLITON) = range(21, 26)

IV_BATHYMETRY_STATES = {
    ("shallow water", "flow over bump"): (IV_SW_FLOW_OVER_BUMP, (
        ("flow type", 0, "transcritical", ("transcritical", "subsonic"),
         "Flow type must be 'transcritical' or 'subsonic'. "),)),
    ("shallow water", "three bumps dam break"): (IV_SW_THREE_BUMPS_DAM_BREAK, (
        ("well balancing validation", 0, False, (False, True), "\"well balancing validation\" takes a boolean"),
        ("left water depth", 1, 1.875), ("right water depth", 2, 0.0), ("cone magnitude", 3, 1.0))),
    ("shallow water", "hou test"): (IV_SW_HOU_TEST, (("reservoir water depth", 0, 35.0),)),
    ("shallow water", "transient experiments"): (IV_SW_TRANSIENT, (
        ("flow state left", 0, (1.0, 0.0)), ("flow state right", 2, (1.0, 0.0)),
        ("experimental configuration", 4, "G1", ("G1", "G2", "G3", "none"),
         "Case must be 'G1', 'G2', 'G3' or 'none'"))),
    ("shallow water", "soliton"): (IV_SW_SOLITON, (("still water depth", 0, 1.0), ("amplitude", 1, 0.1))),
}


def iv_selector_slot(pname: str, value, choices, message: str) -> float:
    """the slot value of a selector parameter: the index of a string or boolean of the reference among `choices`, or
    a number that is passed on as it is (the library refuses what is none of the indices)"""
    if isinstance(value, (str, bool, np.bool_)):
        value = bool(value) if isinstance(value, np.bool_) else value
        if isinstance(value, type(choices[0])) and value in choices:
            return float(choices.index(value))
        raise ValueError(message)
    return float(value)


def iv_family(equation: int) -> str:
    """the first entry of an IV_LIBRARY_STATES key for an EQ_* value"""
    if equation in (EQ_EULER, EQ_EULER_AEOS):
        return "euler"
    if equation == EQ_SHALLOW_WATER:
        return "shallow water"
    return "scalar conservation"


def initial_values_struct(name: str, dim: int, direction=None, position=None, perturbation: float = 0.0,
                          equation=None, **params) -> InitialValues:
    """ryujin_hip_initial_values for a configuration name of the reference with its parameter names (spaces may be
    written as underscores: mach_number=1.0); what is not given takes the reference's default. ValueError for an
    unknown configuration or parameter. `equation` (EQ_*) selects among the states of that Description first
    (IV_LIBRARY_STATES: "uniform" of shallow water is another state than "uniform" of Euler), then in IV_STATES, then
    among the IV_LIBRARY_STATES of the other Descriptions (which the library refuses); without it the name is looked
    up in IV_STATES alone."""
    key = (iv_family(equation), name) if equation is not None else None
    if key in IV_LIBRARY_STATES:
        state, spec = IV_LIBRARY_STATES[key]
    elif key in IV_BATHYMETRY_STATES:
        state, spec = IV_BATHYMETRY_STATES[key]
    elif name in IV_STATES:
        state, _, spec = IV_STATES[name]
    else:
        # a state of another Description only: the struct is built, the library refuses it with its own status
        tables = {**IV_LIBRARY_STATES, **IV_BATHYMETRY_STATES}
        other = [k for k in tables if k[1] == name] if equation is not None else []
        if not other:
            raise ValueError(f"Could not find an initial state description with name \"{name}\"")
        state, spec = tables[other[0]]
    iv = InitialValues()
    iv.state = state
    given = {k.replace("_", " "): v for k, v in params.items()}
    for pname, slot, default, *selector in spec:
        value = given.pop(pname, default)
        if selector:
            iv.params[slot] = iv_selector_slot(pname, value, *selector)
            continue
        values = tuple(value) if isinstance(default, tuple) else (value,)
        if len(values) != (len(default) if isinstance(default, tuple) else 1):
            raise ValueError(f"parameter \"{pname}\" of \"{name}\" takes {len(default)} values")
        for q, v in enumerate(values):
            iv.params[slot + q] = float(v)
    if given:
        raise ValueError(f"\"{name}\" has no parameter {sorted(given)}")
    d = (1.0,) + (0.0,) * (dim - 1) if direction is None else tuple(np.atleast_1d(direction).astype(float))
    x = (0.0,) * dim if position is None else tuple(np.atleast_1d(position).astype(float))
    if len(d) != dim or len(x) != dim:
        raise ValueError(f"direction and position take {dim} components")
    for q in range(dim):
        iv.direction[q], iv.position[q] = d[q], x[q]
    iv.perturbation = float(perturbation)
    return iv


# The function state (configuration = function of the reference): the parameter names of its expressions in primitive
# order and the reference's defaults (source/<eq>/initial_state_function.h).
EXPR_MAX_INSTRUCTIONS, EXPR_MAX_STACK = 256, 16


def function_expression_names(equation: int, dim: int) -> tuple[tuple[str, str], ...]:
    """((parameter name, default expression), ...) of the "function" state of a Description, in primitive order"""
    velocity = tuple((f"velocity {a} expression", d) for a, d in zip("xyz"[:dim], ("3.0", "0.0", "0.0")))
    if equation in (EQ_EULER, EQ_EULER_AEOS):
        return (("density expression", "1.4"), *velocity, ("pressure expression", "1.0"))
    if equation == EQ_SHALLOW_WATER:
        return (("water depth expression", "1.4"), *velocity)
    if equation == EQ_SCALAR_CONSERVATION:
        return (("expression", "0.25 * x"),)
    raise ValueError(f"unknown equation {equation}")


def function_expressions(equation: int, dim: int, expressions) -> tuple[str, ...]:
    """The expressions of the "function" state in primitive order from a sequence in that order, or from a dict keyed
    by the reference's parameter names (spaces may be written as underscores) in which a missing key takes the
    reference's default. ValueError for a wrong count or an unknown key."""
    names = function_expression_names(equation, dim)
    if isinstance(expressions, str):
        expressions = (expressions,)
    if isinstance(expressions, dict):
        given = {k.replace("_", " "): v for k, v in expressions.items()}
        out = tuple(str(given.pop(name, default)) for name, default in names)
        if given:
            raise ValueError(f"the function state has no parameter {sorted(given)}")
        return out
    out = tuple(str(e) for e in expressions)
    if len(out) != len(names):
        raise ValueError(f"the function state takes {len(names)} expressions: {[n for n, _ in names]}")
    return out


def expression_evaluate(expr: str, dim: int, points, t: float) -> np.ndarray:
    """[n]: the expression over the first `dim` of x y z, then t, at points [n, dim], through the library's host
    interpreter (ryujin_hip_expression_evaluate; no device). RuntimeError with .status for a refused expression."""
    lib = load_hip()
    points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, dim)
    out = np.zeros(points.shape[0], dtype=np.float64)
    rc = lib.ryujin_hip_expression_evaluate(expr.encode(), dim, as_ptr(points, c_double_p) if points.size else None,
                                            points.shape[0], float(t), as_ptr(out, c_double_p) if out.size else None)
    if rc < 0:
        error = RuntimeError(f"ryujin_hip_expression_evaluate failed with status {rc}: "
                             f"{lib.ryujin_hip_last_error().decode()}")
        error.status = rc
        raise error
    return out


def flux_function_evaluate(expr: str, dim: int, u, delta: float = 1e-10, gradient: bool = True):
    """(value [n, dim], gradient [n, dim] or None) of the function flux `expr` -- one string in u, `dim` components
    separated by ';' -- at the states u [n], through the library's host interpreter
    (ryujin_hip_flux_function_evaluate; no device). RuntimeError with .status for a refused expression."""
    lib = load_hip()
    u = np.ascontiguousarray(u, dtype=np.float64).reshape(-1)
    value = np.zeros((u.size, dim), dtype=np.float64)
    grad = np.zeros((u.size, dim), dtype=np.float64) if gradient else None
    rc = lib.ryujin_hip_flux_function_evaluate(expr.encode(), dim, float(delta),
                                               as_ptr(u, c_double_p) if u.size else None, u.size,
                                               as_ptr(value, c_double_p) if value.size else None,
                                               as_ptr(grad, c_double_p) if gradient and grad.size else None)
    if rc < 0:
        error = RuntimeError(f"ryujin_hip_flux_function_evaluate failed with status {rc}: "
                             f"{lib.ryujin_hip_last_error().decode()}")
        error.status = rc
        raise error
    return value, grad


def eos_function_evaluate(which: int, expr, rho, second) -> np.ndarray:
    """[n]: function `which` (EOS_PRESSURE, ...) of the function equation of state given as the expression `expr`
    (None: the reference's default) at (rho [n], second [n]) -- second is e, or p for the specific internal energy --
    through the library's host interpreter (ryujin_hip_eos_function_evaluate; no device). RuntimeError with .status
    for a refused expression."""
    lib = load_hip()
    rho = np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
    second = np.ascontiguousarray(second, dtype=np.float64).reshape(-1)
    if rho.size != second.size:
        raise ValueError("rho and the second variable take the same number of points")
    out = np.zeros(rho.size, dtype=np.float64)
    rc = lib.ryujin_hip_eos_function_evaluate(int(which), None if expr is None else str(expr).encode(),
                                              as_ptr(rho, c_double_p) if rho.size else None,
                                              as_ptr(second, c_double_p) if rho.size else None, rho.size,
                                              as_ptr(out, c_double_p) if rho.size else None)
    if rc < 0:
        error = RuntimeError(f"ryujin_hip_eos_function_evaluate failed with status {rc}: "
                             f"{lib.ryujin_hip_last_error().decode()}")
        error.status = rc
        raise error
    return out


def component_names(equation: int, dim: int) -> tuple[tuple[str, ...], tuple[str, ...]]:
    """(View::component_names, View::primitive_component_names) of a Description
    (source/<eq>/hyperbolic_system.h)."""
    def vec(name: str) -> tuple[str, ...]:
        return (name,) if dim == 1 else tuple(f"{name}_{d + 1}" for d in range(dim))
    if equation == EQ_EULER:
        return ("rho", *vec("m"), "E"), ("rho", *vec("v"), "p")
    if equation == EQ_EULER_AEOS:
        return ("rho", *vec("m"), "E"), ("rho", *vec("v"), "e")
    if equation == EQ_SHALLOW_WATER:
        return ("h", *vec("m")), ("h", *vec("v"))
    if equation == EQ_SCALAR_CONSERVATION:
        return ("u",), ("u",)
    raise ValueError(f"unknown equation {equation}")


def output_names(equation: int, dim: int) -> dict:
    """The name tables of "vtu output quantities" (source/<eq>/hyperbolic_system.h): conserved, primitive, precomputed
    and initial_precomputed names of a Description, as ryujin_amd/csrc/output_selection.hpp holds them."""
    conserved, primitive = component_names(equation, dim)

    def vec(name: str) -> tuple[str, ...]:
        return (name,) if dim == 1 else tuple(f"{name}_{d + 1}" for d in range(dim))
    precomputed = {EQ_EULER: ("s", "eta_h"),
                   EQ_EULER_AEOS: ("p", "surrogate_gamma", "surrogate_specific_entropy", "surrogate_harten_entropy"),
                   EQ_SHALLOW_WATER: ("eta_m", "h_star"),
                   EQ_SCALAR_CONSERVATION: (*vec("f"), *vec("df"))}[equation]
    initial = ("bathymetry",) if equation == EQ_SHALLOW_WATER else ()
    return dict(conserved=conserved, primitive=primitive, precomputed=precomputed, initial_precomputed=initial)


def resolve_component(equation: int, dim: int, name: str) -> tuple[int, int]:
    """(is_primitive, index) of a component name: the conserved names first, the primitive names second, as
    Postprocessor::prepare() (source/postprocessor.template.h:73-93); ValueError for an unknown name."""
    for is_primitive, names in enumerate(component_names(equation, dim)):
        if name in names:
            return is_primitive, names.index(name)
    raise ValueError(f"Invalid component name »{name}«")


def as_ptr(a: np.ndarray, typ):
    return a.ctypes.data_as(typ)


def np_from_ptr(ptr, n: int, dtype) -> np.ndarray:
    """Copy n items from a ctypes pointer into a fresh numpy array."""
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


# --------------------------------------------------------------------------- synth

_synth = None


def load_synth():
    global _synth
    if _synth is None:
        path = os.environ.get("RYUJIN_SYNTH_LIB", _build.SYNTH_SO)  # (the sanitizer builds: scripts/sanitizer_run.sh)
        if not os.path.exists(path):
            _build.build_synth()
        lib = C.CDLL(path)
        lib.ryujin_synth_build.restype = C.c_void_p
        lib.ryujin_synth_build.argtypes = [C.POINTER(SynthSpec)]
        lib.ryujin_synth_free.argtypes = [C.c_void_p]
        lib.ryujin_synth_last_error.restype = C.c_char_p
        lib.ryujin_synth_offline.restype = C.POINTER(Offline)
        lib.ryujin_synth_offline.argtypes = [C.c_void_p]
        lib.ryujin_synth_nnz.restype = C.c_uint64
        lib.ryujin_synth_nnz.argtypes = [C.c_void_p]
        lib.ryujin_synth_n_global.restype = C.c_uint64
        lib.ryujin_synth_n_global.argtypes = [C.c_void_p]
        lib.ryujin_synth_positions.restype = c_double_p
        lib.ryujin_synth_positions.argtypes = [C.c_void_p]
        lib.ryujin_synth_global_ids.restype = c_u64_p
        lib.ryujin_synth_global_ids.argtypes = [C.c_void_p]
        lib.ryujin_synth_bdry_positions.restype = c_double_p
        lib.ryujin_synth_bdry_positions.argtypes = [C.c_void_p]
        lib.ryujin_synth_bdry_mass.restype = c_double_p
        lib.ryujin_synth_bdry_mass.argtypes = [C.c_void_p]
        lib.ryujin_synth_n_cells.restype = C.c_uint64
        lib.ryujin_synth_n_cells.argtypes = [C.c_void_p]
        lib.ryujin_synth_cells.restype = c_u32_p
        lib.ryujin_synth_cells.argtypes = [C.c_void_p]
        lib.ryujin_synth_ghost_row_send_entries.restype = C.c_size_t
        lib.ryujin_synth_ghost_row_send_entries.argtypes = [c_u64_p, c_u32_p, c_u32_p, C.c_size_t, C.c_uint32,
                                                            C.c_uint32, c_u32_p, c_u32_p]
        # OfflineData dumps (include/ryujin_offline_io.h)
        lib.ryujin_offline_write.restype = C.c_int
        lib.ryujin_offline_write.argtypes = [C.c_char_p, C.POINTER(Offline), C.c_int, C.c_int, c_double_p,
                                             c_double_p]
        lib.ryujin_offline_read.restype = C.c_void_p
        lib.ryujin_offline_read.argtypes = [C.c_char_p]
        lib.ryujin_offline_file_free.argtypes = [C.c_void_p]
        lib.ryujin_offline_io_last_error.restype = C.c_char_p
        lib.ryujin_offline_file_view.restype = C.POINTER(Offline)
        lib.ryujin_offline_file_view.argtypes = [C.c_void_p]
        lib.ryujin_offline_file_dim.argtypes = [C.c_void_p]
        lib.ryujin_offline_file_n_initial_precomputed.argtypes = [C.c_void_p]
        lib.ryujin_offline_file_nnz.restype = C.c_uint64
        lib.ryujin_offline_file_nnz.argtypes = [C.c_void_p]
        lib.ryujin_offline_file_positions.restype = c_double_p
        lib.ryujin_offline_file_positions.argtypes = [C.c_void_p]
        lib.ryujin_offline_file_b_positions.restype = c_double_p
        lib.ryujin_offline_file_b_positions.argtypes = [C.c_void_p]
        _synth = lib
    return _synth


# --------------------------------------------------------------------------- hip

HIP_SYMBOLS = [
    "ryujin_hip_comm_unique_id", "ryujin_hip_comm_init", "ryujin_hip_comm_init_local",
    "ryujin_hip_comm_init_loopback",
    "ryujin_hip_comm_destroy", "ryujin_hip_comm_info", "ryujin_hip_exchange_info", "ryujin_hip_device_count",
    "ryujin_hip_time_step_fn", "ryujin_hip_debug_addresses",
    "ryujin_hip_host_register", "ryujin_hip_host_unregister", "ryujin_hip_state_download_owned",
    "ryujin_hip_state_download_prepared", "ryujin_hip_layout_info", "ryujin_hip_chain_info", "ryujin_hip_stencil_class_info", "ryujin_hip_tile_statistics",
    "ryujin_hip_next_tile_mask_info", "ryujin_hip_debug_fill",
    "ryujin_hip_default_params", "ryujin_hip_create", "ryujin_hip_destroy",
    "ryujin_hip_state_alloc", "ryujin_hip_state_free", "ryujin_hip_state_upload",
    "ryujin_hip_state_download", "ryujin_hip_state_download_precomputed", "ryujin_hip_state_integrals",
    "ryujin_hip_prepare_state_vector", "ryujin_hip_step", "ryujin_hip_sadd", "ryujin_hip_time_step", "ryujin_hip_time_step_n",
    "ryujin_hip_get_timers_accum",
    "ryujin_hip_set_cfl", "ryujin_hip_get_cfl", "ryujin_hip_set_id_violation_strategy",
    "ryujin_hip_get_alpha", "ryujin_hip_get_counters", "ryujin_hip_limiter_statistics", "ryujin_hip_debug_fetch", "ryujin_hip_debug_plan",
    "ryujin_hip_set_timers", "ryujin_hip_get_timers", "ryujin_hip_synchronize",
    "ryujin_hip_event_record", "ryujin_hip_event_elapsed_ms", "ryujin_hip_last_error",
    "ryujin_hip_version", "ryujin_hip_debug_layout", "ryujin_hip_debug_pow", "ryujin_hip_debug_function", "ryujin_hip_debug_rk_outcome",
    "ryujin_hip_postprocess_configure", "ryujin_hip_postprocess_compute", "ryujin_hip_postprocess_download",
    "ryujin_hip_postprocess_bounds",
    "ryujin_hip_quantities_add_manifold", "ryujin_hip_quantities_reset", "ryujin_hip_quantities_clear_statistics",
    "ryujin_hip_quantities_accumulate", "ryujin_hip_quantities_instantaneous", "ryujin_hip_quantities_time_averaged",
    "ryujin_hip_quantities_time_series",
    "ryujin_hip_initial_values_configure", "ryujin_hip_initial_values_evaluate",
    "ryujin_hip_initial_values_interpolate", "ryujin_hip_prepare_state_vector_iv", "ryujin_hip_time_step_iv",
    "ryujin_hip_initial_values_configure_function", "ryujin_hip_expression_evaluate",
    "ryujin_hip_initial_values_interpolate_initial_precomputed",
    "ryujin_hip_initial_values_evaluate_initial_precomputed", "ryujin_hip_get_initial_precomputed",
    "ryujin_hip_error_norms_configure", "ryujin_hip_error_norms_compute",
    "ryujin_hip_flux_configure_function", "ryujin_hip_flux_function_evaluate", "ryujin_hip_flux_info",
    "ryujin_hip_eos_configure_function", "ryujin_hip_eos_function_evaluate",
    "ryujin_hip_eos_function_evaluate_device", "ryujin_hip_eos_info",
    "ryujin_hip_output_configure", "ryujin_hip_output_info", "ryujin_hip_output_selection",
    "ryujin_hip_output_levelset_values", "ryujin_hip_output_extract",
]


def _declare_module_api(lib, prefix: str):
    """Declare argtypes of the HyperbolicModule C ABI on `lib` (same signatures for the HIP
    library, prefix 'ryujin_hip_', and the CPU oracle, prefix 'ryujin_oracle_')."""
    p = lambda n: getattr(lib, prefix + n)  # noqa: E731
    vp = C.c_void_p
    p("default_params").argtypes = [C.POINTER(Params), C.c_int, C.c_int]
    p("default_params").restype = None
    p("create").argtypes = [C.POINTER(vp), C.POINTER(Offline), C.POINTER(Params), vp, C.c_int]
    p("destroy").argtypes = [vp]
    p("destroy").restype = None
    p("state_alloc").argtypes = [vp, c_int_p]
    p("state_free").argtypes = [vp, C.c_int]
    p("state_upload").argtypes = [vp, C.c_int, c_double_p]
    p("state_download").argtypes = [vp, C.c_int, c_double_p]
    p("state_download_precomputed").argtypes = [vp, C.c_int, c_double_p]
    if hasattr(lib, prefix + "state_integrals"):  # device library only
        p("state_integrals").argtypes = [vp, C.c_int, c_double_p]
    p("prepare_state_vector").argtypes = [vp, C.c_int, C.c_double, c_double_p]
    p("step").argtypes = [vp, C.c_int, C.c_int, c_int_p, c_double_p, C.c_int, C.c_double,
                          C.c_double, c_double_p]
    p("sadd").argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_int]
    p("set_cfl").argtypes = [vp, C.c_double]
    p("get_cfl").argtypes = [vp, c_double_p]
    p("set_id_violation_strategy").argtypes = [vp, C.c_int]
    p("get_alpha").argtypes = [vp, c_double_p]
    p("get_counters").argtypes = [vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    p("debug_fetch").argtypes = [vp, C.c_int, c_double_p, C.c_size_t]
    p("last_error").restype = C.c_char_p


_hip = None


def load_hip():
    """Load the HIP library. Fails loudly if it is missing: there is no CPU fallback."""
    global _hip
    if _hip is None:
        path = os.environ.get("RYUJIN_HIP_LIB", _build.HIP_SO)  # A/B variants of the same library
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build it with `python -m ryujin_amd._build` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback for the product path.")
        lib = C.CDLL(path, mode=C.RTLD_GLOBAL)
        _declare_module_api(lib, "ryujin_hip_")
        vp = C.c_void_p
        lib.ryujin_hip_comm_unique_id.argtypes = [C.c_char_p]
        lib.ryujin_hip_comm_init.argtypes = [C.POINTER(vp), C.c_char_p, C.c_int, C.c_int, C.c_int]
        lib.ryujin_hip_comm_init_local.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
        lib.ryujin_hip_comm_init_loopback.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int]
        lib.ryujin_hip_comm_destroy.argtypes = [vp]
        lib.ryujin_hip_comm_destroy.restype = None
        lib.ryujin_hip_comm_info.argtypes = [vp, c_int_p, c_int_p, c_int_p, c_int_p, c_int_p]
        lib.ryujin_hip_exchange_info.argtypes = [vp, c_int_p, c_int_p, C.c_int, C.POINTER(C.c_ulonglong),
                                                 C.POINTER(C.c_ulonglong)]
        lib.ryujin_hip_set_timers.argtypes = [vp, C.c_int]
        lib.ryujin_hip_get_timers.argtypes = [vp, c_double_p]
        lib.ryujin_hip_get_timers_accum.argtypes = [vp, c_double_p, C.POINTER(C.c_uint), C.c_int]
        lib.ryujin_hip_time_step.argtypes = [vp, C.c_int, C.c_int, c_int_p, c_double_p, C.c_double, C.c_int,
                                             C.c_double, C.c_double, c_double_p]
        lib.ryujin_hip_time_step_n.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_int_p, c_double_p, C.c_double,
                                               C.c_int, C.c_double, C.c_double, c_double_p]
        lib.ryujin_hip_time_step_fn.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_int_p, C.c_double, DIRICHLET_FN,
                                                C.c_void_p, C.c_double, C.c_int, C.c_double, C.c_double, c_double_p]
        lib.ryujin_hip_device_count.argtypes = [c_int_p]
        lib.ryujin_hip_layout_info.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
        lib.ryujin_hip_chain_info.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
        if hasattr(lib, "ryujin_hip_stencil_class_info"):  # (A/B libraries of earlier trees do not have it)
            lib.ryujin_hip_stencil_class_info.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong),
                                                          C.POINTER(C.c_double)]
        if hasattr(lib, "ryujin_hip_debug_fill"):
            lib.ryujin_hip_debug_fill.argtypes = [vp, C.c_int, C.c_double]
        if hasattr(lib, "ryujin_hip_next_tile_mask_info"):  # (A/B libraries of earlier trees do not have it)
            lib.ryujin_hip_next_tile_mask_info.argtypes = [vp, c_int_p, C.POINTER(C.c_ulonglong),
                                                           C.POINTER(C.c_ulonglong)]
        lib.ryujin_hip_tile_statistics.argtypes = [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        lib.ryujin_hip_host_register.argtypes = [vp, C.c_void_p, C.c_size_t]
        lib.ryujin_hip_host_unregister.argtypes = [vp, C.c_void_p]
        lib.ryujin_hip_state_download_owned.argtypes = [vp, C.c_int, c_double_p]
        lib.ryujin_hip_state_download_prepared.argtypes = [vp, C.c_int, c_double_p]
        lib.ryujin_hip_debug_addresses.argtypes = [vp, c_u64_p]
        lib.ryujin_hip_debug_plan.argtypes = [vp, c_int_p, C.c_int]
        lib.ryujin_hip_synchronize.argtypes = [vp]
        lib.ryujin_hip_event_record.argtypes = [vp, C.c_int]
        lib.ryujin_hip_event_elapsed_ms.argtypes = [vp, c_double_p]
        lib.ryujin_hip_version.restype = C.c_char_p
        lib.ryujin_hip_debug_layout.argtypes = [C.POINTER(Offline), c_u64_p, c_u32_p, c_u64_p,
                                                c_double_p, C.c_uint32, c_double_p]
        lib.ryujin_hip_debug_pow.argtypes = [C.c_int, c_double_p, c_double_p, c_double_p, C.c_size_t]
        lib.ryujin_hip_debug_rk_outcome.argtypes = [C.c_int, C.c_int, C.c_int]
        lib.ryujin_hip_debug_function.argtypes = [C.c_int, C.POINTER(Params), C.c_int, c_double_p, c_double_p,
                                                  C.c_size_t]
        lib.ryujin_hip_postprocess_configure.argtypes = [vp, C.c_int, C.POINTER(PostprocessQuantity), C.c_double,
                                                         C.c_int]
        lib.ryujin_hip_postprocess_compute.argtypes = [vp, C.c_int]
        lib.ryujin_hip_postprocess_download.argtypes = [vp, C.c_int, c_double_p, C.c_int]
        lib.ryujin_hip_postprocess_bounds.argtypes = [vp, C.c_int, c_double_p, c_double_p]
        lib.ryujin_hip_quantities_add_manifold.argtypes = [vp, C.c_uint32, c_u32_p, c_double_p, C.c_int, c_int_p]
        lib.ryujin_hip_quantities_reset.argtypes = [vp]
        lib.ryujin_hip_quantities_clear_statistics.argtypes = [vp]
        lib.ryujin_hip_quantities_accumulate.argtypes = [vp, C.c_int, C.c_double]
        lib.ryujin_hip_quantities_instantaneous.argtypes = [vp, C.c_int, C.c_int, C.c_double, c_double_p]
        lib.ryujin_hip_quantities_time_averaged.argtypes = [vp, C.c_int, c_double_p, c_double_p, c_double_p]
        lib.ryujin_hip_quantities_time_series.argtypes = [vp, C.c_int, c_double_p, C.c_size_t,
                                                          C.POINTER(C.c_size_t), C.c_int]
        lib.ryujin_hip_initial_values_configure.argtypes = [vp, C.POINTER(InitialValues), c_double_p, c_double_p]
        lib.ryujin_hip_initial_values_evaluate.argtypes = [vp, c_double_p, C.c_size_t, C.c_double, c_double_p]
        lib.ryujin_hip_initial_values_interpolate.argtypes = [vp, C.c_int, C.c_double]
        lib.ryujin_hip_initial_values_interpolate_initial_precomputed.argtypes = [vp]
        lib.ryujin_hip_initial_values_evaluate_initial_precomputed.argtypes = [vp, c_double_p, C.c_size_t, c_double_p]
        lib.ryujin_hip_get_initial_precomputed.argtypes = [vp, c_double_p]
        lib.ryujin_hip_prepare_state_vector_iv.argtypes = [vp, C.c_int, C.c_double]
        lib.ryujin_hip_time_step_iv.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_int_p, C.c_double, C.c_double,
                                                C.c_int, C.c_double, C.c_double, c_double_p]
        lib.ryujin_hip_initial_values_configure_function.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), c_double_p,
                                                                     c_double_p, c_double_p, c_double_p]
        lib.ryujin_hip_expression_evaluate.argtypes = [C.c_char_p, C.c_int, c_double_p, C.c_size_t, C.c_double,
                                                       c_double_p]
        lib.ryujin_hip_error_norms_configure.argtypes = [vp, C.c_uint32, C.c_int, c_u32_p, C.c_int, c_double_p,
                                                         c_double_p, c_double_p, C.c_int]
        lib.ryujin_hip_error_norms_compute.argtypes = [vp, C.c_int, C.c_int, C.c_int, c_int_p, C.c_int, c_double_p,
                                                       c_double_p]
        lib.ryujin_hip_flux_configure_function.argtypes = [vp, C.c_char_p, C.c_double]
        lib.ryujin_hip_flux_function_evaluate.argtypes = [C.c_char_p, C.c_int, C.c_double, c_double_p, C.c_size_t,
                                                          c_double_p, c_double_p]
        lib.ryujin_hip_flux_info.argtypes = [vp, c_int_p, c_int_p, c_int_p]
        lib.ryujin_hip_eos_configure_function.argtypes = [vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p,
                                                          C.c_double, C.c_double, C.c_double]
        lib.ryujin_hip_eos_function_evaluate.argtypes = [C.c_int, C.c_char_p, c_double_p, c_double_p, C.c_size_t,
                                                         c_double_p]
        lib.ryujin_hip_eos_function_evaluate_device.argtypes = [vp, C.c_int, c_double_p, c_double_p, C.c_size_t,
                                                                c_double_p]
        lib.ryujin_hip_eos_info.argtypes = [vp, c_int_p, c_int_p, c_int_p]
        lib.ryujin_hip_output_configure.argtypes = [vp, C.c_int, C.POINTER(C.c_char_p), c_double_p, C.c_uint32, C.c_int,
                                                    c_u32_p, C.c_int, C.POINTER(C.c_char_p)]
        lib.ryujin_hip_output_info.argtypes = [vp, c_u32_p, c_u32_p]
        lib.ryujin_hip_output_selection.argtypes = [vp, c_u32_p, c_u32_p, c_u32_p]
        lib.ryujin_hip_output_levelset_values.argtypes = [vp, C.c_int, c_double_p]
        lib.ryujin_hip_output_extract.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_void_p]
        _hip = lib
    return _hip
