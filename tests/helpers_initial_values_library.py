"""Yardsticks of tests/test_gpu_initial_values_library.py and tests/test_initial_values_library_cpu.py: the numpy side
of the Riemann-data, shock-front, ramp-up and Noh states (capi.IV_LIBRARY_STATES,
ryujin_amd/csrc/initial_states_library_device.hpp). Everything tests/helpers_initial_values.py has -- the affine
transform, the error arithmetic Err, the clearance rule of the jumps, the meshes, run_driver -- is imported from there.

reference(): ryujin_amd.initial_states (euler_*_primitive, ramp_up_blend, sw_*_primitive: the specification) behind
affine_transform, through euler_from_primitive / aeos_from_primitive, the momentum rotated back.

tolerance(): the same statements in the error arithmetic of helpers_initial_values (its docstring, 3.). What enters
beyond + - * /: sqrt (1 ulp) in the norm of noh and in a_R of the shock front, cos (3 ulp) in the ramp. A
piecewise-constant state copies parameters: its primitive state has tolerance 0, the conserved one the roundings of
from_initial_state. The constants the host forms (the state behind the shock and S3, D and the interior state of noh,
(x1 - x0)^6 of the smooth wave) go through the same arithmetic.

jump_clearance(): the region boundaries of every state, in the coordinate the device compares:
    contrast, sw contrast        x' = 0
    three state contrast         x' = left length, x' = left + middle length
    four state contrast          x' = 0 and y' = 0
    shock front                  x' = S3 t
    noh                          |x'| = D t (t > 0; t == 0 is never interior)
    smooth wave                  x' - mach t = 0.1 and 0.3 (kinks, the polynomial vanishes there)
    astro jet                    x' = 1e-12 and |y'| = jet width (the whole lines, a superset of the jet's outline)
    ramp up, uniform             none in space (the ramp's tests on t are exact comparisons of the same doubles)
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import helpers_eos_function as he
import helpers_initial_values as hiv
from helpers_initial_values import NASG, Err, affine_transform, affine_transform_vector, e_cos, e_sqrt
from ryujin_amd import HyperbolicModule, capi
from ryujin_amd import initial_states as ist

EULER_STATES = ("contrast", "three state contrast", "four state contrast", "shock front", "ramp up", "noh",
                "smooth wave", "astro jet")
SW_STATES = ("uniform", "contrast")
JUMP_STATES = ("contrast", "three state contrast", "four state contrast", "shock front", "noh", "smooth wave",
               "astro jet")
MIN_DIM = {"four state contrast": 2, "astro jet": 2}
N_REGIONS = {"three state contrast": 3, "four state contrast": 4}


@dataclass
class Case(hiv.Case):
    """helpers_initial_values.Case for a state of capi.IV_LIBRARY_STATES; eos_function: the equation of state of
    `edits` written as expressions (HyperbolicModule.eos_configure_function) before the state is configured"""
    eos_function: bool = False

    def key(self):
        return (capi.iv_family(self.equation), self.name)

    def get(self, pname):
        spec = {p[0]: p[2] for p in capi.IV_LIBRARY_STATES[self.key()][1]}
        return self.params.get(pname, spec[pname])


# --------------------------------------------------------------------------- cases

PARAMS = {
    "contrast": {"primitive state left": (1.0, 0.75, 1.0), "primitive state right": (0.125, -0.25, 0.1)},
    "three state contrast": {"primitive state left": (1.0, 0.5, 1.0e3), "left region length": 0.1,
                             "primitive state middle": (1.25, -0.25, 1.0e-2), "middle region length": 0.8,
                             "primitive state right": (0.75, 0.125, 1.0e2)},
    "four state contrast": {"primitive state bottom left": (0.138, 1.206, 1.206, 0.029),
                            "primitive state bottom right": (0.5323, 0.0, 1.206, 0.3),
                            "primitive state top left": (0.5323, 1.206, 0.0, 0.3),
                            "primitive state top right": (1.5, 0.0, 0.0, 1.5)},
    "shock front": {"primitive state": (1.4, 0.1, 1.0), "mach number": 2.5, "gamma": 1.4},
    "ramp up": {"primitive state initial": (1.4, 0.5, 1.0), "primitive state final": (1.2, 3.0, 1.5),
                "time initial": 0.1, "time final": 0.3},
    "noh": {"reference density": 1.0, "reference velocity magnitude": 1.25, "reference pressure": 1.0e-12,
            "gamma": 1.4},
    "smooth wave": {"reference density": 1.0, "reference pressure": 1.5, "mach number": 1.0},
    "astro jet": {"jet width": 0.2, "primitive jet state": (5.0, 30.0, 0.4127),
                  "primitive ambient right": (0.5, 0.25, 0.4127), "gamma": 5.0 / 3.0},
}
# three times per state: t = 0 and two positive ones. ramp up: before "time initial", inside the ramp, after "time
# final"; noh: D t = 0.15 and 0.5 with D = 0.25, points of [-1, 1]^dim on both sides; shock front: the front at
# x' = 0, 0.296, 0.74 of S3 = 2.96
TIMES = {"ramp up": (0.0, 0.2, 0.4), "noh": (0.0, 0.6, 2.0), "shock front": (0.0, 0.1, 0.25)}
POSITION_1D = {"three state contrast": (-0.05,)}      # x' in [-0.95, 1.05]: all three regions


def _case(tag, eq, edits, name, dim, eos_function=False):
    direction = None if dim == 1 else (1.0,) * dim
    position = POSITION_1D.get(name, (0.1,)) if dim == 1 else (0.25, -0.125, 0.0625)[:dim]
    label = f"{tag} {name} {dim}d" + ("" if dim == 1 else " (" + ",".join("1" * dim) + ")")
    return Case(label, eq, dim, name, dict(PARAMS[name]), direction, position, edits=dict(edits),
                times=TIMES.get(name, (0.0, 0.15, 0.4)), eos_function=eos_function)


def function_cases():
    """GPU test A: every new state for Euler, for EulerAEOS with the polytropic gas and with NASG, in 1-D, in 2-D along
    (1, 1) and in 3-D along (1, 1, 1) from a non-zero position where the state has the dimension; ramp up, shock front
    (whose constants take the covolume of the interpolation) and noh once more on a context with the function
    equation of state; the two shallow-water states in 1-D and 2-D."""
    cases = []
    for eq, tag, edits in ((capi.EQ_EULER, "euler", {}),
                           (capi.EQ_EULER_AEOS, "aeos-pg", dict(eos=capi.EOS_POLYTROPIC_GAS)),
                           (capi.EQ_EULER_AEOS, "aeos-nasg", NASG)):
        for name in EULER_STATES:
            cases += [_case(tag, eq, edits, name, dim) for dim in (1, 2, 3) if dim >= MIN_DIM.get(name, 1)]
    cases += [_case("aeos-fn", capi.EQ_EULER_AEOS, NASG, "ramp up", 2, eos_function=True),
              _case("aeos-fn", capi.EQ_EULER_AEOS, NASG, "shock front", 1, eos_function=True),
              _case("aeos-fn", capi.EQ_EULER_AEOS, NASG, "noh", 3, eos_function=True)]
    g = dict(gravity=9.81)
    for dim in (1, 2):
        direction = None if dim == 1 else (1.0, 1.0)
        position = (0.1,) if dim == 1 else (0.25, -0.125)
        suffix = f"{dim}d" + ("" if dim == 1 else " (1,1)")
        cases += [
            Case(f"sw uniform {suffix}", capi.EQ_SHALLOW_WATER, dim, "uniform", {"primitive state": (1.5, 0.75)},
                 direction, position, edits=g),
            Case(f"sw contrast {suffix}", capi.EQ_SHALLOW_WATER, dim, "contrast",
                 {"primitive state left": (2.0, 0.5), "primitive state right": (0.5, -0.25)}, direction, position,
                 edits=g),
        ]
    return cases


def is_jump_state(case: Case):
    return case.name in JUMP_STATES or (case.equation == capi.EQ_SHALLOW_WATER and case.name == "contrast")


def module_for(case: Case, off=None):
    off = hiv.tiny_mesh(case.dim) if off is None else off
    p = hiv.make_params(case.equation, case.dim, **case.edits)
    m = HyperbolicModule(off, p, backend="hip")
    if case.eos_function:
        m.eos_configure_function(**he.member_expressions(p))
    hiv.configure(m, case)
    return m


points_for = hiv.points_for


def state_gamma(case: Case, p):
    """the gamma the state's own constants are formed with: the system's for Euler, the parameter for EulerAEOS"""
    return p.gamma if case.equation == capi.EQ_EULER else case.get("gamma")


def interpolation_b(case: Case, p):
    """eos_interpolation_b of the context: the covolume for NASG (closed form or as expressions), else 0"""
    if case.equation == capi.EQ_EULER_AEOS and p.eos == capi.EOS_NOBLE_ABEL_STIFFENED_GAS:
        return p.eos_covolume_b
    return 0.0


# --------------------------------------------------------------------------- jumps

def boundaries(case: Case, X, t):
    """[(coordinate per point, boundary value), ...] of the docstring's table"""
    Xt = affine_transform(case.dir(), case.pos(), X)
    x = Xt[:, 0]
    p = hiv.make_params(case.equation, case.dim, **case.edits)
    if case.name == "contrast":
        return [(x, 0.0)]
    if case.equation == capi.EQ_SHALLOW_WATER:
        return []
    if case.name == "three state contrast":
        return [(x, case.get("left region length")),
                (x, case.get("left region length") + case.get("middle region length"))]
    if case.name == "four state contrast":
        return [(x, 0.0), (Xt[:, 1], 0.0)]
    if case.name == "shock front":
        _, S3 = ist.euler_shock_front_constants(case.get("primitive state"), case.get("mach number"),
                                                state_gamma(case, p), interpolation_b(case, p))
        return [(x, S3 * t)]
    if case.name == "noh":
        if t == 0.0:
            return []
        D, _, _ = ist.euler_noh_constants(case.dim, case.get("reference density"),
                                          case.get("reference velocity magnitude"), state_gamma(case, p))
        return [(np.linalg.norm(Xt, axis=1), D * t)]
    if case.name == "smooth wave":
        xb = x - case.get("mach number") * t
        return [(xb, ist.SMOOTH_WAVE_LEFT), (xb, ist.SMOOTH_WAVE_RIGHT)]
    if case.name == "astro jet":
        return [(x, 1.0e-12), (np.abs(Xt[:, 1]), case.get("jet width"))]
    return []


def jump_clearance(case: Case, X, t):
    """helpers_initial_values.jump_clearance for the states here: min over the region boundaries of
    |coordinate - boundary| - 1e-9 (1 + |coordinate|), per point (> 0: clear); +inf without a boundary"""
    out = np.full(len(X), np.inf)
    for coordinate, bound in boundaries(case, X, t):
        out = np.minimum(out, np.abs(coordinate - bound) - 1.0e-9 * (1.0 + np.abs(coordinate)))
    return out


def assert_clear_of_jumps(case: Case, X, t):
    clearance = jump_clearance(case, X, t)
    assert (clearance > 0.0).all(), (case.label, t, int((clearance <= 0.0).sum()))


def region_ids(case: Case, X, t):
    """an integer per point that tells the regions of a piecewise state apart (which side of every boundary)"""
    ids = np.zeros(len(X), dtype=np.int64)
    for coordinate, bound in boundaries(case, X, t):
        ids = 2 * ids + (coordinate >= bound)
    return ids


# --------------------------------------------------------------------------- the expected states

def primitive(case: Case, Xt, t, p):
    """(rho, velocity [n, dim], pressure) in the frame of the state: every Euler state but ramp up"""
    name = case.name
    if name == "contrast":
        return ist.euler_contrast_primitive(Xt, case.get("primitive state left"), case.get("primitive state right"))
    if name == "three state contrast":
        return ist.euler_three_state_contrast_primitive(
            Xt, case.get("primitive state left"), case.get("left region length"), case.get("primitive state middle"),
            case.get("middle region length"), case.get("primitive state right"))
    if name == "four state contrast":
        return ist.euler_four_state_contrast_primitive(
            Xt, case.get("primitive state bottom left"), case.get("primitive state bottom right"),
            case.get("primitive state top left"), case.get("primitive state top right"))
    if name == "shock front":
        return ist.euler_shock_front_primitive(Xt, t, case.get("primitive state"), case.get("mach number"),
                                               state_gamma(case, p), interpolation_b(case, p))
    if name == "noh":
        return ist.euler_noh_primitive(Xt, t, case.get("reference density"), case.get("reference velocity magnitude"),
                                       case.get("reference pressure"), state_gamma(case, p))
    if name == "smooth wave":
        return ist.euler_smooth_wave_primitive(Xt, t, case.get("reference density"), case.get("reference pressure"),
                                               case.get("mach number"))
    assert name == "astro jet"
    return ist.euler_astro_jet_primitive(Xt, case.get("jet width"), case.get("primitive jet state"),
                                         case.get("primitive ambient right"))


def _conserved(case: Case, p, rho, vel, pr):
    if case.equation == capi.EQ_EULER_AEOS:
        return ist.aeos_from_primitive(p, rho, vel, pr)
    return ist.euler_from_primitive(rho, vel, pr, p.gamma)


def reference(case: Case, X, t):
    """the expected conserved states [n, k] at the points X [n, dim]"""
    X = np.asarray(X, dtype=np.float64)
    n, dim = X.shape
    p = hiv.make_params(case.equation, case.dim, **case.edits)
    Xt = affine_transform(case.dir(), case.pos(), X)
    if case.equation == capi.EQ_SHALLOW_WATER:
        if case.name == "uniform":
            h, u = ist.sw_uniform_primitive(Xt, case.get("primitive state"))
        else:
            h, u = ist.sw_contrast_primitive(Xt, case.get("primitive state left"), case.get("primitive state right"))
        m = np.zeros((n, dim))
        m[:, 0] = h * u
        return np.column_stack([h, affine_transform_vector(case.dir(), m)])
    if case.name == "ramp up":
        ends = []
        for key in ("primitive state initial", "primitive state final"):
            rho0, u0, p0 = case.get(key)
            vel = np.zeros((n, dim))
            vel[:, 0] = u0
            ends.append(_conserved(case, p, np.full(n, float(rho0)), vel, np.full(n, float(p0))))
        U = ist.ramp_up_blend(ends[0], ends[1], t, case.get("time initial"), case.get("time final"))
    else:
        U = _conserved(case, p, *primitive(case, Xt, t, p))
    U[:, 1:-1] = affine_transform_vector(case.dir(), U[:, 1:-1])
    return U


# --------------------------------------------------------------------------- the derived tolerance

def _const(n, c):
    c = Err.lift(c)
    return Err(np.full(n, c.v), np.full(n, c.e))


def _select(masks_and_values, otherwise):
    out = otherwise
    for mask, value in reversed(masks_and_values):
        out = value.where(mask, out)
    return out


def _primitive_err(case: Case, x, t, p):
    """(rho, [v_d], pressure) in the frame of the state, in the error arithmetic"""
    n, dim = len(x[0].v), case.dim
    zero = Err(np.zeros(n))
    name = case.name

    def tube(masks_and_states, otherwise):
        rho, u, pr = (_select([(m, _const(n, s[q])) for m, s in masks_and_states], _const(n, otherwise[q]))
                      for q in range(3))
        return rho, [u] + [zero] * (dim - 1), pr

    if name == "contrast":
        return tube([(x[0].v > 0.0, case.get("primitive state right"))], case.get("primitive state left"))
    if name == "three state contrast":
        left, middle = case.get("left region length"), case.get("middle region length")
        return tube([(x[0].v >= left + middle, case.get("primitive state right")),
                     (x[0].v >= left, case.get("primitive state middle"))], case.get("primitive state left"))
    if name == "four state contrast":
        east, north = x[0].v >= 0.0, x[1].v >= 0.0
        bl, br = case.get("primitive state bottom left"), case.get("primitive state bottom right")
        tl, tr = case.get("primitive state top left"), case.get("primitive state top right")
        q = [_select([(north & east, _const(n, tr[k])), (north, _const(n, tl[k])), (east, _const(n, br[k]))],
                     _const(n, bl[k])) for k in range(4)]
        return q[0], [q[1], q[2]] + [zero] * (dim - 2), q[3]
    if name == "shock front":
        # the constructor: on the host with the C library, in numpy on the other side
        g, b = Err(state_gamma(case, p)), interpolation_b(case, p)
        rho_R, u_R, p_R = (Err(c) for c in case.get("primitive state"))
        mach = Err(case.get("mach number"))
        a_R = e_sqrt(g * p_R / rho_R / (1.0 - b * rho_R))
        mach_R = u_R / a_R
        S3 = mach * a_R
        dm = mach_R - mach
        rho_L = rho_R * (g + 1.0) * dm * dm / ((g - 1.0) * dm * dm + 2.0)
        u_L = (1.0 - rho_R / rho_L) * S3 + rho_R / rho_L * u_R
        p_L = p_R * (2.0 * g * dm * dm - (g - 1.0)) / (g + 1.0)
        right = (x[0] - S3 * t).v > 0.0
        rho, u, pr = (_const(n, r).where(right, _const(n, l)) for r, l in ((rho_R, rho_L), (u_R, u_L), (p_R, p_L)))
        return rho, [u] + [zero] * (dim - 1), pr
    if name == "noh":
        g = Err(state_gamma(case, p))
        rho0, u0, p0 = (Err(case.get(k)) for k in ("reference density", "reference velocity magnitude",
                                                  "reference pressure"))
        D = u0 * (g - 1.0) / 2.0
        ratio = (g + 1.0) / (g - 1.0)
        ratio_dim, plus_dim, minus_dim1 = ratio, g + 1.0, Err(1.0)
        for _ in range(dim - 1):
            ratio_dim, plus_dim, minus_dim1 = ratio_dim * ratio, plus_dim * (g + 1.0), minus_dim1 * (g - 1.0)
        rho_in = rho0 * ratio_dim
        p_in = (0.5 * rho0 * u0 * u0) * (plus_dim / minus_dim1)
        norm2 = x[0] * x[0]
        for d in range(1, dim):
            norm2 = norm2 + x[d] * x[d]
        norm = e_sqrt(norm2)
        denominator = norm + ist.NOH_MIN
        interior = np.zeros(n, dtype=bool) if t == 0.0 else norm.v / t < D.v
        growth = 1.0 + Err(t) / denominator
        power = Err(np.ones(n))
        for _ in range(dim - 1):
            power = power * growth
        rho = _const(n, rho_in).where(interior, rho0 * power)
        vel = [zero.where(interior, (-u0 * x[d]) / denominator) for d in range(dim)]
        return rho, vel, _const(n, p_in).where(interior, _const(n, p0))
    if name == "smooth wave":
        left, right = ist.SMOOTH_WAVE_LEFT, ist.SMOOTH_WAVE_RIGHT
        mach, rho_ref = case.get("mach number"), case.get("reference density")
        xb = x[0] - Err(mach) * t
        a, b = xb - left, right - xb
        w2 = Err(right - left) * (right - left)
        polynomial = 64.0 * (a * (a * a)) * (b * (b * b)) / (w2 * (w2 * w2))
        inside = (left <= xb.v) & (xb.v <= right)
        rho = (rho_ref + polynomial).where(inside, _const(n, rho_ref))
        return rho, [_const(n, mach)] + [zero] * (dim - 1), _const(n, case.get("reference pressure"))
    assert name == "astro jet"
    jet = (x[0].v < 1.0e-12) & (np.abs(x[1].v) <= case.get("jet width"))
    return tube([(jet, case.get("primitive jet state"))], case.get("primitive ambient right"))


def _conserved_err(case: Case, p, rho, vel, pr):
    v2 = vel[0] * vel[0]
    for v in vel[1:]:
        v2 = v2 + v * v
    kinetic = 0.5 * rho * v2
    if case.equation == capi.EQ_EULER_AEOS:
        E = rho * hiv._eos_energy_err(p, rho, pr) + kinetic
    else:
        E = pr / (Err(p.gamma) - 1.0) + kinetic
    return [rho, *[rho * v for v in vel], E]


def tolerance(case: Case, X, t):
    """(values [n, k] of the error arithmetic, bound [n, k] on |device - numpy|)"""
    X = np.asarray(X, dtype=np.float64)
    n, dim = X.shape
    p = hiv.make_params(case.equation, case.dim, **case.edits)
    x = hiv._transform_err(case, X)
    zero = Err(np.zeros(n))
    if case.equation == capi.EQ_SHALLOW_WATER:
        if case.name == "uniform":
            h, u = (_const(n, c) for c in case.get("primitive state"))
        else:
            east = x[0].v > 0.0
            left, right = case.get("primitive state left"), case.get("primitive state right")
            h, u = (_const(n, right[q]).where(east, _const(n, left[q])) for q in range(2))
        comps = [h, *hiv._rotate_err(case, [h * u] + [zero] * (dim - 1))]
    else:
        if case.name == "ramp up":
            ends = []
            for key in ("primitive state initial", "primitive state final"):
                rho0, u0, p0 = case.get(key)
                ends.append(_conserved_err(case, p, _const(n, rho0), [_const(n, u0)] + [zero] * (dim - 1),
                                           _const(n, p0)))
            t_i, t_f = case.get("time initial"), case.get("time final")
            if t <= t_i:
                comps = ends[0]
            elif t >= t_f:
                comps = ends[1]
            else:
                factor = e_cos(Err(0.5 * np.pi) * (Err(t) - t_i) / (Err(t_f) - t_i))
                alpha = factor * factor
                beta = 1.0 - alpha
                comps = [alpha * a + beta * b for a, b in zip(*ends)]
        else:
            comps = _conserved_err(case, p, *_primitive_err(case, x, t, p))
        comps = [comps[0], *hiv._rotate_err(case, list(comps[1:-1])), comps[-1]]
    return np.column_stack([c.v for c in comps]), np.column_stack([c.e for c in comps])


# --------------------------------------------------------------------------- the two verification setups

SMOOTH_WAVE_GOLDEN = "euler_verification-smooth_wave-erk33.baseline"
SHOCK_FRONT_GOLDEN = "euler_verification-shock_front-erk33.baseline"
VERIFICATION_TOL = dict(rtol_t=5e-6, rtol_err=1.5e-3)
# prm/verification/euler-{smooth_wave,shock_front}-erk33.prm at their coarsest mesh: [0, 1], 400 cells, Dirichlet ends,
# ERK33, gamma 1.4, the states' defaults. name -> (golden, state, kwargs of initial_values_configure, cfl, limiter
# relaxation factor, final time)
VERIFICATION = {
    "smooth wave": (SMOOTH_WAVE_GOLDEN, "smooth wave", dict(position=(0.1,)), 0.3, 1.0, 0.6),
    "shock front": (SHOCK_FRONT_GOLDEN, "shock front", dict(position=(0.25,)), 0.1, 8.0, 0.25),
}


def verification_params(default_params, relaxation_factor):
    p = default_params(capi.EQ_EULER, 1)
    p.gamma = 1.4
    p.limiter_iterations = 2
    p.limiter_newton_max_iterations = 2
    p.limiter_newton_tolerance = 1e-10
    p.limiter_relaxation_factor = relaxation_factor
    return p


def verification_exact(name):
    """exact(positions, t) of a setup: the numpy restatement with the reference's defaults"""
    _, state, kwargs, _, _, _ = VERIFICATION[name]
    case = Case(name, capi.EQ_EULER, 1, state, {}, None, kwargs["position"], edits=dict(gamma=1.4))
    return lambda positions, t: reference(case, positions, t)


def verification_mesh():
    return hiv.interval(400, 0.0, 1.0, capi.BC_DIRICHLET, capi.BC_DIRICHLET)
