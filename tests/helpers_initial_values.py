"""Yardsticks of tests/test_gpu_initial_values.py and tests/test_initial_values_cpu.py: the numpy side of the
device-resident InitialValues (ryujin_hip_initial_values_*, ryujin_amd/csrc/initial_states_device.hpp).

1. The affine transform of source/initial_values.template.h:66-148 restated in numpy (affine_transform,
   affine_transform_vector): translate by `position`, roll the NORMALISED `direction` onto the x-axis -- about y first
   (takes the z-component away; dim = 3), then about z (takes the y-component away; dim >= 2) --, rotate a momentum
   back in the opposite order. Each roll is skipped where its norm is <= 1e-14, and, as in the reference, the second
   roll uses the components of the ORIGINAL direction: for (1, 1, 1) / sqrt(3) both rolls are by 45 degrees.

2. reference(): the expected state of a case = ryujin_amd.initial_states (the specification; several of its functions
   are pinned to 16 digits by the reference's baselines under tests/golden/) composed with that transform.

3. tolerance(): DERIVED, not tuned. The device follows the restatement statement by statement, so the two sides differ
   by (a) one rounding per operation wherever their inputs differ, (b) the library functions. The formulas are
   evaluated once more in a first-order error arithmetic (class Err) that carries a bound on |device - numpy|:
       x + y, x - y : e = e_x + e_y + EPS |result|
       x * y        : e = |x| e_y + |y| e_x + e_x e_y + EPS |result|
       x / y        : e = (e_x + |result| e_y) / (|y| - e_y) + EPS |result|
       f(x)         : e = |f'(x)| e_x (the condition number times the incoming error) + B_f EPS |result|
   EPS = 2^-52 covers the two roundings (one per side, 2^-53 each). B_f is the sum of the two implementations' stated
   errors in ulp: exp 1 (ocml) + 1 (numpy) = 2; sin, cos 2 + 1 = 3; sqrt 0.5 + 0.5 = 1; pow: the device's dev_pow is
   held to 2.5 x 1.1e-16 x (1 + |y ln x|) by tests/test_gpu_parity.py::test_device_pow_accuracy, numpy's to 1 ulp:
   B_pow = 2.5 (1 + |y ln x|), which covers both. Constants formed at configure time on the host (the normalised
   direction: 4 EPS; the fan constants of the rarefaction, sqrt(g h_L), the depth of the incline) go through the same
   arithmetic. Nothing else enters: a component both sides copy from a parameter has tolerance 0.
   The bound holds on ONE branch of a piecewise state; near a jump it says nothing, so the tests assert
   (assert_clear_of_jumps) that every point is further than 1e-9 (1 + |x|) from every region boundary.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field

import numpy as np

from ryujin_amd import HyperbolicModule, capi, offline
from ryujin_amd import initial_states as ist

EPS = float(np.finfo(np.float64).eps)


# --------------------------------------------------------------------------- 1. the affine transform

def _rolls(direction):
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    dim = d.size
    roll_z = roll_y = None
    if dim == 3:
        norm = np.sqrt(d[0] * d[0] + d[2] * d[2])
        if norm > 1.0e-14:
            roll_z = (d[0] / norm, d[2] / norm)
    if dim >= 2:
        norm = np.sqrt(d[0] * d[0] + d[1] * d[1])
        if norm > 1.0e-14:
            roll_y = (d[0] / norm, d[1] / norm)
    return roll_z, roll_y


def affine_transform(direction, position, x):
    """initial_values.template.h:70-109; x: [n, dim]"""
    x = np.asarray(x, dtype=np.float64)
    y = x - np.asarray(position, dtype=np.float64)
    roll_z, roll_y = _rolls(direction)
    if roll_z is not None:
        n_x, n_z = roll_z
        y0, y2 = n_x * y[:, 0] + n_z * y[:, 2], -n_z * y[:, 0] + n_x * y[:, 2]
        y = np.column_stack([y0, y[:, 1], y2])
    if roll_y is not None:
        n_x, n_y = roll_y
        y0, y1 = n_x * y[:, 0] + n_y * y[:, 1], -n_y * y[:, 0] + n_x * y[:, 1]
        y = np.column_stack([y0, y1, *([y[:, 2]] if y.shape[1] == 3 else [])])
    return y


def affine_transform_vector(direction, m):
    """initial_values.template.h:115-149; m: [n, dim]"""
    m = np.array(m, dtype=np.float64)
    roll_z, roll_y = _rolls(direction)
    if roll_y is not None:
        n_x, n_y = roll_y
        m0, m1 = n_x * m[:, 0] - n_y * m[:, 1], n_y * m[:, 0] + n_x * m[:, 1]
        m = np.column_stack([m0, m1, *([m[:, 2]] if m.shape[1] == 3 else [])])
    if roll_z is not None:
        n_x, n_z = roll_z
        m0, m2 = n_x * m[:, 0] - n_z * m[:, 2], n_z * m[:, 0] + n_x * m[:, 2]
        m = np.column_stack([m0, m[:, 1], m2])
    return m


# --------------------------------------------------------------------------- cases

EULER_STATES = ("uniform", "radial contrast", "isentropic vortex", "leblanc", "rarefaction")
JUMP_STATES = ("radial contrast", "leblanc", "rarefaction", "circular dam break", "ritter dam break")

LEBLANC_SPEEDS = (-1.0 / 3.0, 0.49578489518897934, 0.62183867139173454, 0.82911836253346982)


@dataclass
class Case:
    label: str
    equation: int
    dim: int
    name: str                       # configuration name of the reference
    params: dict = field(default_factory=dict)   # the reference's parameter names
    direction: tuple | None = None
    position: tuple | None = None
    edits: dict = field(default_factory=dict)    # ryujin_hip_params fields (equation of state, gravity, ...)
    box: tuple = (-1.0, 1.0)        # the points are drawn from box^dim
    times: tuple = (0.0, 0.15, 0.4)

    def dir(self):
        return (1.0,) + (0.0,) * (self.dim - 1) if self.direction is None else tuple(self.direction)

    def pos(self):
        return (0.0,) * self.dim if self.position is None else tuple(self.position)

    def get(self, pname):
        spec = {p[0]: p[2] for p in capi.IV_STATES[self.name][2]}
        return self.params.get(pname, spec[pname])


NASG = dict(eos=capi.EOS_NOBLE_ABEL_STIFFENED_GAS, eos_covolume_b=0.02, eos_q=0.3, eos_pinf=0.5)


def function_cases():
    """GPU test A: every state of the table for both Descriptions where it applies (EulerAEOS with the polytropic gas
    and with NASG), 1-D profiles also in 2-D / 3-D along (1, 1) / (1, 1, 1) from a non-zero position."""
    cases = []
    for eq, tag, edits in ((capi.EQ_EULER, "euler", {}), (capi.EQ_EULER_AEOS, "aeos-pg", dict(eos=capi.EOS_POLYTROPIC_GAS)),
                           (capi.EQ_EULER_AEOS, "aeos-nasg", NASG)):
        cases += [
            Case(f"{tag} uniform 1d", eq, 1, "uniform", {"primitive state": (1.4, 3.0, 1.0)}, edits=edits),
            Case(f"{tag} uniform 2d (1,1)", eq, 2, "uniform", {"primitive state": (1.4, 3.0, 1.0)}, (1.0, 1.0),
                 (0.25, -0.125), edits=edits),
            Case(f"{tag} uniform 3d (1,1,1)", eq, 3, "uniform", {"primitive state": (1.4, 3.0, 1.0)},
                 (1.0, 1.0, 1.0), (0.25, -0.125, 0.0625), edits=edits),
            Case(f"{tag} radial contrast 2d", eq, 2, "radial contrast",
                 {"primitive state inner": (1.0, 0.0, 100.0), "primitive state outer": (0.125, 0.0, 0.1),
                  "radius": 0.5}, position=(0.1, -0.05), edits=edits),
            Case(f"{tag} isentropic vortex", eq, 2, "isentropic vortex", {"mach number": 1.0, "beta": 5.0},
                 (1.0, 1.0), (-1.0, -1.0), edits=edits, box=(-5.0, 5.0), times=(0.0, 0.5, 2.0)),
            Case(f"{tag} leblanc 1d", eq, 1, "leblanc", position=(0.326732673267,), edits=dict(edits, gamma=5.0 / 3.0),
                 box=(0.0, 1.0), times=(0.0, 0.2, 2.0 / 3.0)),
            Case(f"{tag} leblanc 2d (1,1)", eq, 2, "leblanc", {}, (1.0, 1.0), (0.25, -0.125),
                 edits=dict(edits, gamma=5.0 / 3.0), times=(0.0, 0.2, 2.0 / 3.0)),
            Case(f"{tag} leblanc 3d (1,1,1)", eq, 3, "leblanc", {}, (1.0, 1.0, 1.0), (0.25, -0.125, 0.0625),
                 edits=dict(edits, gamma=5.0 / 3.0), times=(0.0, 0.2, 2.0 / 3.0)),
            Case(f"{tag} rarefaction 1d", eq, 1, "rarefaction", position=(0.2,), edits=edits, box=(0.0, 1.0),
                 times=(0.0, 0.1, 0.30558)),
        ]
    g = dict(gravity=9.81)
    cases += [
        Case("sw circular dam break 2d", capi.EQ_SHALLOW_WATER, 2, "circular dam break",
             {"still water depth": 0.5, "radius": 2.5, "dam amplitude": 2.5}, edits=g, box=(-3.0, 3.0)),
        Case("sw paraboloid 1d", capi.EQ_SHALLOW_WATER, 1, "paraboloid",
             {"free surface radius": 3000.0, "water height": 10.0, "paraboloid length": 10000.0, "speed": 2.0},
             edits=g, box=(0.0, 10000.0), times=(0.0, 300.0, 1345.71)),
        Case("sw paraboloid 1d with friction", capi.EQ_SHALLOW_WATER, 1, "paraboloid",
             {"free surface radius": 3000.0, "water height": 10.0, "paraboloid length": 10000.0, "speed": 2.0},
             edits=dict(g, manning_friction_coefficient=0.002), box=(0.0, 10000.0), times=(0.0, 300.0, 1345.71)),
        Case("sw ritter dam break 1d", capi.EQ_SHALLOW_WATER, 1, "ritter dam break",
             {"time initial": 1.0, "left water depth": 0.005}, position=(5.0,), edits=g, box=(0.0, 10.0),
             times=(0.0, 2.0, 6.0)),
        Case("sw ritter dam break 2d (1,1)", capi.EQ_SHALLOW_WATER, 2, "ritter dam break",
             {"time initial": 1.0, "left water depth": 0.005}, (1.0, 1.0), (0.25, -0.125), edits=g,
             times=(0.0, 2.0, 6.0)),
        Case("sw smooth vortex", capi.EQ_SHALLOW_WATER, 2, "smooth vortex",
             {"reference depth": 2.0, "mach number": 1.0, "beta": 2.0}, (1.0, 1.0), (-1.0, -1.0), edits=g,
             box=(-6.0, 6.0), times=(0.0, 0.5, 2.0)),
        Case("sw sloping friction 1d", capi.EQ_SHALLOW_WATER, 1, "sloping friction",
             {"ramp slope": 1.0e-2, "initial discharge": 1.0e-1}, edits=dict(g, manning_friction_coefficient=1.0e-2),
             box=(0.0, 20.0)),
    ]
    return cases


def make_params(equation, dim, **edits):
    p = capi.Params()
    capi.load_hip().ryujin_hip_default_params(C.byref(p), equation, dim)
    for name, value in edits.items():
        setattr(p, name, value)
    return p


def tiny_mesh(dim, bc=capi.BC_DIRICHLET):
    """a context to evaluate on: the smallest mesh of the dimension"""
    if dim == 1:
        return offline.SyntheticOffline(offline.MeshSpec(1, (4,), (0.0,), (1.0,), (bc, bc)))
    if dim == 2:
        return offline.SyntheticOffline(offline.rectangle_2d(3, bc=bc))
    return offline.SyntheticOffline(offline.box_3d(2, bc=bc))


def module_for(case: Case, off=None):
    off = tiny_mesh(case.dim) if off is None else off
    m = HyperbolicModule(off, make_params(case.equation, case.dim, **case.edits), backend="hip")
    configure(m, case)
    return m


def configure(m, case: Case):
    m.initial_values_configure(case.name, direction=case.direction, position=case.position,
                               **{k.replace(" ", "_"): v for k, v in case.params.items()})


def points_for(case: Case, n=1000, seed=5):
    rng = np.random.default_rng(seed)
    lo, hi = case.box
    return rng.uniform(lo, hi, size=(n, case.dim))


def state_gamma(case: Case, p):
    """the gamma of the state itself: the system's for Euler, the state's own parameter for EulerAEOS"""
    if case.name == "leblanc":
        return 5.0 / 3.0
    if case.equation == capi.EQ_EULER or case.name in ("uniform", "radial contrast"):
        return p.gamma
    return case.get("gamma")


# --------------------------------------------------------------------------- jumps

def jump_clearance(case: Case, X, t):
    """min over the region boundaries of |coordinate - boundary| - 1e-9 (1 + |coordinate|), per point (> 0: clear);
    +inf for a smooth state"""
    Xt = affine_transform(case.dir(), case.pos(), X)
    x = Xt[:, 0]
    if case.name == "leblanc":
        bounds = [s * t for s in LEBLANC_SPEEDS]
    elif case.name == "rarefaction":
        gamma = state_gamma(case, make_params(case.equation, case.dim, **case.edits))
        c_l = np.sqrt(gamma * 1.0 / 3.0)
        p_r = np.power(0.5 / 3.0, gamma)
        c_r = np.sqrt(gamma * p_r / 0.5)
        u_r = c_l + 2.0 * (c_l - c_r) / (gamma - 1.0)
        tt = 0.2 / (u_r - c_l) + t
        bounds = [0.0, tt * (u_r - c_r)]
    elif case.name == "ritter dam break":
        aL = np.sqrt(9.81 * case.get("left water depth"))
        ts = t + case.get("time initial")
        bounds = [-ts * aL, 2.0 * ts * aL]
    elif case.name == "radial contrast":
        x, bounds = np.linalg.norm(Xt, axis=1), [case.get("radius")]
    elif case.name == "circular dam break":
        x, bounds = np.sum(Xt * Xt, axis=1), [case.get("radius")]
    else:
        return np.full(len(X), np.inf)
    return np.min([np.abs(x - b) for b in bounds], axis=0) - 1.0e-9 * (1.0 + np.abs(x))


def assert_clear_of_jumps(case: Case, X, t):
    clearance = jump_clearance(case, X, t)
    assert (clearance > 0.0).all(), (case.label, t, int((clearance <= 0.0).sum()))


# --------------------------------------------------------------------------- 2. the expected states

def _expand(direction, rho_or_h, m1, dim, tail=None):
    """conserved n-D state of a 1-D profile: momentum along `direction`"""
    m = np.zeros((len(m1), dim))
    m[:, 0] = m1
    m = affine_transform_vector(direction, m)
    cols = [rho_or_h, *[m[:, d] for d in range(dim)]]
    if tail is not None:
        cols.append(tail)
    return np.column_stack(cols)


def euler_primitive(case: Case, X, t, p):
    """(rho, velocity in the frame of the state [n, dim], pressure) through ryujin_amd.initial_states"""
    n, dim = X.shape
    Xt = affine_transform(case.dir(), case.pos(), X)
    v = np.zeros((n, dim))
    if case.name == "uniform":
        rho0, u0, p0 = case.get("primitive state")
        rho, v[:, 0], pr = np.full(n, rho0), u0, np.full(n, p0)
    elif case.name == "radial contrast":
        inner, outer = case.get("primitive state inner"), case.get("primitive state outer")
        inside = np.linalg.norm(Xt, axis=1) <= case.get("radius")
        rho, v[:, 0], pr = (np.where(inside, inner[q], outer[q]) for q in range(3))
    elif case.name == "isentropic vortex":
        rho, v[:, 0], v[:, 1], pr, _ = ist.euler_isentropic_vortex_primitive(
            X, t, case.get("mach number"), case.get("beta"), state_gamma(case, p), case.dir(), case.pos())
    elif case.name == "leblanc":
        rho, v[:, 0], pr = ist.euler_leblanc_primitive(Xt[:, :1], t, 0.0)
    else:
        rho, v[:, 0], pr = ist.euler_rarefaction_primitive(Xt[:, :1], t, state_gamma(case, p), 0.0)
    return rho, v, pr


def reference(case: Case, X, t):
    """the expected conserved states [n, k] at the points X [n, dim]"""
    X = np.asarray(X, dtype=np.float64)
    p = make_params(case.equation, case.dim, **case.edits)
    dim, d, x0 = case.dim, case.dir(), case.pos()
    Xt = affine_transform(d, x0, X)
    if case.equation == capi.EQ_EULER_AEOS:
        rho, v, pr = euler_primitive(case, X, t, p)
        U = ist.aeos_from_primitive(p, rho, v, pr)
        U[:, 1:-1] = affine_transform_vector(d, U[:, 1:-1])
        return U
    if case.equation == capi.EQ_EULER:
        if case.name == "uniform":
            rho0, u0, p0 = case.get("primitive state")
            U = ist.euler_uniform(X, rho0, u0, p0, p.gamma)     # momentum along +x, rotated like every 1-D profile
            U[:, 1:-1] = affine_transform_vector(d, U[:, 1:-1])
            return U
        if case.name == "radial contrast":
            return ist.euler_radial_contrast(X, case.get("primitive state inner"), case.get("primitive state outer"),
                                             case.get("radius"), p.gamma, center=x0)
        if case.name == "isentropic vortex":
            return ist.euler_isentropic_vortex(X, t, case.get("mach number"), case.get("beta"), p.gamma, d, x0)
        if case.name == "leblanc":
            U = ist.euler_leblanc(X, t, x0[0]) if dim == 1 else ist.euler_leblanc(Xt[:, :1], t, 0.0)
        else:
            U = ist.euler_rarefaction(X, t, p.gamma, x0[0]) if dim == 1 else \
                ist.euler_rarefaction(Xt[:, :1], t, p.gamma, 0.0)
        return _expand(d, U[:, 0], U[:, 1], dim, U[:, 2])
    # shallow water
    if case.name == "circular dam break":
        return ist.sw_circular_dam_break(Xt, case.get("dam amplitude"), case.get("still water depth"),
                                         case.get("radius"))
    if case.name == "paraboloid":
        return ist.sw_paraboloid_1d(Xt, t, p.gravity, p.manning_friction_coefficient, case.get("free surface radius"),
                                    case.get("water height"), case.get("paraboloid length"), case.get("speed"))[0]
    if case.name == "ritter dam break":
        U = ist.sw_ritter_dam_break(X, t, p.gravity, case.get("time initial"), case.get("left water depth"), x0[0]) \
            if dim == 1 else ist.sw_ritter_dam_break(Xt[:, :1], t, p.gravity, case.get("time initial"),
                                                     case.get("left water depth"), 0.0)
        return _expand(d, U[:, 0], U[:, 1], dim)
    if case.name == "smooth vortex":
        return ist.sw_smooth_vortex(X, t, p.gravity, case.get("reference depth"), case.get("mach number"),
                                    case.get("beta"), d, x0)
    U = ist.sw_sloping_friction(Xt, p.manning_friction_coefficient, case.get("ramp slope"),
                                case.get("initial discharge"))[0]
    return _expand(d, U[:, 0], U[:, 1], dim)


# --------------------------------------------------------------------------- 3. the derived tolerance

class Err:
    """a value and a bound on |device - numpy| for it (module docstring)"""

    __array_ufunc__ = None      # numpy scalars defer to the operators below

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, dtype=np.float64)
        self.e = np.asarray(e, dtype=np.float64) + 0.0 * self.v

    @staticmethod
    def lift(x):
        return x if isinstance(x, Err) else Err(x)

    def __add__(self, o):
        o = Err.lift(o)
        v = self.v + o.v
        return Err(v, self.e + o.e + EPS * np.abs(v))

    __radd__ = __add__

    def __sub__(self, o):
        o = Err.lift(o)
        v = self.v - o.v
        return Err(v, self.e + o.e + EPS * np.abs(v))

    def __rsub__(self, o):
        return Err.lift(o) - self

    def __neg__(self):
        return Err(-self.v, self.e)

    def __mul__(self, o):
        o = Err.lift(o)
        v = self.v * o.v
        return Err(v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e + EPS * np.abs(v))

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Err.lift(o)
        v = self.v / o.v
        return Err(v, (self.e + np.abs(v) * o.e) / (np.abs(o.v) - o.e) + EPS * np.abs(v))

    def __rtruediv__(self, o):
        return Err.lift(o) / self

    def where(self, mask, other):
        other = Err.lift(other)
        return Err(np.where(mask, self.v, other.v), np.where(mask, self.e, other.e))


def e_exp(x):
    v = np.exp(x.v)
    return Err(v, v * np.expm1(x.e) + 2.0 * EPS * v)


def e_sin(x):
    v = np.sin(x.v)
    return Err(v, x.e + 3.0 * EPS * np.abs(v))


def e_cos(x):
    v = np.cos(x.v)
    return Err(v, x.e + 3.0 * EPS * np.abs(v))


def e_sqrt(x):
    v = np.sqrt(x.v)
    return Err(v, x.e / (2.0 * np.sqrt(np.maximum(x.v - x.e, 1e-300))) + EPS * v)


def e_pow(x, y):
    y = Err.lift(y)
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.power(x.v, y.v)
        ylogx = np.abs(y.v * np.log(x.v))
        e = v * (np.abs(y.v) * x.e / (np.abs(x.v) - x.e) + np.abs(np.log(x.v)) * y.e) + \
            2.5 * (1.0 + ylogx) * EPS * np.abs(v)
    return Err(v, e)


def e_max0(x):
    return Err(np.maximum(x.v, 0.0), x.e)


def _transform_err(case: Case, X):
    """affine_transform in the error arithmetic: the translation is the same operation on the same doubles on both
    sides (exact); the cosines of the rolls are formed on the host from the normalised direction -- two square roots
    and two divisions away from numpy's: 4 EPS each"""
    y = [Err(X[:, d] - case.pos()[d]) for d in range(case.dim)]
    roll_z, roll_y = _rolls(case.dir())
    coeff = lambda c: Err(c, 4.0 * EPS * abs(c))  # noqa: E731
    if roll_z is not None:
        n_x, n_z = coeff(roll_z[0]), coeff(roll_z[1])
        y[0], y[2] = n_x * y[0] + n_z * y[2], -n_z * y[0] + n_x * y[2]
    if roll_y is not None:
        n_x, n_y = coeff(roll_y[0]), coeff(roll_y[1])
        y[0], y[1] = n_x * y[0] + n_y * y[1], -n_y * y[0] + n_x * y[1]
    return y


def _rotate_err(case: Case, m):
    roll_z, roll_y = _rolls(case.dir())
    coeff = lambda c: Err(c, 4.0 * EPS * abs(c))  # noqa: E731
    if roll_y is not None:
        n_x, n_y = coeff(roll_y[0]), coeff(roll_y[1])
        m[0], m[1] = n_x * m[0] - n_y * m[1], n_y * m[0] + n_x * m[1]
    if roll_z is not None:
        n_x, n_z = coeff(roll_z[0]), coeff(roll_z[1])
        m[0], m[2] = n_x * m[0] - n_z * m[2], n_z * m[0] + n_x * m[2]
    return m


def _euler_primitive_err(case: Case, x, t, gamma):
    """(rho, v1, v2, p) in the frame of the state"""
    n = len(x[0].v)
    zero = Err(np.zeros(n))
    const = lambda c: Err(np.full(n, c))  # noqa: E731
    if case.name == "uniform":
        rho0, u0, p0 = case.get("primitive state")
        return const(rho0), const(u0), zero, const(p0)
    if case.name == "radial contrast":
        inner, outer = case.get("primitive state inner"), case.get("primitive state outer")
        inside = np.sqrt(sum(c.v * c.v for c in x)) <= case.get("radius")
        return tuple(const(inner[q]).where(inside, const(outer[q])) for q in (0, 1)) + \
            (zero, const(inner[2]).where(inside, const(outer[2])))
    if case.name == "isentropic vortex":
        mach, beta = case.get("mach number"), case.get("beta")
        xb, yb = x[0] - Err(mach) * t, x[1]
        r2 = xb * xb + yb * yb
        factor = (Err(beta) / (Err(2.0) * np.pi)) * e_exp(0.5 - 0.5 * r2)
        T = 1.0 - (Err(gamma) - 1.0) / (2.0 * Err(gamma)) * factor * factor
        u, v = mach - factor * yb, factor * xb
        rho = e_pow(T, 1.0 / (Err(gamma) - 1.0))
        return rho, u, v, e_pow(rho, gamma)
    if case.name == "leblanc":
        xx = x[0]
        s_left, s_fan, s_contact, s_shock = LEBLANC_SPEEDS
        left = xx.v <= s_left * t
        fan = ~left & (xx.v < s_fan * t)
        pre = ~left & ~fan & (xx.v < s_contact * t)
        post = ~left & ~fan & ~pre & (xx.v < s_shock * t)
        with np.errstate(divide="ignore", invalid="ignore"):
            chi = xx / Err(np.where(fan, t, 1.0))
        b = 0.75 - 0.75 * chi
        b3 = b * b * b
        b3 = Err(b3.v, b3.e + EPS * np.abs(b3.v))            # numpy: one pow instead of two products
        b5 = b3 * b * b
        b5 = Err(b5.v, b5.e + EPS * np.abs(b5.v))
        rho = const(1.0e-3).where(~(left | fan | pre | post), const(0.0))
        u, pr = zero, const(2.0 / 3.0 * 1.0e-10).where(~(left | fan | pre | post), const(0.0))
        rho = const(1.0).where(left, b3.where(fan, const(5.4079335349316249e-02).where(
            pre, const(3.9999980604299963e-03).where(post, rho))))
        u = (0.75 * (1.0 / 3.0 + chi)).where(fan, const(0.62183867139173454).where(pre | post, zero))
        pr = const(2.0 / 3.0 * 1.0e-1).where(left, ((1.0 / 15.0) * b5).where(fan, const(
            0.51557792765096996e-03).where(pre | post, pr)))
        return rho, u, zero, pr
    # rarefaction: the constants are formed on the host with the C library, in numpy on the other side
    g = Err(gamma)
    rho_l, p_l = Err(3.0), Err(1.0)
    c_l = e_sqrt(g * p_l / rho_l)
    u_l = c_l
    rho_r = Err(0.5)
    p_r = e_pow(rho_r / rho_l, g) * p_l
    c_r = e_sqrt(g * p_r / rho_r)
    u_r = u_l + 2.0 * (c_l - c_r) / (g - 1.0)
    k1 = 2.0 / (g + 1.0)
    k2 = (g - 1.0) / ((g + 1.0) * c_l)
    k3 = c_l + ((g - 1.0) / 2.0) * u_l
    tt = 0.2 / (u_r - u_l) + t
    xx = x[0]
    chi = xx / tt
    left = xx.v <= (tt * (u_l - c_l)).v
    fan = ~left & (xx.v <= (tt * (u_r - c_r)).v)
    with np.errstate(invalid="ignore"):
        base = k1 + k2 * (u_l - chi)
        base = Err(np.where(fan, base.v, 1.0), np.where(fan, base.e, 0.0))
        rho_f = rho_l * e_pow(base, 2.0 / (g - 1.0))
        p_f = p_l * e_pow(base, 2.0 * g / (g - 1.0))
    bc = lambda c: Err(np.full(n, c.v), np.full(n, c.e))  # noqa: E731
    rho = bc(rho_l).where(left, rho_f.where(fan, bc(rho_r)))
    u = bc(u_l).where(left, (k1 * (k3 + chi)).where(fan, bc(u_r)))
    pr = bc(p_l).where(left, p_f.where(fan, bc(p_r)))
    return rho, u, zero, pr


def _eos_energy_err(p, rho, pr):
    g = Err(p.gamma)
    if p.eos == capi.EOS_POLYTROPIC_GAS:
        return pr / (rho * (g - 1.0))
    assert p.eos == capi.EOS_NOBLE_ABEL_STIFFENED_GAS
    return p.eos_q + (pr + g * p.eos_pinf) * (1.0 - p.eos_covolume_b * rho) / (rho * (g - 1.0))


def _sw_err(case: Case, x, t, p):
    """(h, m1, m2) in the frame of the state"""
    n = len(x[0].v)
    zero = Err(np.zeros(n))
    const = lambda c: Err(np.full(n, c))  # noqa: E731
    g, k = p.gravity, p.manning_friction_coefficient
    if case.name == "circular dam break":
        inside = sum(c.v * c.v for c in x) <= case.get("radius")
        return const(case.get("dam amplitude")).where(inside, const(case.get("still water depth"))), zero, zero
    if case.name == "paraboloid":
        a, h0 = Err(case.get("free surface radius")), Err(case.get("water height"))
        length, B = case.get("paraboloid length"), Err(case.get("speed"))
        xc = x[0] - 0.5 * length
        z = h0 / (a * a) * (xc * xc)
        pp = e_sqrt(8.0 * Err(g) * h0) / a
        s = e_sqrt(pp * pp - Err(k) * k) / 2.0
        term1 = (a * a * B * B) / (8.0 * Err(g) * g * h0) * e_exp(Err(-k * t))
        term1 = term1 * ((0.25 * Err(k) * k - s * s) * e_cos(2.0 * s * t) - s * k * e_sin(2.0 * s * t))
        term2 = -(B * B / (4.0 * Err(g))) * e_exp(Err(-k * t))
        term3 = -(B / g) * e_exp(Err(-0.5 * k * t))
        term3 = term3 * (s * e_cos(s * t) + 0.5 * k * e_sin(s * t)) * xc
        h = e_max0((h0 - z) + (term1 + term2 + term3))
        v = B * e_exp(Err(-0.5 * k * t)) * e_sin(s * t)
        return h, h * v, zero
    if case.name == "ritter dam break":
        aL = e_sqrt(Err(g) * case.get("left water depth"))
        ts = Err(t + case.get("time initial"))
        xA, xB = -ts * aL, 2.0 * ts * aL
        left = x[0].v <= xA.v
        fan = ~left & (x[0].v <= xB.v)
        tmp = aL - x[0] / (2.0 * ts)
        h_exp = 4.0 / (9.0 * Err(g)) * tmp * tmp
        v_exp = 2.0 / 3.0 * (x[0] / ts + aL)
        h = const(case.get("left water depth")).where(left, h_exp.where(fan, zero))
        return h, (h_exp * v_exp).where(fan, zero), zero
    if case.name == "smooth vortex":
        mach, beta = case.get("mach number"), case.get("beta")
        xb, yb = x[0] - Err(mach) * t, x[1]
        r2 = xb * xb + yb * yb
        factor = (Err(beta) / (Err(2.0) * np.pi)) * e_exp(0.5 - 0.5 * r2)
        h = case.get("reference depth") - 1.0 / (2.0 * Err(g)) * factor * factor
        return h, h * (mach - factor * yb), h * (factor * xb)
    n_m, slope, q0 = Err(k), Err(case.get("ramp slope")), Err(case.get("initial discharge"))
    h = e_pow(n_m * n_m * q0 * q0 / slope, 1.0 / (Err(2.0) + 4.0 / 3.0))
    return Err(np.full(n, h.v), np.full(n, h.e)), const(q0.v), zero


def tolerance(case: Case, X, t):
    """(values [n, k] of the error arithmetic, bound [n, k] on |device - numpy|)"""
    X = np.asarray(X, dtype=np.float64)
    p = make_params(case.equation, case.dim, **case.edits)
    dim = case.dim
    x = _transform_err(case, X)
    zero = Err(np.zeros(len(X)))
    if case.equation == capi.EQ_SHALLOW_WATER:
        h, m1, m2 = _sw_err(case, x, t, p)
        m = _rotate_err(case, [m1, m2, zero][:dim])
        comps = [h, *m]
    else:
        gamma = state_gamma(case, p)
        rho, v1, v2, pr = _euler_primitive_err(case, x, t, gamma)
        m = _rotate_err(case, [rho * v1, rho * v2, zero][:dim])
        kinetic = 0.5 * rho * (v1 * v1 + v2 * v2)
        if case.equation == capi.EQ_EULER_AEOS:
            E = rho * _eos_energy_err(p, rho, pr) + kinetic
        else:
            E = pr / (Err(gamma) - 1.0) + kinetic
        comps = [rho, *m, E]
    return np.column_stack([c.v for c in comps]), np.column_stack([c.e for c in comps])


# --------------------------------------------------------------------------- meshes and cases of tests B - D

def interval(n_cells, lower, upper, bc_left, bc_right):
    return offline.SyntheticOffline(offline.MeshSpec(1, (n_cells,), (lower,), (upper,), (bc_left, bc_right),
                                                     name="interval"))


VORTEX = Case("euler isentropic vortex", capi.EQ_EULER, 2, "isentropic vortex", {"mach number": 1.0, "beta": 5.0},
              (1.0, 1.0), (-1.0, -1.0), edits=dict(cfl=0.3))
LEBLANC_EDITS = dict(gamma=1.66666666666667, limiter_relaxation_factor=8.0, cfl=0.1)
LEBLANC = Case("euler leblanc", capi.EQ_EULER, 1, "leblanc", position=(0.326732673267,), edits=LEBLANC_EDITS)
AEOS_LEBLANC = Case("aeos leblanc", capi.EQ_EULER_AEOS, 1, "leblanc", position=(0.326732673267,),
                    edits=dict(LEBLANC_EDITS, eos=capi.EOS_POLYTROPIC_GAS, compute_strict_bounds=0,
                               indicator_evc_factor=0.0))
INCLINE = Case("sw steady incline", capi.EQ_SHALLOW_WATER, 1, "sloping friction",
               {"ramp slope": 1.0e-2, "initial discharge": 1.0e-1},
               edits=dict(gravity=9.81, manning_friction_coefficient=1.0e-2, reference_water_depth=1.0,
                          dry_state_relaxation_factor=0.2, dry_state_relaxation_small=1e4,
                          dry_state_relaxation_large=1e4, cfl=0.5))


def vortex_mesh(n=32, ny=None, bc=capi.BC_DIRICHLET):
    return offline.SyntheticOffline(offline.rectangle_2d(n, (-5.0, -5.0), (5.0, 5.0), bc=bc, ny=ny))


def incline_mesh(n_cells=200):
    off = interval(n_cells, 0.0, 20.0, capi.BC_DYNAMIC, capi.BC_DYNAMIC)
    off.set_initial_precomputed(ist.sw_sloping_friction(off.positions, ramp_slope=1.0e-2)[1])
    return off


N_TEMPS = {"erk 43": 4, "erk 54": 5}


def run_driver(m, case: Case, U0, scheme, n_steps, device: bool, cfl_recovery="none", cfl_min=None, cfl_max=None,
               b_positions=None):
    """n_steps Runge-Kutta steps from the uploaded state U0: ryujin_hip_time_step_iv (device=True) or
    ryujin_hip_time_step_fn with a callback that returns initial_values_evaluate(b_positions, time) -- the same device
    function on the same doubles. Returns (states after every step, taus, n_restarts)."""
    cfl = case.edits.get("cfl", 0.2)
    cfl_min = cfl if cfl_min is None else cfl_min
    cfl_max = cfl if cfl_max is None else cfl_max
    m.cfl = cfl_max
    bpos = m.offline.b_positions if b_positions is None else b_positions
    state = m.new_state_vector(U0)
    temps = [m.new_state_vector() for _ in range(N_TEMPS.get(scheme, 3))]
    fn = None if device else (lambda time: m.initial_values_evaluate(bpos, time))
    states, taus, t = [], [], 0.0
    for _ in range(n_steps):
        tau = m.time_step(scheme, state, temps, "device" if device else None, cfl_recovery=cfl_recovery,
                          cfl_min=cfl_min, cfl_max=cfl_max, t=t, dirichlet_fn=fn)
        t += tau
        taus.append(tau)
        states.append(state.download())
    return states, taus, m.n_restarts()


# GPU test D: the initial-values configuration of the reference's 1-D verification runs, keyed as
# tests/test_oracle_golden_verification.py::CASES
VERIFICATION = {
    "euler_leblanc_1d": ("leblanc", dict(position=(0.326732673267,))),
    "euler_rarefaction_1d": ("rarefaction", dict(position=(0.2,))),
    "sw_ritter_dam_break": ("ritter dam break", dict(position=(5.0,), time_initial=1.0, left_water_depth=0.005)),
    "sw_steady_incline": ("sloping friction", dict(ramp_slope=1.0e-2, initial_discharge=1.0e-1)),
}


def run_verification_on_device(config):
    """A stand-in for test_oracle_golden_verification.run_verification with the same signature and result: the
    initial state comes from initial_values_interpolate, every Runge-Kutta step is ryujin_hip_time_step_iv, the last
    prepare_state_vector takes its Dirichlet data on the device. `exact` stays the reference of the error norms."""
    import time

    import test_oracle_golden_verification as tv
    name, kwargs = config

    def run(backend, off, params, exact, components, scheme="erk 33", cfl=0.1, t_final=1.0, bathymetry=None,
            with_dirichlet=True):
        assert backend == "hip-iv" and off.dim == 1
        if bathymetry is not None:
            off.set_initial_precomputed(bathymetry)
        started = time.perf_counter()
        m = HyperbolicModule(off, params, backend="hip")
        m.initial_values_configure(name, **kwargs)
        sv = m.new_state_vector()
        m.initial_values_interpolate(sv, 0.0)
        from ryujin_amd.module import DeviceResidentTimeIntegrator
        ti = DeviceResidentTimeIntegrator(m, scheme, cfl_min=cfl, cfl_max=cfl, cfl_recovery_strategy="none",
                                          dirichlet="device")
        t, n_steps = 0.0, 0
        while t < t_final:
            sv, tau = ti.step(sv, t)
            t += tau
            n_steps += 1
        m.prepare_state_vector(sv, t, "device")
        U, A = sv.download(), exact(off.positions, t)
        run.seconds = time.perf_counter() - started
        h = (off.spec.upper[0] - off.spec.lower[0]) / off.spec.n_cells[0]
        order = np.argsort(off.positions[:, 0])
        linf = l1 = l2 = 0.0
        for c in components:
            a, e = A[order, c], (U[order, c] - A[order, c])
            (l1a, l2a), (l1e, l2e) = tv.norms_1d(a, h), tv.norms_1d(e, h)
            linf += np.abs(e).max() / np.abs(a).max()
            l1 += l1e / l1a
            l2 += l2e / l2a
        return dict(t=t, linf=linf, l1=l1, l2=l2, dofs=off.n_owned, n_steps=n_steps, warnings=m.n_warnings(),
                    restarts=m.n_restarts())

    run.seconds = float("nan")
    return run
