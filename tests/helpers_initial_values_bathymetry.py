"""Yardsticks of tests/test_gpu_initial_values_bathymetry.py and tests/test_initial_values_bathymetry_cpu.py: the numpy
side of the shallow-water states that bring their own bathymetry (capi.IV_BATHYMETRY_STATES,
ryujin_amd/csrc/initial_states_bathymetry_device.hpp) and of the bed of every shallow-water state. The affine transform,
the error arithmetic Err and the meshes come from tests/helpers_initial_values.py.

reference(): ryujin_amd.initial_states (sw_flow_over_bump, sw_three_bumps_dam_break, sw_hou_test, sw_transient,
sw_soliton: the specification) behind affine_transform; a state is (h, q), the discharge along the first axis of the
frame, rotated back. Returns the conserved states and the bed.

tolerance(): the same statements in the error arithmetic of helpers_initial_values (its docstring, 3.). Beyond
+ - * / and sqrt (1 ulp) enter: pow (B_pow of e_pow: the host's for cBer, the device's dev_pow for (-Q)^-1.5), acos
(condition 1 / sqrt(1 - a^2); 2 ulp of the device's library + 1 of the host's = 3), cos (3 ulp), cosh (condition
sinh; 3 ulp). max and min of two values carry the larger of the two bounds: |max(a, b) - max(a', b')| <=
max(|a - a'|, |b - b'|), whichever operand either side selects -- a continuous kink needs no clearance.

boundaries(): where a state or its bed JUMPS or switches formula, in the coordinate the device compares:
    flow over bump          x' = 8, 12 (the bed's support), x' = 10 and 11.7 (the roots of the transcritical flow);
                            transcritical and t >= 1e-12: also 1 - |a| >= 1e-3 for the argument a of acos
    three bumps dam break   x' = 16 (the dam)
    hou test                x' = -100, (x' - 200)^2 + (y' + 10)^2 = 1000, |x' - 380| = 40, |y' - 50| = 40
    transient experiments   x' = 1e-8, x' = 0, x' = 3.26, the rectangle's |u + v| + |u - v| = 1; G3: y' = +-(semi circle
                            - 0.12) and |x' - xc| = 0.155
    soliton                 none
points_for() draws in the FRAME of the state, maps the draw to the lab frame, and keeps the first 1000 points whose
HOST values are clear of every boundary; the tests assert the clearance again on the points they use.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

import helpers_initial_values as hiv
from helpers_initial_values import EPS, Err, affine_transform, affine_transform_vector, e_cos, e_pow, e_sqrt
from ryujin_amd import HyperbolicModule, capi
from ryujin_amd import initial_states as ist

G = 9.81
NEW_STATES = ("flow over bump", "three bumps dam break", "hou test", "transient experiments", "soliton")
DIMS = {"flow over bump": (1, 2), "three bumps dam break": (1, 2), "hou test": (2,), "transient experiments": (2,),
        "soliton": (1, 2)}
# the frame's box per axis
BOX = {"flow over bump": ((5.0, 15.0), (-1.0, 1.0)), "three bumps dam break": ((0.0, 75.0), (0.0, 30.0)),
       "hou test": ((-400.0, 500.0), (-150.0, 150.0)), "transient experiments": ((-0.5, 4.5), (-0.3, 0.3)),
       "soliton": ((-10.0, 10.0), (-1.0, 1.0)), "paraboloid": ((0.0, 10000.0),), "sloping friction": ((0.0, 20.0),)}
# t = 0, one below and one above the state's switch (t < 1e-12; t <= 1e-10); no switch: the wave has moved
TIMES = {"flow over bump": (0.0, 5.0e-13, 1.0), "three bumps dam break": (0.0, 5.0e-11, 1.0)}
ACOS_MARGIN = 1.0e-3


@dataclass
class Case(hiv.Case):
    """helpers_initial_values.Case for a shallow-water state of capi.IV_BATHYMETRY_STATES or capi.IV_STATES"""

    def key(self):
        return ("shallow water", self.name)

    def spec(self):
        if self.key() in capi.IV_BATHYMETRY_STATES:
            return capi.IV_BATHYMETRY_STATES[self.key()][1]
        return capi.IV_STATES[self.name][2]

    def get(self, pname):
        return self.params.get(pname, {p[0]: p[2] for p in self.spec()}[pname])


def _case(name, dim, params, transform, suffix=""):
    direction, position = {
        "shift": (None, (0.25, -0.125)[:dim]),
        "rotated": ((1.0, 1.0)[:dim], (0.25, -0.125)[:dim]),
    }[transform]
    label = f"{name} {dim}d {transform}" + (f" {suffix}" if suffix else "")
    return Case(label, capi.EQ_SHALLOW_WATER, dim, name, dict(params), direction, position, edits=dict(gravity=G),
                times=TIMES.get(name, (0.0, 0.15, 0.4)))


def function_cases():
    """GPU test A: every new state in every dimension it has, each behind a non-zero `position` (the transform is the
    same subtraction on both sides: the polynomial beds are bit for bit) and, in 2-D, once more along (1, 1)"""
    cases = []
    variants = {
        "flow over bump": [({}, "transcritical"), ({"flow type": "subsonic"}, "subsonic")],
        "three bumps dam break": [({"cone magnitude": 0.75}, ""),
                                  ({"well balancing validation": True, "right water depth": 0.5}, "validation")],
        "hou test": [({}, "")],
        "transient experiments": [({"flow state left": (1.25, 0.5), "flow state right": (0.75, -0.25),
                                    "experimental configuration": which}, which) for which in ("G1", "G2", "G3", "none")],
        "soliton": [({"still water depth": 1.5, "amplitude": 0.25}, "")],
    }
    for name in NEW_STATES:
        for dim in DIMS[name]:
            for params, suffix in variants[name]:
                cases.append(_case(name, dim, params, "shift", suffix))
            if dim == 2:
                cases.append(_case(name, dim, variants[name][0][0], "rotated"))
    return cases


def module_for(case: Case, off=None, bc=capi.BC_DIRICHLET):
    off = hiv.tiny_mesh(case.dim, bc) if off is None else off
    m = HyperbolicModule(off, hiv.make_params(case.equation, case.dim, **case.edits), backend="hip")
    hiv.configure(m, case)
    return m


def is_transcritical(case: Case):
    return case.name == "flow over bump" and case.get("flow type") == "transcritical"


# --------------------------------------------------------------------------- the region boundaries

def boundaries(case: Case, X):
    """[(coordinate per point, boundary value), ...] of the docstring's table"""
    Xt = affine_transform(case.dir(), case.pos(), X)
    x = Xt[:, 0]
    y = Xt[:, 1] if case.dim == 2 else None
    name = case.name
    if name == "flow over bump":
        return [(x, 8.0), (x, 12.0), (x, ist.FLOW_OVER_BUMP_XM), (x, ist.FLOW_OVER_BUMP_XS)]
    if name == "three bumps dam break":
        return [(x, 16.0)]
    if name == "hou test":
        return [(x, -100.0), ((x - 200.0) * (x - 200.0) + (y + 10.0) * (y + 10.0), 1000.0),
                (np.abs(x - 380.0), 40.0), (np.abs(y - 50.0), 40.0)]
    if name == "transient experiments":
        which = case.get("experimental configuration")
        out = [(x, 1.0e-8), (x, 0.0), (x, 326.0 / 100.0)]
        if which == "none":
            return out
        out.append((ist._transient_rectangle(x, y, ist.TRANSIENT_CENTERS["G1" if which == "G1" else "rectangle"]), 1.0))
        if which == "G3":
            xc = ist.TRANSIENT_CENTERS["G3"]
            semi = ist._transient_semi_circle(x, xc)
            out += [(y - (semi - 24.0 / 2.0 / 100.0), 0.0), (y - (-semi + 24.0 / 2.0 / 100.0), 0.0),
                    (np.abs(x - xc), ist.TRANSIENT_HALF_WIDTH)]
        return out
    return []


def jump_clearance(case: Case, X):
    """min over the boundaries of |coordinate - boundary| - 1e-9 (1 + |coordinate|), per point (> 0: clear); for the
    transcritical flow over the bump also (1 - |a|) - 1e-3 with a the argument of acos; +inf without a boundary. None
    of these boundaries moves in time."""
    out = np.full(len(X), np.inf)
    for coordinate, bound in boundaries(case, X):
        out = np.minimum(out, np.abs(coordinate - bound) - 1.0e-9 * (1.0 + np.abs(coordinate)))
    if is_transcritical(case):
        Xt = affine_transform(case.dir(), case.pos(), X)
        a = ist.sw_flow_over_bump_acos_argument(Xt, G, "transcritical")
        out = np.minimum(out, (1.0 - np.abs(a)) - ACOS_MARGIN)
    return out


def assert_clear_of_jumps(case: Case, X):
    clearance = jump_clearance(case, X)
    assert (clearance > 0.0).all(), (case.label, int((clearance <= 0.0).sum()))


def points_for(case: Case, n=1000, seed=5):
    rng = np.random.default_rng(seed)
    box = BOX[case.name][: case.dim]
    frame = np.column_stack([rng.uniform(lo, hi, size=2 * n) for lo, hi in box])
    # the lab frame: rotate the draw along `direction`, shift by `position` (the transform back is the device's job)
    X = affine_transform_vector(case.dir(), frame) + np.asarray(case.pos())
    X = X[jump_clearance(case, X) > 0.0][:n]
    assert len(X) == n, (case.label, len(X))
    return np.ascontiguousarray(X)


# --------------------------------------------------------------------------- the expected states and beds

def frame_state(case: Case, Xt, t, gravity=G):
    """((h, q) [n, 2], bed [n]) in the frame of the state through ryujin_amd.initial_states"""
    name = case.name
    if name == "flow over bump":
        return ist.sw_flow_over_bump(Xt, t, gravity, case.get("flow type"))
    if name == "three bumps dam break":
        return ist.sw_three_bumps_dam_break(Xt, t, gravity, case.get("well balancing validation"),
                                            case.get("left water depth"), case.get("right water depth"),
                                            case.get("cone magnitude"))
    if name == "hou test":
        return ist.sw_hou_test(Xt, case.get("reservoir water depth"))
    if name == "transient experiments":
        return ist.sw_transient(Xt, case.get("flow state left"), case.get("flow state right"),
                                case.get("experimental configuration"))
    assert name == "soliton"
    return ist.sw_soliton(Xt, t, gravity, case.get("still water depth"), case.get("amplitude"))


def reference(case: Case, X, t):
    """(conserved states [n, k], bed [n]) at the points X [n, dim]"""
    X = np.asarray(X, dtype=np.float64)
    n, dim = X.shape
    Xt = affine_transform(case.dir(), case.pos(), X)
    hq, bed = frame_state(case, Xt, t, case.edits.get("gravity", G))
    m = np.zeros((n, dim))
    m[:, 0] = hq[:, 1]
    return np.column_stack([hq[:, 0], affine_transform_vector(case.dir(), m)]), bed


def reference_bed(case: Case, X):
    """the bed of ANY shallow-water state at the points X: the restatement for the seven states that have one, zeros
    for the others"""
    X = np.asarray(X, dtype=np.float64)
    Xt = affine_transform(case.dir(), case.pos(), X)
    if case.name == "paraboloid":
        return ist.sw_paraboloid_1d_bathymetry(Xt, case.get("free surface radius"), case.get("water height"),
                                               case.get("paraboloid length"))
    if case.name == "sloping friction":
        return ist.sw_sloping_friction_bathymetry(Xt, case.get("ramp slope"))
    if case.name in NEW_STATES:
        return reference(case, X, 0.0)[1]
    return np.zeros(len(X))


# --------------------------------------------------------------------------- the derived tolerance

def _const(n, c):
    c = Err.lift(c)
    return Err(np.full(n, c.v), np.full(n, c.e))


def e_max(a, b):
    """std::max(a, b); see the module docstring"""
    a, b = Err.lift(a), Err.lift(b)
    return Err(np.where(a.v < b.v, b.v, a.v), np.maximum(a.e, b.e))


def e_min(a, b):
    a, b = Err.lift(a), Err.lift(b)
    return Err(np.where(b.v < a.v, b.v, a.v), np.maximum(a.e, b.e))


def e_abs(a):
    return Err(np.abs(a.v), a.e)


def e_acos(a):
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.arccos(a.v)
        reach = np.minimum(np.abs(a.v) + a.e, 1.0)
        return Err(v, a.e / np.sqrt(1.0 - reach * reach) + 3.0 * EPS * np.abs(v))


def e_cosh(a):
    v = np.cosh(a.v)
    return Err(v, np.sinh(np.abs(a.v) + a.e) * a.e + 3.0 * EPS * v)


def _cube(a):
    return a * (a * a)


def _bed_err(case: Case, x):
    """the bed in the error arithmetic; x: the frame coordinates as Err"""
    n = len(x[0].v)
    zero = Err(np.zeros(n))
    name = case.name
    xx = x[0]
    yy = x[1] if case.dim == 2 else None
    if name == "paraboloid":
        a, h0 = Err(case.get("free surface radius")), Err(case.get("water height"))
        xc = xx - 0.5 * case.get("paraboloid length")
        return h0 / (a * a) * (xc * xc)
    if name == "sloping friction":
        return -(Err(case.get("ramp slope")) * xx)
    if name == "flow over bump":
        bump = (0.2 / 64.0) * _cube(xx - 8.0) * _cube(12.0 - xx)
        return bump.where((8.0 <= xx.v) & (xx.v <= 12.0), zero)
    if name == "three bumps dam break":
        magnitude = case.get("cone magnitude")
        if case.dim == 1:
            a = xx - 47.5
            return magnitude * e_max(3.0 - 3.0 / 10.0 * e_sqrt(a * a), zero)
        z = [top - slope * e_sqrt((xx - cx) * (xx - cx) + (yy - cy) * (yy - cy))
             for cx, cy, top, slope in ist.THREE_BUMPS_CONES_2D]
        return magnitude * e_max(e_max(e_max(z[0], z[1]), z[2]), zero)
    if name == "hou test":
        xp, xm, y50 = xx + 250.0, xx - 250.0, yy - 50.0
        base1 = xp * xp / 1600.0 + yy * yy / 400.0
        base2 = xx * xx / 225.0 + y50 * y50 / 225.0
        base3 = xm * xm / 1225.0 + yy * yy / 225.0 - 10.0
        base = e_min(e_min(base1, base2), base3)
        bump1 = 80.0 - xp * xp / 50.0 - yy * yy / 50.0
        bump2 = _const(n, 10.0).where(((xx.v - 200.0) ** 2 + (yy.v + 10.0) ** 2) <= 1000.0, zero)
        bump3 = _const(n, 20.0).where((np.abs(xx.v - 380.0) <= 40.0) & (np.abs(yy.v - 50.0) <= 40.0), zero)
        return e_max(base, e_max(e_max(bump1, bump2), bump3))
    if name == "transient experiments":
        knee = 326.0 / 100.0
        slope = -0.0404 * (xx - knee) - 0.00092 * 326.0 / 100.0
        bath = (-0.00092 * xx).where((xx.v >= 0.0) & (xx.v <= knee), slope.where(xx.v > knee, zero))
        which = case.get("experimental configuration")
        if which == "none":
            return bath

        def rectangle(xc):
            return ist._transient_rectangle(xx.v, yy.v, xc) <= 1.0

        def semi_circle(xc):
            ratio = (xx - xc) / ist.TRANSIENT_HALF_WIDTH
            number = 1.0 - ratio * ratio
            radicand = 0.5 * (e_abs(number) + number)
            # sqrt at 0: the bound of e_sqrt grows without limit there; sqrt(r) - sqrt(r') <= sqrt(|r - r'|)
            v = np.sqrt(radicand.v)
            e = np.minimum(e_sqrt(Err(np.maximum(radicand.v, 1e-300), radicand.e)).e, np.sqrt(radicand.e)) + EPS * v
            return 7.3 / 100.0 * Err(v, e)

        obstacle = zero
        seven = _const(n, 7.0 / 100.0)
        if which == "G1":
            obstacle = seven.where(rectangle(ist.TRANSIENT_CENTERS["G1"]), obstacle)
        elif which == "G2":
            obstacle = e_max(semi_circle(ist.TRANSIENT_CENTERS["G2"]), zero)
            obstacle = seven.where(rectangle(ist.TRANSIENT_CENTERS["rectangle"]), obstacle)
        else:
            xc = ist.TRANSIENT_CENTERS["G3"]
            semi = ist._transient_semi_circle(xx.v, xc)
            inside = np.abs(xx.v - xc) <= ist.TRANSIENT_HALF_WIDTH
            wall = _const(n, 21.0 / 100.0)
            obstacle = wall.where((yy.v < semi - 24.0 / 2.0 / 100.0) & inside, obstacle)
            obstacle = wall.where((yy.v > -semi + 24.0 / 2.0 / 100.0) & inside, obstacle)
            obstacle = seven.where(rectangle(ist.TRANSIENT_CENTERS["rectangle"]), obstacle)
        return bath + obstacle
    return zero


def _state_err(case: Case, x, t, g):
    """(h, q) in the frame of the state, in the error arithmetic"""
    n = len(x[0].v)
    zero = Err(np.zeros(n))
    name = case.name
    xx = x[0]
    if name == "flow over bump":
        bath = _bed_err(case, x)
        h_inflow, q_inflow = Err(0.28205279813802181), Err(0.18)
        cBer = 0.2 + 1.5 * e_pow(q_inflow * q_inflow / g, Err(1.0 / 3.0))
        if case.get("flow type") == "subsonic":
            q_inflow, h_inflow = Err(4.42), Err(2.0)
            ratio = q_inflow / h_inflow
            cBer = ratio * ratio / (2.0 * Err(g)) + h_inflow
        d = q_inflow * q_inflow / (2.0 * Err(g))
        q = _const(n, q_inflow)
        if t < 1.0e-12:
            return h_inflow - bath, q
        b = bath - cBer
        Q = -(b * b) / 9.0
        R = -(27.0 * d + 2.0 * _cube(b)) / 54.0
        theta = e_acos(e_pow(-Q, Err(-1.5)) * R)
        root = 2.0 * e_sqrt(-Q)
        h = root * e_cos(theta / 3.0) - b / 3.0
        if case.get("flow type") == "transcritical":
            second = root * e_cos((4.0 * np.pi + theta) / 3.0) - b / 3.0
            middle = (ist.FLOW_OVER_BUMP_XM <= xx.v) & (xx.v < ist.FLOW_OVER_BUMP_XS)
            h = second.where(middle, _const(n, ist.FLOW_OVER_BUMP_H_OUTFLOW).where(ist.FLOW_OVER_BUMP_XS < xx.v, h))
        return h, q
    if name == "three bumps dam break":
        left, right = case.get("left water depth"), case.get("right water depth")
        if t <= 1.0e-10 or case.get("well balancing validation"):
            h = _const(n, left).where(xx.v < 16.0, _const(n, right))
            return e_max(h - _bed_err(case, x), zero), zero
        a = e_sqrt(Err(g) * left)
        return _const(n, left), _const(n, left * a)
    if name == "hou test":
        h = e_max(case.get("reservoir water depth") - _bed_err(case, x), zero).where(xx.v < -100.0, zero)
        return h, zero
    if name == "transient experiments":
        east = xx.v > 1.0e-8
        left, right = case.get("flow state left"), case.get("flow state right")
        return tuple(_const(n, right[q]).where(east, _const(n, left[q])) for q in range(2))
    assert name == "soliton"
    depth, amp = Err(case.get("still water depth")), Err(case.get("amplitude"))
    celerity = e_sqrt(Err(g) * (amp + depth))
    width = e_sqrt(3.0 * amp / (4.0 * depth * depth * (amp + depth)))
    c = e_cosh(width * (xx - celerity * t))
    profile = depth + amp * (1.0 / (c * c))
    h = e_max(profile, zero)
    v = celerity * (profile - depth) / profile
    return h, h * v


def tolerance(case: Case, X, t):
    """(bound [n, k] on |device - numpy| of the conserved state, bound [n] of the bed)"""
    X = np.asarray(X, dtype=np.float64)
    x = hiv._transform_err(case, X)
    zero = Err(np.zeros(len(X)))
    h, q = _state_err(case, x, t, case.edits.get("gravity", G))
    m = hiv._rotate_err(case, [q, zero][: case.dim])
    return np.column_stack([c.e for c in [h, *m]]), _bed_err(case, x).e


def bed_tolerance(case: Case, X):
    return _bed_err(case, hiv._transform_err(case, np.asarray(X, dtype=np.float64))).e


def exact_transform(case: Case):
    """the affine transform of the case is the same subtraction on both sides (no roll that rounds)"""
    return case.direction is None


def bitwise_bed_mask(case: Case, X):
    """the points at which the bed is demanded bit for bit (exact_transform cases): three bumps dam break away from a
    cone's sqrt (the bed is the 0 of the max), all of hou test, transient experiments outside the half circle of G2 /
    G3; None for the other states"""
    Xt = affine_transform(case.dir(), case.pos(), X)
    if case.name == "three bumps dam break":
        return reference_bed(case, X) == 0.0
    if case.name == "hou test":
        return np.ones(len(X), dtype=bool)
    if case.name == "transient experiments":
        which = case.get("experimental configuration")
        if which in ("G2", "G3"):
            return np.abs(Xt[:, 0] - ist.TRANSIENT_CENTERS[which]) > ist.TRANSIENT_HALF_WIDTH
        return np.ones(len(X), dtype=bool)
    return None
