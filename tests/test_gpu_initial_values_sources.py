"""Every (state source, Description) pair the host can select for the device-resident InitialValues
(ryujin_amd/csrc/kernels_initial_values.hpp: k_initial_state_points<Source>, k_initial_state_dirichlet<Source>;
ryujin_hip.hip: with_initial_state_source), once each on the smallest all-Dirichlet mesh of its dimension:

  analytic and library     Euler 1/2/3, EulerAEOS 1/2/3, shallow water 1/2
  bathymetry               shallow water 1/2
  function                 Euler, EulerAEOS and scalar conservation 1/2/3, shallow water 1/2
  eos-function             EulerAEOS 1/2/3, an analytic state on a context with the function equation of state
  library-eos-function     EulerAEOS 1/2/3, a library state on such a context

The three consumers of one source give the same bits: interpolate + download == evaluate(positions) on every row,
prepare_state_vector with device Dirichlet data leaves evaluate(b_positions) in the boundary rows, and evaluate at 65
points (one block and one lane: 63 inactive lanes in the second block, which an interpreted source keeps until its
interpreter has run) equals evaluate of the same points one at a time. No time stepping: the stage time with c != 0
is covered by test_time_step_iv_equals_the_callback_path_bit_for_bit of each family.

The pad lane of an odd state (k = 1, 3, 5: K != KP) is written by the same kernel, but no entry point of the library
hands it out: state_download copies K doubles per row. It is not asserted here."""
import dataclasses

import numpy as np
import pytest

import helpers_eos_function as he
import helpers_initial_values as hiv
import helpers_initial_values_bathymetry as hb
import helpers_initial_values_library as hl
from ryujin_amd import HyperbolicModule, capi

pytestmark = pytest.mark.gpu

EULER, AEOS, SW, SCALAR = capi.EQ_EULER, capi.EQ_EULER_AEOS, capi.EQ_SHALLOW_WATER, capi.EQ_SCALAR_CONSERVATION
T = 0.2     # inside the ramp of "ramp up", the fans of the Riemann solutions open


def _analytic(tag, dim):
    """a state of helpers_initial_values.function_cases() that depends on position and time"""
    if tag == "sw":
        label = {1: "sw ritter dam break 1d", 2: "sw smooth vortex"}[dim]
    else:
        label = {1: f"{tag} rarefaction 1d", 2: f"{tag} isentropic vortex", 3: f"{tag} leblanc 3d (1,1,1)"}[dim]
    case = next(c for c in hiv.function_cases() if c.label == label)
    if label == "sw ritter dam break 1d":
        case = dataclasses.replace(case, position=(0.5,))      # the fan lies on the mesh [0, 1]
    return case


def _library(tag, dim):
    if tag == "sw":
        label = f"sw contrast {dim}d" + ("" if dim == 1 else " (1,1)")
        return next(c for c in hl.function_cases() if c.label == label)
    eq, edits = {"euler": (EULER, {}), "aeos-nasg": (AEOS, hiv.NASG)}[tag]
    return hl._case(tag, eq, edits, "ramp up", dim)


def _bathymetry(dim):
    """`position` moves the corner of the mesh onto the bump (1-D) and between the bumps (2-D)"""
    if dim == 1:
        return hb._case("flow over bump", 1, {}, "shift")
    return dataclasses.replace(hb._case("three bumps dam break", 2, {"cone magnitude": 0.75}, "shift"),
                               position=(-29.5, -5.5))


FUNCTION_EDITS = {EULER: {}, AEOS: hiv.NASG, SW: dict(gravity=9.81), SCALAR: {}}


def _function_expressions(equation, dim):
    """a positive density / depth / scalar, a velocity in every coordinate the dimension has, a positive last
    component where the Description has one; all of them move in time"""
    n = len(capi.function_expression_names(equation, dim))
    velocity = ["0.1 * x + 0.25 * t", "0.1 * y - 0.5 * t", "0.2 * z * t"][:dim]
    return (["1.5 + 0.5 * sin(x - t)"] + velocity + ["2 + 0.1 * cos(x + t)"])[:n]


def _eos_function_module(case):
    """NASG written as expressions, the state configured before it"""
    m = hiv.module_for(case)
    m.eos_configure_function(**he.member_expressions(hiv.make_params(case.equation, case.dim, **case.edits)))
    return m


def _function_module(equation, dim):
    m = HyperbolicModule(hiv.tiny_mesh(dim), hiv.make_params(equation, dim, **FUNCTION_EDITS[equation]), backend="hip")
    m.initial_values_configure_function(_function_expressions(equation, dim), direction=(1.0,) * dim, position=(0.25, -0.125, 0.0625)[:dim])
    return m


def _sources():
    out = []
    for tag, dims in (("euler", (1, 2, 3)), ("aeos-nasg", (1, 2, 3)), ("sw", (1, 2))):
        out += [(f"analytic {tag} {dim}d", lambda tag=tag, dim=dim: hiv.module_for(_analytic(tag, dim))) for dim in dims]
        out += [(f"library {tag} {dim}d", lambda tag=tag, dim=dim: hl.module_for(_library(tag, dim))) for dim in dims]
    out += [(f"bathymetry sw {dim}d", lambda dim=dim: hb.module_for(_bathymetry(dim))) for dim in (1, 2)]
    for tag, eq, dims in (("euler", EULER, (1, 2, 3)), ("aeos-nasg", AEOS, (1, 2, 3)), ("scalar", SCALAR, (1, 2, 3)),
                          ("sw", SW, (1, 2))):
        out += [(f"function {tag} {dim}d", lambda eq=eq, dim=dim: _function_module(eq, dim)) for dim in dims]
    out += [(f"eos-function {dim}d", lambda dim=dim: _eos_function_module(_analytic("aeos-nasg", dim)))
            for dim in (1, 2, 3)]
    out += [(f"library-eos-function {dim}d",
             lambda dim=dim: hl.module_for(hl._case("aeos-fn", AEOS, hiv.NASG, "shock front", dim, eos_function=True)))
            for dim in (1, 2, 3)]
    return out


SOURCES = _sources()


@pytest.mark.parametrize("make", [s[1] for s in SOURCES], ids=[s[0] for s in SOURCES])
def test_the_consumers_of_every_source_give_the_same_bits(make):
    m = make()
    off = m.offline
    assert (off.b_id == capi.BC_DIRICHLET).all() and off.n_bdry >= 2

    expected = m.initial_values_evaluate(off.positions, T)
    assert expected.shape == (off.n_relevant, m.k)
    assert np.isfinite(expected).all() and np.abs(expected).max() > 0.0
    sv = m.new_state_vector(np.full((off.n_relevant, m.k), np.nan))
    m.initial_values_interpolate(sv, T)
    np.testing.assert_array_equal(sv.download(), expected)

    U0 = 1.5 * m.initial_values_evaluate(off.positions, 0.0)    # admissible, and not the boundary data
    if m.params.equation == SW:
        U0[:, 0] += 1.0                                         # a dry node of the state is wet here
    boundary = m.initial_values_evaluate(off.b_positions, T)
    assert (U0[off.b_i] != boundary).any(axis=1).all()
    a = m.new_state_vector(U0)
    m.prepare_state_vector(a, T, "device")
    np.testing.assert_array_equal(a.download()[off.b_i], boundary)

    X = np.random.default_rng(7).uniform(-1.0, 1.0, size=(65, m.dim))
    together = m.initial_values_evaluate(X, T)
    assert np.isfinite(together).all()
    one_by_one = np.concatenate([m.initial_values_evaluate(X[i:i + 1], T) for i in range(65)])
    np.testing.assert_array_equal(together, one_by_one)
    m.close()
