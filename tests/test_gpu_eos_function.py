"""The function equation of state of EulerAEOS on the device: the interpreter kernels of cycle 0 of the
precomputation (k_precompute_aeos0_function), of the analytic initial and Dirichlet states on a function-EOS context
and of ryujin_hip_eos_function_evaluate_device, against the host interpreter, against the closed-form members ON THE
SAME DEVICE bit for bit, and against the oracle.

The meshes are the smallest that meet every launch shape: 200 nodes in 1-D (a last slice of 8 lanes, Dirichlet rows),
47 x 48 nodes in 2-D (n_owned no multiple of 64), box_3d(10); boundary conditions folded into the pre-pass and as a
launch of their own; three ranks of the in-process transport, the middle one without a boundary in x."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np
import pytest

import helpers_eos_function as he
import helpers_expression as hx
import helpers_initial_values as hiv
from helpers_initial_values import EPS
from ryujin_amd import HyperbolicModule, capi, offline
from ryujin_amd.initial_states import aeos_from_primitive_state

pytestmark = pytest.mark.gpu


def mesh(dim, bc=capi.BC_DIRICHLET):
    if dim == 1:
        return offline.SyntheticOffline(offline.MeshSpec(1, (199,), (0.0,), (1.0,), (bc, bc)))
    if dim == 2:
        return offline.SyntheticOffline(offline.rectangle_2d(46, (-1.0, -1.0), (1.0, 1.0), ny=47, bc=bc))
    return offline.SyntheticOffline(offline.box_3d(10, bc=bc))


def smooth_state(positions):
    """an admissible state as a function of the position alone (the same on every partition): rho in [0.6, 1.8], e in
    [3.5, 6.5] -- the box of helpers_eos_function.admissible_points --, velocities of 0.3"""
    x = np.asarray(positions, dtype=np.float64)
    dim = x.shape[1]
    phase = sum((d + 1.0) * x[:, d] for d in range(dim))
    rho = 1.2 + 0.6 * np.sin(2.0 * np.pi * phase)
    e = 5.0 + 1.5 * np.cos(3.0 * phase + 0.3)
    vel = np.stack([0.3 * np.sin(2.0 * phase + d) for d in range(dim)], axis=1)
    return aeos_from_primitive_state(rho, vel, e)


def member(dim, name, **edits):
    return he.member_params(hiv.make_params(capi.EQ_EULER_AEOS, dim, **edits), name)


def function_module(off, p_closed, **kw):
    """a device module created with the closed-form member of `p_closed`, then switched to the same member written as
    expressions"""
    m = HyperbolicModule(off, p_closed, backend="hip", **kw)
    m.eos_configure_function(**he.member_expressions(p_closed))
    return m


def prepared(m, off, U):
    sv = m.new_state_vector(U)
    dirichlet = U[np.asarray(off.b_i).astype(np.int64)] if off.n_bdry else None
    m.prepare_state_vector(sv, 0.0, dirichlet)
    out = sv.download()[: off.n_owned].copy(), sv.download_precomputed()[: off.n_owned].reshape(off.n_owned, 4).copy()
    sv.free()
    return out


def internal(U):
    """(rho, e) of states [n, k] in the operation order of EulerAeos::internal_energy and precompute_cycle0"""
    rho = U[:, 0]
    m2 = U[:, 1] * U[:, 1]
    for d in range(2, U.shape[1] - 1):
        m2 = m2 + U[:, d] * U[:, d]
    rho_e = U[:, -1] - 0.5 * m2 * (1.0 / rho)
    return rho, rho_e / rho


# --------------------------------------------------------------------------- 1: evaluate_device against the host

def test_evaluate_device_of_arithmetic_programs_bit_for_bit():
    """polytropic, NASG and van der Waals written as expressions (+ - * / sqrt), and the if() equation of state: all
    four programs at 1000 points, 1000 being no multiple of the block"""
    off = hiv.tiny_mesh(1)
    rho, e = he.admissible_points("nasg")
    rho[:3] = 1.0, np.nextafter(1.0, 0.0), np.nextafter(1.0, 2.0)
    for name in ("polytropic", "nasg", "vdw"):
        p = member(1, name)
        m = function_module(off, p)
        expressions = he.member_expressions(p)
        for which in range(4):
            want = capi.eos_function_evaluate(which, he.expression_of(expressions, which), rho, e)
            np.testing.assert_array_equal(m.eos_function_evaluate_device(which, rho, e), want)
        m.close()
    m = HyperbolicModule(off, member(1, "polytropic"), backend="hip")
    m.eos_configure_function(**he.LINEARISED_IF)
    for which, key in ((0, "pressure"), (1, "specific_internal_energy")):
        want = capi.eos_function_evaluate(which, he.LINEARISED_IF[key], rho, e)
        np.testing.assert_array_equal(m.eos_function_evaluate_device(which, rho, e), want)
    # temperature and speed of sound were left at their defaults
    np.testing.assert_array_equal(m.eos_function_evaluate_device(2, rho, e), e / 718.)
    np.testing.assert_array_equal(m.eos_function_evaluate_device(3, rho, e), np.sqrt(1.4 * (1.4 - 1.0) * e))
    assert m.eos_function_evaluate_device(0, [], []).shape == (0,)
    m.close()


@pytest.mark.parametrize("name", ["exp", "sin", "cos", "log", "tanh", "erf"])
def test_evaluate_device_of_library_functions_within_the_function_caps(name):
    """one library function each in all four programs, device interpreter against host interpreter on the same
    operand: the caps of tests/test_gpu_flux_function.py (helpers_expression.FUNCTIONS)"""
    _, _, lower, upper, _, b_f = next(f for f in hx.FUNCTIONS if f[0] == name)
    x = hx.function_points(lower, upper)[:, 0]
    rho = np.random.default_rng(2).uniform(0.5, 2.0, size=x.size)
    off = hiv.tiny_mesh(1)
    m = HyperbolicModule(off, member(1, "polytropic"), backend="hip")
    in_e, in_p = f"{name}(e) + rho", f"{name}(p) + rho"
    m.eos_configure_function(in_e, in_p, in_e, in_e)
    for which in range(4):
        second = "p" if which == 1 else "e"
        want = capi.eos_function_evaluate(which, f"{name}({second}) + rho", rho, x)
        f = capi.eos_function_evaluate(which, f"{name}({second})", rho, x)
        got = m.eos_function_evaluate_device(which, rho, x)
        # the function's cap on f alone, and the one rounding of the sum, which may land on the other neighbour
        bound = hx.function_bound(f, b_f) + EPS * np.abs(want)
        assert (np.abs(got - want) <= bound).all(), (name, which, (np.abs(got - want) / bound).max())
    m.close()


# --------------------------------------------------------------------------- 2: precomputed values, same device

@pytest.mark.parametrize("fold", [True, False], ids=["bc-folded", "bc-launch"])
@pytest.mark.parametrize("dim", [1, 2, 3])
@pytest.mark.parametrize("name", ["polytropic", "nasg", "vdw", "jwl"])
def test_precomputed_values_equal_the_closed_form_member_bit_for_bit(name, dim, fold):
    """all four precomputed values (p, gamma_min, s, eta) after both cycles. Jones-Wilkins-Lee included: both sides
    call the same device exp on the same operand."""
    off = mesh(dim)
    edits = {} if fold else dict(debug_bc_fold_max_slices=-1)
    p = member(dim, name, **edits)
    U = smooth_state(off.positions)
    m_fn, m_closed = function_module(off, p), HyperbolicModule(off, p, backend="hip")
    (U_fn, prec_fn), (U_closed, prec_closed) = prepared(m_fn, off, U), prepared(m_closed, off, U)
    assert np.isfinite(prec_closed).all() and (prec_closed[:, 0] != 0.0).all()
    np.testing.assert_array_equal(U_fn, U_closed)
    np.testing.assert_array_equal(prec_fn, prec_closed)
    info = m_fn.eos_info()
    assert info["kind"] == capi.EOS_FUNCTION and info["precompute_interpreted"] == 1
    assert all(n > 0 for n in info["n_instructions"])
    assert m_closed.eos_info() == dict(kind=p.eos, n_instructions=(0, 0, 0, 0), precompute_interpreted=0)
    m_fn.close()
    m_closed.close()


# --------------------------------------------------------------------------- 3: one update against the oracle

@pytest.mark.parametrize("eos_name", ["nasg", "vdw", "jwl"])
def test_one_update_against_the_oracle(oracle, eos_name):
    """helpers_parity.compare_step unchanged, on the mesh, the data and the parameters of
    tests/test_gpu_parity.py::test_aeos_step_parity_equations_of_state: the oracle runs the closed-form member, the
    device the same member as expressions with the matching interpolation parameters"""
    from helpers_parity import compare_step
    from ryujin_amd.initial_states import aeos_from_primitive
    from test_gpu_parity import _perturbed
    off = offline.SyntheticOffline(offline.rectangle_2d(48, (-1.0, -1.0), (1.0, 1.0)))
    p = he.member_params(oracle.default_params(capi.EQ_EULER_AEOS, 2), eos_name)
    p.cfl = 0.9
    r = np.linalg.norm(off.positions, axis=1)
    U0 = _perturbed(aeos_from_primitive(p, np.where(r < 0.4, 2.0, 1.0), np.zeros((off.n_relevant, 2)),
                                        np.where(r < 0.4, 10.0, 1.0)))
    mg = function_module(off, p)
    old, new = mg.new_state_vector(U0), mg.new_state_vector()
    for _ in range(15):
        mg.prepare_state_vector(old, 0.0, None)
        mg.step(old, [], [], new)
        old, new = new, old
    U = old.download()
    mc = HyperbolicModule(off, p, backend=oracle.backend())
    mods = [(mg, old, new), (mc, mc.new_state_vector(U), mc.new_state_vector())]
    g, c = compare_step(off, mods, None, 0.0, oracle=oracle, params=p, label=f"eos function {eos_name}")
    print(f"eos function {eos_name}: " + " ".join(f"{k}={v:.2e}" for k, v in g["measured"].items()))
    n = off.n_owned
    assert np.ptp(g["prec"][:n, 1]) > 1e-3 or eos_name == "nasg"   # the surrogate gamma varies
    assert (g["U"][:n, 0] > 0).all()
    assert mg.eos_info()["precompute_interpreted"] == 1
    for m in (mg, mc):
        m.close()


# --------------------------------------------------------------------------- 4: twenty Runge-Kutta steps

def twenty_steps(m, part, scheme):
    U0 = smooth_state(part.positions)
    dirichlet = U0[np.asarray(part.b_i).astype(np.int64)] if part.n_bdry else None
    state = m.new_state_vector(U0)
    temps = [m.new_state_vector() for _ in range(3)]
    states, taus = [], []
    for _ in range(20):
        taus.append(m.time_step(scheme, state, temps, dirichlet, cfl_min=0.3, cfl_max=0.3))
        states.append(state.download()[: part.n_owned])
    return states, taus


@pytest.mark.parametrize("scheme, fold", [("ssprk 33", True), ("erk 33", True), ("erk 33", False)])
def test_twenty_steps_equal_the_closed_form_member_bit_for_bit(scheme, fold):
    """the device-resident driver (a pending pre-pass between the stages), stage vectors through the function pre-pass
    (ERK33), NASG: every state and every tau identical"""
    off = mesh(2)
    p = member(2, "nasg", **({} if fold else dict(debug_bc_fold_max_slices=-1)))
    m_fn, m_closed = function_module(off, p), HyperbolicModule(off, p, backend="hip")
    (s_fn, t_fn), (s_closed, t_closed) = twenty_steps(m_fn, off, scheme), twenty_steps(m_closed, off, scheme)
    assert t_fn == t_closed and all(t > 0.0 for t in t_fn)
    for step, (a, b) in enumerate(zip(s_fn, s_closed)):
        assert np.isfinite(a).all()
        np.testing.assert_array_equal(a, b, err_msg=f"after step {step}")
    assert not np.array_equal(s_fn[0], s_fn[-1])
    assert m_fn.eos_info()["precompute_interpreted"] == 1 and m_closed.eos_info()["precompute_interpreted"] == 0
    m_fn.close()
    m_closed.close()


def partition(dim, rank):
    if dim == 1:
        spec = offline.MeshSpec(1, (199,), (0.0,), (1.0,), (capi.BC_DIRICHLET, capi.BC_DIRICHLET), n_ranks=3, rank=rank)
    else:
        spec = offline.rectangle_2d(39, (-1.0, -1.0), (1.0, 1.0), ny=47, bc=capi.BC_DIRICHLET, n_ranks=3, rank=rank)
    return offline.SyntheticOffline(spec)


@pytest.mark.parametrize("scheme, dim", [("ssprk 33", 2), ("erk 33", 2), ("erk 33", 1)])
def test_three_ranks_equal_the_closed_form_member_bit_for_bit(scheme, dim):
    """three ranks of the in-process transport (export and interior launches with slice_begin != 0), every rank's
    context configured by its own call: U and tau identical to the closed-form run on the same partition. In 1-D the
    middle rank owns no boundary."""
    from helpers_partitioned import run_hip_ranks
    parts = [partition(dim, r) for r in range(3)]
    assert all(part.n_owned % 64 for part in parts)
    if dim == 1:
        assert [part.n_bdry for part in parts] == [1, 0, 1]
    expressions = he.member_expressions(member(dim, "vdw"))

    def body(function):
        def run(m, part, rank):
            if function:
                m.eos_configure_function(**expressions)
            out = twenty_steps(m, part, scheme)
            assert m.eos_info()["precompute_interpreted"] == (1 if function else 0)
            return out
        return run
    out_fn = run_hip_ranks(parts, lambda: member(dim, "vdw"), body(True))
    out_closed = run_hip_ranks(parts, lambda: member(dim, "vdw"), body(False))
    for rank in range(3):
        assert out_fn[rank][1] == out_closed[rank][1] == out_fn[0][1]
        for step in range(20):
            np.testing.assert_array_equal(out_fn[rank][0][step], out_closed[rank][0][step],
                                          err_msg=f"rank {rank} after step {step}")


# --------------------------------------------------------------------------- 5: analytic states

IV_CASES = [
    hiv.Case("uniform 1d", capi.EQ_EULER_AEOS, 1, "uniform", {"primitive state": (1.4, 3.0, 1.0)}, edits=hiv.NASG),
    hiv.Case("radial contrast 2d", capi.EQ_EULER_AEOS, 2, "radial contrast",
             {"primitive state inner": (1.0, 0.0, 100.0), "primitive state outer": (0.125, 0.0, 0.1), "radius": 0.5},
             position=(0.1, -0.05), edits=hiv.NASG),
    hiv.Case("isentropic vortex", capi.EQ_EULER_AEOS, 2, "isentropic vortex", {"mach number": 1.0, "beta": 5.0},
             (1.0, 1.0), (-1.0, -1.0), edits=hiv.NASG, box=(-5.0, 5.0), times=(0.0, 0.5, 2.0)),
    hiv.Case("leblanc 3d (1,1,1)", capi.EQ_EULER_AEOS, 3, "leblanc", {}, (1.0, 1.0, 1.0), (0.25, -0.125, 0.0625),
             edits=dict(hiv.NASG, gamma=5.0 / 3.0), times=(0.0, 0.2, 2.0 / 3.0)),
    hiv.Case("rarefaction 1d", capi.EQ_EULER_AEOS, 1, "rarefaction", position=(0.2,), edits=hiv.NASG, box=(0.0, 1.0),
             times=(0.0, 0.1, 0.30558)),
]


@pytest.mark.parametrize("order", ["eos-first", "state-first"])
@pytest.mark.parametrize("case", IV_CASES, ids=[c.label for c in IV_CASES])
def test_analytic_states_equal_the_closed_form_kernels_bit_for_bit(case, order):
    """NASG as expressions against the closed-form NASG kernels: evaluate at 1000 points (no multiple of the block),
    interpolate and the Dirichlet kernel give the same bits, in both orders of initial_values_configure and
    eos_configure_function"""
    off = mesh(case.dim)
    p = hiv.make_params(case.equation, case.dim, **case.edits)
    m_closed = HyperbolicModule(off, p, backend="hip")
    hiv.configure(m_closed, case)
    m_fn = HyperbolicModule(off, p, backend="hip")
    if order == "eos-first":
        m_fn.eos_configure_function(**he.member_expressions(p))
        hiv.configure(m_fn, case)
    else:
        hiv.configure(m_fn, case)
        m_fn.eos_configure_function(**he.member_expressions(p))
    X = hiv.points_for(case)
    for t in case.times:
        want = m_closed.initial_values_evaluate(X, t)
        assert np.isfinite(want).all()
        np.testing.assert_array_equal(m_fn.initial_values_evaluate(X, t), want)
        a, b = m_fn.new_state_vector(), m_closed.new_state_vector()
        m_fn.initial_values_interpolate(a, t)
        m_closed.initial_values_interpolate(b, t)
        nodes = a.download()
        np.testing.assert_array_equal(nodes, b.download())
        np.testing.assert_array_equal(nodes, m_fn.initial_values_evaluate(off.positions, t))
        # the Dirichlet kernel: the boundary rows after prepare_state_vector_iv hold the state at their positions
        m_fn.prepare_state_vector(a, t, "device")
        m_closed.prepare_state_vector(b, t, "device")
        np.testing.assert_array_equal(a.download(), b.download())
        np.testing.assert_array_equal(a.download_precomputed(), b.download_precomputed())
        a.free()
        b.free()
    m_fn.close()
    m_closed.close()


def test_time_step_iv_equals_the_callback_path_bit_for_bit():
    """20 ERK33 steps of the isentropic vortex on a function-EOS context: Dirichlet data at the stage times from the
    device kernel (time_step_iv) and from a callback that returns initial_values_evaluate"""
    case = hiv.Case("vortex", capi.EQ_EULER_AEOS, 2, "isentropic vortex", {"mach number": 1.0, "beta": 5.0},
                    (1.0, 1.0), (-1.0, -1.0), edits=dict(hiv.NASG, cfl=0.3))
    off = hiv.vortex_mesh(23, ny=24)
    p = hiv.make_params(case.equation, 2, **case.edits)
    runs = []
    for device in (True, False):
        m = function_module(off, p)
        hiv.configure(m, case)
        sv = m.new_state_vector()
        m.initial_values_interpolate(sv, 0.0)
        runs.append(hiv.run_driver(m, case, sv.download(), "erk 33", 20, device))
        m.close()
    (s_dev, t_dev, _), (s_fn, t_fn, _) = runs
    assert t_dev == t_fn and all(t > 0.0 for t in t_dev)
    for step, (a, b) in enumerate(zip(s_dev, s_fn)):
        np.testing.assert_array_equal(a, b, err_msg=f"after step {step}")
    assert not np.array_equal(s_dev[0], s_dev[-1])


@pytest.mark.parametrize("scheme", ["ssprk 33", "erk 33"])
def test_isentropic_vortex_l5_baseline_with_the_default_expressions(golden_dir, scheme):
    """tests/euler_aeos/verification-isentropic_vortex-pge-2d-*-l5 on a context created with RYUJIN_EOS_FUNCTION (the
    reference's defaults: the polytropic gas with 1.4), device resident from initial_values_interpolate on, with the
    tolerance of tests/test_gpu_parity.py::test_aeos_isentropic_vortex_golden_on_gpu"""
    from ryujin_amd.initial_states import euler_isentropic_vortex
    from ryujin_amd.module import DeviceResidentTimeIntegrator
    from test_oracle_golden_integration import _cell_norms, _golden_vortex
    dofs, t_ref, linf_ref, l1_ref, l2_ref = _golden_vortex(golden_dir, scheme, 5,
                                                          "euler_aeos_verification-isentropic_vortex-pge-2d")
    n = 32
    off = offline.SyntheticOffline(offline.rectangle_2d(n, (-5.0, -5.0), (5.0, 5.0), bc=capi.BC_DIRICHLET))
    m = HyperbolicModule(off, hiv.make_params(capi.EQ_EULER_AEOS, 2, eos=capi.EOS_FUNCTION), backend="hip")
    m.initial_values_configure("isentropic vortex", mach_number=1.0, beta=5.0, direction=(1.0, 1.0),
                               position=(-1.0, -1.0))
    sv = m.new_state_vector()
    m.initial_values_interpolate(sv, 0.0)
    ti = DeviceResidentTimeIntegrator(m, scheme, cfl_min=0.2, cfl_max=0.2, cfl_recovery_strategy="none",
                                      dirichlet="device")
    t = 0.0
    while t < 2.0:
        sv, tau = ti.step(sv, t)
        t += tau
    m.prepare_state_vector(sv, t, "device")
    assert m.eos_info() == dict(kind=capi.EOS_FUNCTION, n_instructions=(7, 7, 3, 8), precompute_interpreted=1)
    U, A = sv.download(), euler_isentropic_vortex(off.positions, t, mach=1.0, beta=5.0)
    h = 10.0 / n
    order = np.lexsort((off.positions[:, 0], off.positions[:, 1]))
    linf = l1 = l2 = 0.0
    for c in range(4):
        a = A[order, c].reshape(n + 1, n + 1).T
        e = (U[order, c] - A[order, c]).reshape(n + 1, n + 1).T
        (l1a, l2a), (l1e, l2e) = _cell_norms(a, h), _cell_norms(e, h)
        linf += np.abs(e).max() / np.abs(a).max()
        l1 += l1e / l1a
        l2 += l2e / l2a
    print(f"{scheme}: t {t!r} ({t_ref!r}), Linf {linf!r} ({linf_ref!r}), L1 {l1!r} ({l1_ref!r}), L2 {l2!r} ({l2_ref!r})")
    assert off.n_owned == dofs
    assert abs(t - t_ref) < 1e-10
    assert abs(linf - linf_ref) < 1e-8 * linf_ref
    assert abs(l1 - l1_ref) < 1e-8 * l1_ref
    assert abs(l2 - l2_ref) < 1e-8 * l2_ref
    m.close()


# --------------------------------------------------------------------------- 6: an equation of state the library lacks

@pytest.mark.parametrize("with_if", [False, True], ids=["linearised", "linearised-if"])
@pytest.mark.parametrize("dim", [1, 2, 3])
def test_precomputed_pressure_of_an_unknown_equation_of_state(dim, with_if):
    """p = (1.4 - 1) rho e + c^2 (rho - 1) with p_infty = c^2, and its if() variant: the precomputed p equals the host
    interpreter at the device's own U, bit for bit"""
    off = mesh(dim)
    expressions = he.LINEARISED_IF if with_if else he.LINEARISED
    m = HyperbolicModule(off, member(dim, "polytropic"), backend="hip")
    m.eos_configure_function(**expressions)
    U = smooth_state(off.positions)
    U_dev, prec = prepared(m, off, U)
    rho, e = internal(U_dev)
    assert (rho < 1.0).any() and (rho > 1.0).any()
    want = capi.eos_function_evaluate(0, expressions["pressure"], rho, e)
    np.testing.assert_array_equal(prec[:, 0], want)
    np.testing.assert_array_equal(want, he.linearised_pressure(rho, e, with_if))
    m.close()


@pytest.mark.parametrize("with_if", [False, True], ids=["linearised", "linearised-if"])
def test_riemann_problem_with_an_unknown_equation_of_state(with_if):
    """200 nodes, (rho, v, p) = (1.5, 0, 2) | (0.8, 0, 0.5) with the jump in the middle, 50 forward Euler updates with
    Dirichlet ends: status 0, rho > 0, and the mass balance. No wave reaches an end (asserted), and the ends are at
    rest, so the boundary flux of mass is m = 0 at both: sum m_i rho_i stays what it was, within the forward bound
    of the updates' own roundings, 8 eps steps sum m_i |rho_i| (the sums are formed exactly, math.fsum) -- the bound
    of the Buckley-Leverett test of tests/test_gpu_flux_function.py."""
    off = mesh(1)
    expressions = he.LINEARISED_IF if with_if else he.LINEARISED
    m = HyperbolicModule(off, member(1, "polytropic", cfl=0.5), backend="hip")
    m.eos_configure_function(**expressions)
    x = np.asarray(off.positions).reshape(-1)[: off.n_owned]
    left = x < 0.5
    rho, pressure = np.where(left, 1.5, 0.8), np.where(left, 2.0, 0.5)
    e = capi.eos_function_evaluate(1, expressions["specific_internal_energy"], rho, pressure)
    U0 = aeos_from_primitive_state(rho, np.zeros((off.n_owned, 1)), e)
    dirichlet = U0[np.asarray(off.b_i).astype(np.int64)]
    a, b = m.new_state_vector(U0), m.new_state_vector()
    t, steps = 0.0, 50
    for _ in range(steps):
        m.prepare_state_vector(a, 0.0, dirichlet)
        t += m.step(a, [], [], b)
        assert m.last_status == 0
        a, b = b, a
    U = a.download()[: off.n_owned]
    order = np.argsort(x)
    assert np.isfinite(U).all() and (U[:, 0] > 0.0).all()
    untouched = 8.0 * EPS * steps
    assert (np.abs(U[order[:10]] - U0[order[:10]]) <= untouched * np.abs(U0[order[:10]]).max()).all()
    assert (np.abs(U[order[-10:]] - U0[order[-10:]]) <= untouched * np.abs(U0[order[-10:]]).max()).all()
    assert np.abs(U[:, 1]).max() > 0.1 and t > 0.01   # the waves developed
    mi = np.asarray(off.mi)[: off.n_owned]
    mass = math.fsum(mi * U[:, 0]) - math.fsum(mi * U0[:, 0])
    bound = 8.0 * EPS * steps * math.fsum(mi * np.abs(U[:, 0]))
    print(f"\nRiemann problem, if={with_if}: t = {t!r}, min rho = {U[:, 0].min()!r}, mass balance {mass!r}, bound {bound!r}")
    assert abs(mass) <= bound
    assert m.eos_info()["precompute_interpreted"] == 1
    m.close()


# --------------------------------------------------------------------------- 7: refusals

def one_update(m, off, U):
    old, new = m.new_state_vector(U), m.new_state_vector()
    m.prepare_state_vector(old, 0.0, U[np.asarray(off.b_i).astype(np.int64)])
    m.step(old, [], [], new)
    out = new.download()[: off.n_owned].copy(), old.download_precomputed()[: off.n_owned].copy()
    old.free()
    new.free()
    return out


def test_refused_configure_leaves_the_equation_of_state_and_configure_replaces_it():
    lib = capi.load_hip()
    off = mesh(2)
    p = member(2, "nasg")
    m = HyperbolicModule(off, p, backend="hip")
    U = smooth_state(off.positions)
    before = one_update(m, off, U)
    assert m.eos_info() == dict(kind=capi.EOS_NOBLE_ABEL_STIFFENED_GAS, n_instructions=(0, 0, 0, 0),
                                precompute_interpreted=0)
    nan, inf = float("nan"), float("inf")
    for args, status, needle in (
            ((b"rho*p", None, None, None, 0.0, 0.0, 0.0), capi.RYUJIN_ERR_ARG, b"eos: pressure: "),
            ((None, b"rho*e", None, None, 0.0, 0.0, 0.0), capi.RYUJIN_ERR_ARG, b"eos: specific internal energy: "),
            ((None, None, b"rho + x", None, 0.0, 0.0, 0.0), capi.RYUJIN_ERR_ARG, b"eos: temperature: "),
            ((None, None, None, b"rho*rand()", 0.0, 0.0, 0.0), capi.RYUJIN_ERR_UNSUPPORTED, b"eos: speed of sound: "),
            ((None, None, None, b"rho*rand()", 0.0, 0.0, 0.0), capi.RYUJIN_ERR_UNSUPPORTED, b"at character 4 "),
            ((None, None, None, None, nan, 0.0, 0.0), capi.RYUJIN_ERR_ARG, b"covolume"),
            ((None, None, None, None, 0.0, inf, 0.0), capi.RYUJIN_ERR_ARG, b"reference pressure"),
            ((None, None, None, None, 0.0, 0.0, -inf), capi.RYUJIN_ERR_ARG, b"specific internal energy")):
        assert lib.ryujin_hip_eos_configure_function(m._ctx, *args) == status
        assert needle in lib.ryujin_hip_last_error(), lib.ryujin_hip_last_error()
    after = one_update(m, off, U)
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)
    assert m.eos_info()["kind"] == capi.EOS_NOBLE_ABEL_STIFFENED_GAS
    # evaluate_device needs the function equation of state
    one = np.ones(1)
    ptr = capi.as_ptr(one, capi.c_double_p)
    assert lib.ryujin_hip_eos_function_evaluate_device(m._ctx, 0, ptr, ptr, 1, ptr) == capi.RYUJIN_ERR_ARG
    # an accepted call replaces it: other bits, and the same bits as the closed-form member once it is NASG again
    m.eos_configure_function(**he.LINEARISED)
    other = one_update(m, off, U)
    assert not np.array_equal(other[1], before[1])
    assert lib.ryujin_hip_eos_function_evaluate_device(m._ctx, 4, ptr, ptr, 1, ptr) == capi.RYUJIN_ERR_ARG
    # a refused call on the function equation of state leaves that one running
    assert lib.ryujin_hip_eos_configure_function(m._ctx, b"rho*", None, None, None, 0.0, 0.0, 0.0) \
        == capi.RYUJIN_ERR_ARG
    for a, b in zip(other, one_update(m, off, U)):
        np.testing.assert_array_equal(a, b)
    m.eos_configure_function(**he.member_expressions(p))
    for a, b in zip(before, one_update(m, off, U)):
        np.testing.assert_array_equal(a, b)
    assert m.eos_info()["kind"] == capi.EOS_FUNCTION
    m.close()


def test_created_with_the_function_equation_of_state_equals_the_polytropic_gas():
    off = mesh(2)
    U = smooth_state(off.positions)
    m_fn = HyperbolicModule(off, hiv.make_params(capi.EQ_EULER_AEOS, 2, eos=capi.EOS_FUNCTION), backend="hip")
    assert m_fn.eos_info() == dict(kind=capi.EOS_FUNCTION, n_instructions=(7, 7, 3, 8), precompute_interpreted=0)
    m_pg = HyperbolicModule(off, hiv.make_params(capi.EQ_EULER_AEOS, 2, eos=capi.EOS_POLYTROPIC_GAS, gamma=1.4),
                            backend="hip")
    for a, b in zip(one_update(m_fn, off, U), one_update(m_pg, off, U)):
        np.testing.assert_array_equal(a, b)
    assert m_fn.eos_info()["precompute_interpreted"] == 1
    m_fn.close()
    m_pg.close()
    with pytest.raises(RuntimeError, match="unknown equation of state"):
        HyperbolicModule(off, hiv.make_params(capi.EQ_EULER_AEOS, 2, eos=9), backend="hip")


def test_other_descriptions_debug_entries_and_wide_rows_are_refused(oracle):
    lib = capi.load_hip()
    off = mesh(2)
    for equation in (capi.EQ_EULER, capi.EQ_SHALLOW_WATER, capi.EQ_SCALAR_CONSERVATION):
        m = HyperbolicModule(off, hiv.make_params(equation, 2), backend="hip")
        assert lib.ryujin_hip_eos_configure_function(m._ctx, None, None, None, None, 0.0, 0.0, 0.0) \
            == capi.RYUJIN_ERR_UNSUPPORTED
        kind = C.c_int(-7)
        assert lib.ryujin_hip_eos_info(m._ctx, C.byref(kind), None, None) == capi.RYUJIN_ERR_UNSUPPORTED
        one = np.ones(1)
        ptr = capi.as_ptr(one, capi.c_double_p)
        assert lib.ryujin_hip_eos_function_evaluate_device(m._ctx, 0, ptr, ptr, 1, ptr) == capi.RYUJIN_ERR_UNSUPPORTED
        assert kind.value == -7 and one[0] == 1.0
        m.close()
    # the debug entries that form p from a closed-form member inside their kernel
    p = hiv.make_params(capi.EQ_EULER_AEOS, 2, eos=capi.EOS_FUNCTION)
    data, out = np.ones(10), np.full(1, 7.0)
    for which in (capi.DEBUG_AEOS_DIJ_2D, capi.DEBUG_AEOS_DIJ_RECORDS_2D):
        assert lib.ryujin_hip_debug_function(0, C.byref(p), which, capi.as_ptr(data, capi.c_double_p),
                                             capi.as_ptr(out, capi.c_double_p), 1) == capi.RYUJIN_ERR_UNSUPPORTED
        assert out[0] == 7.0
    # rows wider than 32 entries: EulerAEOS refuses the update before any launch, as with the closed-form members
    # (tests/test_gpu_row_widths.py)
    import helpers_plan_cases as plan_cases
    import helpers_row_width_cases as cases
    refused = cases.AEOS_REFUSED
    case = dict(refused["accepted"], mesh=cases._lattice(refused["shape"], refused["width"]))
    off_wide, U0, dirichlet, _ = plan_cases.build(case)
    assert off_wide.max_row_len == 33
    p = plan_cases.params_of(case, oracle, off_wide.dim)
    p.eos = capi.EOS_FUNCTION
    m = HyperbolicModule(off_wide, p, backend="hip")
    old, new = m.new_state_vector(U0), m.new_state_vector(np.zeros_like(U0))
    m.prepare_state_vector(old, 0.0, dirichlet)
    with pytest.raises(RuntimeError, match=f"status {capi.RYUJIN_ERR_UNSUPPORTED}: {refused['message']}"):
        m.step(old, [], [], new)
    assert np.array_equal(old.download(), U0) and not new.download().any()
    m.close()
