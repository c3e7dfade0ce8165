"""The compact node record of Euler in 1-D and 2-D (ryujin_amd/csrc/euler_device.hpp, kRecordNeedsState): memory holds
(a, pw, a / pw, 1 / p) of a node, 32 bytes, and every kernel that reads a record forms rho, p and v from the node's
state by the expressions node_record() used -- the same operands into the same operations. The default library is
compared with a build that stores the whole 64-byte record (RYUJIN_COMPACT_RECORD=0): after one SSPRK33 step (three
updates) from a developed, non-constant state d_ij (both triangles and the diagonal), alpha, tau, the new U and its
precomputed values are the same bits. The cases reach every kernel that writes or reads a record:

  step_2d                    61 % uniform slices, both loop instances of k_dij_alpha_records in one launch
  step_2d_large_mesh_kernels ... through the kernels of large meshes: a boundary launch of its own behind the step that
                             left the records (k_apply_bc_records), slip and Dirichlet rows, k_dij_boundary
  step_2d_newton             Newton iterations of the Riemann solver on: k_alpha + k_dij_records<E, true>
  below_one_slice            63 rows
  rows_of_length_1           a lattice with rows cut to the diagonal (constrained DoFs)
  line_1d                    Euler<1>
each through the stage-wise driver (k_precompute_records in front of every update) and through the device-resident
Runge-Kutta driver (the last sweep of an update leaves the records: fused_precompute); and on two ranks over the
in-process transport (k_ghost_precompute_records).

The table of |c_ij| and 1 / |c_ij| next to the stencil classes (SellLayout::class_norms) is host arithmetic that must
equal the device's bit for bit: debug_stencil_classes = 0 (classes and norms), 1 (classes without the norms) and -1
(neither) give the same arrays."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from ryujin_amd import HyperbolicModule, TimeIntegrator, _build, capi, offline  # noqa: E402
from ryujin_amd.initial_states import euler_uniform  # noqa: E402

FULL_RECORD_SO = os.path.join(_build.LIBDIR, "libryujin_hip_full_record.so")


def build_full_record_variant():
    """the library that stores the whole node record (travels to the GPU box like the product library)"""
    src = _build._sources(_build.CSRC, (".hpp", ".h", ".hip")) + _build._headers()
    if os.path.exists(FULL_RECORD_SO) and all(os.path.getmtime(s) <= os.path.getmtime(FULL_RECORD_SO) for s in src):
        return FULL_RECORD_SO
    if _build.hipcc_path() is None:
        return FULL_RECORD_SO if os.path.exists(FULL_RECORD_SO) else None
    return _build.build_hip(defines=("RYUJIN_COMPACT_RECORD=0",), out=FULL_RECORD_SO)


_variant_lib = None


def _variant():
    global _variant_lib
    if _variant_lib is None:
        path = build_full_record_variant()
        assert path is not None, "libryujin_hip_full_record.so is built where hipcc is (__graft_entry__.build())"
        lib = C.CDLL(path)
        capi._declare_module_api(lib, "ryujin_hip_")
        vp = C.c_void_p
        lib.ryujin_hip_comm_init_local.argtypes = [C.POINTER(vp), C.c_int, C.c_int]
        lib.ryujin_hip_comm_destroy.argtypes = [vp]
        lib.ryujin_hip_comm_destroy.restype = None
        lib.ryujin_hip_time_step_n.argtypes = [vp, C.c_int, C.c_int, C.c_int, capi.c_int_p, capi.c_double_p, C.c_double,
                                               C.c_int, C.c_double, C.c_double, capi.c_double_p]
        lib.ryujin_hip_debug_plan.argtypes = [vp, capi.c_int_p, C.c_int]
        _variant_lib = lib
    return _variant_lib


LARGE = dict(debug_no_small_mesh_split=1, debug_bc_fold_max_slices=-1)


def _step_2d():
    off = offline.SyntheticOffline(offline.mach3_step_2d(60))
    return off, euler_uniform(off.positions), euler_uniform(off.b_positions)


def _small(name):
    import helpers_small_meshes as sm
    spec = sm.CASES[name]["spec"]
    off = offline.SyntheticOffline(spec)
    dirichlet = sm.state("euler", spec, off.b_positions) if name.startswith("euler_1d") else None
    return off, sm.state("euler", spec, off.positions), dirichlet


def _cut_lattice():
    import helpers_postprocessor_cases as pc
    off = pc.mesh("G_lattice_15x8")
    assert int(np.diff(np.ctypeslib.as_array(off.c.contents.row_starts, shape=(off.n_relevant + 1,))).min()) == 1
    return off, pc.case_state("G_lattice_15x8"), None


# case -> (mesh and data, parameter edits, updates that develop the flow)
CASES = {
    "step_2d": (_step_2d, {}, 40),
    "step_2d_large_mesh_kernels": (_step_2d, LARGE, 40),
    "step_2d_newton": (_step_2d, dict(LARGE, riemann_newton_max_iterations=2), 40),
    "below_one_slice": (lambda: _small("euler_2d_8x6"), {}, 3),
    "rows_of_length_1": (_cut_lattice, {}, 3),
    "line_1d": (lambda: _small("euler_1d_127"), {}, 5),
}

_started = {}


def _developed(case):
    """(offline data, Dirichlet data, the developed state) of a case, on the default library; once per case"""
    if case not in _started:
        make, edits, n_develop = CASES[case]
        off, U0, dirichlet = make()
        m = HyperbolicModule(off, equation=capi.EQ_EULER, backend="hip")
        m.cfl = 0.9
        a, b = m.new_state_vector(U0), m.new_state_vector()
        for _ in range(n_develop):
            m.prepare_state_vector(a, 0.0, dirichlet)
            m.step(a, [], [], b)
            a, b = b, a
        U_start = a.download()
        m.close()
        assert np.isfinite(U_start).all()
        assert float(np.ptp(U_start[: off.n_owned, 0])) > 1e-3, "a constant state would test nothing"
        U_start.setflags(write=False)
        _started[case] = (off, dirichlet, U_start)
    return _started[case]


def _params(lib, dim, edits):
    p = capi.Params()
    lib.ryujin_hip_default_params(C.byref(p), capi.EQ_EULER, dim)
    p.cfl = 0.9
    for key, value in edits.items():
        setattr(p, key, value)
    return p


def _ssprk33(m, off, U_start, dirichlet, driver):
    """one SSPRK33 step; what the module holds afterwards"""
    state = m.new_state_vector(U_start)
    if driver == "device_resident":
        temps = [m.new_state_vector() for _ in range(3)]
        tau = m.time_step("ssprk 33", state, temps, dirichlet)
    else:
        integrator = TimeIntegrator(m, "ssprk 33", cfl_recovery_strategy="none",
                                    dirichlet_fn=(lambda t: dirichlet) if dirichlet is not None else None)
        state, tau = integrator.step(state, 0.0)
    out = dict(tau=np.float64(tau), dij=m.debug_fetch("dij").copy(), alpha=m.alpha().copy(),
               U=state.download()[: off.n_owned].copy())
    # the precomputed values of the new vector: what the last sweep left (and the boundary launch redid), or the pre-pass
    m.prepare_state_vector(state, 0.0, dirichlet)
    out["prec"] = state.download_precomputed()[: off.n_owned].copy()
    return out


def _run(lib, case, driver, more=None):
    off, dirichlet, U_start = _developed(case)
    p = _params(lib, off.dim, dict(CASES[case][1], **(more or {})))
    m = HyperbolicModule(off, p, backend=(lib, "ryujin_hip_"))
    out = _ssprk33(m, off, U_start, dirichlet, driver)
    out["step2"] = m.last_plan()["step2"]
    m.close()
    return out


def _assert_same_bits(x, y, label):
    for name in ("tau", "dij", "alpha", "U", "prec"):
        assert np.array_equal(x[name], y[name]), (label, name)
    assert np.isfinite(x["U"]).all() and np.isfinite(x["dij"]).all() and float(np.abs(x["dij"]).max()) > 0.0, label


@pytest.mark.parametrize("driver", ["stage_wise", "device_resident"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_compact_record_gives_the_bits_of_the_whole_record(case, driver):
    got = _run(capi.load_hip(), case, driver)
    ref = _run(_variant(), case, driver)
    # the Newton case runs the Riemann sweep as a kernel of its own, every other case the fused step 2
    assert got["step2"] == ref["step2"] == ("alpha_then_dij" if case == "step_2d_newton" else "records"), got["step2"]
    _assert_same_bits(got, ref, (case, driver))


def test_stage_wise_and_device_resident_drivers_agree():
    """the records of k_precompute_records and those the last sweep leaves (fused_precompute) are the same records"""
    lib = capi.load_hip()
    _assert_same_bits(_run(lib, "step_2d_large_mesh_kernels", "stage_wise"),
                      _run(lib, "step_2d_large_mesh_kernels", "device_resident"), "drivers")


@pytest.mark.parametrize("case", ["step_2d", "step_2d_large_mesh_kernels"])
def test_norm_table_gives_the_bits_the_kernel_computes(case):
    lib = capi.load_hip()
    off = _developed(case)[0]
    m = HyperbolicModule(off, _params(lib, 2, CASES[case][1]), backend="hip")
    info = m.stencil_class_info()
    m.close()
    assert info["n_uniform_slices"] == 89 and info["n_classes"] == 3, info   # tests/test_gpu_stencil_classes.py
    ref = _run(lib, case, "device_resident", dict(debug_stencil_classes=0))
    for classes in (1, -1):
        _assert_same_bits(ref, _run(lib, case, "device_resident", dict(debug_stencil_classes=classes)), (case, classes))


def test_values_above_one_are_refused():
    off = _developed("below_one_slice")[0]
    with pytest.raises(RuntimeError, match="debug_stencil_classes"):
        HyperbolicModule(off, _params(capi.load_hip(), 2, dict(debug_stencil_classes=2)), backend="hip")


def _two_ranks(lib, parts, U_local):
    """one SSPRK33 step (device-resident driver) on the ranks of `parts`, in-process transport of `lib`"""
    n_ranks = len(parts)
    comms = (C.c_void_p * n_ranks)()
    assert lib.ryujin_hip_comm_init_local(comms, n_ranks, 0) == 0
    out = {}

    def worker(r):
        try:
            m = HyperbolicModule(parts[r], _params(lib, parts[r].dim, {}), backend=(lib, "ryujin_hip_"),
                                 comm=C.c_void_p(comms[r]))
            out[r] = _ssprk33(m, parts[r], U_local[r], None, "device_resident")
            m.close()
        except BaseException as e:  # noqa: BLE001 -- surfaced in the main thread
            out[r] = e

    try:
        threads = [threading.Thread(target=worker, args=(r,)) for r in range(n_ranks)]
        for t in threads:
            t.start()
        for t in threads:
            t.join(timeout=300)
            assert not t.is_alive(), "rank thread hung"
    finally:
        for r in range(n_ranks):
            lib.ryujin_hip_comm_destroy(C.c_void_p(comms[r]))
    for r in range(n_ranks):
        if isinstance(out[r], BaseException):
            raise out[r]
    return [out[r] for r in range(n_ranks)]


def test_two_ranks_ghost_records():
    """a rectangle of 24 x 10 cells between slip walls on two ranks: the records of the ghost rows are made locally
    from the exchanged states (k_ghost_precompute_records)"""
    import helpers_small_meshes as sm
    specs = [sm.rectangle(24, 10, sm.SLIP, 2, r) for r in range(2)]
    parts = [offline.SyntheticOffline(s) for s in specs]
    assert all(p.n_relevant > p.n_owned for p in parts)
    U_local = sm.rank_states("euler", specs, parts)
    got = _two_ranks(capi.load_hip(), parts, U_local)
    ref = _two_ranks(_variant(), parts, U_local)
    for r in range(2):
        _assert_same_bits(got[r], ref[r], ("rank", r))
