"""Host-side mirror of ryujin::HyperbolicModule / ryujin::TimeIntegrator over the C ABI.

Same member names, argument meaning and error behaviour as the reference
(source/hyperbolic_module.h:110-278, source/time_integrator.h:279-302) so that the
parity tests read like the reference's own. The production shim is the C++ header
ryujin_amd/csrc/hyperbolic_module_shim.hpp; this Python twin exists for pytest/bench.py.

The class is backend-agnostic: `backend="hip"` binds libryujin_hip.so (the product);
tests may pass a (lib, prefix) pair for the CPU oracle, which exports the same call
surface. There is NO silent fallback: a missing HIP library raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


class Restart(Exception):
    """Mirror of ryujin::Restart (source/hyperbolic_module.h:49-57)."""


class TauError(RuntimeError):
    """tau_max is NaN/inf/<=0 (AssertThrow at hyperbolic_module.template.h:573-576)."""


class StateVector:
    """Device-resident (U, precomputed) pair behind an integer handle (source/state_vector.h:47-51)."""

    def __init__(self, module: "HyperbolicModule"):
        self.module = module
        h = C.c_int(-1)
        module._check(module._f("state_alloc")(module._ctx, C.byref(h)))
        self.handle = h.value

    def upload(self, U: np.ndarray) -> None:
        U = np.ascontiguousarray(U, dtype=np.float64)
        assert U.size == self.module.n_relevant * self.module.k
        self.module._check(self.module._f("state_upload")(
            self.module._ctx, self.handle, capi.as_ptr(U, capi.c_double_p)))

    def download(self) -> np.ndarray:
        U = np.empty((self.module.n_relevant, self.module.k), dtype=np.float64)
        self.module._check(self.module._f("state_download")(
            self.module._ctx, self.handle, capi.as_ptr(U, capi.c_double_p)))
        return U

    def download_precomputed(self) -> np.ndarray:
        P = np.empty((self.module.n_relevant, self.module.n_prec), dtype=np.float64)
        self.module._check(self.module._f("state_download_precomputed")(
            self.module._ctx, self.handle, capi.as_ptr(P, capi.c_double_p)))
        return P

    def free(self) -> None:
        if self.handle >= 0 and self.module._ctx:
            self.module._f("state_free")(self.module._ctx, self.handle)
        self.handle = -1


class HyperbolicModule:
    # run-time switches of the library (ryujin_hip_params::system_scope_events / debug_*) applied to every module
    # constructed while set: the parity suite re-runs whole test functions through the branches a small mesh does
    # not take by itself (monkeypatch.setattr(HyperbolicModule, "library_switches", {...}))
    library_switches: dict = {}

    def __init__(self, offline, params: capi.Params | None = None, *, equation=capi.EQ_EULER,
                 backend="hip", comm=None, device: int = 0):
        if backend == "hip":
            self._lib, self._prefix = capi.load_hip(), "ryujin_hip_"
        else:
            self._lib, self._prefix = backend  # (ctypes lib, prefix): the test oracle
        self.offline = offline
        self.dim = offline.dim
        if params is None:
            params = self.default_params(equation, self.dim)
        for name, value in type(self).library_switches.items():
            setattr(params, name, value)
        self.params = params
        self.equation = params.equation
        # problem_dimension, n_precomputed_values, Limiter::n_bounds of the Description
        self.k, self.n_prec, self.n_bounds = {
            capi.EQ_EULER: (self.dim + 2, 2, 3),            # source/euler/{hyperbolic_system,limiter}.h
            capi.EQ_SHALLOW_WATER: (self.dim + 1, 2, 5),    # source/shallow_water/...
            capi.EQ_EULER_AEOS: (self.dim + 2, 4, 4),       # source/euler_aeos/...
            capi.EQ_SCALAR_CONSERVATION: (1, 2 * self.dim, 2),  # source/scalar_conservation/...
        }[self.equation]
        self.n_owned, self.n_relevant = offline.n_owned, offline.n_relevant
        self._ctx = C.c_void_p()
        self._comm = comm
        rc = self._f("create")(C.byref(self._ctx), offline.c, C.byref(params),
                               comm if comm is not None else None, device)
        self._check(rc)

    # ------------------------------------------------------------------ plumbing
    def _f(self, name):
        return getattr(self._lib, self._prefix + name)

    def _check(self, rc: int) -> int:
        if rc < 0:
            msg = self._f("last_error")()
            raise RuntimeError(f"{self._prefix}* failed with status {rc}: {msg.decode() if msg else ''}")
        return rc

    def default_params(self, equation, dim) -> capi.Params:
        p = capi.Params()
        self._f("default_params")(C.byref(p), equation, dim)
        return p

    def close(self):
        if getattr(self, "_ctx", None):
            self._f("destroy")(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ reference API
    def new_state_vector(self, U: np.ndarray | None = None) -> StateVector:
        sv = StateVector(self)
        if U is not None:
            sv.upload(U)
        return sv

    def prepare_state_vector(self, state: StateVector, t: float, dirichlet: np.ndarray | str | None = None):
        """dirichlet: [n_bdry, k] values of initial_state(position, t), None, or "device": evaluated by the library
        from the configured analytic state (initial_values_configure; ryujin_hip_prepare_state_vector_iv)."""
        if isinstance(dirichlet, str):
            if dirichlet != "device":
                raise ValueError(f"dirichlet={dirichlet!r}")
            self._check(self._f("prepare_state_vector_iv")(self._ctx, state.handle, float(t)))
            return
        ptr = None
        if dirichlet is not None:
            dirichlet = np.ascontiguousarray(dirichlet, dtype=np.float64)
            assert dirichlet.size == self.offline.n_bdry * self.k
            ptr = capi.as_ptr(dirichlet, capi.c_double_p)
        self._check(self._f("prepare_state_vector")(self._ctx, state.handle, float(t), ptr))

    def step(self, old: StateVector, stage_state_vectors, stage_weights, new: StateVector,
             tau: float = 0.0, tau_max: float = np.finfo(np.float64).max) -> float:
        """step<stages>(): returns the tau used; raises Restart like the reference."""
        stages = len(stage_state_vectors)
        assert stages == len(stage_weights)
        hs = (C.c_int * max(stages, 1))(*[s.handle for s in stage_state_vectors])
        ws = (C.c_double * max(stages, 1))(*[float(w) for w in stage_weights])
        tau_out = C.c_double(0.0)
        rc = self._f("step")(self._ctx, old.handle, stages, hs, ws, new.handle, float(tau),
                             float(tau_max), C.byref(tau_out))
        if rc == capi.RYUJIN_ERR_TAU:
            raise TauError("I'm sorry, Dave. I'm afraid I can't do that. We crashed.")
        self._check(rc)
        self.last_status = rc
        if rc == capi.RYUJIN_RESTART:
            raise Restart()
        return tau_out.value

    def time_step(self, scheme: str, state: StateVector, temps, dirichlet=None, tau_max=None,
                  cfl_recovery="none", cfl_min=0.45, cfl_max=0.90, t=0.0, dirichlet_fn=None) -> float:
        """Device-resident TimeIntegrator::step (ryujin_hip_time_step): one host synchronisation per
        RK step. `state` names the solution before and after the call. dirichlet_fn(time) -> [n_bdry, k]:
        time-dependent Dirichlet data, evaluated by the library at the stage times t + c_s tau
        (ryujin_hip_time_step_fn)."""
        if dirichlet_fn is not None:
            return self._time_step_fn(scheme, state, temps, t, dirichlet_fn, tau_max, cfl_recovery, cfl_min, cfl_max)
        if isinstance(dirichlet, str):
            if dirichlet != "device":
                raise ValueError(f"dirichlet={dirichlet!r}")
            return self._time_step_iv(scheme, state, temps, t, tau_max, cfl_recovery, cfl_min, cfl_max)
        schemes = {"ssprk 22": capi.SCHEME_SSPRK_22, "ssprk 33": capi.SCHEME_SSPRK_33,
                   "erk 11": capi.SCHEME_ERK_11, "erk 22": capi.SCHEME_ERK_22, "erk 33": capi.SCHEME_ERK_33,
                   "erk 43": capi.SCHEME_ERK_43, "erk 54": capi.SCHEME_ERK_54}
        ptr = None
        if dirichlet is not None:
            dirichlet = np.ascontiguousarray(dirichlet, dtype=np.float64)
            ptr = capi.as_ptr(dirichlet, capi.c_double_p)
        hs = (C.c_int * len(temps))(*[t.handle for t in temps])
        tau = C.c_double(0.0)
        rc = self._f("time_step_n")(self._ctx, schemes[scheme], state.handle, len(temps), hs, ptr,
                                  float(np.finfo(np.float64).max if tau_max is None else tau_max),
                                  capi.CFL_RECOVERY_BANG_BANG if cfl_recovery == "bang bang control"
                                  else capi.CFL_RECOVERY_NONE, float(cfl_min), float(cfl_max), C.byref(tau))
        if rc == capi.RYUJIN_ERR_TAU:
            raise TauError("I'm sorry, Dave. I'm afraid I can't do that. We crashed.")
        self._check(rc)
        self.last_status = rc
        if rc == capi.RYUJIN_RESTART:
            raise Restart()
        return tau.value

    SCHEMES = {"ssprk 22": capi.SCHEME_SSPRK_22, "ssprk 33": capi.SCHEME_SSPRK_33, "erk 11": capi.SCHEME_ERK_11,
               "erk 22": capi.SCHEME_ERK_22, "erk 33": capi.SCHEME_ERK_33, "erk 43": capi.SCHEME_ERK_43,
               "erk 54": capi.SCHEME_ERK_54}

    def _time_step_fn(self, scheme, state, temps, t, dirichlet_fn, tau_max, cfl_recovery, cfl_min, cfl_max):
        n = self.offline.n_bdry * self.k

        failure = []

        def callback(user, time, out):
            # ctypes prints and swallows an exception raised inside a callback; the library has zero-filled the
            # stage's Dirichlet data, so the stage would run on -- silently -- with zeros. Keep the exception, poison
            # the values (NaN: the step cannot pass unnoticed) and re-raise once the call has returned.
            try:
                values = np.ascontiguousarray(dirichlet_fn(time), dtype=np.float64).reshape(-1)
                if values.size != n:
                    raise ValueError(f"dirichlet_fn returned {values.size} values, expected {n}")
                C.memmove(out, values.ctypes.data, n * 8)
            except Exception as e:  # noqa: BLE001
                failure.append(e)
                nan = np.full(n, np.nan)
                C.memmove(out, nan.ctypes.data, n * 8)
            except BaseException as e:  # KeyboardInterrupt, SystemExit: poison the data as well, re-raised first
                failure.insert(0, e)
                nan = np.full(n, np.nan)
                C.memmove(out, nan.ctypes.data, n * 8)
        cb = capi.DIRICHLET_FN(callback)
        hs = (C.c_int * len(temps))(*[x.handle for x in temps])
        tau = C.c_double(0.0)
        rc = self._f("time_step_fn")(self._ctx, self.SCHEMES[scheme], state.handle, len(temps), hs, float(t), cb,
                                     None, float(np.finfo(np.float64).max if tau_max is None else tau_max),
                                     capi.CFL_RECOVERY_BANG_BANG if cfl_recovery == "bang bang control"
                                     else capi.CFL_RECOVERY_NONE, float(cfl_min), float(cfl_max), C.byref(tau))
        if failure:
            raise failure[0]
        if rc == capi.RYUJIN_ERR_TAU:
            raise TauError("I'm sorry, Dave. I'm afraid I can't do that. We crashed.")
        self._check(rc)
        self.last_status = rc
        if rc == capi.RYUJIN_RESTART:
            raise Restart()
        return tau.value

    def _time_step_iv(self, scheme, state, temps, t, tau_max, cfl_recovery, cfl_min, cfl_max):
        """ryujin_hip_time_step_iv: the Dirichlet data of every stage evaluated on the device at t + c_s tau"""
        hs = (C.c_int * len(temps))(*[x.handle for x in temps])
        tau = C.c_double(0.0)
        rc = self._f("time_step_iv")(self._ctx, self.SCHEMES[scheme], state.handle, len(temps), hs, float(t),
                                     float(np.finfo(np.float64).max if tau_max is None else tau_max),
                                     capi.CFL_RECOVERY_BANG_BANG if cfl_recovery == "bang bang control"
                                     else capi.CFL_RECOVERY_NONE, float(cfl_min), float(cfl_max), C.byref(tau))
        if rc == capi.RYUJIN_ERR_TAU:
            raise TauError("I'm sorry, Dave. I'm afraid I can't do that. We crashed.")
        self._check(rc)
        self.last_status = rc
        if rc == capi.RYUJIN_RESTART:
            raise Restart()
        return tau.value

    # ------------------------------------------------------------------ InitialValues (device backend only)
    def initial_values_configure(self, name: str, *, direction=None, position=None, perturbation: float = 0.0,
                                 **params) -> None:
        """Select the analytic state of subsection "E - InitialValues" (ryujin_hip_initial_values_configure):
        `name` and the parameter names are the reference's ("isentropic vortex", mach_number=1.0 for "mach number");
        the node and boundary positions come from the offline data. A second call replaces the first."""
        iv = capi.initial_values_struct(name, self.dim, direction, position, perturbation,
                                        equation=self.equation, **params)
        pos = np.ascontiguousarray(self.offline.positions, dtype=np.float64).reshape(-1)
        assert pos.size == self.n_relevant * self.dim
        bpos = np.ascontiguousarray(self.offline.b_positions, dtype=np.float64).reshape(-1) \
            if self.offline.n_bdry else np.zeros(0)
        assert bpos.size == self.offline.n_bdry * self.dim
        self._check(self._f("initial_values_configure")(
            self._ctx, C.byref(iv), capi.as_ptr(pos, capi.c_double_p) if pos.size else None,
            capi.as_ptr(bpos, capi.c_double_p) if bpos.size else None))

    def initial_values_configure_function(self, expressions, *, direction=None, position=None) -> None:
        """Select the expression-defined state "function" (ryujin_hip_initial_values_configure_function): one
        expression in x [y [z]] and t per primitive component -- a sequence in primitive order, or a dict keyed by the
        reference's parameter names ("density expression", "velocity x expression", ..., "pressure expression";
        "water depth expression"; "expression") in which a missing key takes the reference's default. The grammar is
        tabulated in include/ryujin_hip.h. Replaces an earlier initial_values_configure and is replaced by it."""
        texts = capi.function_expressions(self.params.equation, self.dim, expressions)
        d = (1.0,) + (0.0,) * (self.dim - 1) if direction is None else tuple(np.atleast_1d(direction).astype(float))
        x = (0.0,) * self.dim if position is None else tuple(np.atleast_1d(position).astype(float))
        if len(d) != self.dim or len(x) != self.dim:
            raise ValueError(f"direction and position take {self.dim} components")
        d3 = np.array(d + (0.0,) * (3 - self.dim))
        x3 = np.array(x + (0.0,) * (3 - self.dim))
        pos = np.ascontiguousarray(self.offline.positions, dtype=np.float64).reshape(-1)
        assert pos.size == self.n_relevant * self.dim
        bpos = np.ascontiguousarray(self.offline.b_positions, dtype=np.float64).reshape(-1) \
            if self.offline.n_bdry else np.zeros(0)
        assert bpos.size == self.offline.n_bdry * self.dim
        array = (C.c_char_p * len(texts))(*[e.encode() for e in texts])
        self._check(self._f("initial_values_configure_function")(
            self._ctx, len(texts), array, capi.as_ptr(d3, capi.c_double_p), capi.as_ptr(x3, capi.c_double_p),
            capi.as_ptr(pos, capi.c_double_p) if pos.size else None,
            capi.as_ptr(bpos, capi.c_double_p) if bpos.size else None))

    def initial_values_evaluate(self, points, t: float) -> np.ndarray:
        """[n, k]: initial_state(points[n, dim], t) of the configured state, evaluated on the device"""
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self.dim)
        out = np.zeros((points.shape[0], self.k), dtype=np.float64)
        self._check(self._f("initial_values_evaluate")(
            self._ctx, capi.as_ptr(points, capi.c_double_p) if points.size else None, points.shape[0], float(t),
            capi.as_ptr(out, capi.c_double_p) if out.size else None))
        return out

    def initial_values_interpolate(self, state: StateVector, t: float) -> None:
        """InitialValues::interpolate_hyperbolic_vector(t) into `state`, ghost rows included (an enqueue)"""
        self._check(self._f("initial_values_interpolate")(self._ctx, state.handle, float(t)))

    def initial_values_interpolate_initial_precomputed(self) -> None:
        """InitialValues::interpolate_initial_precomputed_vector(): the context's bathymetry := the bed of the
        configured state at every node, ghost rows included (an enqueue); exact zeros for a state without a bed.
        Replaces what the offline data gave as initial_precomputed. Shallow water only."""
        self._check(self._f("initial_values_interpolate_initial_precomputed")(self._ctx))

    def initial_values_evaluate_initial_precomputed(self, points) -> np.ndarray:
        """[n]: initial_precomputations(points[n, dim]) of the configured state, the bed, evaluated on the device"""
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, self.dim)
        out = np.zeros(points.shape[0], dtype=np.float64)
        self._check(self._f("initial_values_evaluate_initial_precomputed")(
            self._ctx, capi.as_ptr(points, capi.c_double_p) if points.size else None, points.shape[0],
            capi.as_ptr(out, capi.c_double_p) if out.size else None))
        return out

    def initial_precomputed(self) -> np.ndarray:
        """[n_relevant]: the bathymetry the context holds now (ryujin_hip_get_initial_precomputed): what the offline
        data gave, or zeros, until initial_values_interpolate_initial_precomputed replaces it. Like the two calls
        above it needs an initial_values_configure or initial_values_configure_function first (include/ryujin_hip.h)."""
        out = np.zeros(self.n_relevant, dtype=np.float64)
        self._check(self._f("get_initial_precomputed")(
            self._ctx, capi.as_ptr(out, capi.c_double_p) if out.size else None))
        return out

    # ------------------------------------------------------------------ FluxLibrary "function" (device backend only)
    def flux_configure_function(self, expression: str, delta: float = 1e-10) -> None:
        """Switch a scalar conservation module to the expression-defined flux "function"
        (ryujin_hip_flux_configure_function): one string in u, a component per space dimension separated by ';'
        ("sin(u); cos(u)"), and the step of the central difference quotient. The grammar is tabulated in
        include/ryujin_hip.h. Takes effect at the next prepare_state_vector; a refused call (RuntimeError) leaves the
        earlier flux in place."""
        self._check(self._f("flux_configure_function")(self._ctx, str(expression).encode(), float(delta)))

    def flux_info(self) -> dict:
        """What the latest update ran (ryujin_hip_flux_info): kind (capi.FLUX_*), n_instructions of the function
        flux, step2_interpreted -- whether step 2 ran the interpreter kernel (function flux with averaged entropy)."""
        kind, n, interpreted = C.c_int(0), C.c_int(0), C.c_int(0)
        self._check(self._f("flux_info")(self._ctx, C.byref(kind), C.byref(n), C.byref(interpreted)))
        return dict(kind=kind.value, n_instructions=n.value, step2_interpreted=interpreted.value)

    # ------------------------------------------------- EquationOfStateLibrary "function" (device backend only)
    def eos_configure_function(self, pressure=None, specific_internal_energy=None, temperature=None,
                               speed_of_sound=None, interpolation_b: float = 0.0, interpolation_pinfty: float = 0.0,
                               interpolation_q: float = 0.0) -> None:
        """Switch an EulerAEOS module to the expression-defined equation of state "function"
        (ryujin_hip_eos_configure_function): pressure(rho, e), specific internal energy(rho, p), temperature(rho, e)
        and speed of sound(rho, e) as strings (None: the reference's default), and the three interpolation parameters
        of the surrogate. The grammar is tabulated in include/ryujin_hip.h. Takes effect at the next
        prepare_state_vector, and for an analytic initial state configured before or after this call; a refused call
        (RuntimeError) leaves the earlier equation of state in place."""
        texts = [None if e is None else str(e).encode()
                 for e in (pressure, specific_internal_energy, temperature, speed_of_sound)]
        self._check(self._f("eos_configure_function")(self._ctx, *texts, float(interpolation_b),
                                                      float(interpolation_pinfty), float(interpolation_q)))

    def eos_function_evaluate_device(self, which: int, rho, second) -> np.ndarray:
        """[n]: program `which` (capi.EOS_PRESSURE, ...) of the configured function equation of state at (rho [n],
        second [n]) through the device interpreter (ryujin_hip_eos_function_evaluate_device)"""
        rho = np.ascontiguousarray(rho, dtype=np.float64).reshape(-1)
        second = np.ascontiguousarray(second, dtype=np.float64).reshape(-1)
        if rho.size != second.size:
            raise ValueError("rho and the second variable take the same number of points")
        out = np.zeros(rho.size, dtype=np.float64)
        self._check(self._f("eos_function_evaluate_device")(
            self._ctx, int(which), capi.as_ptr(rho, capi.c_double_p) if rho.size else None,
            capi.as_ptr(second, capi.c_double_p) if rho.size else None, rho.size,
            capi.as_ptr(out, capi.c_double_p) if rho.size else None))
        return out

    def eos_info(self) -> dict:
        """What the latest prepare_state_vector ran (ryujin_hip_eos_info): kind (capi.EOS_*), n_instructions of the
        four programs of the function equation of state, precompute_interpreted -- whether cycle 0 of the
        precomputation ran the interpreter kernel."""
        kind, interpreted = C.c_int(0), C.c_int(0)
        n = (C.c_int * 4)()
        self._check(self._f("eos_info")(self._ctx, C.byref(kind), n, C.byref(interpreted)))
        return dict(kind=kind.value, n_instructions=tuple(n), precompute_interpreted=interpreted.value)

    def integrals(self, state: StateVector) -> np.ndarray:
        """sum_i m_i U_i over the owned DoFs of all ranks, computed on the device with a fixed
        summation order (ryujin_hip_state_integrals; device backend only)."""
        out = np.zeros(self.k, dtype=np.float64)
        self._check(self._f("state_integrals")(self._ctx, state.handle, capi.as_ptr(out, capi.c_double_p)))
        return out

    # ------------------------------------------------------------------ Postprocessor (device backend only)
    def postprocess_configure(self, schlieren=("rho",), vorticity=(), beta: float = 10.0,
                              recompute_bounds: bool = True) -> list[str]:
        """Select the quantities of postprocess_compute(); returns their names in output order (schlieren first, as
        Postprocessor::prepare()). A name is looked up among the Description's conserved component names first and
        its primitive names second; an unknown one raises ValueError. A call that changes nothing keeps the
        configuration, and with it the bounds that recompute_bounds=False holds on to."""
        entries, names = [], []
        for kind, prefix, wanted in ((capi.PP_SCHLIEREN, "schlieren_", schlieren),
                                     (capi.PP_VORTICITY, "vorticity_", vorticity)):
            for name in wanted:
                is_primitive, index = capi.resolve_component(self.equation, self.dim, name)
                entries.append((kind, is_primitive, index))
                names.append(prefix + name)
        config = (tuple(entries), float(beta), bool(recompute_bounds))
        if getattr(self, "_pp_config", None) != config:
            q = (capi.PostprocessQuantity * max(1, len(entries)))(*[capi.PostprocessQuantity(*e) for e in entries])
            self._pp_config = None
            self._check(self._f("postprocess_configure")(self._ctx, len(entries), q, float(beta),
                                                         int(bool(recompute_bounds))))
            self._pp_config, self._pp_names = config, names
        return list(names)

    def postprocess_reset_bounds(self) -> None:
        """Postprocessor::reset_bounds(): with recompute_bounds=False the next compute takes its bounds afresh."""
        if getattr(self, "_pp_config", None) is not None:
            entries, beta, recompute_bounds = self._pp_config
            q = (capi.PostprocessQuantity * len(entries))(*[capi.PostprocessQuantity(*e) for e in entries])
            self._check(self._f("postprocess_configure")(self._ctx, len(entries), q, beta, int(recompute_bounds)))

    def postprocess_compute(self, state: StateVector) -> None:
        """Postprocessor::compute() on the device (asynchronous; collective over the ranks)."""
        self._check(self._f("postprocess_compute")(self._ctx, state.handle))

    def postprocess_download(self, raw: bool = False) -> dict:
        out = {}
        for q, name in enumerate(self._pp_names):
            a = np.zeros(self.n_owned, dtype=np.float64)
            self._check(self._f("postprocess_download")(self._ctx, q, capi.as_ptr(a, capi.c_double_p), int(bool(raw))))
            out[name] = a
        return out

    def postprocess_bounds(self) -> dict:
        """name -> (q_max, q_min) of the latest postprocess_compute(), over the owned rows of all ranks."""
        out = {}
        for q, name in enumerate(self._pp_names):
            hi, lo = C.c_double(), C.c_double()
            self._check(self._f("postprocess_bounds")(self._ctx, q, C.byref(hi), C.byref(lo)))
            out[name] = (hi.value, lo.value)
        return out

    def postprocess(self, state: StateVector, schlieren=("rho",), vorticity=(), beta: float = 10.0,
                    recompute_bounds: bool = True, raw: bool = False) -> dict:
        """Schlieren and vorticity fields of a state vector (ryujin_hip_postprocess_*): name -> [n_owned] array,
        keys as the reference names them ("schlieren_rho", "vorticity_v_1"); normalised to (-1, 1) on the
        reference's exponential scale, or the values before the normalisation with raw=True."""
        self.postprocess_configure(schlieren, vorticity, beta, recompute_bounds)
        self.postprocess_compute(state)
        return self.postprocess_download(raw)

    # ------------------------------------------------------------------ error norms (device backend only)
    def _require_device(self, what: str) -> None:
        if self._prefix != "ryujin_hip_":
            raise NotImplementedError(f"{what} is offered by the hip backend only")

    def error_norms_configure(self, cells, shape, jxw, weights=None) -> None:
        """The cells of this rank for compute_error() (ryujin_hip_error_norms_configure): cells [n_cells, dofs_per_cell]
        local indices, shape [n_q, dofs_per_cell] the shape values at the quadrature points, and jxw either
        [n_cells, n_q] (JxW per point) or [n_cells] (the cell measure; needs the weights [n_q] of the reference cell).
        error_norms.q1_tables / q1_jxw give them for Q1 with QGauss(3). A second call replaces the first."""
        self._require_device("error_norms_configure")
        shape = np.ascontiguousarray(shape, dtype=np.float64)
        if shape.ndim != 2:
            raise ValueError("shape is [n_q, dofs_per_cell]")
        n_q, dofs_per_cell = shape.shape
        cells = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, dofs_per_cell)
        jxw = np.ascontiguousarray(jxw, dtype=np.float64)
        per_cell = jxw.ndim == 1
        if jxw.size != len(cells) * (1 if per_cell else n_q):
            raise ValueError("jxw is [n_cells, n_q] or [n_cells]")
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(-1)
            if weights.size != n_q:
                raise ValueError("weights is [n_q]")
        self._check(self._f("error_norms_configure")(
            self._ctx, len(cells), dofs_per_cell, capi.as_ptr(cells, capi.c_u32_p) if cells.size else None, n_q,
            capi.as_ptr(shape, capi.c_double_p), capi.as_ptr(weights, capi.c_double_p) if weights is not None else None,
            capi.as_ptr(jxw, capi.c_double_p) if jxw.size else None, int(per_cell)))

    def error_norms_compute(self, state: StateVector, analytic: StateVector, components=None, normalize: bool = True):
        """ryujin_hip_error_norms_compute: ((Linf, L1, L2) consolidated, detail [n_components, 6]); collective"""
        self._require_device("error_norms_compute")
        names = capi.component_names(self.equation, self.dim)[0]
        if components is None:
            components = names  # all of them (time_loop.template.h:170-173)
        index = []
        for name in components:
            if name not in names:
                raise ValueError(f"Unknown component name »{name}«")
            index.append(names.index(name))
        comp = (C.c_int * max(1, len(index)))(*index)
        out = np.zeros(3, dtype=np.float64)
        detail = np.zeros((max(1, len(index)), 6), dtype=np.float64)
        self._check(self._f("error_norms_compute")(self._ctx, state.handle, analytic.handle, len(index), comp,
                                                   int(bool(normalize)), capi.as_ptr(out, capi.c_double_p),
                                                   capi.as_ptr(detail, capi.c_double_p)))
        return (float(out[0]), float(out[1]), float(out[2])), detail[:len(index)]

    def compute_error(self, state: StateVector, t: float, components=None, normalize: bool = True, analytic=None,
                      dirichlet="device"):
        """TimeLoop::compute_error() (source/time_loop.template.h:692-833) without leaving the device:
        prepare_state_vector at t (dirichlet as in prepare_state_vector; "device": from the configured analytic
        state), the analytic vector at t -- the given StateVector, or initial_values_interpolate into a scratch vector
        the module keeps --, then the norms. Returns ((Linf, L1, L2) consolidated, detail [n_components, 6] =
        (Linf, L1, L2 of U - A; Linf, L1, L2 of A) per component). Components by the names of the conserved state;
        default: all of them."""
        self._require_device("compute_error")
        self.prepare_state_vector(state, t, dirichlet)
        if analytic is None:
            if getattr(self, "_en_analytic", None) is None:
                self._en_analytic = self.new_state_vector()
            analytic = self._en_analytic
            self.initial_values_interpolate(analytic, t)
        return self.error_norms_compute(state, analytic, components, normalize)

    # ------------------------------------------------------------------ VTUOutput (device backend only)
    def output_configure(self, names, cells=None, manifolds=(), positions=None) -> tuple[int, int]:
        """"vtu output quantities" and "manifolds" of VTUOutput (ryujin_hip_output_configure): names of conserved,
        primitive, precomputed and initial-precomputed components, "alpha", and the postprocessed fields configured so
        far; cells [n_cells, 2^dim] local indices of this rank's cells (default: those of the offline data); manifolds
        a sequence of level-set expressions in x [y [z]]. The selection is computed here, once. Returns
        (n_selected_cells, n_selected_nodes). A second call replaces the first."""
        self._require_device("output_configure")
        names = [names] if isinstance(names, str) else list(names)
        manifolds = [manifolds] if isinstance(manifolds, str) else list(manifolds)
        if cells is None:
            cells = self.offline.cells
        dofs_per_cell = 2 ** self.dim
        cells = np.ascontiguousarray(cells, dtype=np.uint32).reshape(-1, dofs_per_cell)
        pos = np.ascontiguousarray(self.offline.positions if positions is None else positions,
                                   dtype=np.float64).reshape(-1)
        assert pos.size == self.n_relevant * self.dim
        c_names = (C.c_char_p * max(1, len(names)))(*[str(n).encode() for n in names])
        c_manifolds = (C.c_char_p * max(1, len(manifolds)))(*[str(m).encode() for m in manifolds])
        self._check(self._f("output_configure")(
            self._ctx, len(names), c_names, capi.as_ptr(pos, capi.c_double_p) if pos.size else None, len(cells),
            dofs_per_cell, capi.as_ptr(cells, capi.c_u32_p) if cells.size else None, len(manifolds), c_manifolds))
        self._out_names, self._out_dofs_per_cell = names, dofs_per_cell
        return self.output_info()

    def output_info(self) -> tuple[int, int]:
        """(n_selected_cells, n_selected_nodes) of the configured level-set selection"""
        n_cells, n_nodes = C.c_uint32(0), C.c_uint32(0)
        self._check(self._f("output_info")(self._ctx, C.byref(n_cells), C.byref(n_nodes)))
        return n_cells.value, n_nodes.value

    def output_selection(self):
        """(cell_ids [n_selected_cells], node_ids [n_selected_nodes], connectivity [n_selected_cells, 2^dim]): the
        selected cells as positions in the configured cell list, their nodes as local indices, both ascending, and the
        cells' vertices as indices into node_ids (ryujin_hip_output_selection)"""
        n_cells, n_nodes = self.output_info()
        cell_ids, node_ids = np.zeros(n_cells, dtype=np.uint32), np.zeros(n_nodes, dtype=np.uint32)
        connectivity = np.zeros((n_cells, self._out_dofs_per_cell), dtype=np.uint32)
        self._check(self._f("output_selection")(
            self._ctx, capi.as_ptr(cell_ids, capi.c_u32_p) if n_cells else None,
            capi.as_ptr(node_ids, capi.c_u32_p) if n_nodes else None,
            capi.as_ptr(connectivity, capi.c_u32_p) if n_cells else None))
        return cell_ids, node_ids, connectivity

    def output_levelset_values(self, manifold: int) -> np.ndarray:
        """[n_relevant]: level set `manifold` at the nodes as the device evaluated it"""
        out = np.zeros(self.n_relevant, dtype=np.float64)
        self._check(self._f("output_levelset_values")(self._ctx, int(manifold),
                                                      capi.as_ptr(out, capi.c_double_p) if out.size else None))
        return out

    def output_extract(self, state: StateVector, levelsets: bool = False, precision: str = "float32") -> np.ndarray:
        """[n_quantities, n_nodes]: the configured quantities at all locally relevant nodes, or with levelsets=True at
        the nodes of output_selection(), as float32 (what the writer stores) or float64 (ryujin_hip_output_extract;
        collective over the ranks)."""
        dtype = {"float32": np.float32, "float64": np.float64}[precision]
        n_nodes = self.output_info()[1] if levelsets else self.n_relevant
        out = np.zeros((len(self._out_names), n_nodes), dtype=dtype)
        self._check(self._f("output_extract")(
            self._ctx, state.handle, int(bool(levelsets)),
            capi.OUT_FLOAT64 if precision == "float64" else capi.OUT_FLOAT32,
            out.ctypes.data_as(C.c_void_p) if out.size else None))
        return out

    # ------------------------------------------------------------------ Quantities (device backend only)
    def quantities_add_manifold(self, index, weight, options: int) -> int:
        """A point map of this rank (ryujin_hip_quantities_add_manifold): owned local indices, a positive weight per
        point (interior mass or boundary mass), options a combination of capi.Q_*; returns the manifold id."""
        index = np.ascontiguousarray(index, dtype=np.uint32).reshape(-1)
        weight = np.ascontiguousarray(weight, dtype=np.float64).reshape(-1)
        assert index.size == weight.size
        out = C.c_int(-1)
        self._check(self._f("quantities_add_manifold")(
            self._ctx, index.size, capi.as_ptr(index, capi.c_u32_p) if index.size else None,
            capi.as_ptr(weight, capi.c_double_p) if index.size else None, int(options), C.byref(out)))
        self._q_points = getattr(self, "_q_points", {})
        self._q_points[out.value] = index.size
        return out.value

    def quantities_reset(self) -> None:
        self._check(self._f("quantities_reset")(self._ctx))
        self._q_points = {}

    def quantities_clear_statistics(self) -> None:
        self._check(self._f("quantities_clear_statistics")(self._ctx))

    def quantities_accumulate(self, state: StateVector, t: float) -> None:
        """Quantities::accumulate() on the device: an enqueue (collective over the ranks)."""
        self._check(self._f("quantities_accumulate")(self._ctx, state.handle, float(t)))

    def quantities_instantaneous(self, manifold: int, state: StateVector, t: float) -> np.ndarray:
        """[n_points, 2k]: (V, V o V) per point, V the primitive state"""
        out = np.zeros((self._q_points[manifold], 2 * self.k), dtype=np.float64)
        self._check(self._f("quantities_instantaneous")(self._ctx, manifold, state.handle, float(t),
                                                        capi.as_ptr(out, capi.c_double_p)))
        return out

    def quantities_time_averaged(self, manifold: int):
        """(values [n_points, 2k], t_begin, t_end), or None while nothing has been accumulated"""
        out = np.zeros((self._q_points[manifold], 2 * self.k), dtype=np.float64)
        t0, t1 = C.c_double(), C.c_double()
        rc = self._check(self._f("quantities_time_averaged")(self._ctx, manifold, capi.as_ptr(out, capi.c_double_p),
                                                             C.byref(t0), C.byref(t1)))
        return None if rc == capi.Q_NONE_YET else (out, t0.value, t1.value)

    def quantities_time_series(self, manifold: int, clear: bool = False) -> np.ndarray:
        """[n_rows, 1 + 2k]: (t, mean V, mean V o V) of every accumulate since the last clear"""
        n = C.c_size_t(0)
        fn = self._f("quantities_time_series")
        self._check(fn(self._ctx, manifold, None, 0, C.byref(n), 0))  # rows = NULL, capacity 0: the number of rows
        rows = np.zeros((n.value, 1 + 2 * self.k), dtype=np.float64)
        self._check(fn(self._ctx, manifold, capi.as_ptr(rows, capi.c_double_p), n.value, C.byref(n), int(bool(clear))))
        return rows

    def sadd(self, dst: StateVector, s: float, b: float, src: StateVector):
        self._check(self._f("sadd")(self._ctx, dst.handle, float(s), float(b), src.handle))

    @property
    def cfl(self) -> float:
        v = C.c_double()
        self._check(self._f("get_cfl")(self._ctx, C.byref(v)))
        return v.value

    @cfl.setter
    def cfl(self, value: float):
        self._check(self._f("set_cfl")(self._ctx, float(value)))

    @property
    def id_violation_strategy(self):
        return self._idv if hasattr(self, "_idv") else self.params.id_violation_strategy

    @id_violation_strategy.setter
    def id_violation_strategy(self, s: int):
        self._idv = s
        self._check(self._f("set_id_violation_strategy")(self._ctx, int(s)))

    def alpha(self) -> np.ndarray:
        a = np.empty(self.n_relevant, dtype=np.float64)
        self._check(self._f("get_alpha")(self._ctx, capi.as_ptr(a, capi.c_double_p)))
        return a

    def _counters(self):
        r, w = C.c_uint(), C.c_uint()
        self._check(self._f("get_counters")(self._ctx, C.byref(r), C.byref(w)))
        return r.value, w.value

    def n_restarts(self) -> int:
        return self._counters()[0]

    def n_warnings(self) -> int:
        return self._counters()[1]

    # ------------------------------------------------------------------ introspection
    def exchange_info(self) -> dict:
        """Neighbour ranks of this context and the number of ghost exchanges / scalar all-reduces it has
        enqueued so far (ryujin_hip_exchange_info; device backend only)."""
        n_nbr, nx, nr = C.c_int(0), C.c_ulonglong(0), C.c_ulonglong(0)
        nbr = (C.c_int * 64)()
        self._check(self._f("exchange_info")(self._ctx, C.byref(n_nbr), nbr, 64, C.byref(nx), C.byref(nr)))
        return dict(neighbours=[nbr[q] for q in range(min(n_nbr.value, 64))], n_exchanges=nx.value,
                    n_allreduces=nr.value)

    def limiter_statistics(self) -> dict:
        """Fraction of the 64-row slices in which the first high-order sweep found a limited pair (between the two
        latest host synchronisations), how the latest step kept P_ij ("everywhere" / "per slice") and the fraction
        of slices it was stored in (ryujin_hip_limiter_statistics; device backend only)."""
        f, stored, fs = C.c_double(1.0), C.c_int(1), C.c_double(1.0)
        fn = self._f("limiter_statistics")
        fn.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_double)]
        self._check(fn(self._ctx, C.byref(f), C.byref(stored), C.byref(fs)))
        out = dict(limited_slice_fraction=f.value,
                   pij_stored={1: "everywhere", 2: "per slice", 3: "per tile"}.get(stored.value),
                   pij_stored_slice_fraction=fs.value)
        if stored.value == 3:
            # of the (slice, column) tiles: stored by step 5, read by step 6, formed by step 6 (ryujin_hip_tile_statistics)
            a, b, c = C.c_double(1.0), C.c_double(1.0), C.c_double(0.0)
            self._check(self._lib.ryujin_hip_tile_statistics(self._ctx, C.byref(a), C.byref(b), C.byref(c)))
            out.update(tiles_stored_fraction=a.value, tiles_read_fraction=b.value, tiles_formed_by_step6_fraction=c.value)
        return out

    def layout_info(self) -> dict:
        """tiles (64-entry columns of the SELL-64 slices) of the owned rows and how many the tile map serves from a
        16-byte descriptor (ryujin_hip_layout_info; device backend only)"""
        n, r = C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._lib.ryujin_hip_layout_info(self._ctx, C.byref(n), C.byref(r)))
        ch, ce = C.c_ulonglong(0), C.c_ulonglong(0)
        if hasattr(self._lib, "ryujin_hip_chain_info"):  # (A/B libraries of earlier trees do not have it)
            self._lib.ryujin_hip_chain_info.argtypes = [C.c_void_p, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
            self._check(self._lib.ryujin_hip_chain_info(self._ctx, C.byref(ch), C.byref(ce)))
        return dict(n_tiles=n.value, n_regular_tiles=r.value,
                    regular_tile_fraction=(r.value / n.value if n.value else 0.0),
                    n_chained_tiles=ch.value, chained_tile_fraction=(ch.value / n.value if n.value else 0.0),
                    chained_entry_fraction=(ce.value / (64.0 * n.value) if n.value else 0.0))

    def stencil_class_info(self) -> dict:
        """uniform slices (64 rows with the same c_ij, m_ij and column offsets, column by column) whose c_ij and
        column indices steps 2 and 4 take from the class table, the classes in it and the fraction of the matrix entries in such slices; all
        0 where there is no table (ryujin_hip_stencil_class_info; device backend only)"""
        n, k, f = C.c_ulonglong(0), C.c_ulonglong(0), C.c_double(0.0)
        self._check(self._lib.ryujin_hip_stencil_class_info(self._ctx, C.byref(n), C.byref(k), C.byref(f)))
        return dict(n_uniform_slices=n.value, n_classes=k.value, uniform_entry_fraction=f.value)

    def next_tile_mask_info(self) -> dict:
        """whether the plan of the latest step() handed the tile mask from step 6 to step 7, the off-diagonal (slice,
        column) tiles of the owned rows and how many of them the mask named (ryujin_hip_next_tile_mask_info; device
        backend only; synchronises)"""
        a, n, k = C.c_int(0), C.c_ulonglong(0), C.c_ulonglong(0)
        self._check(self._lib.ryujin_hip_next_tile_mask_info(self._ctx, C.byref(a), C.byref(n), C.byref(k)))
        return dict(active=bool(a.value), n_tiles=n.value, n_named=k.value)

    PLAN_STEP2 = ("alpha_then_dij", "dij_alpha_sc", "records", "dij_alpha")
    PLAN_STEP5 = ("none", "stage0_per_tile", "stage0_per_slice", "stage0_groups", "recompute", "pij_lij")
    PLAN_STEP6 = ("none", "per_slice", "cached", "high_order")
    PLAN_STEP7 = ("none", "last_cached", "high_order")

    def last_plan(self) -> dict:
        """Which kernels the latest step() ran (the StepPlan of ryujin_amd/csrc/step_plan.hpp, field by field) and,
        under "step5_launches" / "step6_launches", what each launch of those two sweeps was given where it was made:
        the number of slices, gridDim.y and -- step 6 -- whether the four waves of a block shared a slice
        (ryujin_hip_debug_plan; device backend only; host values, no synchronisation)."""
        n = 32
        v = (C.c_int * n)()
        rc = self._lib.ryujin_hip_debug_plan(self._ctx, v, n)
        if rc != n:
            self._check(rc if rc < 0 else capi.RYUJIN_ERR_ARG)
        flags = ("step2_split", "fast_riemann", None, "step4_single_walk", "step4_has_stages", "step4_friction",
                 "step4_stores_p", "dg", None, None, "wide", "has_V", None, "tiles_predicted_from_history", None,
                 "step6_flags", None, "fuse_precompute", "checked")
        out = dict(step2=self.PLAN_STEP2[v[0]], diag_width=v[3], step5=self.PLAN_STEP5[v[9]], step5_groups=v[10],
                   pij_stored=v[13], step6=self.PLAN_STEP6[v[15]], step7=self.PLAN_STEP7[v[17]])
        out.update({name: bool(v[1 + q]) for q, name in enumerate(flags) if name})
        out["step5_launches"] = [dict(n_slices=v[22 + 2 * q], grid_y=v[23 + 2 * q]) for q in range(min(v[20], 2))]
        out["step6_launches"] = [dict(n_slices=v[26 + 3 * q], grid_y=v[27 + 3 * q], shares_slices=bool(v[28 + 3 * q]))
                                 for q in range(min(v[21], 2))]
        return out

    def debug_fill(self, what: str, value: float) -> None:
        """test hook: every off-diagonal slot of the owned rows of a module-owned matrix set to `value`
        (ryujin_hip_debug_fill; device backend only)"""
        self._check(self._lib.ryujin_hip_debug_fill(self._ctx, {"lij_next": 5}[what], float(value)))

    def debug_fetch(self, what: str) -> np.ndarray:
        """`*_all`: over all locally relevant rows, i.e. including the ghost rows / ghost range received from
        the neighbour ranks."""
        codes = {"dij": 0, "lij": 1, "pij": 2, "bounds": 3, "r": 4, "lij_next": 5,
                 "dij_all": 6, "lij_all": 7, "lij_next_all": 8, "r_all": 9}
        rs = self.offline.row_starts
        nnz_owned = int(rs[self.n_owned])
        nnz_all = int(rs[self.n_relevant])
        sizes = {"dij": nnz_owned, "lij": nnz_owned, "pij": nnz_owned * self.k,
                 "bounds": self.n_owned * self.n_bounds, "r": self.n_owned * self.k,
                 "lij_next": nnz_owned, "dij_all": nnz_all, "lij_all": nnz_all, "lij_next_all": nnz_all,
                 "r_all": self.n_relevant * self.k}
        out = np.empty(sizes[what], dtype=np.float64)
        self._check(self._f("debug_fetch")(self._ctx, codes[what], capi.as_ptr(out, capi.c_double_p),
                                           out.size))
        return out


class DeviceResidentTimeIntegrator:
    """TimeIntegrator::step(state_vector, t, t_final) executed inside the library (ryujin_hip_time_step_fn): the
    interface of TimeIntegrator below, one host synchronisation per Runge-Kutta step, Dirichlet data evaluated at
    the stage times by a callback (what contrib/hyperbolic_module_hip.h::time_step does on the ryujin side)."""

    def __init__(self, module: "HyperbolicModule", scheme: str = "erk 33", cfl_min=0.45, cfl_max=0.90,
                 cfl_recovery_strategy: str = "bang bang control", dirichlet_fn=None, dirichlet=None):
        """dirichlet="device": the Dirichlet data of every stage is evaluated on the device from the analytic state
        of module.initial_values_configure (ryujin_hip_time_step_iv) instead of through dirichlet_fn."""
        self.m, self.scheme = module, scheme
        self.cfl_min, self.cfl_max, self.cfl_recovery_strategy = cfl_min, cfl_max, cfl_recovery_strategy
        if dirichlet is not None and (dirichlet != "device" or dirichlet_fn is not None):
            raise ValueError("dirichlet is \"device\" or None, and excludes dirichlet_fn")
        self.dirichlet_fn, self.dirichlet = dirichlet_fn, dirichlet
        self.temp = [module.new_state_vector() for _ in range({"erk 43": 4, "erk 54": 5}.get(scheme, 3))]
        module.cfl = cfl_max

    def step(self, state: StateVector, t: float, t_final: float = np.finfo(np.float64).max):
        tau = self.m.time_step(self.scheme, state, self.temp, tau_max=t_final - t,
                               cfl_recovery=self.cfl_recovery_strategy, cfl_min=self.cfl_min, cfl_max=self.cfl_max,
                               t=t, dirichlet_fn=self.dirichlet_fn, dirichlet=self.dirichlet)
        return state, tau


class TimeIntegrator:
    """Explicit schemes of ryujin::TimeIntegrator that consist solely of
    prepare_state_vector + step<s> + sadd (source/time_integrator.template.h:279-470)."""

    def __init__(self, module: HyperbolicModule, scheme: str = "erk 33", cfl_min=0.45, cfl_max=0.90,
                 cfl_recovery_strategy: str = "bang bang control", dirichlet_fn=None):
        self.m = module
        self.scheme = scheme
        self.cfl_min, self.cfl_max = cfl_min, cfl_max
        self.cfl_recovery_strategy = cfl_recovery_strategy
        self.dirichlet_fn = dirichlet_fn  # t -> [n_bdry, k] array or None
        # temp_ vectors per scheme: TimeIntegrator::prepare() (:163-205)
        n_temp = {"erk 43": 4, "erk 54": 5}.get(scheme, 3)
        self.temp = [module.new_state_vector() for _ in range(n_temp)]
        # TimeIntegrator::prepare(): hyperbolic_module_->cfl(cfl_max_)  (:150)
        module.cfl = cfl_max

    def _prepare(self, sv, t):
        self.m.prepare_state_vector(sv, t, self.dirichlet_fn(t) if self.dirichlet_fn else None)

    def step(self, state: StateVector, t: float, t_final: float = np.finfo(np.float64).max):
        """Returns (new_state, tau). The handles are swapped like state_vector.swap(temp)."""
        tau_max = t_final - t
        single = {"ssprk 22": self._ssprk22, "ssprk 33": self._ssprk33, "erk 11": self._erk11,
                  "erk 22": self._erk22, "erk 33": self._erk33, "erk 43": self._erk43,
                  "erk 54": self._erk54}[self.scheme]
        if self.cfl_recovery_strategy == "bang bang control":
            self.m.id_violation_strategy = capi.IDV_RAISE_EXCEPTION
            self.m.cfl = self.cfl_max
        try:
            return single(state, t, tau_max)
        except Restart:
            if self.cfl_recovery_strategy == "none":
                raise
            self.m.id_violation_strategy = capi.IDV_WARN
            self.m.cfl = self.cfl_min
            return single(state, t, tau_max)

    def _swap(self, state, idx):
        new = self.temp[idx]
        self.temp[idx] = state
        return new

    def _erk11(self, sv, t, tau_max):
        self._prepare(sv, t)
        tau = self.m.step(sv, [], [], self.temp[0], 0.0, tau_max)
        return self._swap(sv, 0), tau

    def _ssprk22(self, sv, t, tau_max):
        T = self.temp
        self._prepare(sv, t)
        tau = self.m.step(sv, [], [], T[0], 0.0, tau_max)
        self._prepare(T[0], t + 1.0 * tau)
        self.m.step(T[0], [], [], T[1], tau)
        self.m.sadd(T[1], 1.0 / 2.0, 1.0 / 2.0, sv)
        return self._swap(sv, 1), tau

    def _ssprk33(self, sv, t, tau_max):
        T = self.temp
        self._prepare(sv, t)
        tau = self.m.step(sv, [], [], T[0], 0.0, tau_max)
        self._prepare(T[0], t + 1.0 * tau)
        self.m.step(T[0], [], [], T[1], tau)
        self.m.sadd(T[1], 1.0 / 4.0, 3.0 / 4.0, sv)
        self._prepare(T[1], t + 0.5 * tau)
        self.m.step(T[1], [], [], T[0], tau)
        self.m.sadd(T[0], 2.0 / 3.0, 1.0 / 3.0, sv)
        return self._swap(sv, 0), tau

    def _erk22(self, sv, t, tau_max):
        T = self.temp
        self._prepare(sv, t)
        tau = self.m.step(sv, [], [], T[0], 0.0, tau_max / 2.0)
        self._prepare(T[0], t + 1.0 * tau)
        self.m.step(T[0], [sv], [-1.0], T[1], tau)
        return self._swap(sv, 1), 2.0 * tau

    def _erk33(self, sv, t, tau_max):
        T = self.temp
        self._prepare(sv, t)
        tau = self.m.step(sv, [], [], T[0], 0.0, tau_max / 3.0)
        self._prepare(T[0], t + 1.0 * tau)
        self.m.step(T[0], [sv], [-1.0], T[1], tau)
        self._prepare(T[1], t + 2.0 * tau)
        self.m.step(T[1], [sv, T[0]], [0.75, -2.0], T[2], tau)
        return self._swap(sv, 2), 3.0 * tau

    def _erk43(self, sv, t, tau_max):
        """step_erk_43 (time_integrator.template.h:405-440)"""
        T = self.temp
        self._prepare(sv, t)
        tau = self.m.step(sv, [], [], T[0], 0.0, tau_max / 4.0)
        self._prepare(T[0], t + 1.0 * tau)
        self.m.step(T[0], [sv], [-1.0], T[1], tau)
        self._prepare(T[1], t + 2.0 * tau)
        self.m.step(T[1], [T[0]], [-1.0], T[2], tau)
        self._prepare(T[2], t + 3.0 * tau)
        self.m.step(T[2], [T[0], T[1]], [5.0 / 3.0, -10.0 / 3.0], T[3], tau)
        return self._swap(sv, 3), 4.0 * tau

    ERK54 = dict(c=0.2, a_21=+0.2, a_31=+0.26075582269554909, a_32=+0.13924417730445096,
                 a_41=-0.25856517872570289, a_42=+0.91136274166280729, a_43=-0.05279756293710430,
                 a_51=+0.21623276431503774, a_52=+0.51534223099602405, a_53=-0.81662794199265554,
                 a_54=+0.88505294668159373, a_61=-0.10511678454691901, a_62=+0.87880047152100838,
                 a_63=-0.58903404061484477, a_64=+0.46213380485434047)

    def _erk54(self, sv, t, tau_max):
        """step_erk_54 (time_integrator.template.h:443-510)"""
        T = self.temp
        a = self.ERK54
        c = a["c"]
        self._prepare(sv, t)
        tau = self.m.step(sv, [], [], T[0], 0.0, tau_max / 5.0)
        self._prepare(T[0], t + 1.0 * tau)
        self.m.step(T[0], [sv], [(a["a_31"] - a["a_21"]) / c], T[1], tau)
        self._prepare(T[1], t + 2.0 * tau)
        self.m.step(T[1], [sv, T[0]], [(a["a_41"] - a["a_31"]) / c, (a["a_42"] - a["a_32"]) / c], T[2], tau)
        self._prepare(T[2], t + 3.0 * tau)
        self.m.step(T[2], [sv, T[0], T[1]],
                    [(a["a_51"] - a["a_41"]) / c, (a["a_52"] - a["a_42"]) / c, (a["a_53"] - a["a_43"]) / c],
                    T[3], tau)
        self._prepare(T[3], t + 4.0 * tau)
        self.m.step(T[3], [sv, T[0], T[1], T[2]],
                    [(a["a_61"] - a["a_51"]) / c, (a["a_62"] - a["a_52"]) / c, (a["a_63"] - a["a_53"]) / c,
                     (a["a_64"] - a["a_54"]) / c], T[4], tau)
        return self._swap(sv, 4), 5.0 * tau


class HostStateVector:
    """A HOST state vector as the reference's caller owns it (source/state_vector.h:47-51): U [n_relevant, k] and
    the precomputed values [n_relevant, n_prec] in numpy arrays. swap() exchanges the storage of two of them, as
    std::tuple::swap / dealii Vector::swap do (time_integrator.template.h:296,325)."""

    def __init__(self, module: "HyperbolicModule", U: np.ndarray | None = None):
        self.U = np.zeros((module.n_relevant, module.k)) if U is None else np.array(U, dtype=np.float64, copy=True)
        self.precomputed = np.zeros((module.n_relevant, module.n_prec))

    def swap(self, other: "HostStateVector"):
        self.U, other.U = other.U, self.U
        self.precomputed, other.precomputed = other.precomputed, self.precomputed


class HostMirroredModule:
    """Python twin of the mirroring of contrib/hyperbolic_module_hip.h: what the adapter does when an UNMODIFIED
    TimeIntegrator (host sadd()/swap(), time_integrator.template.h:18-25,279-510) drives it. Device twins are keyed
    by the storage of U (the data pointer), the host array is the authority at every call, and only what a call can
    have changed is written back (ryujin_hip_state_download_prepared / _owned). Used by the parity tests of those
    entry points and by bench.py's host-mirrored line; device library only."""

    def __init__(self, module: HyperbolicModule, pin: bool = True, mirror_derived: bool = True):
        self.m = module
        self.pin, self.mirror_derived = pin, mirror_derived
        self.twins: dict[int, StateVector] = {}
        self._pinned: list[np.ndarray] = []  # kept alive while registered, unregistered by close()
        self.alpha = np.zeros(module.n_relevant)
        if pin:
            self._register(self.alpha)

    def _register(self, a: np.ndarray):
        self.m._check(self.m._lib.ryujin_hip_host_register(self.m._ctx, a.ctypes.data, a.nbytes))
        self._pinned.append(a)

    def twin_of(self, sv: HostStateVector) -> StateVector:
        key = sv.U.ctypes.data
        if key not in self.twins:
            self.twins[key] = StateVector(self.m)
            if self.pin:
                self._register(sv.U)
                self._register(sv.precomputed)
        return self.twins[key]

    def prepare_state_vector(self, sv: HostStateVector, t: float, dirichlet: np.ndarray | None = None):
        m, twin = self.m, self.twin_of(sv)
        twin.upload(sv.U)
        m.prepare_state_vector(twin, t, dirichlet)
        m._check(m._lib.ryujin_hip_state_download_prepared(m._ctx, twin.handle, capi.as_ptr(sv.U, capi.c_double_p)))
        if self.mirror_derived:
            m._check(m._lib.ryujin_hip_state_download_precomputed(m._ctx, twin.handle,
                                                                  capi.as_ptr(sv.precomputed, capi.c_double_p)))

    def step(self, old: HostStateVector, stage_state_vectors, stage_weights, new: HostStateVector,
             tau: float = 0.0, tau_max: float = np.finfo(np.float64).max) -> float:
        m = self.m
        for sv in [old, *stage_state_vectors]:
            assert sv.U.ctypes.data in self.twins, "old and stage state vectors have to be prepared"
        twin_new = self.twin_of(new)
        try:
            return m.step(self.twins[old.U.ctypes.data], [self.twins[s.U.ctypes.data] for s in stage_state_vectors],
                          stage_weights, twin_new, tau, tau_max)
        finally:
            m._check(m._lib.ryujin_hip_state_download_owned(m._ctx, twin_new.handle, capi.as_ptr(new.U, capi.c_double_p)))
            if self.mirror_derived:
                m._check(m._lib.ryujin_hip_get_alpha(m._ctx, capi.as_ptr(self.alpha, capi.c_double_p)))

    def close(self):
        for twin in self.twins.values():
            twin.free()
        self.twins.clear()
        for a in self._pinned:
            self.m._lib.ryujin_hip_host_unregister(self.m._ctx, a.ctypes.data)
        self._pinned.clear()
