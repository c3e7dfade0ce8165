#!/usr/bin/env python3
"""Device time of ryujin_hip_postprocess_compute (reset of the bounds + sweep + normalisation; one rank, so no
exchange) on the developed states of bench.py's workloads, next to the step-5 time of the update measured IN THE
SAME PROCESS and context (boxes and contexts differ by +-3 - 5 %).

  C2 (step2d)   schlieren of rho (the default), and five quantities in one sweep
  C3 (sedov3d)  schlieren of rho

Each figure: events around `--calls` calls behind `--warmup` calls, three passes, the median pass. "own bytes" per
gridpoint, for a stencil of S entries, dim d, padded state width KP, n quantities:
    sweep:      S * 8 d  (c_ij)  +  4 S (column indices, where the sweep does not use the tile map: 3-D)
                + 8 (m_i) + 8 KP (U_j, every node once) + 8 n (raw values stored)
    normalise:  16 n (raw values read, normalised values written)
Usage: postprocessor_timing.py [--calls 40] [--warmup 10] [--updates N] [--skip-3d]   (prints a markdown table)"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ryujin_amd import HyperbolicModule, capi  # noqa: E402
from ryujin_amd import offline  # noqa: E402
from ryujin_amd.workloads import Ssprk33Stages, benchmark_workload, developed_state  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=40)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--updates", type=int, default=0, help="updates on the benchmark mesh (0: the workload's own)")
ap.add_argument("--skip-3d", action="store_true")
args = ap.parse_args()
lib = capi.load_hip()


def timed(ctx, fn, calls):
    passes = []
    for _ in range(3):
        lib.ryujin_hip_synchronize(ctx)
        lib.ryujin_hip_event_record(ctx, 0)
        for _ in range(calls):
            fn()
        lib.ryujin_hip_event_record(ctx, 1)
        e = C.c_double()
        assert lib.ryujin_hip_event_elapsed_ms(ctx, C.byref(e)) == 0
        passes.append(e.value / calls)
    return float(np.median(passes)), min(passes), max(passes)


def own_bytes(dim, kp, stencil, n, tile_map):
    sweep = stencil * 8 * dim + (0 if tile_map else 4 * stencil) + 8 + 8 * kp + 8 * n
    return sweep, 16 * n


print("| case | gridpoints | quantities | own bytes / gridpoint (sweep + normalise) | compute [ms] (min - max) | "
      "TB/s | step 5 [ms] | compute / step 5 |")
print("|---|---|---|---|---|---|---|---|")
for key, label in (("step2d", "C2"), ("sedov3d", "C3")):
    if key == "sedov3d" and args.skip_3d:
        continue
    wl = benchmark_workload(key)
    off = offline.SyntheticOffline(wl.make_spec(wl.resolution, 1, 0))
    U0, _, _ = developed_state(wl, off)
    m = HyperbolicModule(off, equation=wl.equation, backend="hip")
    m.cfl = 0.9
    ctx = m._ctx
    dirichlet = wl.dirichlet_fn(off.b_positions) if (wl.dirichlet_fn is not None and off.n_bdry) else None
    drv = Ssprk33Stages(m, U0, dirichlet)
    n_updates = args.updates or wl.develop_updates
    for _ in range((n_updates + 2) // 3):
        drv.rk_step()
    # step 5 of the update, from the library's own event pairs: 30 updates behind the developed state
    lib.ryujin_hip_set_timers(ctx, 1)
    tmp, n_upd = (C.c_double * 8)(), C.c_uint()
    for _ in range(6):
        drv.update()
    lib.ryujin_hip_get_timers_accum(ctx, tmp, C.byref(n_upd), 1)
    for _ in range(30):
        drv.update()
    lib.ryujin_hip_get_timers_accum(ctx, tmp, C.byref(n_upd), 0)
    step5 = tmp[5] / n_upd.value
    update_ms = sum(tmp[2:8]) / n_upd.value
    lib.ryujin_hip_set_timers(ctx, 0)
    while drv.stage != 0:
        drv.update()

    dim, kp = off.dim, (m.k + 1) // 2 * 2
    stencil = off.nnz / off.n_relevant
    cases = [(("rho",), ())]
    if key == "step2d":
        cases.append((("rho", "p", "E"), ("m_1", "v_1")))
    for schlieren, vorticity in cases:
        names = m.postprocess_configure(schlieren, vorticity)
        fn = lambda: m.postprocess_compute(drv.U)  # noqa: E731
        for _ in range(args.warmup):
            fn()
        ms, lo, hi = timed(ctx, fn, args.calls)
        sweep_b, norm_b = own_bytes(dim, kp, stencil, len(names), dim <= 2)
        tbs = (sweep_b + norm_b) * off.n_owned / (ms * 1e-3) / 1e12
        bounds = m.postprocess_bounds()
        print(f"| {label} | {off.n_owned} | {', '.join(names)} | {sweep_b:.0f} + {norm_b} | {ms:.4f} ({lo:.4f} - {hi:.4f}) | "
              f"{tbs:.2f} | {step5:.4f} | {ms / step5:.2f} |", flush=True)
        print(f"<!-- {label}: sum of steps 2 - 7 {update_ms:.4f} ms per update over {n_upd.value} updates; "
              f"q_max / q_min of {names[0]}: {bounds[names[0]]} -->", flush=True)
    m.close()
    off.close()
