"""Initial/Dirichlet state recipes used as synthetic inputs (formulas restated from
source/euler/initial_state_{uniform,radial_contrast,isentropic_vortex}.h and
source/euler/hyperbolic_system.h:1255-1272 `from_primitive_state`)."""
from __future__ import annotations

import numpy as np

from . import capi


def euler_from_primitive(rho, vel, p, gamma=1.4):
    """vel: [..., dim]. Returns conserved [..., dim+2] = (rho, rho v, p/(gamma-1) + rho |v|^2/2)."""
    rho = np.asarray(rho, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    U = np.empty(vel.shape[:-1] + (vel.shape[-1] + 2,), dtype=np.float64)
    U[..., 0] = rho
    U[..., 1:-1] = rho[..., None] * vel
    U[..., -1] = p / (gamma - 1.0) + 0.5 * rho * np.sum(vel * vel, axis=-1)
    return U


def euler_uniform(positions, rho=1.4, u=3.0, p=1.0, gamma=1.4, direction=None):
    """initial_state_uniform.h:36-50: primitive (rho,u,p) along `direction` (default +x)."""
    n, dim = positions.shape
    vel = np.zeros((n, dim))
    d = np.zeros(dim)
    d[0] = 1.0
    if direction is not None:
        d = np.asarray(direction, dtype=np.float64)
        d = d / np.linalg.norm(d)
    vel[:] = u * d
    return euler_from_primitive(np.full(n, rho), vel, np.full(n, p), gamma)


def euler_radial_contrast(positions, inner=(1.0, 0.0, 100.0), outer=(1.0, 0.0, 0.1), radius=0.1,
                          gamma=1.4, center=None):
    """initial_state_radial_contrast.h:29-62 (|x| <= radius -> inner state)."""
    n, dim = positions.shape
    x = positions if center is None else positions - np.asarray(center)
    r = np.linalg.norm(x, axis=1)
    inside = r <= radius
    rho = np.where(inside, inner[0], outer[0])
    p = np.where(inside, inner[2], outer[2])
    vel = np.zeros((n, dim))
    return euler_from_primitive(rho, vel, p, gamma)


def euler_isentropic_vortex(positions, t, mach=1.0, beta=5.0, gamma=1.4, direction=(1.0, 1.0),
                            position=(-1.0, -1.0)):
    """initial_state_isentropic_vortex.h:54-92 composed with the affine transform of
    initial_values.template.h:66-148 (translate by `position`, rotate onto `direction`)."""
    n, dim = positions.shape
    rho, u, v, p, (nx, ny) = euler_isentropic_vortex_primitive(positions, t, mach, beta, gamma, direction, position)
    E = p / (gamma - 1.0) + 0.5 * rho * (u * u + v * v)
    # affine_transform_vector: rotate the momentum into the lab frame
    mx, my = rho * u, rho * v
    U = np.zeros((n, dim + 2))
    U[:, 0] = rho
    U[:, 1] = nx * mx - ny * my
    U[:, 2] = ny * mx + nx * my
    U[:, -1] = E
    return U


def euler_isentropic_vortex_primitive(positions, t, mach=1.0, beta=5.0, gamma=1.4, direction=(1.0, 1.0),
                                      position=(-1.0, -1.0)):
    """The primitive state of euler_isentropic_vortex in the vortex frame: (rho, u, v, p, (nx, ny)) with (nx, ny) the
    normalised direction the velocity is rotated back with."""
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    nx, ny = d[0], d[1]
    x = positions[:, 0] - position[0]
    y = positions[:, 1] - position[1]
    # affine_transform: rotate the point back into the vortex frame
    xr = nx * x + ny * y
    yr = -ny * x + nx * y
    xb = xr - mach * t
    yb = yr
    r2 = xb * xb + yb * yb
    factor = beta / (2.0 * np.pi) * np.exp(0.5 - 0.5 * r2)
    T = 1.0 - (gamma - 1.0) / (2.0 * gamma) * factor * factor
    u = mach - factor * yb
    v = factor * xb
    rho = T ** (1.0 / (gamma - 1.0))
    p = rho ** gamma
    return rho, u, v, p, (nx, ny)


def sw_circular_dam_break(positions, h_inner=2.5, h_outer=0.5, radius=2.5):
    """source/shallow_water/initial_state_circular_dam_break.h:48-54 (compares |x|^2 with `radius`,
    sic): h = h_inner where |x|^2 <= radius, else h_outer; zero momentum. Returns (h, q) states."""
    n, dim = positions.shape
    r2 = np.sum(positions * positions, axis=1)
    U = np.zeros((n, dim + 1))
    U[:, 0] = np.where(r2 <= radius, h_inner, h_outer)
    return U


def aeos_specific_internal_energy(params, rho, p):
    """EquationOfState::specific_internal_energy(rho, p) of the closed-form equations of state
    (source/euler_aeos/equation_of_state_*.h), vectorised; `params` is a capi.Params. With eos = capi.EOS_FUNCTION
    the "specific internal energy" expression -- the Python attribute `eos_function_sie` of `params`, None or absent:
    the reference's default -- goes through the library's host interpreter (capi.eos_function_evaluate)."""
    rho = np.asarray(rho, dtype=np.float64)
    p = np.asarray(p, dtype=np.float64)
    if params.eos == capi.EOS_FUNCTION:
        rho_b, p_b = np.broadcast_arrays(rho, p)
        e = capi.eos_function_evaluate(capi.EOS_SPECIFIC_INTERNAL_ENERGY, getattr(params, "eos_function_sie", None),
                                       rho_b, p_b)
        return e.reshape(rho_b.shape)
    g = params.gamma
    if params.eos == capi.EOS_POLYTROPIC_GAS:
        return p / (rho * (g - 1.0))
    if params.eos == capi.EOS_NOBLE_ABEL_STIFFENED_GAS:
        b, q, pinf = params.eos_covolume_b, params.eos_q, params.eos_pinf
        return q + (p + g * pinf) * (1.0 - b * rho) / (rho * (g - 1.0))
    if params.eos == capi.EOS_VAN_DER_WAALS:
        a, b = params.eos_vdw_a, params.eos_covolume_b
        return (p + a * rho * rho) * (1.0 - b * rho) / (rho * (g - 1.0)) - a * rho
    ratio = rho / params.jwl_rho_0
    first = params.jwl_A * (1.0 - params.jwl_omega / params.jwl_R1 * ratio) * np.exp(-params.jwl_R1 / ratio)
    second = params.jwl_B * (1.0 - params.jwl_omega / params.jwl_R2 * ratio) * np.exp(-params.jwl_R2 / ratio)
    return (p - first - second) / (rho * params.jwl_omega)


def aeos_from_primitive(params, rho, vel, p):
    """HyperbolicSystemView::from_initial_state (source/euler_aeos/hyperbolic_system.h:1470-1512):
    primitive (rho, v, p) -> conserved state with the selected equation of state."""
    rho = np.asarray(rho, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)
    e = aeos_specific_internal_energy(params, rho, p)
    U = np.empty(vel.shape[:-1] + (vel.shape[-1] + 2,), dtype=np.float64)
    U[..., 0] = rho
    U[..., 1:-1] = rho[..., None] * vel
    U[..., -1] = rho * e + 0.5 * rho * np.sum(vel * vel, axis=-1)
    return U


def aeos_from_primitive_state(rho, vel, e):
    """HyperbolicSystemView::from_primitive_state (source/euler_aeos/hyperbolic_system.h:1473-1493): primitive
    (rho, v, e) with e the SPECIFIC INTERNAL ENERGY -> (rho, rho v, rho e + rho |v|^2 / 2); no equation of state
    enters. What the reference's "function" state calls with its "pressure expression" in the last slot."""
    rho = np.asarray(rho, dtype=np.float64)
    vel = np.asarray(vel, dtype=np.float64)
    e = np.asarray(e, dtype=np.float64)
    U = np.empty(vel.shape[:-1] + (vel.shape[-1] + 2,), dtype=np.float64)
    U[..., 0] = rho
    U[..., 1:-1] = rho[..., None] * vel
    U[..., -1] = rho * e + 0.5 * rho * np.sum(vel * vel, axis=-1)
    return U


# ---------------------------------------------------------------------------
# Analytic solutions of the reference's verification configurations (1-D ones take x relative to
# the `position` of subsection "E - InitialValues", direction +1)

def euler_leblanc(positions, t, position=0.0):
    """source/euler/initial_state_leblanc.h:63-120: the Le Blanc shock tube (gamma = 5/3), conserved
    1-D states (rho, m, E) of the exact Riemann fan at time t."""
    rho, u, p = euler_leblanc_primitive(positions, t, position)
    U = np.empty((rho.size, 3))
    U[:, 0] = rho
    U[:, 1] = rho * u
    U[:, 2] = p / (5.0 / 3.0 - 1.0) + 0.5 * rho * u * u
    return U


def euler_leblanc_primitive(positions, t, position=0.0):
    """The primitive 1-D states (rho, u, p) of euler_leblanc."""
    x = np.asarray(positions, dtype=np.float64)[:, 0] - position
    rarefaction_speed = 0.49578489518897934
    contact_velocity = 0.62183867139173454
    right_shock_speed = 0.82911836253346982
    pre_contact_density = 5.4079335349316249e-02
    post_contact_density = 3.9999980604299963e-03
    contact_pressure = 0.51557792765096996e-03
    rho = np.full_like(x, 1.0e-3)
    u = np.zeros_like(x)
    p = np.full_like(x, 2.0 / 3.0 * 1.0e-10)
    with np.errstate(divide="ignore", invalid="ignore"):
        chi = x / t
    left = x <= -1.0 / 3.0 * t
    fan = ~left & (x < rarefaction_speed * t)
    pre = ~left & ~fan & (x < contact_velocity * t)
    post = ~left & ~fan & ~pre & (x < right_shock_speed * t)
    rho[left], u[left], p[left] = 1.0, 0.0, 2.0 / 3.0 * 1.0e-1
    rho[fan] = np.power(0.75 - 0.75 * chi[fan], 3.0)
    u[fan] = 0.75 * (1.0 / 3.0 + chi[fan])
    p[fan] = (1.0 / 15.0) * np.power(0.75 - 0.75 * chi[fan], 5.0)
    rho[pre], u[pre], p[pre] = pre_contact_density, contact_velocity, contact_pressure
    rho[post], u[post], p[post] = post_contact_density, contact_velocity, contact_pressure
    return rho, u, p


def euler_rarefaction(positions, t, gamma=1.4, position=0.0):
    """source/euler/initial_state_rarefaction.h:40-160: a single 1-rarefaction that has been running
    for t_0 = 0.2 / (u_R - u_L) already; conserved 1-D states at time t_0 + t."""
    rho, u, p = euler_rarefaction_primitive(positions, t, gamma, position)
    U = np.empty((rho.size, 3))
    U[:, 0] = rho
    U[:, 1] = rho * u
    U[:, 2] = p / (gamma - 1.0) + 0.5 * rho * u * u
    return U


def euler_rarefaction_primitive(positions, t, gamma=1.4, position=0.0):
    """The primitive 1-D states (rho, u, p) of euler_rarefaction."""
    x = np.asarray(positions, dtype=np.float64)[:, 0] - position
    rho_l, p_l = 3.0, 1.0
    c_l = np.sqrt(gamma * p_l / rho_l)
    u_l = c_l
    rho_r = 0.5
    p_r = np.power(rho_r / rho_l, gamma) * p_l
    c_r = np.sqrt(gamma * p_r / rho_r)
    u_r = u_l + 2.0 * (c_l - c_r) / (gamma - 1.0)
    k1 = 2.0 / (gamma + 1.0)
    k2 = (gamma - 1.0) / ((gamma + 1.0) * c_l)
    density_exponent = 2.0 / (gamma - 1.0)
    k3 = c_l + ((gamma - 1.0) / 2.0) * u_l
    pressure_exponent = 2.0 * gamma / (gamma - 1.0)
    tt = 0.2 / (u_r - u_l) + t
    chi = x / tt
    left = x <= tt * (u_l - c_l)
    fan = ~left & (x <= tt * (u_r - c_r))
    rho = np.full_like(x, rho_r)
    u = np.full_like(x, u_r)
    p = np.full_like(x, p_r)
    rho[left], u[left], p[left] = rho_l, u_l, p_l
    base = k1 + k2 * (u_l - chi[fan])
    rho[fan] = rho_l * np.power(base, density_exponent)
    u[fan] = k1 * (k3 + chi[fan])
    p[fan] = p_l * np.power(base, pressure_exponent)
    return rho, u, p


def sw_paraboloid_1d(positions, t, gravity=9.81, manning=0.0, free_surface_radius=3000.0,
                     water_height=10.0, length=10000.0, speed=2.0):
    """source/shallow_water/initial_state_paraboloid.h:66-101 (dim 1): the oscillating lake over a
    parabolic bathymetry with wetting and drying; returns ((h, q) states, bathymetry)."""
    x = np.asarray(positions, dtype=np.float64)[:, 0]
    a, h0, B, g, k = free_surface_radius, water_height, speed, gravity, manning
    z = h0 / (a * a) * np.power(x - 0.5 * length, 2)
    p = np.sqrt(8.0 * g * h0) / a
    s = np.sqrt(p * p - k * k) / 2.0
    term1 = (a * a * B * B) / (8.0 * g * g * h0) * np.exp(-k * t)
    term1 *= (1.0 / 4.0 * k * k - s * s) * np.cos(2.0 * s * t) - s * k * np.sin(2.0 * s * t)
    term2 = -(B * B / (4.0 * g)) * np.exp(-k * t)
    term3 = -(B / g) * np.exp(-1.0 / 2.0 * k * t)
    term3 = term3 * (s * np.cos(s * t) + 1.0 / 2.0 * k * np.sin(s * t)) * (x - 1.0 / 2.0 * length)
    htilde = h0 - z
    htilde = htilde + (term1 + term2 + term3)
    h = np.maximum(htilde, 0.0)
    v = B * np.exp(-1.0 / 2.0 * k * t) * np.sin(s * t)
    return np.column_stack([h, h * v]), z


def sw_ritter_dam_break(positions, t, gravity=9.81, time_initial=0.1, left_depth=0.005, position=0.0):
    """source/shallow_water/initial_state_ritter_dam_break.h:58-80: dam break over a dry bed."""
    x = np.asarray(positions, dtype=np.float64)[:, 0] - position
    g = gravity
    aL = np.sqrt(g * left_depth)
    xA = -(t + time_initial) * aL
    xB = 2.0 * (t + time_initial) * aL
    tmp = aL - x / (2.0 * (t + time_initial))
    h_exp = 4.0 / (9.0 * g) * tmp * tmp
    v_exp = 2.0 / 3.0 * (x / (t + time_initial) + aL)
    U = np.zeros((x.size, 2))
    left = x <= xA
    fan = ~left & (x <= xB)
    U[left, 0] = left_depth
    U[fan, 0] = h_exp[fan]
    U[fan, 1] = h_exp[fan] * v_exp[fan]
    return U


def sw_smooth_vortex(positions, t, gravity=9.81, reference_depth=1.0, mach=2.0, beta=0.1,
                     direction=(1.0, 0.0), position=(0.0, 0.0)):
    """source/shallow_water/initial_state_smooth_vortex.h:55-85 (no bathymetry) composed with the affine
    transform of initial_values.template.h:66-148."""
    d = np.asarray(direction, dtype=np.float64)
    d = d / np.linalg.norm(d)
    nx, ny = d
    x = positions[:, 0] - position[0]
    y = positions[:, 1] - position[1]
    xr = nx * x + ny * y
    yr = -ny * x + nx * y
    xb = xr - mach * t
    yb = yr
    r2 = xb * xb + yb * yb
    factor = beta / (2.0 * np.pi) * np.exp(0.5 - 0.5 * r2)
    h = reference_depth - 1.0 / (2.0 * gravity) * factor * factor
    u = mach - factor * yb
    v = factor * xb
    mx, my = h * u, h * v
    return np.column_stack([h, nx * mx - ny * my, ny * mx + nx * my])


def sw_sloping_friction(positions, manning=0.01, ramp_slope=1.0, initial_discharge=0.1):
    """source/shallow_water/initial_state_sloping_friction.h:50-85: uniform flow down an incline in
    balance with Manning friction; returns ((h, q) states, bathymetry)."""
    x = np.asarray(positions, dtype=np.float64)[:, 0]
    exponent = 1.0 / (2.0 + 4.0 / 3.0)
    profile = manning * manning * initial_discharge * initial_discharge / ramp_slope
    h = np.power(profile, exponent)
    U = np.empty((x.size, 2))
    U[:, 0] = h
    U[:, 1] = initial_discharge
    return U, -ramp_slope * x


# ---------------------------------------------------------------------------
# The Riemann-data, shock-front, ramp-up and Noh states (capi.IV_LIBRARY_STATES). Each function takes the positions in
# the FRAME OF THE STATE (behind the affine transform of initial_values.template.h:66-148) and returns the primitive
# state there: (rho, vel [n, dim], p) for Euler / EulerAEOS -- the conserved state is euler_from_primitive or
# aeos_from_primitive of it, the momentum rotated back --, (h, u) for shallow water. `ramp up` blends two CONSERVED
# states and returns the weights. The device follows these statements one by one (initial_states_library_device.hpp).

def _frame(positions):
    x = np.asarray(positions, dtype=np.float64)
    return x, x.shape[0], x.shape[1]


def _piecewise(n, dim, masks_and_states, otherwise):
    """1-D primitive states (rho, u, p) selected by masks, the first that holds; velocity along the first axis"""
    rho, u, p = (np.full(n, otherwise[q], dtype=np.float64) for q in range(3))
    for mask, state in reversed(masks_and_states):
        rho, u, p = (np.where(mask, state[q], c) for q, c in enumerate((rho, u, p)))
    vel = np.zeros((n, dim))
    vel[:, 0] = u
    return rho, vel, p


def euler_contrast_primitive(positions, left=(1.4, 0.0, 1.0), right=(1.4, 0.0, 1.0)):
    """source/euler/initial_state_contrast.h: `right` where x > 0, else `left`."""
    x, n, dim = _frame(positions)
    return _piecewise(n, dim, [(x[:, 0] > 0.0, right)], left)


def euler_three_state_contrast_primitive(positions, left=(1.0, 0.0, 1.0e3), left_length=0.1,
                                         middle=(1.0, 0.0, 1.0e-2), middle_length=0.8, right=(1.0, 0.0, 1.0e2)):
    """source/euler/initial_state_three_state_contrast.h: x >= left_length + middle_length -> right,
    x >= left_length -> middle, else left."""
    x, n, dim = _frame(positions)
    return _piecewise(n, dim, [(x[:, 0] >= left_length + middle_length, right), (x[:, 0] >= left_length, middle)],
                      left)


def euler_four_state_contrast_primitive(positions, bottom_left=(1.4, 0.0, 0.0, 1.0), bottom_right=(1.4, 0.0, 0.0, 1.0),
                                        top_left=(1.4, 0.0, 0.0, 1.0), top_right=(1.4, 0.0, 0.0, 1.0)):
    """source/euler/initial_state_four_state_contrast.h (dim >= 2): states (rho, u, v, p); x >= 0 selects right,
    y >= 0 selects top; a third velocity component is zero (expand_state)."""
    x, n, dim = _frame(positions)
    if dim == 1:
        raise ValueError("four state contrast is not defined for dim = 1")
    east, north = x[:, 0] >= 0.0, x[:, 1] >= 0.0
    top = [np.where(east, top_right[q], top_left[q]) for q in range(4)]
    bottom = [np.where(east, bottom_right[q], bottom_left[q]) for q in range(4)]
    rho, u, v, p = (np.where(north, top[q], bottom[q]) for q in range(4))
    vel = np.zeros((n, dim))
    vel[:, 0], vel[:, 1] = u, v
    return rho, vel, p


def euler_shock_front_constants(right=(1.4, 0.0, 1.0), mach=2.0, gamma=1.4, b=0.0):
    """The constructor of source/euler/initial_state_shock_front.h: (primitive left state (rho, u, p), S3) of the
    shock that runs into `right` with Mach number `mach`; b: the covolume of the interpolatory equation of state
    (eos_interpolation_b; 0 for Euler)."""
    rho_R, u_R, p_R = (float(c) for c in right)
    a_R = np.sqrt(gamma * p_R / rho_R / (1.0 - b * rho_R))
    mach_R = u_R / a_R
    S3 = mach * a_R
    delta_mach = mach_R - mach
    rho_L = rho_R * (gamma + 1.0) * delta_mach * delta_mach / ((gamma - 1.0) * delta_mach * delta_mach + 2.0)
    u_L = (1.0 - rho_R / rho_L) * S3 + rho_R / rho_L * u_R
    p_L = p_R * (2.0 * gamma * delta_mach * delta_mach - (gamma - 1.0)) / (gamma + 1.0)
    return (float(rho_L), float(u_L), float(p_L)), float(S3)


def euler_shock_front_primitive(positions, t, right=(1.4, 0.0, 1.0), mach=2.0, gamma=1.4, b=0.0):
    """source/euler/initial_state_shock_front.h: `right` where x - S3 t > 0, else the post-shock state."""
    x, n, dim = _frame(positions)
    left, S3 = euler_shock_front_constants(right, mach, gamma, b)
    position_1d = x[:, 0] - S3 * t
    return _piecewise(n, dim, [(position_1d > 0.0, right)], left)


def euler_ramp_up_weights(t, time_initial=0.0, time_final=1.0):
    """source/euler/initial_state_ramp_up.h: (alpha, beta) of result = alpha U_initial + beta U_final with the two
    CONSERVED states; (1, 0) up to time_initial and (0, 1) from time_final on mean "the state itself", unblended."""
    if t <= time_initial:
        return 1.0, 0.0
    if t >= time_final:
        return 0.0, 1.0
    factor = np.cos(0.5 * np.pi * (t - time_initial) / (time_final - time_initial))
    alpha = factor * factor
    return float(alpha), float(1.0 - alpha)


def ramp_up_blend(U_initial, U_final, t, time_initial=0.0, time_final=1.0):
    """the blend of euler_ramp_up_weights on conserved states [n, k]"""
    if t <= time_initial:
        return np.array(U_initial, dtype=np.float64)
    if t >= time_final:
        return np.array(U_final, dtype=np.float64)
    alpha, beta = euler_ramp_up_weights(t, time_initial, time_final)
    return alpha * np.asarray(U_initial) + beta * np.asarray(U_final)


NOH_MIN = 10.0 * float(np.finfo(np.float64).tiny)


def euler_noh_constants(dim, rho0=1.0, u0=1.0, gamma=1.4):
    """(D, interior density, interior pressure) of source/euler/initial_state_noh.h; the integer powers
    pow(., dim) and pow(., dim - 1) written out as products, left to right."""
    D = u0 * (gamma - 1.0) / 2.0
    ratio = (gamma + 1.0) / (gamma - 1.0)
    ratio_dim, plus_dim, minus_dim1 = ratio, gamma + 1.0, 1.0
    for _ in range(dim - 1):
        ratio_dim = ratio_dim * ratio
        plus_dim = plus_dim * (gamma + 1.0)
        minus_dim1 = minus_dim1 * (gamma - 1.0)
    rho_in = rho0 * ratio_dim
    p_in = 0.5 * rho0 * u0 * u0
    p_in = p_in * (plus_dim / minus_dim1)
    return float(D), float(rho_in), float(p_in)


def euler_noh_primitive(positions, t, rho0=1.0, u0=1.0, p0=1.0e-12, gamma=1.4):
    """source/euler/initial_state_noh.h: the radial implosion; velocity -u0 x / (|x| + min) in ALL dim components,
    min = 10 DBL_MIN; inside the shock |x| / t < D the state at rest, outside rho0 (1 + t / (|x| + min))^(dim - 1);
    t == 0 is never interior."""
    x, n, dim = _frame(positions)
    D, rho_in, p_in = euler_noh_constants(dim, rho0, u0, gamma)
    norm2 = x[:, 0] * x[:, 0]
    for d in range(1, dim):
        norm2 = norm2 + x[:, d] * x[:, d]
    norm = np.sqrt(norm2)
    denominator = norm + NOH_MIN
    interior = np.zeros(n, dtype=bool) if t == 0.0 else norm / t < D
    growth = 1.0 + t / denominator
    power = np.ones(n)
    for _ in range(dim - 1):
        power = power * growth
    rho = np.where(interior, rho_in, rho0 * power)
    vel = np.where(interior[:, None], 0.0 * x, (-u0 * x) / denominator[:, None])
    p = np.where(interior, p_in, p0)
    return rho, vel, p


SMOOTH_WAVE_LEFT, SMOOTH_WAVE_RIGHT = 0.1, 0.3


def fixed_power_3(x):
    """dealii::Utilities::fixed_power<3>: x * ((x * x) * 1)"""
    return x * (x * x)


def fixed_power_6(x):
    """dealii::Utilities::fixed_power<6>(x) = fixed_power<3>(x * x)"""
    x2 = x * x
    return x2 * (x2 * x2)


def euler_smooth_wave_primitive(positions, t, rho_ref=1.0, p_ref=1.0, mach=1.0):
    """source/euler/initial_state_smooth_wave.h: rho_ref + 64 (x - x0)^3 (x1 - x)^3 / (x1 - x0)^6 on
    x0 = 0.1 <= x - mach t <= x1 = 0.3, rho_ref elsewhere; velocity `mach` along the first axis, pressure p_ref."""
    x, n, dim = _frame(positions)
    left, right = SMOOTH_WAVE_LEFT, SMOOTH_WAVE_RIGHT
    xb = x[:, 0] - mach * t
    polynomial = 64.0 * fixed_power_3(xb - left) * fixed_power_3(right - xb) / fixed_power_6(right - left)
    rho = np.where((left <= xb) & (xb <= right), rho_ref + polynomial, rho_ref)
    vel = np.zeros((n, dim))
    vel[:, 0] = mach
    return rho, vel, np.full(n, float(p_ref))


def euler_astro_jet_primitive(positions, jet_width=0.05, jet=(5.0, 30.0, 0.4127), ambient=(5.0, 0.0, 0.4127)):
    """source/euler/initial_state_astro_jet.h (dim >= 2): the jet state where x < 1e-12 and |y| <= jet_width."""
    x, n, dim = _frame(positions)
    if dim == 1:
        raise ValueError("astro jet is not defined for dim = 1")
    return _piecewise(n, dim, [((x[:, 0] < 1.0e-12) & (np.abs(x[:, 1]) <= jet_width), jet)], ambient)


def sw_uniform_primitive(positions, state=(1.0, 1.0)):
    """source/shallow_water/initial_state_uniform.h: (h, u) everywhere, zero bathymetry."""
    x, n, _ = _frame(positions)
    return np.full(n, float(state[0])), np.full(n, float(state[1]))


def sw_contrast_primitive(positions, left=(1.0, 0.0), right=(1.0, 0.0)):
    """source/shallow_water/initial_state_contrast.h: `right` where x > 0, else `left`; zero bathymetry."""
    x, n, _ = _frame(positions)
    east = x[:, 0] > 0.0
    return np.where(east, right[0], left[0]), np.where(east, right[1], left[1])


# ---------------------------------------------------------------------------
# The shallow-water states that bring their own bathymetry (capi.IV_BATHYMETRY_STATES). Positions in the FRAME OF THE
# STATE, as above. Each sw_<state>() returns ((h, q) with q the discharge along the first axis of the frame, bathymetry);
# each sw_<state>_bathymetry() is initial_precomputations(point) alone. The device follows these statements one by one
# (initial_states_bathymetry_device.hpp): pow(x, 2) and pow(x, 3) are the products a * a and a * (a * a), std::max /
# std::min are the comparisons the C++ library makes ((a < b) ? b : a and (b < a) ? b : a, folded from the left), and
# only pow(q^2 / g, 1/3), pow(-Q, -1.5), acos, cos and cosh are library functions.

def _square(a):
    return a * a


def _cube(a):
    return a * (a * a)


def _std_max(a, *others):
    """std::max(a, b) = (a < b) ? b : a; std::max({a, b, ...}) folds it from the left"""
    out = a
    for b in others:
        out = np.where(out < b, b, out)
    return out


def _std_min(a, b):
    """std::min(a, b) = (b < a) ? b : a"""
    return np.where(b < a, b, a)


FLOW_OVER_BUMP_TYPES = ("transcritical", "subsonic")
FLOW_OVER_BUMP_XM, FLOW_OVER_BUMP_XS = 10.0, 11.7
FLOW_OVER_BUMP_H_OUTFLOW = 0.28205279813802181


def sw_flow_over_bump_bathymetry(positions):
    """source/shallow_water/initial_state_flow_over_bump.h:120-131: 0.2/64 (x - 8)^3 (12 - x)^3 on 8 <= x <= 12."""
    x, _, _ = _frame(positions)
    x = x[:, 0]
    bump = (0.2 / 64.0) * _cube(x - 8.0) * _cube(12.0 - x)
    return np.where((8.0 <= x) & (x <= 12.0), bump, 0.0)


def sw_flow_over_bump_constants(gravity=9.81, flow_type="transcritical"):
    """(h_inflow, q_inflow, cBer, d) of initial_state_flow_over_bump.h:62-80: what does not depend on the point."""
    if flow_type not in FLOW_OVER_BUMP_TYPES:
        raise ValueError("Flow type must be 'transcritical' or 'subsonic'. ")
    g = float(gravity)
    h_inflow, q_inflow = 0.28205279813802181, 0.18
    cBer = 0.2 + 1.5 * float(np.power(q_inflow * q_inflow / g, 1.0 / 3.0))
    if flow_type == "subsonic":
        q_inflow, h_inflow = 4.42, 2.0
        ratio = q_inflow / h_inflow
        cBer = ratio * ratio / (2.0 * g) + h_inflow
    d = q_inflow * q_inflow / (2.0 * g)
    return h_inflow, q_inflow, cBer, d


def sw_flow_over_bump_acos_argument(positions, gravity=9.81, flow_type="transcritical"):
    """pow(-Q, -1.5) R of Cardano's formula: the argument of acos (-1 at x = 10 of the transcritical flow)"""
    _, _, cBer, d = sw_flow_over_bump_constants(gravity, flow_type)
    b = sw_flow_over_bump_bathymetry(positions) - cBer
    Q = -_square(b) / 9.0
    R = -(27.0 * d + 2.0 * _cube(b)) / 54.0
    return np.power(-Q, -1.5) * R


def sw_flow_over_bump(positions, t, gravity=9.81, flow_type="transcritical"):
    """initial_state_flow_over_bump.h:55-106: the inflow state over the bump for t < 1e-12, afterwards the steady
    solution by Cardano's formula (transcritical: the second root on xM <= x < xS, the outflow depth on xS < x;
    x == xS keeps the first root)."""
    x, n, _ = _frame(positions)
    x = x[:, 0]
    h_inflow, q_inflow, cBer, d = sw_flow_over_bump_constants(gravity, flow_type)
    bath = sw_flow_over_bump_bathymetry(positions)
    q = np.full(n, q_inflow)
    if t < 1.0e-12:
        h_initial = h_inflow - bath
        return np.column_stack([h_initial, q]), bath
    b = bath - cBer
    Q = -_square(b) / 9.0
    R = -(27.0 * d + 2.0 * _cube(b)) / 54.0
    with np.errstate(invalid="ignore"):
        theta = np.arccos(np.power(-Q, -1.5) * R)
    h_exact = 2.0 * np.sqrt(-Q) * np.cos(theta / 3.0) - b / 3.0
    if flow_type == "transcritical":
        middle = (FLOW_OVER_BUMP_XM <= x) & (x < FLOW_OVER_BUMP_XS)
        second = 2.0 * np.sqrt(-Q) * np.cos((4.0 * np.pi + theta) / 3.0) - b / 3.0
        h_exact = np.where(middle, second, np.where(FLOW_OVER_BUMP_XS < x, FLOW_OVER_BUMP_H_OUTFLOW, h_exact))
    return np.column_stack([h_exact, q]), bath


THREE_BUMPS_CONES_2D = ((30.0, 6.0, 1.0, 1.0 / 8.0), (30.0, 24.0, 1.0, 1.0 / 8.0), (47.5, 15.0, 3.0, 3.0 / 10.0))


def sw_three_bumps_dam_break_bathymetry(positions, cone_magnitude=1.0):
    """initial_state_three_bumps_dam_break.h:95-122: one cone in 1-D (a square root of a square), three in 2-D."""
    x, _, dim = _frame(positions)
    if dim == 1:
        z3 = 3.0 - 3.0 / 10.0 * np.sqrt(_square(x[:, 0] - 47.5))
        return cone_magnitude * _std_max(z3, 0.0)
    z = [top - slope * np.sqrt(_square(x[:, 0] - cx) + _square(x[:, 1] - cy))
         for cx, cy, top, slope in THREE_BUMPS_CONES_2D]
    return cone_magnitude * _std_max(z[0], z[1], z[2], 0.0)


def sw_three_bumps_dam_break(positions, t, gravity=9.81, well_balancing_validation=False, left_depth=1.875,
                             right_depth=0.0, cone_magnitude=1.0):
    """initial_state_three_bumps_dam_break.h:63-82: the dam at x = 16 over the cones for t <= 1e-10 (or always, with
    "well balancing validation"), afterwards the constant inflow (h_L, h_L sqrt(g h_L)) everywhere."""
    x, n, _ = _frame(positions)
    bath = sw_three_bumps_dam_break_bathymetry(positions, cone_magnitude)
    if t <= 1.0e-10 or well_balancing_validation:
        h = np.where(x[:, 0] < 16.0, float(left_depth), float(right_depth))
        h = _std_max(h - bath, 0.0)
        return np.column_stack([h, np.zeros(n)]), bath
    h = float(left_depth)
    a = float(np.sqrt(gravity * h))
    return np.column_stack([np.full(n, h), np.full(n, h * a)]), bath


def sw_hou_test_bathymetry(positions):
    """initial_state_hou_test.h:74-107 (dim = 2): max(min of three paraboloids, max of a hill and two plateaus)."""
    x, _, dim = _frame(positions)
    if dim != 2:
        raise ValueError("hou test is defined for dim = 2")
    x, y = x[:, 0], x[:, 1]
    base1 = _square(x + 250.0) / 1600.0 + _square(y) / 400.0
    base2 = _square(x) / 225.0 + _square(y - 50.0) / 225.0
    base3 = _square(x - 250.0) / 1225.0 + _square(y) / 225.0 - 10.0
    base = _std_min(base1, base2)
    base = _std_min(base, base3)
    bump1 = 80.0 - _square(x + 250.0) / 50.0 - _square(y) / 50.0
    bump2 = np.where(_square(x - 200.0) + _square(y + 10.0) <= 1000.0, 10.0, 0.0)
    bump3 = np.where((np.abs(x - 380.0) <= 40.0) & (np.abs(y - 50.0) <= 40.0), 20.0, 0.0)
    bumps = _std_max(bump1, bump2)
    bumps = _std_max(bumps, bump3)
    return _std_max(base, bumps)


def sw_hou_test(positions, reservoir_water_depth=35.0):
    """initial_state_hou_test.h:42-60: water up to the reservoir depth where x < -100, dry elsewhere; at rest."""
    x, n, _ = _frame(positions)
    bath = sw_hou_test_bathymetry(positions)
    h = np.where(x[:, 0] < -100.0, _std_max(reservoir_water_depth - bath, 0.0), 0.0)
    return np.column_stack([h, np.zeros(n)]), bath


TRANSIENT_CONFIGURATIONS = ("G1", "G2", "G3", "none")
TRANSIENT_HALF_WIDTH = 31.0 / 2.0 / 100.0           # of the circular bump (G2) and the half circles (G3)
TRANSIENT_CENTERS = {"G1": 205.0 / 100.0 + (16.3 / 2.0 / 100.0), "G2": 184.5 / 100.0 + 31.0 / 2.0 / 100.0,
                     "G3": 194 / 100.0 + 31.0 / 2.0 / 100.0, "rectangle": 235.0 / 100.0 + (16.3 / 2.0 / 100.0)}


def _transient_rectangle(x, y, xc):
    length, width = 16.3 / 100.0, 8.0 / 100.0
    return np.abs((x - xc) / length + y / width) + np.abs((x - xc) / length - y / width)


def _transient_semi_circle(x, xc):
    ratio = (x - xc) / TRANSIENT_HALF_WIDTH
    number = 1.0 - _square(ratio)
    radicand = 0.5 * (np.abs(number) + number)       # positive_part
    return 7.3 / 100.0 * np.sqrt(radicand)


def sw_transient_bathymetry(positions, experimental_configuration="G1"):
    """initial_state_transient.h:90-171 (dim = 2): the tank's floor, flat then two slopes, plus the obstacle of the
    configuration; G2 and G3 overwrite `obstacle` in the order of the reference (the rectangle last)."""
    if experimental_configuration not in TRANSIENT_CONFIGURATIONS:
        raise ValueError("Case must be 'G1', 'G2', 'G3' or 'none'")
    x, n, dim = _frame(positions)
    if dim != 2:
        raise ValueError("transient experiments is defined for dim = 2")
    x, y = x[:, 0], x[:, 1]
    knee = 326.0 / 100.0
    bath = np.where((x >= 0.0) & (x <= knee), -0.00092 * x,
                    np.where(x > knee, -0.0404 * (x - knee) - 0.00092 * 326.0 / 100.0, 0.0))
    which = experimental_configuration
    if which == "none":
        return bath
    obstacle = np.zeros(n)
    if which == "G1":
        obstacle = np.where(_transient_rectangle(x, y, TRANSIENT_CENTERS["G1"]) <= 1.0, 7.0 / 100.0, obstacle)
    elif which == "G2":
        semi_circle = _transient_semi_circle(x, TRANSIENT_CENTERS["G2"])
        obstacle = _std_max(semi_circle, 0.0)
        obstacle = np.where(_transient_rectangle(x, y, TRANSIENT_CENTERS["rectangle"]) <= 1.0, 7.0 / 100.0, obstacle)
    else:
        xc = TRANSIENT_CENTERS["G3"]
        semi_circle = _transient_semi_circle(x, xc)
        inside = np.abs(x - xc) <= TRANSIENT_HALF_WIDTH
        obstacle = np.where((y < semi_circle - 24.0 / 2.0 / 100.0) & inside, 21.0 / 100.0, obstacle)
        obstacle = np.where((y > -semi_circle + 24.0 / 2.0 / 100.0) & inside, 21.0 / 100.0, obstacle)
        obstacle = np.where(_transient_rectangle(x, y, TRANSIENT_CENTERS["rectangle"]) <= 1.0, 7.0 / 100.0, obstacle)
    return bath + obstacle


def sw_transient(positions, flow_state_left=(1.0, 0.0), flow_state_right=(1.0, 0.0), experimental_configuration="G1"):
    """initial_state_transient.h:66-77: the 1-D flow state (h, q) `right` where x > 1e-8, else `left`."""
    x, _, _ = _frame(positions)
    bath = sw_transient_bathymetry(positions, experimental_configuration)
    east = x[:, 0] > 1.0e-8
    h = np.where(east, float(flow_state_right[0]), float(flow_state_left[0]))
    q = np.where(east, float(flow_state_right[1]), float(flow_state_left[1]))
    return np.column_stack([h, q]), bath


def sw_soliton_constants(gravity=9.81, still_water_depth=1.0, amplitude=0.1):
    """(celerity, width) of initial_state_soliton.h:50-52"""
    depth, amp = float(still_water_depth), float(amplitude)
    celerity = float(np.sqrt(gravity * (amp + depth)))
    width = float(np.sqrt(3.0 * amp / (4.0 * depth * depth * (amp + depth))))
    return celerity, width


def sw_soliton(positions, t, gravity=9.81, still_water_depth=1.0, amplitude=0.1):
    """initial_state_soliton.h:43-63: depth + amplitude sech^2(width (x - celerity t)) over a flat bed."""
    x, n, _ = _frame(positions)
    depth, amp = float(still_water_depth), float(amplitude)
    celerity, width = sw_soliton_constants(gravity, depth, amp)
    sech_sqd = 1.0 / _square(np.cosh(width * (x[:, 0] - celerity * t)))
    profile = depth + amp * sech_sqd
    h = _std_max(profile, 0.0)
    v = celerity * (profile - depth) / profile
    return np.column_stack([h, h * v]), np.zeros(n)


def sw_paraboloid_1d_bathymetry(positions, free_surface_radius=3000.0, water_height=10.0, length=10000.0):
    """initial_state_paraboloid.h:137-141 (dim = 1): the statement of sw_paraboloid_1d, on its own"""
    x, _, _ = _frame(positions)
    a, h0 = free_surface_radius, water_height
    return h0 / (a * a) * np.power(x[:, 0] - 0.5 * length, 2)


def sw_sloping_friction_bathymetry(positions, ramp_slope=1.0):
    """initial_state_sloping_friction.h:84-87: the statement of sw_sloping_friction, on its own"""
    x, _, _ = _frame(positions)
    return -ramp_slope * x[:, 0]
