"""Rigid pose refinement against a sampled signed-distance field, in numpy float64: the rules and their restatement.

The model learns two signed-distance fields (hand, object); Model.field_surface(return_values=True) gives them on a per-sample grid.
Fitting the predicted mesh to the field the same network predicts is the test-time step of the SDF line this code descends from
(Grasping Field, AlignSDF, gSDF): a small non-linear least-squares problem per sample.  This module fixes the rules of that fit and
is their yardstick (tests/test_field_fit_oracle.py); it is NOT on the model's path and no fallback - the project's hot paths are HIP:
hoisdf_field_fit (csrc/field_fit.hip, csrc/field_fit_rules.h; ops.field_fit, refine.fit_pair) runs these rules with one workgroup
per sample in the summation order below, as iters + 2 launches - the iteration over steps is the host's - and is held to this module
(tests/test_field_fit_rules_host.py on the CPU, tests/test_gpu_field_fit.py on the GPU).
Limits: the field is the trilinear interpolant of the grid values, not the network; rigid only, no articulation; no gradient.

All arithmetic is float64 on the float32 inputs, every operation rounded on its own (no product fused into a sum), in the order
written here; a parenthesis is evaluated first, otherwise left to right.
Frame and grid: values / grid / n are what hoisdf_iso_extract takes (include/hoisdf.h "iso-surface"): grid = lo xyz, cell xyz, 0, 0;
  node i = ix + n (iy + n iz) sits at lo + ix cell per axis.  The points are in the frame of the field.
Pose: x_i = R (p_i - c) + c + t, per axis k: q = p_i - c, r_k = (R_k0 q_0 + R_k1 q_1) + R_k2 q_2, x_k = (r_k + c_k) + t_k.  It starts at
  R = I, t = 0 (the caller applies its initial pose to the points beforehand).  c = the given pivot or the mean of the points: their
  sum in the order of the sums below, divided by their number.
Field read: u_k = (x_k - lo_k) / cell_k.  A point TAKES PART when 0 <= u_k <= n - 1 on all axes (a NaN fails) and all 8 corner values
  of its cell are finite.  Cell index i_k = min(floor(u_k), n - 2), fraction f_k = u_k - i_k, corner v_xyz = the value of node
  i + (x, y, z).  Along x first: d00 = v100 - v000, d10 = v110 - v010, d01 = v101 - v001, d11 = v111 - v011; c00 = v000 + f_x d00,
  c10 = v010 + f_x d10, c01 = v001 + f_x d01, c11 = v011 + f_x d11; then y: c0 = c00 + f_y (c10 - c00), c1 = c01 + f_y (c11 - c01);
  then z: f = c0 + f_z (c1 - c0), the trilinear interpolant.  Its analytic gradient g - differences of the corners along one axis,
  interpolated on the other two, divided by cell: e0 = d00 + f_y (d10 - d00), e1 = d01 + f_y (d11 - d01),
  g_x = (e0 + f_z (e1 - e0)) / cell_x; h0 = c10 - c00, h1 = c11 - c01, g_y = (h0 + f_z (h1 - h0)) / cell_y; g_z = (c1 - c0) / cell_z.
Cost: Huber with threshold huber (taken as a float32), in field units: rho = 0.5 f f and w = 1 for |f| <= huber, else
  rho = huber (|f| - 0.5 huber) and w = huber / |f|.  cost = sum rho / n_used, n_used = the points that take part.  (The model's
  field is tanh-shaped and saturates away from the surface: hence a robust loss.)
Step: the perturbation is on the left, about the moved pivot c + t: J_i = [g, r x g] (r = the rotated offset above = x - c - t),
  d = [delta, omega].  H = sum (w J_a) J_b / n_used (upper triangle), b = sum (w f) J_a / n_used.  Solve
  (H + lambda diag(H) + 1e-12 I) d = -b, the diagonal as (H_kk + lambda H_kk) + 1e-12, by a 6 x 6 Cholesky factorisation L L^T, column
  by column, every inner sum ascending, then L y = -b ascending and L^T d = y descending.  A pivot that is not > 0 counts as a
  rejected step.  Trial pose: R' = exp(omega) R, t' = t + delta; exp(omega) = I + a K + b K^2 with th^2 = (w_x w_x + w_y w_y) + w_z w_z,
  a = sin(th) / th, b = 0.5 (sin(th / 2) / (th / 2))^2 (a = 1, b = 0.5 at th = 0), entry (i, j) = ((i == j) + a K_ij) +
  b (w_i w_j - (i == j) th^2), and the product (E_i0 R_0j + E_i1 R_1j) + E_i2 R_2j.
  ACCEPT when the trial's n_used is > 0 and 100 n_used >= min_used_percent x the START pose's n_used, and its cost is strictly
  smaller: lambda <- max(lambda / 10, 1e-9), the trial's sums are the next normal equations.  Otherwise lambda <- 10 lambda, and the
  sample stops once lambda > 1e9.  lambda starts at lambda0.
Stop: the stop test comes BEFORE a step is tried.  A sample stops after ``iters`` tried steps (a rejected one included, at most
  MAX_ITERS); or when the solved step has max(|delta|_inf, |omega|_inf extent) < step_tol, extent = max over the points and axes of
  |p_i - c| (that step is not tried and not counted).  A stopped sample does not change again.
A sample with no participating point at the start: R = I, t = 0, cost 0, info 0.
Sums: one order, that of a workgroup of 256 lanes.  Lane l takes points l, l + 256, ... ascending; the 256 partials are combined by an
  xor tree within each wave of 64 (v += v of lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1), then ((wave 0 + wave 1) + wave 2) + wave 3.  With
  ``order="plain"`` one ascending sum instead - the two agree to rounding, which the test shows."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

MAX_ITERS = 64
LANES, WAVE = 256, 64
# H as its upper triangle, row-major: (0,0) (0,1) .. (0,5) (1,1) .. (5,5)
TRI = tuple((a, b) for a in range(6) for b in range(a, 6))


def lane_sum(terms: np.ndarray, order: str = "lanes") -> np.ndarray:
    """terms (n, k) -> (k,): the sum over the n points in the order of the 256 lanes, or ascending"""
    terms = np.asarray(terms, np.float64).reshape(len(terms), -1)
    if order == "plain":
        acc = np.zeros(terms.shape[1])
        for row in terms:
            acc = acc + row
        return acc
    lanes = np.zeros((LANES, terms.shape[1]))
    for s in range(0, len(terms), LANES):                            # lane l: points l, l + 256, ... ascending
        chunk = terms[s:s + LANES]
        lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
    waves = []
    for w in range(LANES // WAVE):
        v = lanes[w * WAVE:(w + 1) * WAVE]
        for o in (32, 16, 8, 4, 2, 1):                               # v += shuffle_xor(v, o): every lane ends with the same bits
            v = v + v[np.arange(WAVE) ^ o]
        waves.append(v[0])
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def field_read(values, grid, n: int, x: np.ndarray):
    """values (n^3,), grid (8,), x (m, 3) float64 -> (takes part (m,) bool, f (m,), g (m, 3)); rows that take no part hold zeros"""
    v = np.asarray(values, np.float32).astype(np.float64)
    g8 = np.asarray(grid, np.float32).astype(np.float64)
    lo, cell = g8[:3], g8[3:6]
    with np.errstate(invalid="ignore", divide="ignore"):
        u = (x - lo) / cell
        ok = np.all((u >= 0.0) & (u <= float(n - 1)), axis=1)
    us = np.where(ok[:, None], u, 0.0)
    i = np.minimum(np.floor(us), n - 2).astype(np.int64)
    fr = us - i
    base = i[:, 0] + n * (i[:, 1] + n * i[:, 2])
    c = {(dx, dy, dz): v[base + dx + n * (dy + n * dz)] for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)}
    ok &= np.all(np.isfinite(np.stack(list(c.values()))), axis=0)
    for k in c:
        c[k] = np.where(ok, c[k], 0.0)
    fx, fy, fz = fr[:, 0], fr[:, 1], fr[:, 2]
    d00, d10, d01, d11 = c[1, 0, 0] - c[0, 0, 0], c[1, 1, 0] - c[0, 1, 0], c[1, 0, 1] - c[0, 0, 1], c[1, 1, 1] - c[0, 1, 1]
    c00, c10, c01, c11 = c[0, 0, 0] + fx * d00, c[0, 1, 0] + fx * d10, c[0, 0, 1] + fx * d01, c[0, 1, 1] + fx * d11
    c0, c1 = c00 + fy * (c10 - c00), c01 + fy * (c11 - c01)
    f = c0 + fz * (c1 - c0)
    e0, e1 = d00 + fy * (d10 - d00), d01 + fy * (d11 - d01)
    gx = (e0 + fz * (e1 - e0)) / cell[0]
    h0, h1 = c10 - c00, c11 - c01
    gy = (h0 + fz * (h1 - h0)) / cell[1]
    gz = (c1 - c0) / cell[2]
    grad = np.stack([gx, gy, gz], 1)
    return ok, np.where(ok, f, 0.0), np.where(ok[:, None], grad, 0.0)


def pose_points(R, t, c, p) -> np.ndarray:
    """x = R (p - c) + c + t, per axis ((R_k0 q_0 + R_k1 q_1) + R_k2 q_2) + c_k) + t_k -> (rotated offsets R q, x)"""
    q = p - c
    rq = np.stack([(R[k, 0] * q[:, 0] + R[k, 1] * q[:, 1]) + R[k, 2] * q[:, 2] for k in range(3)], 1)
    return rq, (rq + c) + t


def normal_equations(values, grid, n: int, p, c, R, t, huber: float, order: str = "lanes") -> Dict:
    """the sums of one pose: n_used, cost, H (21,), b (6,) - all divided by n_used - and ``abs`` (28,): the same sums over the
    terms' magnitudes (the scale against which another implementation's sums are compared), in the order H, b, cost"""
    rq, x = pose_points(R, t, c, p)
    ok, f, g = field_read(values, grid, n, x)
    n_used = int(ok.sum())
    a = np.abs(f)
    small = a <= huber
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(small, 1.0, huber / a)
    rho = np.where(small, 0.5 * f * f, huber * (a - 0.5 * huber))
    J = np.concatenate([g, np.stack([rq[:, 1] * g[:, 2] - rq[:, 2] * g[:, 1], rq[:, 2] * g[:, 0] - rq[:, 0] * g[:, 2],
                                     rq[:, 0] * g[:, 1] - rq[:, 1] * g[:, 0]], 1)], 1)
    wJ, wf = w[:, None] * J, w * f
    terms = np.concatenate([np.stack([wJ[:, i] * J[:, j] for i, j in TRI], 1), wf[:, None] * J, rho[:, None]], 1)
    terms = np.where(ok[:, None], terms, 0.0)
    s, sa = lane_sum(terms, order), lane_sum(np.abs(terms), order)
    d = float(max(n_used, 1))
    s, sa = s / d, sa / d
    return {"n_used": n_used, "cost": float(s[27]), "H": s[:21], "b": s[21:27], "abs": sa, "normal": s.copy()}


def solve_step(H21, b, lam: float) -> Optional[np.ndarray]:
    """(H + lam diag(H) + 1e-12 I) d = -b by Cholesky in ascending index order -> d (6,) = delta, omega; None: a pivot was not positive"""
    A = np.zeros((6, 6))
    for k, (i, j) in enumerate(TRI):
        A[i, j] = A[j, i] = H21[k]
    for k in range(6):
        A[k, k] = (A[k, k] + lam * A[k, k]) + 1e-12
    L = np.zeros((6, 6))
    for j in range(6):
        s = A[j, j]
        for k in range(j):
            s = s - L[j, k] * L[j, k]
        if not s > 0.0:
            return None
        L[j, j] = np.sqrt(s)
        for i in range(j + 1, 6):
            s = A[i, j]
            for k in range(j):
                s = s - L[i, k] * L[j, k]
            L[i, j] = s / L[j, j]
    y = np.zeros(6)
    for i in range(6):
        s = -b[i]
        for k in range(i):
            s = s - L[i, k] * y[k]
        y[i] = s / L[i, i]
    d = np.zeros(6)
    for i in range(5, -1, -1):
        s = y[i]
        for k in range(i + 1, 6):
            s = s - L[k, i] * d[k]
        d[i] = s / L[i, i]
    return d


def rodrigues(w) -> np.ndarray:
    """exp of the rotation vector: I + a K + b K^2, a = sin(th) / th, b = (sin(th / 2) / (th / 2))^2 / 2, K^2 = w w^T - th^2 I"""
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    if th > 0.0:
        h = 0.5 * th
        sh = np.sin(h) / h
        a, b = np.sin(th) / th, 0.5 * sh * sh
    else:
        a, b = 1.0, 0.5
    K = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    E = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            E[i, j] = ((1.0 if i == j else 0.0) + a * K[i, j]) + b * (w[i] * w[j] - (th2 if i == j else 0.0))
    return E


def matmul3(E, R) -> np.ndarray:
    return np.array([[(E[i, 0] * R[0, j] + E[i, 1] * R[1, j]) + E[i, 2] * R[2, j] for j in range(3)] for i in range(3)])


def fit(values, grid, n: int, points, pivot=None, n_points: Optional[int] = None, iters: int = 32, huber: float = 0.1,
        lambda0: float = 1e-3, step_tol: float = 1e-7, min_used_percent: int = 50, order: str = "lanes") -> Dict:
    """one sample.  -> rot (3, 3), trans (3,), points_out (V', 3) (all float64; an implementation with float32 outputs rounds them once, at the end), cost (2,),
    info (4,) = used at start, used at end, steps tried, steps accepted, normal (28,) / normal_abs (28,) of the START pose, and the
    trace the tests assert on: costs (the accepted costs, the start first), decisions [(trial cost, current cost, accepted)],
    steps (every tested step size), stopped_by ("none" / "step" / "iters" / "lambda")"""
    huber, lam, step_tol = (float(np.float32(v)) for v in (huber, lambda0, step_tol))
    p32 = np.asarray(points, np.float32).reshape(-1, 3)
    V = len(p32) if n_points is None else max(0, min(int(n_points), len(p32)))
    p = p32[:V].astype(np.float64)
    if pivot is None:
        c = lane_sum(p, order) / float(max(V, 1))
    else:
        c = np.asarray(pivot, np.float32).astype(np.float64).reshape(3)
    aq = np.abs(p - c)
    extent = float(np.max(np.where(np.isnan(aq), 0.0, aq))) if V else 0.0
    R, t = np.eye(3), np.zeros(3)
    cur = normal_equations(values, grid, n, p, c, R, t, huber, order)
    n0 = cur["n_used"]
    out = {"normal": cur["normal"], "normal_abs": cur["abs"], "costs": [cur["cost"]], "decisions": [], "steps": [], "stopped_by": "none"}
    if n0 == 0:
        out.update(rot=R, trans=t, points_out=pose_points(R, t, c, p)[1], cost=np.zeros(2), info=np.zeros(4, np.int64),
                   normal=np.zeros(28), normal_abs=np.zeros(28))
        return out
    tried = accepted = 0
    while True:
        if tried >= iters:
            out["stopped_by"] = "iters"
            break
        d = solve_step(cur["H"], cur["b"], lam)
        if d is None:                                                # a rejected step
            tried += 1
            lam = 10.0 * lam
            if lam > 1e9:
                out["stopped_by"] = "lambda"
                break
            continue
        size = max(np.abs(d[:3]).max(), np.abs(d[3:]).max() * extent)
        out["steps"].append(float(size))
        if size < step_tol:
            out["stopped_by"] = "step"
            break
        tried += 1
        R1, t1 = matmul3(rodrigues(d[3:]), R), t + d[:3]
        trial = normal_equations(values, grid, n, p, c, R1, t1, huber, order)
        ok = trial["n_used"] * 100 >= min_used_percent * n0 and trial["n_used"] > 0 and trial["cost"] < cur["cost"]
        out["decisions"].append((trial["cost"], cur["cost"], bool(ok)))
        if ok:
            R, t, cur = R1, t1, trial
            accepted += 1
            lam = max(lam / 10.0, 1e-9)
            out["costs"].append(cur["cost"])
        else:
            lam = 10.0 * lam
            if lam > 1e9:
                out["stopped_by"] = "lambda"
                break
    out.update(rot=R, trans=t, points_out=pose_points(R, t, c, p)[1], cost=np.array([out["costs"][0], cur["cost"]]),
               info=np.array([n0, cur["n_used"], tried, accepted], np.int64))
    return out


# ---- the analytic fields and cases of the tests ------------------------------------------------------------------------------------
BOX_HALF, BOX_RADIUS = (0.5, 0.3, 0.2), 0.02
BOX_N = 24
BOX_GRID = np.float32([-0.9, -0.8, -0.7, 1.8 / (BOX_N - 1), 1.6 / (BOX_N - 1), 1.4 / (BOX_N - 1), 0, 0])


def grid_nodes(grid, n: int) -> np.ndarray:
    """(n^3, 3) float64: node ix + n (iy + n iz) at lo + ix cell of the float32 grid"""
    g = np.asarray(grid, np.float32).astype(np.float64)
    ax = [g[k] + np.arange(n) * g[3 + k] for k in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    return np.stack([x.ravel(), y.ravel(), z.ravel()], 1)


def rounded_box_sdf(x, half=BOX_HALF, radius=BOX_RADIUS) -> np.ndarray:
    """exact signed distance to the box of half sides ``half`` (outer surface) whose edges are rounded with ``radius``"""
    q = np.abs(x) - (np.asarray(half) - radius)
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0) - radius


def box_field(grid=BOX_GRID, n: int = BOX_N) -> np.ndarray:
    """float32 (n^3,): tanh of the rounded box's distance on the grid's nodes"""
    return np.tanh(rounded_box_sdf(grid_nodes(grid, n))).astype(np.float32)


def sphere_field(grid=BOX_GRID, n: int = BOX_N, r: float = 0.3) -> np.ndarray:
    return np.tanh(np.linalg.norm(grid_nodes(grid, n), axis=-1) - r).astype(np.float32)


def box_surface_points(count: int, seed: int) -> np.ndarray:
    """``count`` float64 points on the flat part of the box's six faces, drawn by area"""
    rng = np.random.default_rng(seed)
    h = np.asarray(BOX_HALF)
    area = np.array([h[1] * h[2], h[0] * h[2], h[0] * h[1]])
    axis = rng.choice(3, count, p=area / area.sum())
    pts = rng.uniform(-1.0, 1.0, (count, 3)) * (h - BOX_RADIUS)
    pts[np.arange(count), axis] = np.where(rng.uniform(size=count) < 0.5, -1.0, 1.0) * h[axis]
    return pts


def axis_angle(axis, degrees: float) -> np.ndarray:
    a = np.asarray(axis, np.float64)
    return rodrigues(a / np.linalg.norm(a) * np.deg2rad(degrees))


CASE_MOVES = ((10.0, 0.05), (20.0, 0.1), (30.0, 0.15), (45.0, 0.2))
# one seed per case, chosen so that the fit of the case keeps clear of rounding-level branches (``clear_of_rounding``)
CASE_SEEDS = (30, 14, 21, 4)


def clear_of_rounding(result: Dict, step_tol: float = 1e-7) -> bool:
    """what makes a run comparable across implementations that differ in rounding: every accept / reject decision was taken with
    |trial cost - cost| > 1e-9 cost, and no tested step size lies within a factor 2 of step_tol"""
    decided = all(abs(trial - cur) > 1e-9 * cur for trial, cur, _ in result["decisions"])
    return decided and not any(0.5 * step_tol <= s <= 2.0 * step_tol for s in result["steps"])


def box_case(k: int, count: int = 300, seed: Optional[int] = None) -> Dict:
    """case k of CASE_MOVES: ``count`` points of the box's faces moved by the case's rotation (about a seeded axis, about their
    mean) and translation (along a seeded direction) -> truth (count, 3) float64, points (count, 3) float32 = the moved ones"""
    deg, dist = CASE_MOVES[k]
    seed = CASE_SEEDS[k] if seed is None else seed
    rng = np.random.default_rng(1000 * seed + k)
    truth = box_surface_points(count, 100 * seed + k)
    Rm = axis_angle(rng.normal(size=3), deg)
    d = rng.normal(size=3)
    c = truth.mean(0)
    moved = (truth - c) @ Rm.T + c + dist * d / np.linalg.norm(d)
    return {"truth": truth, "points": moved.astype(np.float32), "degrees": deg, "distance": dist}
