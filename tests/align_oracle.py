"""numpy restatement of the registration rule of semigcn_amd/align.py ("The rule"): the transform, the normal equations of
one point-to-plane step (every term in float64 with plain multiplies and adds, the sums exact through ``math.fsum``), the
host step, and the whole loop with the closest-point query passed in -- the device's, or the float64 oracle of
tests/mesh_distance_oracle.py through ``oracle_query``."""
from __future__ import annotations

import math

import numpy as np

NO_FACE = 0x7FFFFFFF
N_SUMS = 40
TRIU = [(j, k) for j in range(7) for k in range(j, 7)]        # out[0..27]: row-major upper triangle


def pose_of(matrix):
    """(M [3,3], t [3]) float64 of a 4 x 4 matrix."""
    m = np.asarray(matrix, np.float64)
    return m[:3, :3].copy(), m[:3, 3].copy()


def matrix_of(M, t):
    out = np.eye(4)
    out[:3, :3], out[:3, 3] = M, t
    return out


def transform64(matrix, pts):
    """x = ((M_r0 p_x + M_r1 p_y) + M_r2 p_z) + t_r in float64 on the float32 points, not rounded."""
    M, t = pose_of(matrix)
    p = np.asarray(pts, np.float32).astype(np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((M[r, 0] * p[:, 0] + M[r, 1] * p[:, 1]) + M[r, 2] * p[:, 2]) + t[r] for r in range(3)], 1)


def transform(matrix, pts):
    """sg_align_transform: ``transform64`` rounded to float32 once."""
    with np.errstate(invalid="ignore", over="ignore"):
        return transform64(matrix, pts).astype(np.float32)


def rows(vs, faces, pts, matrix, closest, face, dist, max_dist=math.inf, with_scale=False):
    """The per-row quantities of sg_align_accumulate: ``J`` [n_used, 7], ``r`` and ``d`` [n_used] of the used rows, and the
    masks ``used``, ``far``, ``skipped`` over all rows."""
    vs = np.asarray(vs, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64)
    face = np.asarray(face, np.int64)
    x = transform64(matrix, pts)
    has = (face >= 0) & (face != NO_FACE) & np.isfinite(x).all(1)
    f = np.where(has, face, 0)
    A, B, C = (vs[faces[f, k]] for k in range(3))
    u, v = B - A, C - A
    Nf = np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2],
                   u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)
    nn = (Nf[:, 0] * Nf[:, 0] + Nf[:, 1] * Nf[:, 1]) + Nf[:, 2] * Nf[:, 2]
    ok = has & (nn != 0.0)
    d = np.asarray(dist, np.float32).astype(np.float64)
    far = ok & (d > max_dist)
    used = ok & ~far
    x, Nf, nn, d = x[used], Nf[used], nn[used], d[used]
    n = Nf / np.sqrt(nn)[:, None]
    e = x - np.asarray(closest, np.float32).astype(np.float64).reshape(-1, 3)[used]
    r = (n[:, 0] * e[:, 0] + n[:, 1] * e[:, 1]) + n[:, 2] * e[:, 2]
    J = np.zeros((x.shape[0], 7))
    J[:, 0] = x[:, 1] * n[:, 2] - x[:, 2] * n[:, 1]
    J[:, 1] = x[:, 2] * n[:, 0] - x[:, 0] * n[:, 2]
    J[:, 2] = x[:, 0] * n[:, 1] - x[:, 1] * n[:, 0]
    J[:, 3:6] = n
    if with_scale:
        J[:, 6] = (n[:, 0] * x[:, 0] + n[:, 1] * x[:, 1]) + n[:, 2] * x[:, 2]
    return {"J": J, "r": r, "d": d, "used": used, "far": far, "skipped": ~ok}


def terms(q):
    """[n_used, 37]: the terms of the 37 sums of ``rows``' result, in the order of ``out``."""
    J, r, d = q["J"], q["r"], q["d"]
    cols = [J[:, j] * J[:, k] for j, k in TRIU] + [J[:, j] * r for j in range(7)] + [r * r, d * d]
    return np.stack(cols, 1) if J.shape[0] else np.zeros((0, 37))


def accumulate(vs, faces, pts, matrix, closest, face, dist, max_dist=math.inf, with_scale=False, with_abs=False):
    """``out`` float64 [40] of sg_align_accumulate with exact sums (``math.fsum``, rounded once); ``with_abs``: also the 37
    sums of the terms' absolute values, what a bound on another summation order is made of."""
    q = rows(vs, faces, pts, matrix, closest, face, dist, max_dist, with_scale)
    T = terms(q)
    out = np.zeros(N_SUMS)
    out[:37] = [math.fsum(T[:, k]) for k in range(37)]
    out[37], out[38], out[39] = q["used"].sum(), q["far"].sum(), q["skipped"].sum()
    if with_abs:
        return out, np.array([math.fsum(np.abs(T[:, k])) for k in range(37)])
    return out


def cayley(omega):
    """R = ((1 - a) I + 2 k k^T + 2 [k]_x) / (1 + a) with k = omega / 2, a = k.k: a rotation, without trigonometry."""
    k = np.asarray(omega, np.float64) / 2.0
    a = float(k @ k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return ((1.0 - a) * np.eye(3) + 2.0 * np.outer(k, k) + 2.0 * K) / (1.0 + a)


def host_step(out, M, t, with_scale, diag):
    """(M', t', step) of one Gauss-Newton step from the 40 sums, or None when the system is degenerate."""
    k = 7 if with_scale else 6
    if int(out[37]) < k:
        return None
    A = np.zeros((7, 7))
    for q, (i, j) in enumerate(TRIU):
        A[i, j] = A[j, i] = out[q]
    A, g = A[:k, :k], np.asarray(out[28:28 + k], np.float64)
    if not np.isfinite(A).all() or not np.isfinite(g).all():
        return None
    try:
        L = np.linalg.cholesky(A)
    except np.linalg.LinAlgError:
        return None
    delta = np.linalg.solve(L.T, np.linalg.solve(L, -g))
    omega, tau = delta[:3], delta[3:6]
    sigma = float(delta[6]) if with_scale else 0.0
    R, s_d = cayley(omega), 1.0 + sigma
    step = max(float(np.abs(omega).max()), abs(sigma), float(np.abs(tau).max()) / diag)
    return s_d * (R @ M), s_d * (R @ t) + tau, step


def box_diagonal(vs):
    v = np.asarray(vs, np.float64).reshape(-1, 3)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


def centroid_init(src_pts, dst_pts, with_scale):
    """The ``init="centroid"`` matrix: M = s I, t = c_T - s c_S, s = rho_T / rho_S (the RMS radii) or 1."""
    S, T = (np.asarray(x, np.float64).reshape(-1, 3) for x in (src_pts, dst_pts))
    cS, cT = S.mean(0), T.mean(0)
    s = 1.0
    if with_scale:
        s = math.sqrt(((T - cT) ** 2).sum(1).mean()) / math.sqrt(((S - cS) ** 2).sum(1).mean())
    return matrix_of(s * np.eye(3), cT - s * cS)


def oracle_query(surface_oracle):
    """A query function for ``align_loop`` from a ``mesh_distance_oracle.SurfaceOracle``: float64 inside, the device's
    types outside (dist float32, face, closest float32)."""
    def query(x32):
        x = np.asarray(x32, np.float64)
        fin = np.isfinite(x).all(1)
        q = surface_oracle.query(np.where(fin[:, None], x, 0.0))
        dist = np.where(fin, q["dist"], np.inf).astype(np.float32)
        face = np.where(fin, q["face"], NO_FACE)
        closest = np.where(fin[:, None], q["closest"], np.nan).astype(np.float32)
        return dist, face, closest
    return query


def align_loop(pts, vs, faces, query, with_scale=False, init=None, max_dist=None, max_iter=50, tol=1e-6):
    """The whole loop of ``semigcn_amd.align.align`` on given points: transform, ``query(x float32 [N,3]) -> (dist, face,
    closest)``, accumulate, host step.  Returns matrix, iterations, converged, reason, rms and history."""
    M, t = pose_of(np.eye(4) if init is None else init)
    diag = box_diagonal(vs)
    md = math.inf if max_dist is None else float(max_dist)
    history, converged, reason, rms = [], False, "max_iter", float("nan")
    for _ in range(max_iter):
        mat = matrix_of(M, t)
        dist, face, closest = query(transform(mat, pts))
        out = accumulate(vs, faces, pts, mat, closest, face, dist, md, with_scale)
        n_used = int(out[37])
        rms = math.sqrt(out[36] / n_used) if n_used else float("nan")
        rec = {"rms": rms, "n_used": n_used, "n_far": int(out[38]), "n_skipped": int(out[39]), "step": float("nan")}
        history.append(rec)
        res = host_step(out, M, t, with_scale, diag)
        if res is None:
            reason = "degenerate"
            break
        M, t, rec["step"] = res
        if rec["step"] <= tol:
            converged, reason = True, "converged"
            break
    return {"matrix": matrix_of(M, t), "iterations": len(history), "converged": converged, "reason": reason, "rms": rms,
            "history": history}
