"""Plain numpy / float64 restatement of the thin-plate fairing of semigcn_amd.holes (``fair_thin_plate``): the graph, the
rows S, a DENSE M, A and b, the direct solve, the operator applied row by row in ascending neighbour order (the arithmetic
the device must equal bit for bit), and the solvability check: the device is compared with ``numpy.linalg.solve``.

The second half restates the same arithmetic vectorised, for meshes the row-by-row loops cannot reach: a padded ascending
neighbour table, one pass per neighbour slot (so every sum still runs in ascending neighbour order and every product and
sum rounds on its own), ``M^T M x`` over all vertices, and the conjugate-gradient rule of ``fair_thin_plate`` itself --
per-coordinate alpha, beta, stop test and freeze -- with numpy's summation order in the dot products.  That CG serves CPU
premises only; it is never compared bit for bit with the device."""
from __future__ import annotations

import numpy as np


def neighbours(faces, V):
    """N(i) as ascending int64 arrays, one per vertex: the distinct neighbours over the undirected edges of ``faces``."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    key = np.unique(np.concatenate([a * np.int64(V) + b, b * np.int64(V) + a])) if f.size else np.zeros(0, np.int64)
    src, dst = key // max(V, 1), key % max(V, 1)
    starts = np.searchsorted(src, np.arange(V + 1))
    return [dst[starts[i]:starts[i + 1]] for i in range(V)]


class System:
    """Everything the rule names, dense: ``N``, ``d``, ``free_idx``, ``S``, ``M`` [|S|, V], ``A`` [nf, nf], ``b`` [nf, 3]."""

    def __init__(self, vs, faces, free):
        self.x = np.asarray(vs, np.float32).astype(np.float64).reshape(-1, 3)      # the float32 values the device sees
        V = self.V = self.x.shape[0]
        self.free = np.asarray(free, bool).reshape(-1)
        assert self.free.shape[0] == V
        self.N = neighbours(faces, V)
        self.d = np.array([len(n) for n in self.N], np.int64)
        self.free_idx = np.flatnonzero(self.free)
        in_S = self.free.copy()
        for i in self.free_idx:
            in_S[self.N[i]] = True
        self.S = np.flatnonzero(in_S)
        M = np.zeros((len(self.S), V))
        for r, i in enumerate(self.S):
            M[r, i] = 1.0
            M[r, self.N[i]] = -1.0 / self.d[i]
        self.M = M
        Mf = M[:, self.free]
        self.A = Mf.T @ Mf
        fixed = self.x.copy()
        fixed[self.free] = 0.0
        self.b = -(Mf.T @ (M @ fixed))

    def energy(self, x):
        return float(((self.M @ np.asarray(x, np.float64)) ** 2).sum())


def spd_check(faces, V, free):
    """None when A is SPD; else ``(vertex, why)``: the smallest free vertex without edges (``"isolated"``) or, when there
    is none, the smallest vertex of a class of free vertices (under free-free edges) that no edge joins to a fixed vertex
    (``"floating"``)."""
    free = np.asarray(free, bool).reshape(-1)
    N = neighbours(faces, V)
    lonely = [i for i in np.flatnonzero(free) if len(N[i]) == 0]
    if lonely:
        return int(lonely[0]), "isolated"
    seen = np.zeros(V, bool)
    for start in np.flatnonzero(free):                # ascending: a class is met at its smallest vertex first
        if seen[start]:
            continue
        stack, anchored = [start], False
        seen[start] = True
        while stack:
            i = stack.pop()
            for j in N[i]:
                if not free[j]:
                    anchored = True
                elif not seen[j]:
                    seen[j] = True
                    stack.append(j)
        if not anchored:
            return int(start), "floating"
    return None


def solve_direct(vs, faces, free, system=None):
    """float64 [V, 3]: the minimiser of E over the free vertices, every other vertex at its float32 input position."""
    s = System(vs, faces, free) if system is None else system
    out = s.x.copy()
    if len(s.free_idx):
        out[s.free] = np.linalg.solve(s.A, s.b)
    return out


def apply(faces, V, free, p):
    """q = A p for p float64 [nf] over the free list, as the device computes it: ``y_i = p_i - (1/d_i) (sum of p_j over the
    free j in N(i), ascending)`` for i in S (``p_i = 0`` when i is fixed), then ``q_i = y_i - (sum of y_j (1/d_j) over j in
    N(i), ascending)`` for i free; ``1/d`` is the rounded reciprocal; every product and every sum rounds on its own."""
    free = np.asarray(free, bool).reshape(-1)
    N = neighbours(faces, V)
    fidx = np.cumsum(free) - 1
    in_S = free.copy()
    for i in np.flatnonzero(free):
        in_S[N[i]] = True
    p = np.asarray(p, np.float64).reshape(-1)
    one, zero = np.float64(1.0), np.float64(0.0)
    inv = {int(i): one / np.float64(len(N[i])) for i in np.flatnonzero(in_S)}
    y = {}
    for i in np.flatnonzero(in_S):
        s = zero
        for j in N[i]:
            if free[j]:
                s = s + p[fidx[j]]
        y[int(i)] = (p[fidx[i]] if free[i] else zero) - inv[int(i)] * s
    q = np.zeros(int(free.sum()))
    for i in np.flatnonzero(free):
        s = zero
        for j in N[i]:
            s = s + y[int(j)] * inv[int(j)]
        q[fidx[i]] = y[int(i)] - s
    return q


def jacobi_diagonal(faces, V, free):
    """diag(A)_i = 1 + sum over j in N(i), ascending, of (1/d_j) (1/d_j), for the free i."""
    free = np.asarray(free, bool).reshape(-1)
    N = neighbours(faces, V)
    out = []
    for i in np.flatnonzero(free):
        s = np.float64(1.0)
        for j in N[i]:
            w = np.float64(1.0) / np.float64(len(N[j]))
            s = s + w * w
        out.append(s)
    return np.asarray(out, np.float64)


def solve_bound(system, tol):
    """Per coordinate ``tol * ||A^-1||_2 * ||b||_2``: how far an iterate whose residual is ``tol ||b||`` can be from x*."""
    if not len(system.free_idx):
        return np.zeros(3)
    inv_norm = 1.0 / np.linalg.eigvalsh(system.A)[0]
    return tol * inv_norm * np.linalg.norm(system.b, axis=0)


# ---- the same arithmetic, vectorised -----------------------------------------------------------------------------------
class Table:
    """``nbr`` int64 [V, D]: N(i) ascending, padded with -1; ``d`` int64 [V]; ``inv`` float64 [V]: the rounded 1 / d (0 for
    a vertex without edges)."""

    def __init__(self, faces, V):
        f = np.asarray(faces, np.int64).reshape(-1, 3)
        a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
        key = np.unique(np.concatenate([a * np.int64(V) + b, b * np.int64(V) + a])) if f.size else np.zeros(0, np.int64)
        src, dst = key // max(V, 1), key % max(V, 1)
        self.V = V
        self.d = np.bincount(src, minlength=V).astype(np.int64)
        starts = np.concatenate([[0], np.cumsum(self.d)])
        self.nbr = np.full((V, int(self.d.max()) if V and key.size else 0), -1, np.int64)
        self.nbr[src, np.arange(len(key)) - starts[src]] = dst
        self.inv = np.zeros(V)
        self.inv[self.d > 0] = np.float64(1.0) / self.d[self.d > 0].astype(np.float64)


def _two_gathers(t, free, x, first):
    """float64 [nf, C]: ``y_i = x_i - (1/d_i) (sum of x_j over the j in N(i) with first[j], ascending)`` on every vertex,
    then ``q_i = y_i - (sum of y_j (1/d_j) over j in N(i), ascending)`` on the free ones.  Only the rows S of y reach q."""
    inv = t.inv[:, None]
    acc = np.zeros_like(x)
    for k in range(t.nbr.shape[1]):
        col = t.nbr[:, k]
        use = (col >= 0) & first[col]                      # col = -1 reads the last vertex; ``use`` is False there
        acc = np.where(use[:, None], acc + x[col], acc)
    y = x - inv * acc
    yw = y * inv
    rows = np.flatnonzero(free)
    acc = np.zeros((len(rows), x.shape[1]))
    for k in range(t.nbr.shape[1]):
        col = t.nbr[rows, k]
        acc = np.where((col >= 0)[:, None], acc + yw[col], acc)
    return y[rows] - acc


def apply_table(t, free, p):
    """``apply`` on a Table: q = A p for p float64 [nf] or [nf, C], bit for bit what ``apply`` gives column by column."""
    free = np.asarray(free, bool).reshape(-1)
    p = np.asarray(p, np.float64)
    x = np.zeros((t.V, 1 if p.ndim == 1 else p.shape[1]))
    x[free] = p.reshape(len(p), -1)
    return _two_gathers(t, free, x, free).reshape(p.shape)


def normal_rows(t, free, vs, zero_free):
    """``M^T M x`` on the free rows for x float64 [V, C] over ALL vertices; ``zero_free``: with the free ones taken as 0.
    ``b`` is minus the one, the first residual ``r0`` minus the other."""
    free = np.asarray(free, bool).reshape(-1)
    x = np.array(vs, np.float64).reshape(t.V, -1)
    if zero_free:
        x[free] = 0.0
        return _two_gathers(t, free, x, ~free)
    return _two_gathers(t, free, x, np.ones(t.V, bool))


def diagonal_table(t, free):
    """``jacobi_diagonal`` on a Table, bit for bit."""
    rows = np.flatnonzero(np.asarray(free, bool).reshape(-1))
    acc = np.ones(len(rows))
    for k in range(t.nbr.shape[1]):
        col = t.nbr[rows, k]
        w = t.inv[col]
        acc = np.where(col >= 0, acc + w * w, acc)
    return acc


def cg(t, free, vs, tol, max_iter=10000):
    """The solver of ``fair_thin_plate`` restated: Jacobi-preconditioned CG from the float32 positions, every coordinate
    with its own alpha, beta and stop test ``r.r <= tol^2 ref`` on the recursive residual, ``ref = b.b``, or ``r0.r0``
    for a coordinate whose ``b.b`` is 0; a coordinate that has met its test is frozen.  Returns ``(x float64 [nf, C],
    info)`` with the keys of the device's ``info``."""
    free = np.asarray(free, bool).reshape(-1)
    vs = np.asarray(vs, np.float32).astype(np.float64).reshape(t.V, -1)
    x = vs[free].copy()
    b = -normal_rows(t, free, vs, True)
    r = -normal_rows(t, free, vs, False)
    diag = diagonal_table(t, free)[:, None]
    z = r / diag
    p = z.copy()
    bb, rr, rz = (b * b).sum(0), (r * r).sum(0), (r * z).sum(0)
    ref = np.where(bb > 0.0, bb, rr)
    thr = (tol * tol) * ref
    frozen = rr <= thr
    it = 0
    while not frozen.all() and it < max_iter:
        q = apply_table(t, free, p)
        with np.errstate(all="ignore"):
            alpha = np.where(frozen, 0.0, rz / (p * q).sum(0))
        live = ~frozen
        x[:, live] += alpha[live] * p[:, live]
        r[:, live] -= alpha[live] * q[:, live]
        z[:, live] = r[:, live] / diag
        rz_new, rr_new = (r * z).sum(0), (r * r).sum(0)
        stop = frozen | (rr_new <= thr)
        with np.errstate(all="ignore"):
            beta = np.where(stop, 0.0, rz_new / rz)
        p[:, ~stop] = z[:, ~stop] + beta[~stop] * p[:, ~stop]
        rz, rr = np.where(frozen, rz, rz_new), np.where(frozen, rr, rr_new)
        frozen = stop
        it += 1
    with np.errstate(all="ignore"):
        relres = np.where(ref > 0.0, np.sqrt(rr / np.where(ref > 0.0, ref, 1.0)), 0.0)
    return x, {"iterations": it, "relative_residual": [float(v) for v in relres], "converged": bool(frozen.all()),
               "n_free": int(free.sum())}
