"""numpy restatement of semigcn_amd/simplify.py (its module docstring is the specification): serial and dictionary-based like
tests/collapse_oracle.py, whose helpers it uses -- no sorted keys, no twin table, no fan walk through half-edges, no radix
sort for the cut, no atomics; nothing here is shared with the kernels.

float64 arithmetic is done on Python floats one operation at a time, in the order the docstring writes out; the midpoint on
numpy float32 scalars."""
from __future__ import annotations

import math

import numpy as np

from remesh_oracle import MASK, _dot, bits, check_input, edge_table, hash32, valences

F32_MAX = float(np.finfo(np.float32).max)


# ---- quadrics -------------------------------------------------------------------------------------------------------------
def face_quadric(vs, tri):
    """The ten entries (xx, xy, xz, xw, yy, yz, yw, zz, zw, ww) of K = p p^T / (n . n), or None when n . n == 0."""
    a, b, c = ([float(vs[int(v)][i]) for i in range(3)] for v in tri)
    u = [b[i] - a[i] for i in range(3)]
    v = [c[i] - a[i] for i in range(3)]
    n = (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])
    nn = n[0] * n[0] + n[1] * n[1] + n[2] * n[2]
    if nn == 0.0:
        return None
    d = -(n[0] * a[0] + n[1] * a[1] + n[2] * a[2])
    p = (n[0], n[1], n[2], d)
    with np.errstate(all="ignore"):
        return [float(np.float64(p[i] * p[j]) / np.float64(nn)) for i in range(4) for j in range(i, 4)]


def vertex_quadrics(vs, faces):
    """float64 [V, 10]: the sum of the K of the faces at v, in ascending face index, from 0."""
    Q = [[0.0] * 10 for _ in range(len(vs))]
    for tri in faces:                                        # ascending f: every Q[v] receives its faces in that order
        K = face_quadric(vs, tri)
        if K is None:
            continue
        for v in tri:
            row = Q[int(v)]
            for i in range(10):
                row[i] = row[i] + K[i]
    return np.array(Q, np.float64).reshape(-1, 10)


def quadric_form(q, x, y, z):
    """v4^T Q v4 for v4 = (x, y, z, 1), in the written order."""
    s0 = q[0] * x + q[1] * y + q[2] * z + q[3]
    s1 = q[1] * x + q[4] * y + q[5] * z + q[6]
    s2 = q[2] * x + q[5] * y + q[7] * z + q[8]
    s3 = q[3] * x + q[6] * y + q[8] * z + q[9]
    return x * s0 + y * s1 + z * s2 + s3


def midpoint(vs, a, b):
    lo, hi = min(a, b), max(a, b)
    return [np.float32(np.float32(np.float32(vs[lo][i]) + np.float32(vs[hi][i])) * np.float32(0.5)) for i in range(3)]


def _normal_at(p, vs, x, y):
    """n(p, x, y) = (x - p) x (y - p) in float64, ``p`` a point."""
    u = [float(vs[x][i]) - float(p[i]) for i in range(3)]
    v = [float(vs[y][i]) - float(p[i]) for i in range(3)]
    return (u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0])


# ---- one round --------------------------------------------------------------------------------------------------------------
def _faces_at(faces):
    at = {}
    for f, tri in enumerate(faces):
        for v in tri:
            at.setdefault(int(v), []).append(f)
    return at


def _rotated(faces, at, v):
    """The faces at ``v`` rotated to read (v, x, y)."""
    out = []
    for f in at[v]:
        t = [int(u) for u in faces[f]]
        i = t.index(v)
        out.append((t[(i + 1) % 3], t[(i + 2) % 3]))
    return out


def _one_fan(rot):
    """Do the faces (v, x, y) hang together through their edges at v: is the graph of the (x, y) connected?"""
    adj = {}
    for x, y in rot:
        adj.setdefault(x, set()).add(y)
        adj.setdefault(y, set()).add(x)
    start = next(iter(adj))
    seen, todo = {start}, [start]
    while todo:
        for w in adj[todo.pop()]:
            if w not in seen:
                seen.add(w)
                todo.append(w)
    return len(seen) == len(adj)


def candidates(vs, faces, Q, guard=True):
    """({edge: (key, k, r, moves, new position, footprint, float64 cost)} of the legal candidates, the number of refused edges)"""
    table, rank = edge_table(faces)
    val, border = valences(faces)
    at = _faces_at(faces)
    floor = lambda v: 2 if v in border else 3
    ring = {}
    for a, b in table:
        ring.setdefault(a, set()).add(b)
        ring.setdefault(b, set()).add(a)
    legal, refused = {}, 0
    for e, hs in table.items():
        a, b = e
        if len(hs) != 2 or (a in border and b in border):
            continue
        k = a if a in border else (b if b in border else min(a, b))
        r = b if k == a else a
        moves = k not in border
        h0, h1 = hs
        c = int(faces[h0 // 3][(h0 % 3 + 2) % 3])
        d = int(faces[h1 // 3][(h1 % 3 + 2) % 3])
        rot_r, rot_k = _rotated(faces, at, r), _rotated(faces, at, k)
        ok = c != d and _one_fan(rot_r) and _one_fan(rot_k)
        ok = ok and len([w for w in ring[r] if w != k and w in ring[k]]) == 2
        ok = ok and val[c] - 1 >= floor(c) and val[d] - 1 >= floor(d) and val[k] + val[r] - 4 >= floor(k)
        pos = midpoint(vs, a, b) if moves else [np.float32(vs[k][i]) for i in range(3)]
        if ok and guard:
            for v, rot, other in ((r, rot_r, k), (k, rot_k, r)):
                if v == k and not moves:
                    continue
                for x, y in rot:
                    if other in (x, y):
                        continue
                    if not _dot(_normal_at(vs[v], vs, x, y), _normal_at(pos, vs, x, y)) > 0.0:
                        ok = False
        cost = None
        if ok:
            q = [float(Q[k][i]) + float(Q[r][i]) for i in range(10)]
            err = quadric_form(q, float(pos[0]), float(pos[1]), float(pos[2]))
            val_new = val[k] + val[r] - 4
            pen = float(abs(val_new - 6) + 1)
            if val_new == 3:
                pen = pen * 100000.0
            cost = err * pen
            ok = math.isfinite(cost)
        if not ok:
            refused += 1
            continue
        cost = cost if cost > 0.0 else 0.0
        c32 = np.float32(F32_MAX) if cost > F32_MAX else np.float32(cost)
        key = ((MASK - bits(c32)) << 32) | hash32(rank[e])
        legal[e] = (key, k, r, moves, pos, frozenset({k, r} | ring[k] | ring[r]), cost)
    return legal, refused


def simplify_round(vs, faces, Q, need, quadrics="own", guard=True):
    """One round: (vs, faces, Q, new-to-old, old-to-new, (candidates, admitted, winners), refused)"""
    legal, refused = candidates(vs, faces, Q, guard)
    m = min(need, len(legal))
    admitted = sorted(legal, key=lambda e: legal[e][0], reverse=True)[:m]
    at = {}
    for e in admitted:
        for v in legal[e][5]:
            at.setdefault(v, []).append(e)
    winners = [e for e in sorted(admitted) if all(legal[o][0] <= legal[e][0] for v in legal[e][5] for o in at[v])]
    V = len(vs)
    vs, Q = np.array(vs, np.float32), np.array(Q, np.float64)
    into = {}
    for e in winners:
        _, k, r, moves, pos, _, _ = legal[e]
        into[r] = k
        if moves:
            vs[k] = pos
        if quadrics == "sum":
            Q[k] = Q[k] + Q[r]
    assert not set(into) & set(into.values())
    out = []
    for tri in faces:
        t = [int(v) for v in tri]
        hit = [v for v in t if v in into]
        assert len(hit) <= 1
        if hit and into[hit[0]] in t:
            continue
        out.append([into.get(v, v) for v in t])
    keep = [v for v in range(V) if v not in into]
    new = {v: i for i, v in enumerate(keep)}
    old_to_new = np.array([new[into.get(v, v)] for v in range(V)], np.int64)
    out = np.array([[new[v] for v in t] for t in out], np.int64).reshape(-1, 3)
    return vs[keep], out, Q[keep], np.array(keep, np.int64), old_to_new, (len(legal), m, len(winners)), refused


def simplify(vs, faces, target_v, quadrics="own", max_rounds=256, guard=True):
    """(vs, faces, vertex_ids, coarse_of, counts [(candidates, admitted, winners)], reached, refused)"""
    vs, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    check_input(vs, faces)
    Q = vertex_quadrics(vs, faces)
    ids = np.arange(vs.shape[0], dtype=np.int64)
    merged = np.arange(vs.shape[0], dtype=np.int64)
    counts, refused = [], 0
    while vs.shape[0] > target_v and faces.shape[0] > 0:
        new_vs, new_faces, new_Q, keep, old_to_new, c, refused = simplify_round(vs, faces, Q, vs.shape[0] - target_v, quadrics,
                                                                               guard)
        if c[2] == 0 or len(counts) >= max_rounds:
            break
        vs, faces, Q = new_vs, new_faces, new_Q
        ids, merged = ids[keep], old_to_new[merged]
        counts.append(c)
    return vs, faces, ids, merged, counts, vs.shape[0] == target_v, refused


# ---- what the tests measure -------------------------------------------------------------------------------------------------
def unit_quadrics(vs, faces):
    """float64 [V, 4, 4]: the sum over the faces at v of [n | d]^T [n | d], n the unit normal and d = -n . centroid -- what
    ``meshprep._vertex_quadrics`` and tests/test_gpu_parity.py::_cluster_quadric_error use, in numpy."""
    p = np.asarray(vs, np.float64)
    a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
    n = np.cross(b - a, c - a)
    n = n / np.maximum(np.linalg.norm(n, axis=1, keepdims=True), 1e-30)
    d = -(n * ((a + b + c) / 3.0)).sum(1, keepdims=True)
    abcd = np.concatenate([n, d], 1)
    q = abcd[:, :, None] * abcd[:, None, :]
    Q = np.zeros((p.shape[0], 4, 4))
    for k in range(3):
        np.add.at(Q, faces[:, k], q)
    return Q


def cluster_quadric_error(vs, faces, coarse_of, coarse_pos):
    """sum over the coarse vertices of p^T (sum of the members' vertex quadrics) p."""
    Q = unit_quadrics(vs, faces)
    Qc = np.zeros((coarse_pos.shape[0], 4, 4))
    np.add.at(Qc, coarse_of, Q)
    p4 = np.concatenate([np.asarray(coarse_pos, np.float64), np.ones((coarse_pos.shape[0], 1))], 1)
    return float(np.einsum("ci,cij,cj->c", p4, Qc, p4).sum())


def face_normals(vs, faces):
    p = np.asarray(vs, np.float64)
    return np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
