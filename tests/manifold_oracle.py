"""Plain numpy restatement of semigcn_amd.manifold: dictionaries instead of sorts, the serial union-find of
components_oracle instead of the lock-free one, loops instead of scans -- weld, clean, the corner union, the double cover
and the outward step of the module docstring, in that order.  Also the meshes and the manglings the tests share."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from components_oracle import OCT, OCT_VS, TET, _find, _union, fan as _fan_faces, two_tetrahedra_sharing_a_vertex as _two_tets

COUNTS = ("n_welded", "n_degenerate", "n_duplicate_faces", "n_nonmanifold_edges", "n_split_vertices", "n_flipped",
          "n_nonorientable", "n_components", "n_closed")


def vertex_keys(vs):
    """uint32 [V, 3]: the coordinates' bits with -0.0 replaced by +0.0."""
    bits = np.ascontiguousarray(np.asarray(vs, np.float32).reshape(-1, 3)).view(np.uint32).copy()
    bits[bits == 0x80000000] = 0
    return bits


def weld_map(vs):
    first, out = {}, []
    for i, k in enumerate(map(tuple, vertex_keys(vs).tolist())):
        out.append(first.setdefault(k, i))
    return np.asarray(out, np.int64).reshape(-1)


def _edges(faces, live):
    """undirected edge -> [(face, corner index of the half-edge's start, runs from lo to hi)] over the live faces."""
    table = {}
    for f, t in enumerate(faces):
        if live[f]:
            for i in range(3):
                a, b = t[i], t[(i + 1) % 3]
                table.setdefault((min(a, b), max(a, b)), []).append((f, i, a < b))
    return table


def det3(a, b, c):
    """det[a, b, c] in float64, plain multiplies and adds in the order of the module docstring."""
    ax, ay, az = (np.float64(x) for x in a)
    bx, by, bz = (np.float64(x) for x in b)
    cx, cy, cz = (np.float64(x) for x in c)
    return ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)


def run(vs, faces, weld=False, dedup=False, cut=False, orient=False, outward=False, drop=False):
    """The steps that are switched on, on (vs float32 [V, 3], faces int [F, 3]).  Returns a namespace with ``vs``,
    ``faces``, ``vertex_map``, ``vertex_ids``, ``face_ids``, ``flipped``, ``nonorientable``, the counts, and per component
    (keyed by its smallest face, after step 4) ``vol6`` and ``vol_abs`` = sum |term| for the components step 5 looks at."""
    assert drop or not (weld or dedup or cut)
    assert orient or not outward
    vs = np.ascontiguousarray(np.asarray(vs, np.float32).reshape(-1, 3))
    f_in = np.asarray(faces, np.int64).reshape(-1, 3)
    V, F = vs.shape[0], f_in.shape[0]
    if F and (f_in.min() < 0 or f_in.max() >= V):
        raise ValueError("vertex index out of range")
    c = dict.fromkeys(COUNTS, 0)
    identity = np.arange(V, dtype=np.int64)
    if F == 0:
        return SimpleNamespace(vs=vs[:0] if drop else vs, faces=f_in, vertex_map=identity, vertex_ids=identity[:0] if drop else identity,
                               face_ids=np.zeros(0, np.int64), flipped=np.zeros(0, bool), nonorientable=np.zeros(0, bool),
                               vol6={}, vol_abs={}, **c)
    # 1. weld
    vmap = weld_map(vs) if weld else identity
    c["n_welded"] = int((vmap != identity).sum())
    tri = vmap[f_in].tolist()
    # 2. clean
    degen = [t[0] == t[1] or t[1] == t[2] or t[2] == t[0] for t in tri]
    c["n_degenerate"] = sum(degen)
    seen, keep = set(), []
    for f, t in enumerate(tri):
        k = True
        if degen[f]:
            k = not drop
        elif dedup:
            s = tuple(sorted(t))
            if s in seen:
                k = False
                c["n_duplicate_faces"] += 1
            seen.add(s)
        keep.append(k)
    face_ids = [f for f in range(F) if keep[f]]
    tri = [tri[f] for f in face_ids]
    live = [not degen[f] for f in face_ids]
    Fn = len(tri)
    # 3. the corner union and the new vertices
    if drop:
        parent = list(range(3 * Fn))
        if cut:
            for (lo, hi), hs in _edges(tri, live).items():
                if len(hs) == 2:
                    (f, _, _), (g, _, _) = hs
                    _union(parent, 3 * f + tri[f].index(lo), 3 * g + tri[g].index(lo))
                    _union(parent, 3 * f + tri[f].index(hi), 3 * g + tri[g].index(hi))
                elif len(hs) > 2:
                    c["n_nonmanifold_edges"] += 1
        else:
            first = {}
            for k in range(3 * Fn):
                _union(parent, first.setdefault(tri[k // 3][k % 3], k), k)
        roots = [_find(parent, k) for k in range(3 * Fn)]
        classes = sorted({(tri[r // 3][r % 3], r) for r in roots})           # ascending (input vertex, smallest corner)
        number = {r: n for n, (_, r) in enumerate(classes)}
        vertex_ids = np.asarray([v for v, _ in classes], np.int64).reshape(-1)
        tri = [[number[roots[3 * f + k]] for k in range(3)] for f in range(Fn)]
        c["n_split_vertices"] = len(classes) - len({v for v, _ in classes})
    else:
        vertex_ids = identity
    # 4. orient on the double cover
    flipped, nonor = [False] * Fn, [False] * Fn
    vol6, vol_abs = {}, {}
    if orient:
        table = _edges(tri, live)
        cover = list(range(2 * Fn))
        for hs in table.values():
            if len(hs) == 2:
                (f, _, up_f), (g, _, up_g) = hs
                s = 0 if up_f != up_g else 1
                _union(cover, 2 * f, 2 * g + s)
                _union(cover, 2 * f + 1, 2 * g + 1 - s)
        comp = [-1] * Fn
        for f in range(Fn):
            if live[f]:
                r0, r1 = _find(cover, 2 * f), _find(cover, 2 * f + 1)
                nonor[f], flipped[f], comp[f] = r0 == r1, r1 < r0, min(r0, r1) >> 1
        is_open = set()
        for hs in table.values():
            if len(hs) != 2:
                is_open.update(comp[f] for f, _, _ in hs)
        reps = sorted({k for k in comp if k >= 0})
        c["n_components"] = len(reps)
        c["n_closed"] = sum(k not in is_open for k in reps)
        c["n_nonorientable"] = sum(nonor[k] for k in reps)
        # 5. outward
        if outward:
            for f in range(Fn):
                k = comp[f]
                if k < 0 or nonor[f] or k in is_open:
                    continue
                a, b, d = tri[f] if not flipped[f] else (tri[f][0], tri[f][2], tri[f][1])
                t = det3(vs[vertex_ids[a]], vs[vertex_ids[b]], vs[vertex_ids[d]])
                vol6[k] = vol6.get(k, np.float64(0)) + t
                vol_abs[k] = vol_abs.get(k, np.float64(0)) + abs(t)
            for f in range(Fn):
                if comp[f] in vol6 and vol6[comp[f]] < 0:
                    flipped[f] = not flipped[f]
    c["n_flipped"] = sum(flipped)
    out = [[t[0], t[2], t[1]] if fl else list(t) for t, fl in zip(tri, flipped)]
    return SimpleNamespace(vs=vs[vertex_ids] if drop else vs, faces=np.asarray(out, np.int64).reshape(-1, 3), vertex_map=vmap,
                           vertex_ids=vertex_ids, face_ids=np.asarray(face_ids, np.int64).reshape(-1),
                           flipped=np.asarray(flipped, bool).reshape(-1), nonorientable=np.asarray(nonor, bool).reshape(-1),
                           vol6=vol6, vol_abs=vol_abs, **c)


def weld_vertices(vs, faces):
    return run(vs, faces, weld=True, dedup=True, drop=True)


def split_nonmanifold(vs, faces):
    return run(vs, faces, cut=True, drop=True)


def orient_faces(vs, faces, outward=True):
    return run(vs, faces, orient=True, outward=outward)


def make_manifold(vs, faces, weld=True, outward=True):
    return run(vs, faces, weld=weld, dedup=True, cut=True, orient=True, outward=outward, drop=True)


def volume_is_decided(res):
    """The premise of every fixture that tests step 5: |vol6| > 1e-6 sum |term| for every component it looks at."""
    return all(abs(res.vol6[k]) > 1e-6 * res.vol_abs[k] for k in res.vol6)


# ---- invariants of the cut ------------------------------------------------------------------------------------------------
def max_faces_per_edge(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if f.shape[0] == 0:
        return 0
    return max(len(h) for h in _edges(f.tolist(), [True] * f.shape[0]).values())


def every_vertex_is_one_fan(faces):
    """The faces at every vertex, linked where two of them share an edge at that vertex, are connected."""
    tri = np.asarray(faces, np.int64).reshape(-1, 3).tolist()
    parent = list(range(3 * len(tri)))
    for (lo, hi), hs in _edges(tri, [True] * len(tri)).items():
        for (f, _, _), (g, _, _) in zip(hs, hs[1:]):
            _union(parent, 3 * f + tri[f].index(lo), 3 * g + tri[g].index(lo))
            _union(parent, 3 * f + tri[f].index(hi), 3 * g + tri[g].index(hi))
    root_of = {}
    for k in range(3 * len(tri)):
        if root_of.setdefault(tri[k // 3][k % 3], _find(parent, k)) != _find(parent, k):
            return False
    return True


# ---- meshes --------------------------------------------------------------------------------------------------------------
TET_VS = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)        # TET is outward on these


def two_tetrahedra_sharing_a_vertex():
    """(vs [7, 3], faces [8, 3]): vertex 3 is the apex of both."""
    _, f = _two_tets()
    vs = np.concatenate([TET_VS, TET_VS[3] + np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1]], np.float32)])
    return vs, f


def two_tetrahedra_sharing_an_edge():
    """(vs [6, 3], faces [8, 3]): both hold the edge (0, 1); four faces meet on it."""
    vs = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0, -1, 0], [0, 0, -1]], np.float32)
    return vs, np.concatenate([TET, np.array([0, 1, 4, 5])[TET]])


def fan(n):
    """(vs [n + 2, 3], faces [n, 3]): components_oracle.fan with its wings spread round the edge."""
    V, f = _fan_faces(n)
    ang = 2 * np.pi * np.arange(n) / n
    vs = np.concatenate([[[0, 0, 0], [0, 0, 1]], np.stack([np.cos(ang), np.sin(ang), np.full(n, 0.5)], 1)]).astype(np.float32)
    return vs, f


def octahedron_with_fin():
    """(vs [7, 3], faces [9, 3]): a closed octahedron and a ninth face on its edge (0, 2)."""
    return np.concatenate([OCT_VS, [[2, 2, 0]]]).astype(np.float32), np.concatenate([OCT, [[0, 2, 6]]])


def moebius(n=16):
    """(vs [2 n, 3], faces [2 n, 3]): a strip of n quads closed with a half twist."""
    t = 2 * np.pi * np.arange(n) / n
    mid = np.stack([np.cos(t), np.sin(t), np.zeros(n)], 1)
    off = 0.3 * np.stack([np.cos(t / 2) * np.cos(t), np.cos(t / 2) * np.sin(t), np.sin(t / 2)], 1)
    vs = np.stack([mid - off, mid + off], 1).reshape(-1, 3).astype(np.float32)      # 2 i: lower, 2 i + 1: upper
    faces = []
    for i in range(n):
        a, b = 2 * i, 2 * i + 1
        c, d = (2 * (i + 1), 2 * (i + 1) + 1) if i + 1 < n else (1, 0)               # the twist: lower meets upper
        faces += [[a, c, b], [b, c, d]]
    return vs, np.asarray(faces, np.int64)


def torus(nu, nv, R=3.0, r=1.0):
    """(vs [nu nv, 3], faces [2 nu nv, 3]): a clean torus, vertex u * nv + v, faces outward."""
    u, v = np.meshgrid(np.arange(nu), np.arange(nv), indexing="ij")
    th, ph = 2 * np.pi * u / nu, 2 * np.pi * v / nv
    vs = np.stack([(R + r * np.cos(ph)) * np.cos(th), (R + r * np.cos(ph)) * np.sin(th), r * np.sin(ph)], -1).reshape(-1, 3)
    i00, i10 = u * nv + v, ((u + 1) % nu) * nv + v
    i01, i11 = u * nv + (v + 1) % nv, ((u + 1) % nu) * nv + (v + 1) % nv
    f = np.stack([np.stack([i00, i10, i11], -1), np.stack([i00, i11, i01], -1)], 2).reshape(-1, 3)
    return vs.astype(np.float32), f.astype(np.int64)


def cube(inverted=False):
    vs = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    q = [[0, 1, 3, 2], [4, 6, 7, 5], [0, 4, 5, 1], [2, 3, 7, 6], [0, 2, 6, 4], [1, 5, 7, 3]]      # outward quads
    f = np.asarray([t for a, b, c, d in q for t in ([a, b, c], [a, c, d])], np.int64)
    return vs, f[:, [0, 2, 1]] if inverted else f


def patch(n=4, inverted=False):
    """An open n x n grid in the plane z = 0."""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    vs = np.stack([i, j, np.zeros_like(i)], -1).reshape(-1, 3).astype(np.float32)
    a = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([a, a + n, a + n + 1], 1), np.stack([a, a + n + 1, a + 1], 1)]).astype(np.int64)
    return vs, f[:, [0, 2, 1]] if inverted else f


def strip(n_quads):
    """components_oracle.strip with positions: (vs [2 n + 2, 3], faces [2 n, 3])."""
    i = np.arange(n_quads + 1)
    vs = np.stack([np.repeat(i, 2), np.tile([0, 1], n_quads + 1), np.zeros(2 * n_quads + 2)], 1).astype(np.float32)
    k = np.arange(n_quads, dtype=np.int64)
    f = np.stack([np.stack([2 * k, 2 * k + 2, 2 * k + 1], 1), np.stack([2 * k + 1, 2 * k + 2, 2 * k + 3], 1)], 1)
    return vs, f.reshape(-1, 3)


# ---- manglings -----------------------------------------------------------------------------------------------------------
def soup(vs, faces):
    """Every face with three vertices of its own."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return np.ascontiguousarray(np.asarray(vs, np.float32)[f.reshape(-1)]), np.arange(3 * f.shape[0], dtype=np.int64).reshape(-1, 3)


def partial_soup(vs, faces, n):
    """The first ``n`` faces with three vertices of their own, appended after the given ones; the other faces as they are."""
    f = np.array(faces, np.int64).reshape(-1, 3)
    own = np.asarray(vs, np.float32)[f[:n].reshape(-1)]
    f[:n] = vs.shape[0] + np.arange(3 * n).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([np.asarray(vs, np.float32), own])), f


def permuted(vs, faces, seed):
    """One seeded permutation of the vertices and of the faces."""
    rng = np.random.default_rng(seed)
    pv, pf = rng.permutation(vs.shape[0]), rng.permutation(faces.shape[0])
    new_id = np.empty_like(pv)
    new_id[pv] = np.arange(pv.shape[0])
    return np.ascontiguousarray(vs[pv]), np.ascontiguousarray(new_id[faces][pf])


def reversed_faces(faces, mask):
    f = np.array(faces, np.int64)
    f[mask] = f[mask][:, [0, 2, 1]]
    return f


def pinched(faces, pairs):
    """Every (a, b) of ``pairs`` gets the one index a: b is left unused and a becomes a bow-tie."""
    f = np.array(faces, np.int64)
    for a, b in pairs:
        f[f == b] = a
    return f


def join(*meshes):
    vs, faces, base = [], [], 0
    for v, f in meshes:
        vs.append(np.asarray(v, np.float32))
        faces.append(np.asarray(f, np.int64) + base)
        base += v.shape[0]
    return np.concatenate(vs), np.concatenate(faces)


# ---- the fixtures of tests/test_gpu_manifold.py (their premises are pinned in tests/test_manifold_oracle.py) --------------
def negative_zeros(vs, seed):
    """``vs`` with a seeded half of its +0.0 entries written as -0.0."""
    out = np.array(vs, np.float32)
    flat = out.reshape(-1)
    zeros = np.flatnonzero(flat.view(np.uint32) == 0)
    flat[np.random.default_rng(seed).permutation(zeros)[: max(1, zeros.shape[0] // 2)]] = np.float32(-0.0)
    return out


def soup_torus():
    return permuted(*soup(*torus(24, 16)), seed=11)


def half_reversed_torus():
    vs, f = torus(24, 16)
    return vs, reversed_faces(f, np.random.default_rng(12).random(f.shape[0]) < 0.5)


def zigzag_strip(order):
    """A 1 x 20 000 strip with every second face reversed; ``order``: 0 as built, 1 back to front, 2 a seeded permutation."""
    vs, f = strip(20000)
    f = reversed_faces(f, np.arange(f.shape[0]) % 2 == 1)
    if order == 1:
        f = f[::-1]
    elif order == 2:
        f = f[np.random.default_rng(13).permutation(f.shape[0])]
    return vs, np.ascontiguousarray(f)


def reversed_octahedra(n=5000):
    from components_oracle import octahedra
    vs, f = octahedra(n)
    return vs, reversed_faces(f, np.random.default_rng(14).random(f.shape[0]) < 0.3)


def moebius_and_cube():
    vs, f = cube()
    return join(moebius(), (vs + np.float32(5), f))


def tori_sharing_a_ring(nu=24, nv=16):
    """Two tori whose tubes touch along a circle -- the outer equator of the first is the inner equator of the second --
    with one set of indices for that ring: four faces on each of its nu edges."""
    a_vs, a_f = torus(nu, nv, 3.0, 1.0)
    b_vs, b_f = torus(nu, nv, 5.0, 1.0)
    b_f = b_f + a_vs.shape[0]
    for u in range(nu):
        b_f[b_f == a_vs.shape[0] + u * nv + nv // 2] = u * nv
    return np.concatenate([a_vs, b_vs]), np.concatenate([a_f, b_f])


def torus_pinches(nu, nv, k):
    """k pairs (a, b) of vertices of ``torus(nu, nv)`` half the torus apart."""
    return [((i * nu // (2 * k)) * nv, (i * nu // (2 * k) + nu // 2) * nv) for i in range(k)]


def cut_fixture():
    """A 96 x 96 torus with 8 pinches, a fan of 64 faces on one edge and two tori sharing a ring, under one permutation."""
    t_vs, t_f = torus(96, 96, 30.0, 10.0)
    t_f = pinched(t_f, torus_pinches(96, 96, 8))
    f_vs, f_f = fan(64)
    r_vs, r_f = tori_sharing_a_ring()
    return permuted(*join((t_vs, t_f), (f_vs + np.float32(60), f_f), (r_vs + np.float32(100), r_f)), seed=15)
