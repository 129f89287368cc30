"""Plain numpy / float64 restatement of semigcn_amd.holes: a serial walk along the boundary half-edges and the patch
construction of the module docstring, loop by loop, vertex by vertex, face by face -- no sort, no scan, no pointer
jumping, no offsets table.  Also the checks the tests share: closedness, Euler characteristic, edge lengths."""
from __future__ import annotations

import collections

import numpy as np


class Unorderable(ValueError):
    def __init__(self, n_repeated, n_bowtie, vertex):
        super().__init__(f"{n_repeated} repeated half-edges, {n_bowtie} bow-tie vertices, smallest vertex {vertex}")
        self.n_repeated, self.n_bowtie, self.vertex = n_repeated, n_bowtie, vertex


def half_edges(faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    return list(zip(f.reshape(-1).tolist(), f[:, [1, 2, 0]].reshape(-1).tolist()))


def boundary_loops(faces):
    """Loops as lists of vertex ids in canonical form: numbered by ascending smallest vertex, each starting at its smallest
    vertex, each running against the mesh's boundary half-edges."""
    count = collections.Counter(half_edges(faces))
    repeated = {e: c for e, c in count.items() if c > 1}
    out = collections.defaultdict(list)
    for (a, b) in count:
        if count[(a, b)] == 1 and (b, a) not in count:
            out[a].append(b)
    bow = sorted(a for a, bs in out.items() if len(bs) > 1)
    if repeated or bow:
        bad = sorted([a for (a, _b) in repeated] + bow)
        raise Unorderable(sum(c - 1 for c in repeated.values()), len(bow), bad[0])
    against = {bs[0]: a for a, bs in out.items()}      # the mesh has (a, b): after b comes a
    loops, seen = [], set()
    for start in sorted(against):
        if start in seen:
            continue
        loop, v = [], start
        while v not in seen:
            seen.add(v)
            loop.append(v)
            v = against[v]
        assert v == start
        loops.append(loop)
    return loops


def loops_csr(loops):
    ptr = np.concatenate([[0], np.cumsum([len(l) for l in loops])]).astype(np.int64)
    verts = np.asarray([v for l in loops for v in l], np.int64)
    return ptr, verts


def ring_count(n):
    return max(1, (113 * n + 355) // 710)


def ring_sizes(n):
    """[n_0 = n, n_1, ..., n_R = 1]"""
    R = ring_count(n)
    return [n] + [max(3, (2 * n * (R - r) + R) // (2 * R)) for r in range(1, R)] + [1]


def fill_loop(b):
    """b float64 [n, 3], the loop's positions in loop order -> (new positions [k, 3], faces over local ids: 0 .. n - 1 the
    loop, n .. the new vertices)."""
    b = np.asarray(b, np.float64)
    n = len(b)
    if n == 3:
        return np.zeros((0, 3)), np.array([[0, 1, 2]], np.int64)
    cnt = ring_sizes(n)
    R = len(cnt) - 1
    seg = np.linalg.norm(np.roll(b, -1, 0) - b, axis=1)
    cum = np.concatenate([[0.0], np.cumsum(seg)])
    perimeter = cum[-1]
    c = b.mean(0)

    def B(s):
        i = min(int(np.searchsorted(cum, s, side="right")) - 1, n - 1)
        t = (s - cum[i]) / seg[i] if seg[i] > 0 else 0.0
        return b[i] * (1 - t) + b[(i + 1) % n] * t

    ids, new, nxt = [list(range(n))], [], n
    for r in range(1, R + 1):
        row = []
        for j in range(cnt[r]):
            if r == R:
                new.append(c)
            else:
                p = B(j / cnt[r] * perimeter)
                new.append(p + (r / R) * (c - p))
            row.append(nxt)
            nxt += 1
        ids.append(row)
    faces = []
    for r in range(R):
        o, i = ids[r], ids[r + 1]
        m, k = len(o), len(i)
        if k == 1:
            faces += [(o[a], o[(a + 1) % m], i[0]) for a in range(m)]
            continue
        N = m + k
        for t in range(N):
            A, A1 = (t * m) // N, ((t + 1) * m) // N
            Bq = t - A
            faces.append((o[A % m], o[(A + 1) % m], i[Bq % k]) if A1 > A else (o[A % m], i[(Bq + 1) % k], i[Bq % k]))
    return np.asarray(new, np.float64).reshape(-1, 3), np.asarray(faces, np.int64)


def fill_holes(vs, faces, max_hole_edges=None):
    """The raw construction (no fairing): (vs float64 [V + Vn, 3], faces int64 [F + Fn, 3], inserted bool [V + Vn],
    filled bool [L], loops).  ``vs`` is read as the float32 values the device sees."""
    vs = np.asarray(vs, np.float32).astype(np.float64)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    loops = boundary_loops(faces)
    out_v, out_f, filled = [vs], [faces], []
    nxt = vs.shape[0]
    for loop in loops:
        n = len(loop)
        fill = max_hole_edges is None or n <= max_hole_edges
        filled.append(fill)
        if not fill:
            continue
        new, lf = fill_loop(vs[loop])
        lut = np.concatenate([np.asarray(loop, np.int64), nxt + np.arange(len(new), dtype=np.int64)])
        out_v.append(new)
        out_f.append(lut[lf])
        nxt += len(new)
    V2 = nxt
    inserted = np.zeros(V2, bool)
    inserted[vs.shape[0]:] = True
    return np.concatenate(out_v), np.concatenate(out_f), inserted, np.asarray(filled, bool), loops


# ---- checks ------------------------------------------------------------------------------------------------------------
def euler_characteristic(faces):
    """V - E + F over the vertices the faces use."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.sort(np.stack([f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)], 1), 1)
    n_e = np.unique(e[:, 0] * (int(f.max()) + 1) + e[:, 1]).shape[0]
    return int(np.unique(f).shape[0] - n_e + f.shape[0])


def half_edge_stats(faces):
    """(largest multiplicity of a directed half-edge, number of directed half-edges without their opposite)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    a, b = f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)
    W = int(f.max()) + 1
    key, cnt = np.unique(a * W + b, return_counts=True)
    opp = (key % W) * W + key // W
    return int(cnt.max()), int((~np.isin(opp, key)).sum())


def edge_lengths(vs, faces):
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.sort(np.stack([f.reshape(-1), f[:, [1, 2, 0]].reshape(-1)], 1), 1)
    e = np.unique(e, axis=0)
    vs = np.asarray(vs, np.float64)
    return np.linalg.norm(vs[e[:, 0]] - vs[e[:, 1]], axis=1)


def regular_polygon(n, h=1.0):
    """n-gon of edge length h in the plane z = 0, counter-clockwise."""
    rad = h / (2.0 * np.sin(np.pi / n))
    th = 2.0 * np.pi * np.arange(n) / n
    return np.stack([rad * np.cos(th), rad * np.sin(th), np.zeros(n)], 1)
