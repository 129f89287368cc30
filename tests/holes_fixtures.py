"""The meshes the hole-filling and smoothing tests share, in numpy, and two restatements the CPU tests use to pin what those
meshes are for.

  fans(sizes)      disjoint components, one boundary loop each, of exactly the given sizes in loop order: a lone triangle for
                   n = 3 (a loop that adds a face but no vertex and no ring table), otherwise a fan from a hub to a rim of n
                   vertices.  With ``perm`` the vertex ids are shuffled: the loops come in another order and their vertices
                   interleave in the sorted boundary array.
  bipyramid(n)     closed; two hubs of valence n over a rim of n vertices of valence 4.
  coincident()     fans([24, 12, 30]) with zero-length segments at the start, inside and at the end of loop 0, loop 1
                   collapsed to one point (perimeter 0) and loop 2 moved 1e4 away.
  table_form       the new faces, and (loop, ring, index) of every new vertex, found the way csrc/mesh_fill.hip finds them:
                   counts per loop, exclusive scans, a binary search over the L loop offsets and one over the R ring offsets.
                   ``ties="first"`` is that search gone wrong (the first of several equal offsets, not the last): what the
                   fixtures must be able to tell apart.  It restates the tables, not the construction: tests/holes_oracle.py
                   stays the one oracle.
  positions_other_order   the new positions by the construction of semigcn_amd/holes.py in float64, with every sum taken in
                   another order than tests/holes_oracle.py takes it: what the position bound must leave room for.
"""
from __future__ import annotations

import numpy as np

import holes_oracle as HO

#: a loop on both sides of every change of the ring count (9|10, 15|16, 21|22), triangles first, last, alone and in a run
#: between larger loops, two loops that every cap below 40 leaves open, and the square (one ring, one new vertex)
S13 = [3, 40, 3, 9, 10, 3, 40, 15, 16, 21, 22, 4, 3]
#: max_hole_edges -> (new vertices, new faces) of fans(S13), by tests/holes_oracle.py (they depend on the sizes alone)
S13_COUNTS = {None: (293, 749), 20: (34, 116), 9: (2, 17), 3: (0, 4), 2: (0, 0)}
#: n -> (new vertices, new faces) of fans([n]): one chunk of the arc-length scan and one power of two, less, exactly, more
SINGLE_COUNTS = {255: (5101, 10455), 256: (5121, 10496), 257: (5141, 10537), 511: (20441, 41391), 512: (20481, 41472),
                 513: (20778, 42067), 1024: (82945, 166912), 1025: (83026, 167075)}

COLUMNS = 40          # components sit on a grid of this many columns, 3 apart: they never touch


def fans(sizes, seed=0, perm=None, shift=0.0):
    """(vs float32 [V, 3], faces int64 [F, 3]).  Component c: rim vertices first (ids ascending along the rim), then the hub;
    the rim is a circle of radius 1 with a seeded wobble of 0.1 in the radius and 0.2 in height, the hub 0.8 above its
    centre.  ``perm``: the seed of one permutation of all vertex ids.  ``shift`` is added to every coordinate."""
    rng = np.random.default_rng(seed)
    vs, faces, base = [], [], 0
    for c, n in enumerate(sizes):
        assert n >= 3
        centre = np.array([3.0 * (c % COLUMNS), 3.0 * (c // COLUMNS), 0.0])
        ang = 2.0 * np.pi * (np.arange(n) + rng.uniform(-0.2, 0.2, n)) / n
        rad = 1.0 + rng.uniform(-0.1, 0.1, n)
        rim = centre + np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-0.2, 0.2, n)], 1)
        i = np.arange(n)
        if n == 3:
            vs.append(rim)
            faces.append(np.array([[base, base + 1, base + 2]], np.int64))
            base += 3
        else:
            vs += [rim, centre[None] + [[0.0, 0.0, 0.8]]]
            faces.append(np.stack([np.full(n, base + n), base + i, base + (i + 1) % n], 1).astype(np.int64))
            base += n + 1
    vs, faces = np.concatenate(vs) + shift, np.concatenate(faces)
    if perm is not None:
        new_id = np.random.default_rng(perm).permutation(base)
        moved = np.empty_like(vs)
        moved[new_id] = vs
        vs, faces = moved, new_id[faces]
    return np.ascontiguousarray(vs.astype(np.float32)), np.ascontiguousarray(faces.astype(np.int64))


def bipyramid(n, seed=0):
    """(vs float32 [n + 2, 3], faces int64 [2 n, 3]): rim vertices 0 .. n - 1 (wobbled as in ``fans``), hubs n (above) and
    n + 1 (below).  A hub's neighbour list is the whole rim; a rim vertex has its two rim neighbours and the two hubs."""
    rng = np.random.default_rng(seed)
    ang = 2.0 * np.pi * (np.arange(n) + rng.uniform(-0.2, 0.2, n)) / n
    rad = 1.0 + rng.uniform(-0.1, 0.1, n)
    rim = np.stack([rad * np.cos(ang), rad * np.sin(ang), rng.uniform(-0.2, 0.2, n)], 1)
    vs = np.concatenate([rim, [[0.1, -0.05, 1.0], [-0.05, 0.1, -1.2]]])
    i = np.arange(n)
    faces = np.concatenate([np.stack([np.full(n, n), i, (i + 1) % n], 1), np.stack([np.full(n, n + 1), (i + 1) % n, i], 1)])
    return np.ascontiguousarray(vs.astype(np.float32)), np.ascontiguousarray(faces.astype(np.int64))


def coincident():
    """(vs, faces, loops) of ``fans([24, 12, 30])`` with, in loop order: loop 0 -- vertex 1 on vertex 0 (the first segment has
    length 0), vertices 10 and 11 on vertex 9 (two zero segments in a row), the last vertex on vertex 0 (the closing segment
    has length 0); loop 1 -- every vertex on its vertex 0 (perimeter 0); loop 2 -- 1e4 further out in every coordinate."""
    vs, faces = fans([24, 12, 30])
    loops = HO.boundary_loops(faces)
    assert [len(l) for l in loops] == [24, 12, 30]
    a, b, c = loops
    vs[a[1]] = vs[a[0]]
    vs[a[10]] = vs[a[9]]
    vs[a[11]] = vs[a[9]]
    vs[a[-1]] = vs[a[0]]
    vs[b] = vs[b[0]]
    in_c = np.zeros(len(vs), bool)
    in_c[faces[(faces >= min(c)).all(1)].reshape(-1)] = True          # the rim and the hub of the last component
    vs[in_c] += np.float32(1e4)
    return vs, faces, loops


# ---- the kernel's tables ---------------------------------------------------------------------------------------------------
def _search(a, n, x, ties):
    """largest q in [0, n) with a[q] <= x; ``ties="first"``: the smallest q that holds the same value"""
    lo, hi = 0, n
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if a[mid] <= x:
            lo = mid
        else:
            hi = mid
    if ties == "first":
        while lo > 0 and a[lo - 1] == a[lo]:
            lo -= 1
    return lo


def _ring_size(n, R, r):
    return n if r <= 0 else 1 if r >= R else max(3, (2 * n * (R - r) + R) // (2 * R))


def _at(a, i):
    if not 0 <= i < len(a):                     # a read the device would make outside its table
        raise IndexError(i)
    return a[i]


def table_form(V, loops, cap, ties="last"):
    """(new faces int64 [Fn, 3], (loop, ring, index) int64 [Vn, 3]) over ``V`` original vertices and the canonical ``loops``."""
    assert ties in ("last", "first")
    L = len(loops)
    counts = np.zeros((3, L + 1), np.int64)
    ring_v, ring_f, filled = [], [], []
    for l, loop in enumerate(loops):
        n = len(loop)
        fill = n >= 3 and (cap is None or n <= cap)
        filled.append(fill)
        if fill and n == 3:
            counts[1, l] = 1
        elif fill:
            R = HO.ring_count(n)
            nv, nf, m = 0, 0, n
            ring_v.append(0)
            ring_f.append(0)
            for r in range(1, R + 1):
                k = _ring_size(n, R, r)
                nv, nf, m = nv + k, nf + (m if k == 1 else m + k), k
                ring_v.append(nv)
                ring_f.append(nf)
            counts[:, l] = nv, nf, R + 1
    base = np.concatenate([np.zeros((3, 1), np.int64), np.cumsum(counts, 1)[:, :-1]], 1)          # exclusive scans
    vbase, fbase, rbase = base
    Vn, Fn = int(vbase[L]), int(fbase[L])

    where = []
    for g in range(Vn):
        l = _search(vbase, L, g, ties)
        n = len(loops[l])
        R, t0 = HO.ring_count(n), int(rbase[l])
        local = g - int(vbase[l])
        q = _search([_at(ring_v, t0 + r) for r in range(R)], R, local, ties)
        where.append((l, q + 1, local - _at(ring_v, t0 + q)))

    faces = []
    for g in range(Fn):
        l = _search(fbase, L, g, ties)
        lv = loops[l]
        n = len(lv)
        if n == 3:
            faces.append((lv[0], lv[1], lv[2]))
            continue
        R, t0 = HO.ring_count(n), int(rbase[l])
        local = g - int(fbase[l])
        r = _search([_at(ring_f, t0 + q) for q in range(R)], R, local, ties)
        t = local - _at(ring_f, t0 + r)
        m, k = _ring_size(n, R, r), _ring_size(n, R, r + 1)
        first_new = V + int(vbase[l])
        inner0 = first_new + _at(ring_v, t0 + r)
        outer0 = 0 if r == 0 else first_new + _at(ring_v, t0 + r - 1)

        def outer(a):
            return _at(lv, a) if r == 0 else outer0 + a
        if k == 1:
            faces.append((outer(t), outer(0 if t + 1 == m else t + 1), inner0))
        else:
            N = m + k
            A, A1 = (t * m) // N, ((t + 1) * m) // N
            B = t - A
            faces.append((outer(A % m), outer((A + 1) % m), inner0 + B % k) if A1 > A
                         else (outer(A % m), inner0 + (B + 1) % k, inner0 + B % k))
    return np.asarray(faces, np.int64).reshape(-1, 3), np.asarray(where, np.int64).reshape(-1, 3)


def expected_places(loops, cap):
    """(loop, ring, index) of every new vertex straight from the construction's order: loop, then ring, then index."""
    out = []
    for l, loop in enumerate(loops):
        n = len(loop)
        if n > 3 and (cap is None or n <= cap):
            for r, m in enumerate(HO.ring_sizes(n)):
                out += [(l, r, j) for j in range(m)] if r > 0 else []
    return np.asarray(out, np.int64).reshape(-1, 3)


# ---- the positions in another order of summation ---------------------------------------------------------------------------
def _prefix_in_chunks(seg, chunk=256, part=64):
    """(exclusive prefix sums of ``seg``, the total): chunk by chunk with a carry; inside a chunk, sums over ``part`` entries
    each, their exclusive sums, and the exclusive sums inside each part."""
    cum, carry = np.empty(len(seg)), 0.0
    for c0 in range(0, len(seg), chunk):
        s = seg[c0:c0 + chunk]
        offset = 0.0
        for p0 in range(0, len(s), part):
            inside = np.cumsum(s[p0:p0 + part])
            cum[c0 + p0:c0 + p0 + len(inside)] = carry + (offset + np.concatenate([[0.0], inside[:-1]]))
            offset += inside[-1]
        carry += offset
    return cum, carry


def positions_other_order(vs, loops, cap=None):
    """float32 [Vn, 3]: the new vertices of every filled loop, in the order of ``HO.fill_holes``.  float64 throughout and one
    rounding at the end, as the specification has it, but: arc lengths from ``_prefix_in_chunks``, the length of a segment as
    the difference of two prefix sums, the mean summed from the last vertex to the first."""
    vs = np.asarray(vs, np.float32).astype(np.float64)
    out = []
    for loop in loops:
        n = len(loop)
        if n <= 3 or (cap is not None and n > cap):
            continue
        b = vs[loop]
        cum, perim = _prefix_in_chunks(np.linalg.norm(np.roll(b, -1, 0) - b, axis=1))
        length = np.concatenate([cum[1:], [perim]]) - cum
        c = np.cumsum(b[::-1], axis=0)[-1] / n
        sizes = HO.ring_sizes(n)
        R = len(sizes) - 1
        for r in range(1, R):
            s = np.arange(sizes[r]) / sizes[r] * perim
            i = np.searchsorted(cum, s, side="right") - 1
            with np.errstate(invalid="ignore", divide="ignore"):
                t = np.where(length[i] > 0, (s - cum[i]) / length[i], 0.0)[:, None]
            p = b[i] * (1 - t) + b[(i + 1) % n] * t
            out.append(p + (r / R) * (c - p))
        out.append(c[None])
    return np.concatenate(out).astype(np.float32) if out else np.zeros((0, 3), np.float32)
