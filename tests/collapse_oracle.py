"""numpy restatement of "2a. collapse_short_edges" of semigcn_amd/remesh.py (its module docstring is the specification):
serial and dictionary-based like tests/remesh_oracle.py, whose helpers it uses -- no sorted keys, no twin table, no fan walk
through half-edges, no atomics; nothing here is shared with the kernels."""
from __future__ import annotations

import numpy as np

from remesh_oracle import (MASK, _dot, _normal, bits, check_input, edge_table, flip_edges, hash32, len2, split_long_edges,  # noqa: F401
                           split_threshold, valences)


def collapse_threshold(target):
    return np.float32((4.0 / 5.0 * float(target)) ** 2)


def _edge(a, b):
    return (min(a, b), max(a, b))


def _fan(faces, at, r, k):
    """The faces at ``r`` rotated to (r, x, y), in the order of the cycle that starts at the face (r, k, .); None when the
    faces at ``r`` are not one closed cycle."""
    nxt = {}
    for f in at[r]:
        tri = [int(v) for v in faces[f]]
        i = tri.index(r)
        x, y = tri[(i + 1) % 3], tri[(i + 2) % 3]
        if x in nxt:
            return None
        nxt[x] = (y, f)
    fan, x = [], k
    for _ in range(len(at[r])):
        if x not in nxt:
            return None
        y, f = nxt[x]
        fan.append((f, x, y))
        x = y
        if x == k and len(fan) < len(at[r]):
            return None
    return fan if x == k else None


def n_short(vs, faces, lo2):
    return sum(1 for e in edge_table(faces)[0] if len2(vs, *e) < lo2)


def collapse_candidates(vs, faces, lo2, thr2):
    """{edge: (priority, k, r, footprint)} of one round."""
    table, rank = edge_table(faces)
    val, border = valences(faces)
    at = {}
    for f, tri in enumerate(faces):
        for v in tri:
            at.setdefault(int(v), []).append(f)
    floor = lambda v: 2 if v in border else 3
    cands = {}
    for e, hs in table.items():
        l2 = len2(vs, *e)
        if len(hs) != 2 or not l2 < lo2:
            continue
        a, b = e
        if a in border and b in border:
            continue
        k = a if a in border else (b if b in border else min(a, b))
        r = b if k == a else a
        h0, h1 = hs
        c = int(faces[h0 // 3][(h0 % 3 + 2) % 3])
        d = int(faces[h1 // 3][(h1 % 3 + 2) % 3])
        if c == d:
            continue
        fan = _fan(faces, at, r, k)
        if fan is None:
            continue
        ring = [x for _, x, _ in fan]
        assert len(ring) == val[r] and len(set(ring)) == len(ring) and k in ring
        others = [w for w in ring if w != k]
        link = [w for w in others if _edge(k, w) in table]
        if len(link) != 2:
            continue
        assert set(link) == {c, d}
        if val[c] - 1 < floor(c) or val[d] - 1 < floor(d) or val[k] + val[r] - 4 < floor(k):
            continue
        if any(len2(vs, *_edge(k, w)) > thr2 for w in others):
            continue
        if not all(_dot(_normal(vs, r, x, y), _normal(vs, k, x, y)) > 0.0 for _, x, y in fan if k not in (x, y)):
            continue
        cands[e] = ((MASK - bits(l2), hash32(rank[e]), -rank[e]), k, r, frozenset([r] + ring))
    return cands


def select_collapse(vs, faces, lo2, thr2):
    """The selected candidates [(edge, k, r, footprint)] in ascending edge order."""
    cands = collapse_candidates(vs, faces, lo2, thr2)
    at = {}
    for e, (_, _, _, foot) in cands.items():
        for v in foot:
            at.setdefault(v, []).append(e)
    selected = []
    for e in sorted(cands):
        p, k, r, foot = cands[e]
        if all(cands[o][0] <= p for v in foot for o in at[v]):
            selected.append((e, k, r, foot))
    return selected


def collapse_round(vs, faces, lo2, thr2):
    """(vs, faces, new-to-old [V'], old-to-new [V], the selected candidates)"""
    vs, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    selected = select_collapse(vs, faces, lo2, thr2)
    V = vs.shape[0]
    into = {r: k for _, k, r, _ in selected}
    assert not set(into) & set(into.values())
    out = []
    for tri in faces:
        t = [int(v) for v in tri]
        hit = [v for v in t if v in into]
        assert len(hit) <= 1
        if hit and into[hit[0]] in t:
            continue                                        # one of the two faces of the edge
        out.append([into.get(v, v) for v in t])
    keep = [v for v in range(V) if v not in into]
    new = {v: i for i, v in enumerate(keep)}
    old_to_new = np.array([new[into.get(v, v)] for v in range(V)], np.int64)
    out = np.array([[new[v] for v in t] for t in out], np.int64).reshape(-1, 3)
    return vs[keep], out, np.array(keep, np.int64), old_to_new, selected


def collapse_short_edges(vs, faces, target, max_rounds=128, thresholds=None):
    """(vs, faces, vertex_ids, merged_into, counts, n_short)"""
    vs, faces = np.asarray(vs, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    check_input(vs, faces)
    lo2, thr2 = thresholds if thresholds is not None else (collapse_threshold(target), split_threshold(target))
    ids = np.arange(vs.shape[0], dtype=np.int64)
    merged = np.arange(vs.shape[0], dtype=np.int64)
    counts = []
    while len(counts) < max_rounds:
        new_vs, new_faces, keep, old_to_new, selected = collapse_round(vs, faces, lo2, thr2)
        if not selected:
            break
        vs, faces = new_vs, new_faces
        ids, merged = ids[keep], old_to_new[merged]
        counts.append(len(selected))
    return vs, faces, ids, merged, counts, n_short(vs, faces, lo2)


def octa_sphere(level=3):
    """``synth.octahedron_sphere(level)``: valence-4 poles, every edge near length 1."""
    from semigcn_amd import synth
    m = synth.octahedron_sphere(level)
    return m.vs.astype(np.float32), m.faces.astype(np.int64)
