"""The premises of the thin-plate fairing, on the CPU: the numpy oracle (tests/fair_oracle.py) on the shared fixtures
(tests/fair_fixtures.py).  What tests/test_gpu_fair.py takes for granted is asserted here: the fixtures are what their table
says, A is symmetric positive definite, the row-by-row operator is the dense one, the error bound of the solve test fits
under float32 rounding, a plane stays a plane, and a sphere cap comes back rounder than under the Laplacian smoothing."""
import numpy as np
import pytest

import fair_fixtures as FX
import fair_oracle as FO
import holes_oracle as HO
import prepare_oracle as PO
from semigcn_amd import synth

ALL = FX.NAMES + ("a_tilted", "e_tilted")
TOL = 1e-10                  # the default of fair_thin_plate


def free_classes(case):
    """the connected classes of the free vertices under free-free edges"""
    N = FO.neighbours(case.faces, len(case.vs))
    seen, classes = set(), []
    for start in np.flatnonzero(case.free):
        if start in seen:
            continue
        comp, stack = [], [int(start)]
        seen.add(int(start))
        while stack:
            i = stack.pop()
            comp.append(i)
            for j in N[i]:
                if case.free[j] and int(j) not in seen:
                    seen.add(int(j))
                    stack.append(int(j))
        classes.append(sorted(comp))
    return classes


def test_fixtures_are_what_the_table_says():
    a, d, e, f = (FX.case(n) for n in "adef")
    assert a.V == 36 and int(a.free.sum()) == 1 and FX.system("a").d[36] == 4            # the centre of a fan of four
    assert len(FX.icosphere(3)[0]) == 642
    for n, rings in (("b", 2), ("c", 3)):
        c = FX.case(n)
        disc = FX.within(FX.icosphere(3)[1], 642, [200], rings)
        assert c.V == 642 - int(disc.sum()) and len(HO.boundary_loops(c.open_faces)) == 1 and int(c.free.sum()) > 1
        assert np.abs(np.linalg.norm(c.open_vs.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert len(free_classes(d)) == 3
    # e: one loop filled, the hole of 18 edges and the outer border open, and a row of S with a neighbour on a border
    loops = HO.boundary_loops(e.faces)
    assert sorted(len(l) for l in loops) == [18, 42] and int(e.free.sum()) == 7
    border = {v for l in loops for v in l}
    s = FX.system("e")
    assert any(int(j) in border for i in s.S for j in s.N[i]) and not any(int(i) in border for i in s.S)
    # f: a vertex of the filled loop has valence 3
    s = FX.system("f")
    assert 3 in s.d[s.S[~f.free[s.S]]].tolist()
    for n in FX.NAMES:
        c = FX.case(n)
        assert np.array_equal(c.vs[:c.V].view(np.uint32), c.open_vs.view(np.uint32)) and c.free[c.V:].all() and not c.free[:c.V].any()


@pytest.mark.parametrize("name", ALL)
def test_system_is_symmetric_positive_definite(name):
    c, s = FX.case(name), FX.system(name)
    assert FO.spd_check(c.faces, len(c.vs), c.free) is None
    assert np.array_equal(s.A, s.A.T) or np.abs(s.A - s.A.T).max() <= 1e-15 * np.abs(s.A).max()
    np.linalg.cholesky(s.A)
    # the rows: S = free u N(free), every row sums to 0 (L 1 = 0), diag(A) as the rule states it
    assert set(s.S) == set(np.flatnonzero(c.free)) | {int(j) for i in np.flatnonzero(c.free) for j in s.N[i]}
    assert np.abs(s.M.sum(1)).max() <= 1e-15
    assert np.abs(FO.jacobi_diagonal(c.faces, len(c.vs), c.free) - np.diag(s.A)).max() <= 4e-16 * np.diag(s.A).max() * 16


@pytest.mark.parametrize("name", ALL)
def test_row_by_row_apply_is_the_dense_operator(name):
    c, s = FX.case(name), FX.system(name)
    rng = np.random.default_rng(5)
    nf = int(c.free.sum())
    for p in [rng.standard_normal(nf)] + [np.eye(nf)[k] for k in (0, nf - 1)]:
        q = FO.apply(c.faces, len(c.vs), c.free, p)
        # two gathers of at most 10 terms each: a few roundings of magnitude <= ||A||_inf |p|_max
        assert np.abs(q - s.A @ p).max() <= 64 * 2.0 ** -53 * np.abs(s.A).sum(1).max() * np.abs(p).max()


@pytest.mark.parametrize("name", ALL)
def test_bound_of_the_solve_test_fits_under_float32_rounding(name):
    """tol ||A^-1|| ||b|| <= u / 4 with u = 2^-23 max |coordinate| over the free vertices of x*: an iterate that has met the
    stop test rounds to float32(x*) or to one of its neighbours."""
    c, s = FX.case(name), FX.system(name)
    x = FO.solve_direct(c.vs, c.faces, c.free, s)
    u = 2.0 ** -23 * np.abs(x[c.free]).max(0)
    bound = FO.solve_bound(s, TOL)
    print(f"{name}: nf {int(c.free.sum())}, cond(A) {np.linalg.cond(s.A):.1f}, bound {bound}, u / 4 {u / 4}")
    assert (bound <= u / 4).all()
    # the minimiser is one: the gradient of E vanishes on the free vertices
    g = (s.M[:, c.free].T @ (s.M @ x))
    assert np.abs(g).max() <= 1e-12 * max(np.abs(x).max(), 1.0)
    assert s.energy(x) <= s.energy(c.vs.astype(np.float64)) * (1 + 1e-12)      # (a) starts at its minimiser


@pytest.mark.parametrize("name", ["a_tilted", "e_tilted"])
def test_a_tilted_plane_stays_a_plane(name):
    """Exact by linearity: L 1 = 0 and L is linear, so the in-plane positions with every free vertex in the plane have a
    gradient whose normal component is 0; what remains is float64 rounding of numpy.linalg.solve."""
    c, s = FX.case(name), FX.system(name)
    n = FX.TILT_NORMAL / np.linalg.norm(FX.TILT_NORMAL)
    assert np.abs(c.open_vs.astype(np.float64) @ n).max() <= 2.0 ** -22 * np.abs(c.open_vs).max()     # float32 grid points
    x = FO.solve_direct(c.vs, c.faces, c.free, s)
    off = np.abs(x[c.free] @ n).max()
    print(f"{name}: largest distance of a free vertex from the plane {off:.3e}")
    assert off <= 2.0 ** -22 * np.abs(c.open_vs).max()


@pytest.mark.parametrize("name", ["b", "c"])
def test_a_sphere_cap_comes_back_rounder_than_under_the_laplacian(name):
    c, s = FX.case(name), FX.system(name)

    def deviation(p):
        return float(np.abs(np.linalg.norm(p[c.free], axis=1) - 1.0).max())
    raw = deviation(c.vs.astype(np.float64))
    lap = deviation(PO.smooth(c.vs.astype(np.float64), c.faces, 30, movable=c.free))
    thin = deviation(FO.solve_direct(c.vs, c.faces, c.free, s))
    print(f"{name}: largest radial deviation of an inserted vertex: raw {raw:.5f}, 30 Laplacian steps {lap:.5f}, "
          f"thin plate {thin:.5f}")
    assert thin < lap


def test_spd_check():
    m = synth.octahedron_sphere(1)
    V = m.num_vertices
    assert FO.spd_check(m.faces, V, np.ones(V, bool)) == (0, "floating")
    one_fixed = np.ones(V, bool)
    one_fixed[3] = False
    assert FO.spd_check(m.faces, V, one_fixed) is None
    assert FO.spd_check(m.faces, V, np.zeros(V, bool)) is None
    # two more vertices that no face uses: free and isolated comes first, whatever else is wrong
    free = np.ones(V + 2, bool)
    assert FO.spd_check(m.faces, V + 2, free) == (V, "isolated")
    free[V:] = False
    assert FO.spd_check(m.faces, V + 2, free) == (0, "floating")
