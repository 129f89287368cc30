"""The premises of the thin-plate fairing, on the CPU: the numpy oracle (tests/fair_oracle.py) on the shared fixtures
(tests/fair_fixtures.py).  What tests/test_gpu_fair.py takes for granted is asserted here: the fixtures are what their table
says, A is symmetric positive definite, the row-by-row operator is the dense one, the error bound of the solve test fits
under float32 rounding, a plane stays a plane, and a sphere cap comes back rounder than under the Laplacian smoothing.

The second half does the same for the vectorised oracle and the masked fixtures of tests/test_gpu_fair_sizes.py: the
vectorised operator equals the row-by-row one bit for bit, every solve fixture is SPD with its bound under float32
rounding at the tolerance its test uses, the rule's own CG lands on the direct solve, the blocks fixture really is block
diagonal, the soup has the clean mesh's graph, and a coordinate with b = 0 but r0 != 0 stops."""
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


# ---- the vectorised oracle and the masked fixtures ------------------------------------------------------------------------
U32 = 2.0 ** -23


def mesh_of(name):
    return FX.case(name) if name in FX.NAMES else FX.masked(name)


@pytest.mark.parametrize("name", FX.NAMES + FX.SMALL)
def test_vectorised_apply_and_diagonal_equal_the_row_by_row_ones_bit_for_bit(name):
    c, t = mesh_of(name), FX.table(name)
    V, nf = len(c.vs), int(c.free.sum())
    N = FO.neighbours(c.faces, V)
    assert all(np.array_equal(t.nbr[i, :t.d[i]], N[i]) and (t.nbr[i, t.d[i]:] == -1).all() for i in range(V))
    assert np.array_equal(FO.diagonal_table(t, c.free).view(np.uint64), FO.jacobi_diagonal(c.faces, V, c.free).view(np.uint64))
    rng = np.random.default_rng(7)
    ps = np.stack([rng.standard_normal(nf)] + [np.eye(nf)[k] for k in sorted({0, nf // 2, nf - 1})], 1)
    got = FO.apply_table(t, c.free, ps)                                         # the columns at once ...
    for k in range(ps.shape[1]):
        want = FO.apply(c.faces, V, c.free, ps[:, k])
        assert np.array_equal(got[:, k].view(np.uint64), want.view(np.uint64))
        assert np.array_equal(FO.apply_table(t, c.free, ps[:, k]).view(np.uint64), want.view(np.uint64))    # ... and one


@pytest.mark.parametrize("name", ["e", "disc", "grid_mask", "wheel_rim", "soup", "plane_off"])
def test_vectorised_right_hand_side_and_first_residual_are_the_dense_ones(name):
    c, t = mesh_of(name), FX.table(name)
    s = FX.system(name) if name in FX.NAMES else FX.masked_system(name)
    Mf = s.M[:, s.free]
    scale = 64 * 2.0 ** -53 * np.abs(s.M).sum(1).max() ** 2 * max(np.abs(s.x).max(), 1.0)
    assert np.abs(-FO.normal_rows(t, c.free, c.vs, True) - s.b).max() <= scale
    assert np.abs(-FO.normal_rows(t, c.free, c.vs, False) - (s.b - s.A @ s.x[s.free])).max() <= scale


def test_masked_fixtures_are_what_the_table_says():
    disc = FX.masked("disc")
    assert len(disc.vs) == 4096 and int(disc.free.sum()) == 1288
    for k in FX.SWEEP:
        c = FX.masked(f"sweep{k}")
        assert int(c.free.sum()) == k and np.array_equal(np.flatnonzero(c.free), np.flatnonzero(disc.free)[:k])
        assert np.array_equal(c.faces, disc.faces)
    # borders, far valences, free classes that meet only in a fixed row
    g, t = FX.masked("grid_mask"), FX.table("grid_mask")
    border = t.d < 6
    assert (g.free & border).any() and (g.free & ~border).any()
    s = FX.masked_system("grid_mask")
    labels = np.full(len(g.vs), -1)
    for k, cl in enumerate(free_classes(g)):
        labels[cl] = k
    assert any(len(set(labels[s.N[i]][g.free[s.N[i]]])) > 1 for i in s.S if not g.free[i])
    assert FX.table("wheel_hub").d[0] == 40 and set(FX.table("wheel_rim").d[1:]) == {3}
    assert FX.masked("wheel_hub").free.sum() == 1 and FX.masked("wheel_rim").free.sum() == 40
    for name in FX.PLANES:
        c = FX.masked(name)
        assert int(c.free.sum()) == 232 and not c.vs[~c.free, 2].any()
    assert FX.masked("plane_off").vs[:, 2].any() and not FX.masked("plane_in").vs[:, 2].any()
    assert np.array_equal(FX.masked("plane_off").vs[:, :2], FX.masked("plane_in").vs[:, :2])


def test_the_soup_has_the_graph_of_the_clean_mesh():
    soup, clean = FX.masked("soup"), FX.masked("soup_clean")
    assert len(soup.faces) > len(clean.faces) and np.array_equal(soup.vs, clean.vs) and np.array_equal(soup.free, clean.free)
    key = lambda f: {tuple(np.roll(r, -int(np.argmin(r)))) for r in f}                   # a face up to rotation
    assert len(key(soup.faces)) < len(soup.faces)                                        # repeats ...
    assert any(tuple(np.roll(r[::-1], -int(np.argmin(r[::-1])))) in key(soup.faces) for r in soup.faces)    # ... and reversed ones
    a, b = 3 * 7 + 3, 4 * 7 + 4
    assert sum(1 for r in clean.faces if a in r and b in r) == 3                         # the fin's edge
    assert np.array_equal(FX.table("soup").nbr, FX.table("soup_clean").nbr)
    N, M = FO.neighbours(soup.faces, 50), FO.neighbours(clean.faces, 50)
    assert all(np.array_equal(x, y) for x, y in zip(N, M))


SOLVE_TOL = {**{f"sweep{k}": 1e-13 for k in FX.SWEEP}, "disc": 1e-13, **{n: 1e-10 for n in FX.MASKS}}


@pytest.mark.parametrize("name", sorted(SOLVE_TOL))
def test_masked_systems_are_spd_and_their_bound_fits_under_float32_rounding(name):
    c, s = FX.masked(name), FX.masked_system(name)
    assert FO.spd_check(c.faces, len(c.vs), c.free) is None
    assert np.abs(s.A - s.A.T).max() <= 1e-15 * np.abs(s.A).max()
    np.linalg.cholesky(s.A)
    x = FO.solve_direct(c.vs, c.faces, c.free, s)
    u = U32 * np.abs(x[c.free]).max(0)
    bound = FO.solve_bound(s, SOLVE_TOL[name])
    print(f"{name}: nf {int(c.free.sum())}, cond(A) {np.linalg.cond(s.A):.1f}, bound {bound}, u / 4 {u / 4}")
    assert (s.b != 0).any(0).all() and (bound <= u / 4).all()
    assert (np.abs(x[c.free]).max(0) >= 0.1 * np.abs(s.x).max(0)).all()      # u is not measured on a minimiser that is 0
    assert np.abs(x[c.free] - c.vs[c.free]).max() > 0.01                     # the start is not the minimiser


@pytest.mark.parametrize("name", [f"sweep{k}" for k in FX.SWEEP] + ["disc"])
def test_the_cg_of_the_rule_ends_on_the_direct_solve(name):
    """within u / 4 of x*: only the device's summation order then separates the device from this run"""
    c, s = FX.masked(name), FX.masked_system(name)
    want = FO.solve_direct(c.vs, c.faces, c.free, s)[c.free]
    x, info = FO.cg(FX.table(name), c.free, c.vs, SOLVE_TOL[name])
    err, u = np.abs(x - want).max(0), U32 * np.abs(want).max(0)
    print(f"{name}: {info}; max |cg - x*| {err}, u / 4 {u / 4}")
    assert info["converged"] and 1 < info["iterations"] < 2000 and (err <= u / 4).all()
    assert all(r <= SOLVE_TOL[name] for r in info["relative_residual"])


def test_the_blocks_fixture_is_block_diagonal_and_its_bound_fits():
    c, t, e = FX.masked("blocks"), FX.table("blocks"), FX.blocks_exact()
    nf = int(c.free.sum())
    assert nf == 266256 > 1024 * 256 and e.A.shape == (29584, 9, 9) and np.array_equal(np.sort(e.rows.ravel()), np.arange(nf))
    # a column of A read at one class only would not be symmetric if another class reached into it
    assert np.abs(e.A - e.A.transpose(0, 2, 1)).max() <= 1e-15 * np.abs(e.A).max()
    # nothing of A lies outside the blocks: A times a vector is the blocks times its pieces
    p = np.random.default_rng(3).standard_normal(nf)
    q = np.empty(nf)
    q[e.rows.ravel()] = (e.A @ p[e.rows][:, :, None]).ravel()
    assert np.abs(FO.apply_table(t, c.free, p) - q).max() <= 64 * 2.0 ** -53 * np.abs(e.A).sum(2).max() * np.abs(p).max()
    assert e.min_eig > 0.2
    u = U32 * np.abs(e.x).max(0)
    bound = 1e-12 / e.min_eig * np.linalg.norm(e.b, axis=0)
    print(f"blocks: smallest eigenvalue {e.min_eig:.4f}, bound {bound}, u / 4 {u / 4}")
    assert (bound <= u / 4).all() and np.abs(e.x - c.vs[c.free]).max() > 0.01
    x, info = FO.cg(t, c.free, c.vs, 1e-12)
    err = np.abs(x - e.x).max(0)
    print(f"blocks: {info}; max |cg - x*| {err}")
    assert info["converged"] and 1 < info["iterations"] < 100 and (err <= u / 4).all()


def test_a_coordinate_with_zero_b_is_measured_against_its_first_residual():
    """z of plane_off: every fixed vertex has z = 0, so b = 0, and the free ones start off the plane, so r0 != 0.  The stop
    test ``r.r <= tol^2 b.b`` could never be met; against ``r0.r0`` the coordinate stops like the other two."""
    c, s, t = FX.masked("plane_off"), FX.masked_system("plane_off"), FX.table("plane_off")
    r0 = -FO.normal_rows(t, c.free, c.vs, False)
    assert not s.b[:, 2].any() and r0[:, 2].any() and s.b[:, :2].any(0).all()
    x, info = FO.cg(t, c.free, c.vs, 1e-10)
    bound = 1e-10 / np.linalg.eigvalsh(s.A)[0] * np.linalg.norm(r0[:, 2])
    print(f"plane_off: {info}; max |z| {np.abs(x[:, 2]).max():.3e}, bound {bound:.3e}")
    assert info["converged"] and info["iterations"] < 1000 and np.isfinite(x).all()
    assert np.abs(x[:, 2]).max() <= bound and all(r <= 1e-10 for r in info["relative_residual"])
    # started in the plane the coordinate has nothing to do, and the other two do not notice
    x_in, info_in = FO.cg(t, FX.masked("plane_in").free, FX.masked("plane_in").vs, 1e-10)
    assert info_in["converged"] and not x_in[:, 2].any() and info_in["relative_residual"][2] == 0.0
    assert np.array_equal(x_in[:, :2], x[:, :2])
