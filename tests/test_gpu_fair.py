"""The thin-plate fairing on the device (csrc/mesh_fair.hip) against the numpy oracle (tests/fair_oracle.py) on the fixtures
of tests/fair_fixtures.py; the premises used here (A is SPD, the bound fits under float32 rounding, a plane stays a plane,
a sphere cap comes back rounder) are asserted on the CPU in tests/test_fair_oracle.py.

  apply   sg_fair_apply and sg_fair_diagonal equal the oracle bit for bit (float64, ascending neighbour order, no fused
          multiply-add);
  solve   |device - float32(x*)| <= u + bound per coordinate, x* from numpy.linalg.solve, bound = tol ||A^-1|| ||b||,
          u = 2^-23 max |coordinate| over the free vertices;
  the rest: determinism and independence of check_every, what must not move, planes and sphere caps, caps and errors, the
          hand-over to prepare_inputs and the command line."""
import json

import numpy as np
import pytest
import torch

import fair_fixtures as FX
import fair_oracle as FO
from semigcn_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TOL = 1e-10


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared fixtures are read-only
    return t if dtype is None else t.to(dtype)


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


# ---- apply -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FX.NAMES)
def test_apply_and_diagonal_equal_the_oracle_bit_for_bit(name):
    from semigcn_amd import capi
    c, s = FX.case(name), FX.system(name)
    V, nf = len(c.vs), int(c.free.sum())
    rng = np.random.default_rng(11)
    ps = [rng.standard_normal(nf)] + [np.eye(nf)[k] for k in sorted({0, nf // 2, nf - 1})]
    with capi.FairPlan(dev(c.faces), V, dev(c.free)) as plan:
        assert (plan.num_free, plan.num_rows, plan.bad_vertex, plan.solvable) == (nf, len(s.S), -1, True)
        assert plan.nnz == int(s.d[s.S].sum()) and plan.launches_per_iteration <= 4
        diag = plan.diagonal().cpu().numpy()
        got = [plan.apply(dev(p)).cpu().numpy() for p in ps]
    assert np.array_equal(diag.view(np.uint64), FO.jacobi_diagonal(c.faces, V, c.free).view(np.uint64))
    for p, q in zip(ps, got):
        want = FO.apply(c.faces, V, c.free, p)
        assert np.array_equal(q.view(np.uint64), want.view(np.uint64)), np.abs(q - want).max()


# ---- solve -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", FX.NAMES + ("a_tilted", "e_tilted"))
def test_solve_against_the_direct_solve(name):
    from semigcn_amd import holes
    c, s = FX.case(name), FX.system(name)
    want = FO.solve_direct(c.vs, c.faces, c.free, s)
    u = 2.0 ** -23 * np.abs(want[c.free]).max(0)
    bound = FO.solve_bound(s, TOL)
    assert (bound <= u / 4).all()
    out, info = holes.fair_thin_plate(dev(c.vs), dev(c.faces), dev(c.free), tol=TOL, return_info=True)
    got = out.cpu().numpy()
    err = np.abs(got[c.free].astype(np.float64) - want[c.free].astype(np.float32).astype(np.float64)).max(0)
    print(f"{name}: {info}; max |device - float32(x*)| {err}, u + bound {u + bound}")
    assert info["converged"] and info["n_free"] == int(c.free.sum()) and info["iterations"] >= 0
    assert all(r <= TOL * (1 + 2.0 ** -50) for r in info["relative_residual"])        # the test is on the squares
    assert (err <= u + bound).all()
    assert out.dtype == torch.float32 and np.array_equal(got[~c.free].view(np.uint32), c.vs[~c.free].view(np.uint32))


# ---- determinism -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c", "d"])
def test_two_runs_and_two_polling_rates_give_identical_bytes(name):
    from semigcn_amd import holes
    c = FX.case(name)
    args = (dev(c.vs), dev(c.faces), dev(c.free))
    a, ia = holes.fair_thin_plate(*args, return_info=True)
    b, ib = holes.fair_thin_plate(*args, return_info=True)
    e, ie = holes.fair_thin_plate(*args, check_every=1, return_info=True)
    assert torch.equal(bits(a), bits(b)) and ia == ib
    assert torch.equal(bits(a), bits(e)) and ia == ie and ia["iterations"] > 1
    assert torch.equal(bits(a), bits(holes.fair_thin_plate(*args, check_every=7)))


# ---- what must not move ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["d", "e"])
def test_fill_holes_moves_only_the_inserted_vertices(name):
    from semigcn_amd import holes
    c = FX.case(name)
    mesh = (dev(c.open_vs), dev(c.open_faces))
    V, F = c.V, c.open_faces.shape[0]
    raw = holes.fill_holes(mesh, max_hole_edges=c.max_hole_edges, fair_steps=0)
    assert np.array_equal(raw.faces.cpu().numpy(), c.faces) and np.array_equal(raw.inserted.cpu().numpy(), c.free)
    thin = holes.fill_holes(mesh, max_hole_edges=c.max_hole_edges, fair="thin_plate", timings=True)
    assert torch.equal(thin.faces, raw.faces) and torch.equal(thin.inserted, raw.inserted)
    assert torch.equal(bits(thin.vs[:V]), bits(mesh[0])) and torch.equal(thin.faces[:F], mesh[1])
    assert not torch.equal(thin.vs[V:], raw.vs[V:])
    assert thin.fair_info["converged"] and thin.fair_info["n_free"] == int(c.free.sum()) and thin.stage_ms["fair_ms"] >= 0.0
    # the same solve as the function on its own, from the device's raw construction
    assert torch.equal(bits(thin.vs), bits(holes.fair_thin_plate(raw.vs, raw.faces, raw.inserted)))
    # fair_steps is ignored, except that 0 is the raw construction
    assert torch.equal(bits(holes.fill_holes(mesh, max_hole_edges=c.max_hole_edges, fair="thin_plate", fair_steps=3).vs), bits(thin.vs))
    zero = holes.fill_holes(mesh, max_hole_edges=c.max_hole_edges, fair="thin_plate", fair_steps=0)
    assert torch.equal(bits(zero.vs), bits(raw.vs)) and zero.fair_info is None
    # the default is what it was
    old, new = holes.fill_holes(mesh, max_hole_edges=c.max_hole_edges), holes.fill_holes(mesh, max_hole_edges=c.max_hole_edges, fair="laplacian")
    assert torch.equal(bits(old.vs), bits(new.vs)) and torch.equal(old.faces, new.faces) and old.fair_info is None
    want = holes.prepare.laplacian_smooth(raw.vs, raw.faces, steps=holes.prepare.SMOOTH_ITER, movable=raw.inserted)
    assert torch.equal(bits(old.vs), bits(want))


# ---- geometry ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a_tilted", "e_tilted"])
def test_a_tilted_plane_stays_a_plane(name):
    from semigcn_amd import holes
    c = FX.case(name)
    out = holes.fill_holes((dev(c.open_vs), dev(c.open_faces)), max_hole_edges=c.max_hole_edges, fair="thin_plate")
    new = out.vs[c.V:].cpu().numpy().astype(np.float64)
    n = FX.TILT_NORMAL / np.linalg.norm(FX.TILT_NORMAL)
    u = 2.0 ** -23 * np.abs(new).max()
    off = np.abs(new @ n).max()
    print(f"{name}: {new.shape[0]} inserted vertices, largest distance from the plane {off:.3e}, 2 u = {2 * u:.3e}")
    assert new.shape[0] == int(c.free.sum()) and off <= 2 * u


@pytest.mark.parametrize("name", ["b", "c"])
def test_a_sphere_cap_comes_back_rounder_than_under_the_laplacian(name):
    from semigcn_amd import holes
    c = FX.case(name)
    mesh = (dev(c.open_vs), dev(c.open_faces))

    def deviation(filled):
        return float((filled.vs[c.V:].double().norm(dim=1) - 1.0).abs().max())
    lap, thin = deviation(holes.fill_holes(mesh)), deviation(holes.fill_holes(mesh, fair="thin_plate"))
    print(f"{name}: largest radial deviation of an inserted vertex: laplacian {lap:.5f}, thin plate {thin:.5f}")
    assert thin < lap


# ---- caps and errors ---------------------------------------------------------------------------------------------------
def test_max_iter_is_a_cap_that_is_reported():
    from semigcn_amd import holes
    c = FX.case("c")
    out, info = holes.fair_thin_plate(dev(c.vs), dev(c.faces), dev(c.free), max_iter=1, return_info=True)
    assert info["converged"] is False and info["iterations"] == 1 and max(info["relative_residual"]) > TOL
    assert bool(torch.isfinite(out).all()) and not torch.equal(out, dev(c.vs))
    out0, info0 = holes.fair_thin_plate(dev(c.vs), dev(c.faces), dev(c.free), max_iter=0, return_info=True)
    assert info0["converged"] is False and info0["iterations"] == 0 and torch.equal(bits(out0), bits(dev(c.vs)))
    filled = holes.fill_holes((dev(c.open_vs), dev(c.open_faces)), fair="thin_plate", fair_max_iter=1)
    assert filled.fair_info["converged"] is False and filled.fair_info["iterations"] == 1


def test_singular_systems_raise_and_name_the_vertex():
    from semigcn_amd import capi, holes
    m = synth.octahedron_sphere(1)
    vs, faces, V = dev(m.vs, torch.float32), dev(m.faces), m.num_vertices
    with pytest.raises(ValueError, match=r"smallest vertex is 0$"):
        holes.fair_thin_plate(vs, faces, torch.ones(V, dtype=torch.bool, device=DEV))
    # one fixed vertex anchors the whole sphere
    free = torch.ones(V, dtype=torch.bool, device=DEV)
    free[3] = False
    out, info = holes.fair_thin_plate(vs, faces, free, return_info=True)
    assert info["converged"] and torch.equal(bits(out[3]), bits(vs[3]))
    c = FX.case("d")                                    # a closed surface of another kind, with three patches
    with pytest.raises(ValueError, match=r"smallest vertex is 0$"):
        holes.fair_thin_plate(dev(c.vs), dev(c.faces), torch.ones(len(c.vs), dtype=torch.bool, device=DEV))
    # two vertices that no face uses: a free one is an error of its own, and comes first
    vs2 = torch.cat([vs, vs[:2] + 5.0])
    free2 = torch.zeros(V + 2, dtype=torch.bool, device=DEV)
    free2[V + 1] = True
    with pytest.raises(ValueError, match=rf"free vertex {V + 1} has no edges"):
        holes.fair_thin_plate(vs2, faces, free2)
    with capi.FairPlan(faces, V + 2, free2) as plan:
        assert (plan.bad_kind, plan.bad_vertex, plan.solvable) == (1, V + 1, False)
        with pytest.raises(capi.SemigcnLibraryError, match="singular"):
            plan.solve(vs2)
    with pytest.raises(capi.SemigcnLibraryError, match="outside"):
        holes.fair_thin_plate(vs, faces + 1, free)


def test_an_empty_mask_gives_a_copy():
    from semigcn_amd import holes
    c = FX.case("b")
    vs = dev(c.vs)
    out, info = holes.fair_thin_plate(vs, dev(c.faces), np.zeros(len(c.vs), bool), return_info=True)
    assert torch.equal(bits(out), bits(vs)) and out.data_ptr() != vs.data_ptr()
    assert info == {"iterations": 0, "relative_residual": [0.0, 0.0, 0.0], "converged": True, "n_free": 0}
    m = synth.octahedron_sphere(1)                      # closed: nothing to fill, nothing to fair
    filled = holes.fill_holes((m.vs.astype(np.float32), m.faces), fair="thin_plate")
    assert filled.fair_info["n_free"] == 0 and filled.fair_info["converged"]


# ---- downstream --------------------------------------------------------------------------------------------------------
def test_cut_torus_is_the_fixture_and_feeds_prepare_inputs():
    from semigcn_amd import holes, prepare
    c = FX.case("d")
    vs, faces = holes.cut_torus(24, 48, 3)
    assert np.array_equal(faces.cpu().numpy(), c.open_faces) and np.array_equal(vs.cpu().numpy().view(np.uint32), c.open_vs.view(np.uint32))
    out = holes.fill_holes((vs, faces), fair="thin_plate")
    assert out.fair_info["converged"] and int(out.filled.sum()) == 3
    p = prepare.prepare_inputs(initial=(out.vs, out.faces), original=(vs, faces))
    mask = p.v_mask.cpu().numpy()
    assert mask[:c.V].all() and mask.shape[0] == out.vs.shape[0]
    assert bool(torch.isfinite(p.initial_vs).all()) and float(p.scale) > 0


def test_repair_passes_fair_through():
    from semigcn_amd import holes, repair
    c = FX.case("d")
    mesh = (dev(c.open_vs), dev(c.open_faces))
    vs, faces, report = repair.repair(mesh, max_rounds=0, fair="thin_plate")
    want = holes.fill_holes(mesh, fair="thin_plate")
    assert torch.equal(bits(vs), bits(want.vs)) and torch.equal(faces, want.faces) and report.rounds == 0
    vs_l, _, _ = repair.repair(mesh, max_rounds=0)
    assert torch.equal(bits(vs_l), bits(holes.fill_holes(mesh).vs)) and not torch.equal(vs_l, vs)


def test_command_line(capsys):
    from semigcn_amd import holes
    assert holes.main(["--torus", "24", "48", "--cut", "3", "--fair", "thin-plate"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["fair"] == "thin-plate" and rec["fair_converged"] is True and rec["fair_iterations"] > 1
    assert rec["n_filled"] == 3 and rec["n_inserted_vertices"] == int(FX.case("d").free.sum()) and rec["fair_ms"] >= 0.0
    assert holes.main(["--torus", "24", "48", "--cut", "3", "--fair", "laplacian"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["fair"] == "laplacian" and rec["fair_iterations"] is None and rec["fair_converged"] is None
    assert holes.main(["--torus", "24", "48", "--cut", "3"]) == 0              # without the option the line is what it was
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert not any(k in plain for k in ("fair", "fair_iterations", "fair_converged"))
    assert all(plain[k] == rec[k] for k in plain if not k.endswith("_ms"))
    with pytest.raises(SystemExit):
        holes.main(["--torus", "24", "48", "--fair", "membrane"])
