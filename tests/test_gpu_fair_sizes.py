"""The thin-plate fairing on the device (csrc/mesh_fair.hip) past one wavefront, one block and 1024 blocks, and under masks
of the caller's: the masked fixtures of tests/fair_fixtures.py against the vectorised oracle of tests/fair_oracle.py.  The
premises (every system is SPD, its bound fits under float32 rounding at the tolerance used here, the blocks fixture is
block diagonal, the rule's own CG lands on the direct solve) are asserted on the CPU in tests/test_fair_oracle.py.

Every test reads the path it is on from the plan: ``num_partials == min(ceil(nf / 256), 1024)``, which is 1, 2, 3, 5 and 6
on the sweep and the disc and 1024 on the blocks fixture, where ``chunk`` is 512 and every thread takes two indices.

  apply        sg_fair_apply and sg_fair_diagonal equal the oracle bit for bit, with unit vectors at the ends of a
               wavefront, of a block and of the 1024 x 256 indices that one index per thread reaches;
  solve        |device - float32(x*)| <= u + bound per coordinate, as in tests/test_gpu_fair.py; x* from numpy.linalg.solve,
               dense or block by block;
  identities   two runs and three polling rates give the same bytes; the coordinates do not see each other; a factor 2
               goes through exactly;
  b = 0        a coordinate whose right-hand side is 0 stops against its first residual, or at once when that is 0 too."""
import functools

import numpy as np
import pytest
import torch

import fair_fixtures as FX
import fair_oracle as FO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U32 = 2.0 ** -23
SOLVE = tuple(f"sweep{k}" for k in (65, 257, 513, 1025)) + ("disc", "blocks") + FX.MASKS
TOL = {**{f"sweep{k}": 1e-13 for k in FX.SWEEP}, "disc": 1e-13, "blocks": 1e-12, **{n: 1e-10 for n in FX.MASKS}}
PARTIALS = {"sweep63": 1, "sweep64": 1, "sweep65": 1, "sweep255": 1, "sweep256": 1, "sweep257": 2, "sweep513": 3,
            "sweep1025": 5, "disc": 6, "blocks": 1024}


def dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)          # a copy: the shared fixtures are read-only


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def open_plan(name):
    """the plan of a fixture, on the path its name stands for"""
    from semigcn_amd import capi
    c = FX.masked(name)
    nf = int(c.free.sum())
    plan = capi.FairPlan(dev(c.faces), len(c.vs), dev(c.free))
    blocks = -(-nf // 256)
    assert plan.solvable and plan.num_free == nf
    assert plan.num_partials == min(blocks, 1024) == PARTIALS.get(name, 1)
    assert plan.chunk == 256 * -(-blocks // plan.num_partials)
    if name == "blocks":
        assert nf > 1024 * 256 and plan.chunk == 512
    else:
        assert plan.chunk == 256
    return plan


def solve(name, vs=None, **kw):
    with open_plan(name) as plan:
        return plan.solve(dev(FX.masked(name).vs) if vs is None else vs, **kw)


@functools.lru_cache(maxsize=None)
def exact(name):
    """(x* float64 [nf, 3], bound [3]) at the fixture's tolerance"""
    c = FX.masked(name)
    if name == "blocks":
        e = FX.blocks_exact()
        return e.x, TOL[name] / e.min_eig * np.linalg.norm(e.b, axis=0)
    s = FX.masked_system(name)
    return FO.solve_direct(c.vs, c.faces, c.free, s)[c.free], FO.solve_bound(s, TOL[name])


# ---- apply -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tuple(f"sweep{k}" for k in FX.SWEEP) + ("disc", "blocks") + FX.MASKS + FX.PLANES)
def test_apply_and_diagonal_equal_the_vectorised_oracle_bit_for_bit(name):
    c, t = FX.masked(name), FX.table(name)
    nf = int(c.free.sum())
    at = {0, 63, 64, 255, 256, nf - 1}
    if name == "blocks":
        last = (nf - 1) // 512                          # the last block with an index of its own; the ones above add 0
        assert 0 < last < 1023
        at |= {1024 * 256 - 1, 1024 * 256, last * 512}
    at = sorted(k for k in at if 0 <= k < nf)
    ps = np.zeros((nf, 1 + len(at)))
    ps[:, 0] = np.random.default_rng(13).standard_normal(nf)
    ps[at, 1 + np.arange(len(at))] = 1.0
    in_s = c.free | ((t.nbr >= 0) & c.free[t.nbr]).any(1)                     # S = free u N(free)
    with open_plan(name) as plan:
        assert (plan.num_rows, plan.nnz) == (int(in_s.sum()), int(t.d[in_s].sum()))
        diag = plan.diagonal().cpu().numpy()
        got = np.stack([plan.apply(dev(np.ascontiguousarray(ps[:, k]))).cpu().numpy() for k in range(ps.shape[1])], 1)
    assert np.array_equal(diag.view(np.uint64), FO.diagonal_table(t, c.free).view(np.uint64))
    want = FO.apply_table(t, c.free, ps)
    for k in range(ps.shape[1]):
        assert np.array_equal(got[:, k].view(np.uint64), want[:, k].view(np.uint64)), (k, np.abs(got[:, k] - want[:, k]).max())


def test_the_soup_gives_the_plan_of_the_clean_mesh():
    soup, clean = FX.masked("soup"), FX.masked("soup_clean")
    with open_plan("soup") as a, open_plan("soup_clean") as b:
        assert (a.num_free, a.num_rows, a.nnz) == (b.num_free, b.num_rows, b.nnz)
        assert torch.equal(bits(a.diagonal()), bits(b.diagonal()))
        out_a, info_a = a.solve(dev(soup.vs))
        out_b, info_b = b.solve(dev(clean.vs))
    assert torch.equal(bits(out_a), bits(out_b)) and info_a == info_b and info_a["converged"]


# ---- solve -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOLVE)
def test_solve_against_the_exact_solution(name):
    c = FX.masked(name)
    want, bound = exact(name)
    u = U32 * np.abs(want).max(0)
    assert (bound <= u / 4).all()
    out, info = solve(name, tol=TOL[name])
    got = out.cpu().numpy()
    err = np.abs(got[c.free].astype(np.float64) - want.astype(np.float32).astype(np.float64)).max(0)
    print(f"{name}: {info}; max |device - float32(x*)| {err}, u + bound {u + bound}")
    assert info["converged"] and info["n_free"] == int(c.free.sum())
    assert info["iterations"] > 1 or (info["iterations"] == 1 and len(want) == 1)        # one unknown: one step is exact
    assert all(r <= TOL[name] * (1 + 2.0 ** -50) for r in info["relative_residual"])
    assert (err <= u + bound).all()
    assert out.dtype == torch.float32 and np.array_equal(got[~c.free].view(np.uint32), c.vs[~c.free].view(np.uint32))


# ---- identities --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["disc", "blocks"])
def test_two_runs_and_three_polling_rates_give_identical_bytes(name):
    vs = dev(FX.masked(name).vs)
    with open_plan(name) as plan:
        a, ia = plan.solve(vs, tol=TOL[name])
        runs = [plan.solve(vs, tol=TOL[name])] + [plan.solve(vs, tol=TOL[name], check_every=k) for k in (1, 7, 32)]
    assert ia["converged"] and ia["iterations"] > 1
    for b, ib in runs:
        assert torch.equal(bits(a), bits(b)) and ia == ib


@pytest.mark.parametrize("max_iter", [100, 10000])
def test_the_coordinates_do_not_see_each_other(max_iter):
    """every coordinate has its own alpha, beta and freeze, and its own slots in the partials"""
    c = FX.masked("disc")
    free = dev(c.free)
    vs = dev(c.vs)
    turn = [1, 2, 0]
    other = vs.clone()
    other[:, 1] = vs[:, 0] * 0.5 - vs[:, 2]
    other[:, 2] = torch.from_numpy(np.random.default_rng(17).standard_normal(len(c.vs)).astype(np.float32)).to(DEV)
    with open_plan("disc") as plan:
        a, ia = plan.solve(vs, tol=1e-13, max_iter=max_iter)
        b, ib = plan.solve(vs[:, turn].contiguous(), tol=1e-13, max_iter=max_iter)
        o, _ = plan.solve(other, tol=1e-13, max_iter=max_iter)
    assert ia["converged"] == (max_iter > 1000) and (ia["iterations"] == 100 if max_iter == 100 else ia["iterations"] > 100)
    assert torch.equal(bits(b[free]), bits(a[:, turn][free]))
    assert ib["relative_residual"] == [ia["relative_residual"][k] for k in turn]
    assert torch.equal(bits(o[free][:, 0]), bits(a[free][:, 0])) and not torch.equal(o[free][:, 1], a[free][:, 1])


def test_a_factor_two_goes_through_exactly():
    """powers of two are exact in every product, sum and quotient of the solve, and in both sides of the stop test"""
    vs = dev(FX.masked("disc").vs)
    with open_plan("disc") as plan:
        a, ia = plan.solve(vs, tol=1e-13)
        b, ib = plan.solve(2 * vs, tol=1e-13)
    assert torch.equal(bits(b), bits(2 * a)) and ib == ia and ia["converged"] and ia["iterations"] > 100


# ---- b = 0 -------------------------------------------------------------------------------------------------------------
def test_a_coordinate_with_nothing_to_do_is_frozen_while_the_others_run():
    c = FX.masked("plane_in")
    out, info = solve("plane_in")
    assert info["converged"] and info["iterations"] > 1 and info["relative_residual"][2] == 0.0
    assert torch.equal(bits(out[:, 2]), bits(dev(c.vs)[:, 2]))
    assert not torch.equal(out[:, :2], dev(c.vs)[:, :2])
    # the other two are the ones of the fixture started off the plane
    off, _ = solve("plane_off")
    assert torch.equal(bits(out[:, :2]), bits(off[:, :2]))


def test_zero_right_hand_side_with_a_first_residual_converges():
    """z of plane_off: b = 0 because every fixed vertex has z = 0, r0 != 0 because the free ones start off the plane.  The
    stop test is then ``r.r <= tol^2 r0.r0``, and z stops with x and y (140 iterations in the numpy CG of the rule).
    Against ``tol^2 b.b = 0`` the coordinate could freeze only at ``r.r == 0``: measured on an MI355X before the rule was
    restated, ``max_iter`` 400 and 1000 ended unconverged with a relative residual of inf, and the default 10 000 ran 1242
    iterations, until ``r.r`` had underflowed to exactly 0 (z was then 2e-15 from the plane; no NaN on the device)."""
    from semigcn_amd import holes
    c, s, t = FX.masked("plane_off"), FX.masked_system("plane_off"), FX.table("plane_off")
    tol = 1e-10
    r0 = -FO.normal_rows(t, c.free, c.vs, False)
    assert not s.b[:, 2].any() and r0[:, 2].any()
    want = FO.solve_direct(c.vs, c.faces, c.free, s)[c.free]
    assert not want[:, 2].any()                                               # the minimiser is the plane
    u = U32 * np.abs(want).max(0)
    bound = FO.solve_bound(s, tol)
    bound[2] = tol / np.linalg.eigvalsh(s.A)[0] * np.linalg.norm(r0[:, 2])
    out, info = holes.fair_thin_plate(dev(c.vs), dev(c.faces), dev(c.free), tol=tol, return_info=True)
    got = out.cpu().numpy()
    err = np.abs(got[c.free].astype(np.float64) - want.astype(np.float32).astype(np.float64)).max(0)
    print(f"plane_off: {info}; max |device - float32(x*)| {err}, u + bound {u + bound}")
    assert info["converged"] and np.isfinite(got).all()
    assert 1 < info["iterations"] < 1000                                      # max_iter is 10 000
    assert all(r <= tol * (1 + 2.0 ** -50) for r in info["relative_residual"])
    assert (err <= u + bound).all()
    assert np.array_equal(got[~c.free].view(np.uint32), c.vs[~c.free].view(np.uint32))
