"""semigcn_amd.simplify on the device where the ten fixtures of tests/test_gpu_simplify.py do not go: the clauses of the rule
(the module docstring of semigcn_amd/simplify.py) that none of them executes.  The fixtures are in
tests/simplify_fixtures.py, their premises are pinned on the CPU in tests/test_simplify_oracle.py, and every comparison with
the oracle (tests/simplify_oracle.py) is exact, as in ``test_device_equals_the_oracle_bit_for_bit``: no tolerance anywhere.

Which line of the rule each fixture holds the kernels to (``CLAUSE``) is printed with the case."""
import numpy as np
import pytest
import torch

import simplify_fixtures as SF
import simplify_oracle as SO

pytestmark = pytest.mark.gpu

DEV = "cuda:0"

CLAUSE = {
    "touch_closed": "'The faces at r or the faces at k are not one fan': two closed fans, walk_ring closes after the first; "
                    "dropped, the eight edges at the shared vertex are legal and the first round differs",
    "touch_open": "'... not one fan': two open fans at a border vertex that is kept; the walk at k ends at both borders of one fan",
    "touch_mixed": "'... not one fan': the kept border vertex has a closed fan and an open one; from an edge into the closed fan "
                   "the walk at k closes after it",
    "flat_face": "'A face with nn == 0 contributes nothing' and 'n_old . n_new > 0 strictly': the dot product is exactly 0 for 13 "
                 "edges; with >= they are legal, without the skip the quadrics are NaN",
    "sphere66_2^60": "the cost and the priority far from unit scale: nothing special, the rounds of the unit sphere",
    "sphere66_2^100": "'the float32 maximum when cost is above it': all 192 costs are clamped and the hash alone orders",
    "sphere66_2^-70": "'c32 = float32(cost) (round to nearest even)': every cost is a float32 subnormal; flushed to zero they tie",
    "sphere66_2^-80": "'c32 = float32(cost)': every non-zero float64 cost rounds to +0",
    "sphere66_2^-140": "'the float32 midpoint (vs[lo] + vs[hi]) * 0.5f' and the float64 widening on subnormal coordinates",
    "hub_sphere": "'Link' and the fan of r and of k at valence 80: walk_ring with a limit of 80, has_edge once per ring vertex, "
                  "footprints of 83 vertices",
    "hub_disc": "'Apply' with val_new = 81: the first round's winner keeps the centre, and its footprint of 83 bids and checks",
    "unused3": "'need = V_now - target_v' counts vertices no face uses; they pass the compaction and the maps untouched",
    "torus32x24": "a round with 25 winners over 18 workgroups, bit for bit",
}


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared fixtures are read-only
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def run_mesh(want, quadrics, max_rounds=256):
    """(vs, faces, vertex_ids, coarse_of, counts, reached, refused) of ``simplify.simplify_mesh`` on the oracle's input."""
    from semigcn_amd import simplify
    got = simplify.simplify_mesh(dev(want.in_vs), dev(want.in_faces), target_v=want.target, quadrics=quadrics,
                                 max_rounds=max_rounds)
    assert got.report["n_vertices"] == got.vs.shape[0] and got.report["rounds"] == len(got.counts)
    return (host(got.vs), host(got.faces), host(got.vertex_ids), host(got.coarse_of), got.counts, got.reached,
            got.report["n_refused"])


def run_plan(want, quadrics, max_rounds=256):
    """The same of ``RemeshPlan.simplify``, ``export`` and ``collapse_maps``."""
    from semigcn_amd import capi
    with capi.RemeshPlan(dev(want.in_vs), dev(want.in_faces)) as plan:
        counts, refused = plan.simplify(want.target, quadrics, max_rounds)
        vs, faces, _, _ = plan.export()
        ids, into = plan.collapse_maps()
        assert plan.num_vertices == vs.shape[0]
        return host(vs), host(faces), host(ids), host(into), counts, vs.shape[0] == want.target, refused


def equal_the_oracle(want, quadrics, max_rounds=256, run=run_mesh):
    """The comparison of tests/test_gpu_simplify.py::test_device_equals_the_oracle_bit_for_bit."""
    got = run(want, quadrics, max_rounds)
    print(want.name, quadrics, "oracle rounds", want.counts, "device rounds", got[4], "refused", want.refused, got[6])
    assert got[4] == [tuple(c) for c in want.counts]
    assert got[5] == want.reached and got[6] == want.refused
    assert np.array_equal(got[1], want.faces)
    assert np.array_equal(got[2], want.vertex_ids) and np.array_equal(got[3], want.coarse_of)
    assert got[0].tobytes() == want.vs.tobytes()
    again = run(want, quadrics, max_rounds)
    for a, b in zip(got[:4], again[:4]):
        assert a.tobytes() == b.tobytes()
    assert got[4:] == again[4:]
    return got


@pytest.mark.parametrize("name,ratio,quadrics", [(n, r, q) for n, r, qs in SF.EDGE_CASES for q in qs])
def test_edge_fixtures_equal_the_oracle_bit_for_bit(name, ratio, quadrics):
    """One clause of the rule per fixture, listed in ``CLAUSE``: touching fans, a face without area, the float32 end of the
    priority (clamp, subnormal costs, costs that round to +0, subnormal coordinates), rings of 80, a collapse into a hub,
    vertices no face uses, and a mesh of 18 workgroups."""
    print(name, "holds:", CLAUSE[name])
    equal_the_oracle(SF.case(name, ratio, quadrics), quadrics)


def test_quadrics_skip_the_face_without_area():
    """'A face with nn == 0 contributes nothing': the ``continue`` of ``vertex_quadrics``.  Without it the three corners of the
    flat face of ``flat_face`` get 0 / 0."""
    from semigcn_amd import capi
    vs, faces = SF.mesh("flat_face")
    with capi.RemeshPlan(dev(vs), dev(faces)) as plan:
        got = host(plan.quadrics())
    want = SO.vertex_quadrics(vs, faces)
    assert np.isfinite(got).all() and got.shape == (36, 10) and got.tobytes() == want.tobytes()


@pytest.mark.parametrize("quadrics", ["own", "sum"])
def test_a_budget_below_what_the_used_vertices_reach_is_reported(quadrics):
    """'the stage stops early when a round selects nothing ..., which is reported (reached=False), not raised', with three
    vertices no face uses in ``V_now``: asked for 5, the stage stops at 7 -- a tetrahedron and the three."""
    want = SF.run("unused3", 5, quadrics)
    got = equal_the_oracle(want, quadrics)
    assert not got[5] and got[0].shape[0] == 7 and got[6] == 6 and got[4][0] == (192, 64, 5)
    assert set(SF.UNUSED) <= set(got[2].tolist())


@pytest.mark.parametrize("run", [run_mesh, run_plan], ids=["simplify_mesh", "RemeshPlan"])
@pytest.mark.parametrize("quadrics", ["own", "sum"])
def test_round_cap_and_the_ends_of_the_budget(quadrics, run):
    """'Rounds repeat while V_now > target_v; the stage stops early ... after max_rounds rounds, which is reported': the host
    loop's ``round >= max_rounds`` against the oracle's ``len(counts) >= max_rounds`` at 0, 1 and 3, with ``n_refused`` of the
    round that was analysed and not applied; 'A = min(need, C)' at need == 1 (the cut is the top key); and no round at all
    when ``target_v`` is V: untouched bytes and identity maps."""
    vs, faces = SF.mesh("sphere66")
    for cap, V_out in ((0, 66), (1, 61), (3, 55)):
        want = SF.run("sphere66", 39, quadrics, True, cap)
        got = equal_the_oracle(want, quadrics, cap, run)
        assert not got[5] and len(got[4]) == cap and got[0].shape[0] == (V_out if quadrics == "own" or cap < 3 else 53)
    got = equal_the_oracle(SF.run("sphere66", 65, quadrics), quadrics, run=run)
    assert got[4] == [(192, 1, 1)] and got[5]
    got = equal_the_oracle(SF.run("sphere66", 66, quadrics), quadrics, run=run)
    assert got[4] == [] and got[5] and got[6] == 0 and got[0].tobytes() == vs.tobytes() and np.array_equal(got[1], faces)
    assert np.array_equal(got[2], np.arange(66)) and np.array_equal(got[3], np.arange(66))


def test_past_the_radix_sorts_switch_by_properties():
    """1 179 648 half-edges: above 1 048 576 keys rocPRIM's radix sort is onesweep, below it a merge sort, and at ratio 0.6 the
    call passes the switch on its way down -- the 64-bit priority sort of the cut ('only the A = min(need, C) of highest
    priority are admitted') and every sort of the analysis run on both.  No oracle at this size: what any result of the rule
    must satisfy, with numpy on the host."""
    from semigcn_amd import simplify
    vs, faces = SF.big_torus()
    V, F = vs.shape[0], faces.shape[0]
    target = int(V * 0.6)
    d_vs, d_faces = dev(vs), dev(faces)
    out = simplify.simplify_mesh(d_vs, d_faces, target_v=target, quadrics="sum", error_report=False)
    o_vs, o_faces, ids, into = host(out.vs), host(out.faces), host(out.vertex_ids), host(out.coarse_of)
    print("rounds", len(out.counts), out.counts[:3], "...", out.counts[-3:], "refused", out.report["n_refused"])
    assert 3 * F > 1 << 20 and out.reached and o_vs.shape[0] == target and sum(c[2] for c in out.counts) == V - target
    now, below = V, 0
    for C, A, W in out.counts:
        assert A == min(now - target, C) and 1 <= W <= A
        below += 3 * (F - 2 * (V - now)) < 1 << 20
        now -= W
    assert now == target and below >= 2 and len(out.counts) - below >= 2      # rounds on both sides of the switch
    a, b = o_faces.reshape(-1), o_faces[:, [1, 2, 0]].reshape(-1)
    und, cnt = np.unique(np.minimum(a, b) * target + np.maximum(a, b), return_counts=True)
    assert o_faces.min() >= 0 and o_faces.max() < target and (a != b).all()
    assert (cnt == 2).all() and np.unique(a * target + b).shape[0] == a.shape[0]      # two faces, in opposite directions
    assert target - und.shape[0] + o_faces.shape[0] == 0 and o_faces.shape[0] == F - 2 * (V - target)
    assert np.array_equal(into[ids], np.arange(target)) and (np.diff(ids) > 0).all()
    first = np.unique(into, return_index=True)[1]            # the first, i.e. smallest, member of every cluster
    assert np.array_equal(first, ids)
    c = into[faces]
    alive = (c[:, 0] != c[:, 1]) & (c[:, 1] != c[:, 2]) & (c[:, 2] != c[:, 0])
    assert np.array_equal(c[alive], o_faces)                 # the stable compaction
    assert (o_vs >= vs.min(0)).all() and (o_vs <= vs.max(0)).all() and np.isfinite(o_vs).all()
    again = simplify.simplify_mesh(d_vs, d_faces, target_v=target, quadrics="sum", error_report=False)
    for x, y in ((out.vs, again.vs), (out.faces, again.faces), (out.vertex_ids, again.vertex_ids), (out.coarse_of, again.coarse_of)):
        assert torch.equal(x, y)
    assert host(out.vs).tobytes() == host(again.vs).tobytes() and out.counts == again.counts
