"""semigcn_amd.simplify on the device against the numpy restatement in tests/simplify_oracle.py.  Every comparison with the
oracle is exact: positions bit-identical, faces, vertex_ids, coarse_of and the per-round (candidates, admitted, winners) equal.

Shapes (tests/simplify_fixtures.py): the 258-vertex sphere at 0.6 and 0.2 (1536 half-edges: sorts, scans and compaction span 6
workgroups; 16 and 43 rounds), the 20 x 12 torus, the two open meshes (border vertices kept, open fans walked both ways), and
the hand fixtures of tests/test_simplify_oracle.py: the two fold-over grids (kept end on the border, kept end at the
midpoint), the valence-3 vertex, the all-zero costs and the float32 ties of the 66-vertex sphere."""
import numpy as np
import pytest
import torch

import simplify_fixtures as SF
import simplify_oracle as SO
from semigcn_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared fixtures are read-only
    return t if dtype is None else t.to(dtype)


def host(t):
    return t.cpu().numpy()


def manifold_report(vs, faces):
    """(every directed half-edge once, the largest number of faces on an edge, V - E + F)"""
    V = vs.shape[0]
    a, b = faces.reshape(-1), faces[:, [1, 2, 0]].reshape(-1)
    directed = a * V + b
    und, cnt = np.unique(np.minimum(a, b) * V + np.maximum(a, b), return_counts=True)
    return np.unique(directed).shape[0] == directed.shape[0], int(cnt.max()), V - und.shape[0] + faces.shape[0]


@pytest.mark.parametrize("quadrics", ["own", "sum"])
@pytest.mark.parametrize("name,ratio", SF.CASES)
def test_device_equals_the_oracle_bit_for_bit(name, ratio, quadrics):
    from semigcn_amd import simplify
    want = SF.case(name, ratio, quadrics)
    got = simplify.simplify_mesh(dev(want.in_vs), dev(want.in_faces), target_v=want.target, quadrics=quadrics)
    print(name, ratio, quadrics, "oracle rounds", want.counts, "device rounds", got.counts, "refused", want.refused,
          got.report["n_refused"])
    assert got.counts == [tuple(c) for c in want.counts]
    assert got.reached == want.reached and got.report["n_refused"] == want.refused
    assert np.array_equal(host(got.faces), want.faces)
    assert np.array_equal(host(got.vertex_ids), want.vertex_ids) and np.array_equal(host(got.coarse_of), want.coarse_of)
    assert host(got.vs).tobytes() == want.vs.tobytes()
    assert got.report["n_vertices"] == want.vs.shape[0] and got.report["largest_cluster"] == int(np.bincount(want.coarse_of).max())
    again = simplify.simplify_mesh(dev(want.in_vs), dev(want.in_faces), target_v=want.target, quadrics=quadrics)
    for a, b in ((got.vs, again.vs), (got.faces, again.faces), (got.vertex_ids, again.vertex_ids), (got.coarse_of, again.coarse_of)):
        assert host(a).tobytes() == host(b).tobytes()
    assert got.counts == again.counts


@pytest.mark.parametrize("name", ["sphere258", "wavy12"])
def test_quadrics_kernel_equals_numpy_bit_for_bit(name):
    """float64 division and the summation order (ascending face index) on this compiler against numpy."""
    from semigcn_amd import capi
    vs, faces = SF.mesh(name)
    with capi.RemeshPlan(dev(vs), dev(faces)) as plan:
        got = host(plan.quadrics())
    want = SO.vertex_quadrics(vs, faces)
    differ = np.nonzero((got.view(np.uint64) != want.view(np.uint64)).any(1))[0]
    print(name, "vertices whose quadric differs in a bit:", differ.shape[0], "of", vs.shape[0],
          "largest difference", float(np.abs(got - want).max()))
    assert got.shape == (vs.shape[0], 10) and got.tobytes() == want.tobytes()


def test_three_levels_in_a_row_land_on_their_counts():
    from semigcn_amd import simplify
    vs, faces = SF.mesh("torus20x12")
    V = vs.shape[0]
    cur_vs, cur_faces = dev(vs), dev(faces)
    for target in (int(V * 0.6), int(V * 0.36), int(V * 0.216)):          # as MGCN.__init__ asks for them
        out = simplify.simplify_mesh(cur_vs, cur_faces, target_v=target)
        once, most, chi = manifold_report(host(out.vs), host(out.faces))
        assert out.reached and out.vs.shape[0] == target and sum(c[2] for c in out.counts) == cur_vs.shape[0] - target
        assert all(c[1] <= c[0] and c[2] <= c[1] for c in out.counts)
        assert once and most == 2 and chi == 0
        assert np.array_equal(host(out.coarse_of[out.vertex_ids]), np.arange(target))
        cur_vs, cur_faces = out.vs, out.faces


def test_unreachable_targets_are_reported_not_raised():
    from semigcn_amd import simplify
    vs, faces = SF.mesh("tetrahedron")
    out = simplify.simplify_mesh(dev(vs), dev(faces), target_v=3)
    assert not out.reached and out.counts == [] and np.array_equal(host(out.faces), faces) and host(out.vs).tobytes() == vs.tobytes()
    assert out.report["n_refused"] == 6
    vs, faces = SF.mesh("sphere258")
    out = simplify.simplify_mesh(dev(vs), dev(faces), target_v=3)
    once, most, chi = manifold_report(host(out.vs), host(out.faces))
    print("sphere asked down to 3: stopped at", out.vs.shape[0], "vertices after", len(out.counts), "rounds")
    assert not out.reached and 4 <= out.vs.shape[0] < 258 and once and most == 2 and chi == 2


def _cluster_quadric_error(vs, faces, coarse_of, coarse_pos):
    from semigcn_amd.meshprep import _vertex_quadrics
    Q = _vertex_quadrics(vs, faces)
    Qc = torch.zeros((coarse_pos.shape[0], 4, 4), dtype=torch.float64, device=vs.device).index_add_(0, coarse_of, Q)
    p4 = torch.cat([coarse_pos.double(), torch.ones((coarse_pos.shape[0], 1), dtype=torch.float64, device=vs.device)], 1)
    return float(torch.einsum("ci,cij,cj->c", p4, Qc, p4).sum())


@pytest.mark.parametrize("which", ["torus", "sphere"])
def test_device_mesh_collapse_criterion_keeps_the_artefact_contract(which):
    """The contract of tests/test_gpu_parity.py::test_device_hierarchy_by_quadric_error on ``criterion="collapse"``, and no more
    summed cluster quadric error than ``criterion="qem"`` on the same mesh.  ``DeviceMesh`` runs the stage with
    ``quadrics="sum"``; measured on the 40 x 30 torus: 23.06 against 25.29 for "qem" (with "own" 25.93: above), on the
    1026-vertex sphere 8.45 against 8.92 (with "own" 8.88)."""
    from semigcn_amd import meshprep
    m = synth.torus_mesh(40, 30, masks=False) if which == "torus" else synth.octahedron_sphere(4)
    V = m.num_vertices
    fine = meshprep.DeviceMesh(m.x_pos, m.faces, DEV, criterion="collapse")
    target = int(V * 0.6)
    coarse = fine.simplification(target)
    ph = coarse.pool_hash
    Vc = coarse.vs.shape[0]
    assert coarse.criterion == "collapse"
    assert Vc == target and ph.shape == (V, 2) and np.array_equal(ph[:, 0], np.arange(V))
    sizes = np.bincount(ph[:, 1], minlength=Vc)
    assert sizes.min() == 1
    order = np.argsort(ph[:, 1], kind="stable")
    first = np.searchsorted(ph[order, 1], np.arange(Vc))
    assert (np.diff(order[first]) > 0).all()            # closed mesh: cluster ids ascend with the smallest member
    ce = ph[:, 1][m.edge_index]
    ce = ce[:, ce[0] != ce[1]]
    want = np.unique(np.minimum(ce[0], ce[1]) * Vc + np.maximum(ce[0], ce[1]))
    got = coarse.edge_index.cpu().numpy()
    half = got.shape[1] // 2
    assert np.array_equal(got[0, :half] * Vc + got[1, :half], want) and np.array_equal(got[:, half:], got[::-1, :half])
    cf = coarse.faces.cpu().numpy()
    assert ((cf[:, 0] != cf[:, 1]) & (cf[:, 1] != cf[:, 2]) & (cf[:, 2] != cf[:, 0])).all() and cf.max() < Vc
    e = np.sort(np.concatenate([cf[:, [0, 1]], cf[:, [1, 2]], cf[:, [2, 0]]]), 1)
    key, cnt = np.unique(e[:, 0] * Vc + e[:, 1], return_counts=True)
    assert (cnt == 2).all()                              # closed manifold: every edge in two triangles
    assert Vc - key.shape[0] + cf.shape[0] == (0 if which == "torus" else 2)      # Euler characteristic kept
    assert np.array_equal(key, want)                     # the quotient graph IS the edge set of the surviving triangles
    by_qem = fine.simplification(target, criterion="qem")
    e_c = _cluster_quadric_error(fine.vs, fine.faces, torch.from_numpy(ph[:, 1]).to(DEV), coarse.vs)
    e_q = _cluster_quadric_error(fine.vs, fine.faces, torch.from_numpy(by_qem.pool_hash[:, 1]).to(DEV), by_qem.vs)
    print(which, "summed quadric error: collapse", e_c, "qem matching", e_q, "largest cluster", int(sizes.max()))
    assert e_c <= e_q
    c2 = coarse.simplification(int(V * 0.36))
    assert c2.vs.shape[0] == int(V * 0.36) and c2.criterion == "collapse"


def test_mgcn_builds_and_trains_one_step_on_the_collapse_hierarchy():
    from semigcn_amd import meshprep
    from semigcn_amd.meshnet import MGCN
    m = synth.octahedron_sphere(3)
    smo = meshprep.DeviceMesh(m.x_pos, m.faces, DEV, criterion="collapse")
    ini = meshprep.DeviceMesh(m.vs.astype(np.float32), m.faces, DEV, criterion="collapse")
    torch.manual_seed(3)
    net = MGCN(DEV, smo, ini, torch.from_numpy(m.v_mask))
    assert [p.shape[0] for p in net.smposs_list] == [258, 154, 92, 55]
    net.to(DEV).train()

    class D:
        z1 = torch.from_numpy(m.z1).to(DEV)
        x_pos = None
    outs = net(D, None)
    loss = sum(w * ((o - t) ** 2).mean() for w, o, t in zip((0.35, 0.3, 0.2, 0.15), outs, net.poss_list))
    loss.backward()
    grads = [p.grad for p in net.parameters() if p.grad is not None]
    assert bool(torch.isfinite(loss)) and grads and all(bool(torch.isfinite(g).all()) for g in grads)


def test_an_invalid_plan_is_refused_and_nothing_is_written():
    """``simplify_mesh`` raises its ValueError before the entry point is reached; a ``RemeshPlan`` built by hand on a mesh whose
    faces run an edge in the same direction reaches ``sg_remesh_simplify``'s own refusal."""
    import ctypes
    from semigcn_amd import capi, simplify
    vs, faces = SF.mesh("tetrahedron")
    bad = np.concatenate([faces[:3], faces[3:, ::-1]])
    with pytest.raises(ValueError, match="cannot be simplified.*3 edge"):
        simplify.simplify_mesh(dev(vs), dev(bad), target_v=3)
    with capi.RemeshPlan(dev(vs), dev(bad)) as plan:
        assert not plan.valid and plan.n_misoriented == 3
        with pytest.raises(capi.SemigcnLibraryError, match="sg_remesh_simplify.*did not pass validation"):
            plan.simplify(3)
        with pytest.raises(capi.SemigcnLibraryError, match="sg_remesh_quadrics.*did not pass validation"):
            plan.quadrics()
        counts = (ctypes.c_int64 * 12)(*([7] * 12))
        n_rounds, n_refused = ctypes.c_int64(7), ctypes.c_int64(7)
        rc = capi.load().sg_remesh_simplify(plan._h, 3, 0, 4, None, counts, ctypes.byref(n_rounds), ctypes.byref(n_refused))
        assert rc != 0 and list(counts) == [7] * 12 and (n_rounds.value, n_refused.value) == (7, 7)
        assert plan.num_vertices == 4 and np.array_equal(host(plan.export()[1]), bad)
        ids, into = plan.collapse_maps()
        assert np.array_equal(host(ids), np.arange(4)) and np.array_equal(host(into), np.arange(4))


def test_quadrics_asked_for_first_are_the_ones_the_stage_works_on():
    """``RemeshPlan.quadrics`` followed by ``simplify`` does not form the quadrics twice; the result is the one of ``simplify``
    alone, and the next call on the same plan forms its own again."""
    from semigcn_amd import capi
    want = SF.case("wavy12", 0.6, "sum")
    outs = []
    for first in (False, True):
        with capi.RemeshPlan(dev(want.in_vs), dev(want.in_faces)) as plan:
            if first:
                plan.quadrics()
            counts, _ = plan.simplify(want.target, "sum")
            outs.append((counts, host(plan.export()[0]).tobytes(), host(plan.export()[1]).tobytes()))
            if first:                                       # a second level on the same plan: the quadrics of ITS start, not
                t2 = int(want.target * 0.6)                 # the summed ones the first level left behind
                c2, _ = plan.simplify(t2, "sum")
                lvl2 = SO.simplify(want.vs, want.faces, t2, quadrics="sum")
                assert c2 == [tuple(c) for c in lvl2[4]] and host(plan.export()[0]).tobytes() == lvl2[0].tobytes()
    assert outs[0] == outs[1] and outs[0][0] == [tuple(c) for c in want.counts] and outs[0][1] == want.vs.tobytes()


def test_command_line_three_levels(capsys):
    import json
    from semigcn_amd import simplify
    assert simplify.main(["--torus", "20", "12", "--ratio", "0.6", "--levels", "3", "--json"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    want = SF.case("torus20x12", 0.6, "own")
    assert rec["quadrics"] == "own" and [l["n_vertices"] for l in rec["levels"]] == [144, 86, 51]
    assert all(l["reached"] and l["simplify_ms"] > 0 and l["rounds"] == len(l["winners"]) for l in rec["levels"])
    assert rec["levels"][0]["winners"] == [c[2] for c in want.counts] and rec["levels"][0]["n_refused"] == want.refused
