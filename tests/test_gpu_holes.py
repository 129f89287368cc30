"""semigcn_amd.holes on the device against the numpy restatement in tests/holes_oracle.py: the boundary loops (exactly, against
a serial walk), the unorderable cases, the raw patch construction (faces exactly, positions to float32 rounding), closedness
of the result, the size cap, the fairing (bit for bit the existing smoothing), the hand-over to prepare_inputs and the
network, an irregular loop, and the command line.

Shapes: n = 3 and n = 4 (the two special patches); ~200 loops of 4 .. 8 edges (the per-loop offset scans, many loops per
block); one loop of >= 300 edges (the pointer jumping crosses a 64-lane wave and a 256-thread block, the arc-length scan
takes more than one chunk); two loops of 1100 edges (longer than a 1024-thread block, 175 rings).

The offset tables at their edges (meshes from tests/holes_fixtures.py, whose premises tests/test_holes_fixtures.py pins on
the CPU, among them that these fixtures tell the kernel's offset search from one that takes the first of equal offsets):

  fans(S13), caps None / 20 / 9 / 3 / 2   S13 = [3, 40, 3, 9, 10, 3, 40, 15, 16, 21, 22, 4, 3].  A triangle adds a face but no
                      vertex and no ring table, a loop over the cap adds nothing: runs of equal entries in the per-loop
                      vertex, face and ring offsets, first, last and between filled loops, and a loop either side of every
                      change of the ring count.  Cap 3: faces without any ring table (Vn = 0, Fn = 4); cap 2: nothing.
  fans([40, 3, 9, 40]), cap 20            the open loops first and last.
  fans(S13, perm=5), caps None / 20       vertex ids shuffled: another loop order, loops interleaved in the sorted boundary.
  one FillPlan at 20, 3, None, 2          the tables shrink to faces only, grow to everything, shrink to nothing.
  L = 255, 256, 257, 1500 loops of 3 .. 23 edges, caps None / 9     the per-loop kernels run over L + 1 entries: the last
                      single block, the first second block, one more, and six blocks.
  one loop of 255, 256, 257, 511, 512, 513, 1024, 1025 edges        a whole chunk of the arc-length scan, and the pointer
                      jumping's round count at a power of two, one less, one more.
  coincident()        zero-length segments first, two in a row and closing (the ``seg > 0`` branch, the wrap to the
                      perimeter), a loop of perimeter 0 (its new vertices are its point bit for bit), a loop 1e4 away.

Positions are held to ``position_bound``, 2^-23 max|coordinate| (it was 1e-5 x the box diagonal, about 250 times as much).
Measured worst error as a fraction of that bound on the MI355X: tetrahedron, octahedron 0; many_small 0.35; one_large 0.35;
long_strip 0.36; fans(S13) 0.43 at caps None, 20, 9 and for the permuted ids and the one plan; fans([40, 3, 9, 40]) 0.13;
L = 255 .. 1500 loops 0.27; single loops 0.44 .. 0.46 (5.7e-8 .. 6.0e-8 against 1.3e-7); coincident 0.41 (4.9e-4 against
1.2e-3, set by the far loop), its two loops near the origin 0.06 of their own bound (2.7e-8 against 4.7e-7)."""
import functools
import json

import numpy as np
import pytest
import torch

import holes_fixtures as HF
import holes_oracle as HO
import prepare_oracle as PO
from semigcn_amd import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def dev(x, dtype=None):
    t = torch.from_numpy(np.array(x)).to(DEV)             # a copy: the shared fixtures are read-only
    return t if dtype is None else t.to(dtype)


# ---- meshes ------------------------------------------------------------------------------------------------------------
def cut(vs, faces, seeds, rings):
    """Drop the faces that touch a vertex within ``rings`` rings of a seed (meshprep.dilate), then the unused vertices."""
    from semigcn_amd import meshprep
    V = vs.shape[0]
    topo = meshprep.MeshTopology(dev(faces), V, DEV, with_f2f=False)
    mask = torch.zeros((V, 1), dtype=torch.bool, device=DEV)
    mask[dev(np.asarray(seeds, np.int64))] = True
    hole = meshprep.dilate(topo, mask, rings)[:, 0].cpu().numpy()
    return compact(vs, faces[~hole[faces].any(1)])


def compact(vs, faces):
    used = np.zeros(vs.shape[0], bool)
    used[faces.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    return np.ascontiguousarray(vs[used].astype(np.float32)), np.ascontiguousarray(new_id[faces].astype(np.int64))


def tetrahedron():
    vs = np.array([[0.0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], np.float32)
    return vs, np.array([[0, 2, 1], [0, 1, 3], [2, 0, 3]], np.int64)            # (1, 2, 3) is missing


def octahedron():
    vs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    faces = np.array([[2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)       # the four faces at vertex 4 are missing
    return compact(vs, faces)


def many_small():
    m = synth.torus_mesh(96, 96, masks=False)
    seeds = [(6 * i + 2) * 96 + 6 * j + 3 for i in range(14) for j in range(14)]   # 196 vertices, 6 apart: no shared ring
    return cut(m.vs, m.faces, seeds, 0)


def one_large(jitter=0.05):
    m = synth.torus_mesh(96, 96, masks=False, jitter=jitter)
    return cut(m.vs, m.faces, [48 * 96 + 48], 44)


def long_strip():
    m = synth.torus_mesh(1100, 8, masks=False)
    return cut(m.vs, m.faces, [u * 8 + 3 for u in range(1100)], 0)


def planar(n=11, m=10):
    """Open n x m grid in the plane z = 0, every quad cut along the same diagonal (interior valence 6), without the faces
    within one ring of the vertex (5, 5): a hexagonal hole of 12 edges and an outer border of 2 (n - 1) + 2 (m - 1)."""
    i, j = np.meshgrid(np.arange(n), np.arange(m), indexing="ij")
    vs = np.stack([i.ravel(), j.ravel(), np.zeros(n * m)], 1).astype(np.float32)
    faces = []
    for a in range(n - 1):
        for b in range(m - 1):
            v00, v10, v11, v01 = a * m + b, (a + 1) * m + b, (a + 1) * m + b + 1, a * m + b + 1
            faces += [[v00, v10, v11], [v00, v11, v01]]
    return cut(vs, np.asarray(faces, np.int64), [5 * m + 5], 1)


CASES = {"tetrahedron": tetrahedron, "octahedron": octahedron, "many_small": many_small, "one_large": one_large,
         "long_strip": long_strip}
CLOSED = {"many_small": 0, "one_large": 0, "long_strip": 2}          # Euler characteristic once every loop is filled


@functools.lru_cache(maxsize=None)
def case(name):
    """(vs, faces, the oracle's raw fill): computed once, shared, never written to."""
    vs, faces = (CASES[name] if name in CASES else {"planar": planar}[name])()
    want = HO.fill_holes(vs, faces)
    for a in (vs, faces) + want[:4]:
        a.setflags(write=False)
    return vs, faces, want


def diagonal(vs):
    return float(np.linalg.norm(vs.max(0).astype(np.float64) - vs.min(0).astype(np.float64)))


def position_bound(vs):
    """2^-23 max|coordinate|.  Both sides are float64 functions of the same float32 inputs.  The device rounds once to float32:
    at most half an ulp, 2^-24 |x|, and a new vertex is a convex combination of loop vertices, so |x| <= max|coordinate|.
    The float64 sums differ by their order only, n 2^-53 relative: 2^-29 of that half ulp at n = 2^20.  The other half ulp
    is the margin for it (tests/test_holes_fixtures.py: another float64 order takes 0.41 .. 0.46 of the bound, float32 arc
    lengths miss it)."""
    return 2.0 ** -23 * float(np.abs(vs).max())


# ---- loops -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_loops_equal_the_serial_walk(name):
    from semigcn_amd import holes
    vs, faces, want = case(name)
    loops = want[4]
    sizes = [len(l) for l in loops]
    if name == "tetrahedron":
        assert loops == [[1, 2, 3]]
    if name == "octahedron":
        assert sizes == [4]
    if name == "many_small":
        assert len(loops) == 196 and 4 <= min(sizes) and max(sizes) <= 8 and len(set(sizes)) >= 3
    if name == "one_large":
        assert len(loops) == 1 and sizes[0] >= 300
    if name == "long_strip":
        assert sizes == [1100, 1100]
    got = holes.boundary_loops(dev(faces), vs.shape[0])
    ptr, verts = HO.loops_csr(loops)
    assert len(got) == len(loops)
    assert got.ptr.dtype == torch.int64 and got.verts.dtype == torch.int64 and got.sizes.dtype == torch.int64
    assert np.array_equal(got.ptr.cpu().numpy(), ptr)
    assert np.array_equal(got.verts.cpu().numpy(), verts)
    assert np.array_equal(got.sizes.cpu().numpy(), np.diff(ptr))
    # numpy faces are copied to the device
    again = holes.boundary_loops(faces, vs.shape[0])
    assert torch.equal(again.ptr, got.ptr) and torch.equal(again.verts, got.verts)


def test_closed_mesh_has_no_loops():
    from semigcn_amd import holes
    m = synth.octahedron_sphere(1)
    got = holes.boundary_loops(m.faces, m.num_vertices)
    assert len(got) == 0 and got.ptr.cpu().tolist() == [0] and got.verts.numel() == 0
    out = holes.fill_holes((m.vs.astype(np.float32), m.faces))
    assert out.vs.shape[0] == m.num_vertices and torch.equal(out.faces, dev(m.faces)) and out.filled.numel() == 0
    assert not bool(out.inserted.any())


def test_unorderable_boundary_raises():
    from semigcn_amd import holes
    # two fans that share only their apex, vertex 7
    fans = np.array([[7, 0, 1], [7, 1, 2], [7, 2, 3], [7, 4, 5], [7, 5, 6]], np.int64)
    with pytest.raises(HO.Unorderable) as o:
        HO.boundary_loops(fans)
    assert (o.value.n_repeated, o.value.n_bowtie, o.value.vertex) == (0, 1, 7)
    with pytest.raises(ValueError, match=r"0 directed half-edge\(s\).*1 vertex/vertices.*vertex 7$"):
        holes.boundary_loops(fans, 8)
    vs = np.random.default_rng(0).standard_normal((8, 3)).astype(np.float32)
    with pytest.raises(ValueError, match="vertex 7"):
        holes.fill_holes((vs, fans))
    # one face twice
    m = synth.octahedron_sphere(1)
    twice = np.concatenate([m.faces, m.faces[5:6]])
    with pytest.raises(HO.Unorderable) as o:
        HO.boundary_loops(twice)
    assert (o.value.n_repeated, o.value.n_bowtie) == (3, 0)
    with pytest.raises(ValueError, match=rf"3 directed half-edge\(s\).*0 vertex/vertices.*vertex {o.value.vertex}$"):
        holes.boundary_loops(twice, m.num_vertices)
    with pytest.raises(ValueError, match="3 directed"):
        holes.fill_holes((m.vs.astype(np.float32), twice))


# ---- raw construction --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_raw_construction_equals_the_oracle(name):
    """Faces exactly.  Positions: float64 on both sides and one rounding to float32 on the device, within ``position_bound``."""
    from semigcn_amd import holes
    vs, faces, (w_vs, w_faces, w_inserted, w_filled, loops) = case(name)
    V, F = vs.shape[0], faces.shape[0]
    out = holes.fill_holes((dev(vs), dev(faces)), fair_steps=0)
    assert out.vs.dtype == torch.float32 and out.faces.dtype == torch.int64
    assert out.inserted.dtype == torch.bool and out.filled.dtype == torch.bool
    assert (out.num_original_vertices, out.num_original_faces) == (V, F)
    assert tuple(out.vs.shape) == w_vs.shape and tuple(out.faces.shape) == w_faces.shape
    g_vs, g_faces = out.vs.cpu().numpy(), out.faces.cpu().numpy()
    assert np.array_equal(g_faces, w_faces)
    assert np.array_equal(g_faces[:F], faces)
    assert np.array_equal(g_vs[:V].view(np.uint32), vs.view(np.uint32))
    assert np.array_equal(out.inserted.cpu().numpy(), w_inserted) and w_inserted[:V].sum() == 0 and w_inserted[V:].all()
    assert np.array_equal(out.filled.cpu().numpy(), w_filled) and w_filled.all()
    assert len(out.loops) == len(loops)
    err = float(np.abs(g_vs[V:].astype(np.float64) - w_vs[V:]).max()) if w_vs.shape[0] > V else 0.0
    tol = position_bound(vs)
    print(f"{name}: {w_vs.shape[0] - V} new vertices, {w_faces.shape[0] - F} new faces, max|err| {err:.3e}, bound {tol:.3e}")
    assert err <= tol
    if name == "tetrahedron":
        assert g_vs.shape[0] == 4 and g_faces[3].tolist() == [1, 2, 3]
    if name == "octahedron":
        assert g_vs.shape[0] == V + 1 and np.abs(g_vs[V] - vs[loops[0]].astype(np.float64).mean(0)).max() <= tol


@pytest.mark.parametrize("name", list(CLOSED))
def test_filled_mesh_is_closed(name):
    from semigcn_amd import holes, prepare
    from semigcn_amd.meshprep import MeshTopology
    vs, faces, want = case(name)
    out = holes.fill_holes((vs, faces), fair_steps=0)
    g = out.faces.cpu().numpy()
    assert HO.half_edge_stats(g) == (1, 0)                      # every directed half-edge once, each with its opposite
    assert HO.half_edge_stats(faces)[0] == 1
    chi_open, chi = HO.euler_characteristic(faces), HO.euler_characteristic(g)
    assert chi == chi_open + int(out.filled.sum()) == CLOSED[name]
    assert len(holes.boundary_loops(out.faces, out.vs.shape[0])) == 0
    topo = MeshTopology(out.faces, out.vs.shape[0], DEV, with_f2f=True)
    assert topo.manifold and int((topo.f2f >= 0).sum()) == 3 * g.shape[0]
    sm = prepare.laplacian_smooth(out.vs, topo, steps=2)
    assert bool(torch.isfinite(sm).all())


# ---- the cap -----------------------------------------------------------------------------------------------------------
def test_max_hole_edges():
    from semigcn_amd import holes
    vs, faces, want = case("planar")
    sizes = [len(l) for l in want[4]]
    assert sorted(sizes) == [12, 38]
    hole = sizes.index(12)
    V = vs.shape[0]
    capped = holes.fill_holes((vs, faces), max_hole_edges=20, fair_steps=0)
    assert capped.filled.cpu().tolist() == [i == hole for i in range(2)]
    w_vs, w_faces, _, w_filled, _ = HO.fill_holes(vs, faces, max_hole_edges=20)
    assert np.array_equal(capped.faces.cpu().numpy(), w_faces) and w_filled.tolist() == capped.filled.cpu().tolist()
    assert capped.vs.shape[0] == V + 12 // 2 + 1 == w_vs.shape[0]                     # rings [12, 6, 1]
    assert np.abs(capped.vs.cpu().numpy().astype(np.float64) - w_vs).max() <= position_bound(vs)
    rest = holes.boundary_loops(capped.faces, capped.vs.shape[0])
    assert rest.sizes.cpu().tolist() == [38]
    assert not bool(holes.fill_holes((vs, faces), max_hole_edges=11, fair_steps=0).filled.any())
    assert bool(holes.fill_holes((vs, faces), max_hole_edges=38, fair_steps=0).filled.all())
    both = holes.fill_holes((vs, faces), fair_steps=0)
    assert both.filled.cpu().tolist() == [True, True] and np.array_equal(both.faces.cpu().numpy(), want[1])
    assert HO.half_edge_stats(both.faces.cpu().numpy()) == (1, 0) and HO.euler_characteristic(both.faces.cpu().numpy()) == 2


def test_plan_again_on_the_same_plan():
    """``plan`` drops the sizes of the call before it: uncapped, capped at 20, uncapped again on ONE FillPlan, each emit against
    the oracle result test_max_hole_edges asserts (faces and ``filled`` exactly, positions within ``position_bound``)."""
    from semigcn_amd import capi
    vs, faces, uncapped = case("planar")
    V = vs.shape[0]
    d_vs = dev(vs)
    plan = capi.FillPlan(dev(faces), V)
    try:
        plan.plan(None)
        for cap, want in ((20, HO.fill_holes(vs, faces, max_hole_edges=20)), (None, uncapped)):
            w_vs, w_faces, _, w_filled, _ = want
            Vn, Fn = plan.plan(cap)
            assert (Vn, Fn) == (w_vs.shape[0] - V, w_faces.shape[0] - faces.shape[0])
            new_vs = torch.empty((Vn, 3), dtype=torch.float32, device=DEV)
            new_faces = torch.empty((Fn, 3), dtype=torch.int64, device=DEV)
            filled = plan.emit(d_vs, new_vs, new_faces)
            assert np.array_equal(new_faces.cpu().numpy(), w_faces[faces.shape[0]:])
            assert np.array_equal(filled.cpu().numpy(), w_filled)
            assert np.abs(new_vs.cpu().numpy().astype(np.float64) - w_vs[V:]).max() <= position_bound(vs)
        assert w_filled.all() and Vn > 12 // 2 + 1                  # the last round filled the border loop as well
    finally:
        torch.cuda.current_stream().synchronize()                   # the plan's buffers are freed with it
        plan.close()


# ---- the offset tables at their edges ----------------------------------------------------------------------------------
def cycling(L):
    return [3 + i % 21 for i in range(L)]


FANS = {"s13": lambda: HF.fans(HF.S13), "s13_perm": lambda: HF.fans(HF.S13, perm=5), "ends_open": lambda: HF.fans([40, 3, 9, 40]),
        "coincident": lambda: HF.coincident()[:2]}


@functools.lru_cache(maxsize=None)
def fan_case(name, cap=None):
    """(vs, faces, the oracle's raw fill at ``cap``) of FANS[name], of "single<n>" or of "many<L>": computed once, read-only."""
    if name.startswith("single"):
        vs, faces = HF.fans([int(name[6:])])
    elif name.startswith("many"):
        vs, faces = HF.fans(cycling(int(name[4:])))
    else:
        vs, faces = FANS[name]()
    want = HO.fill_holes(vs, faces, cap)
    for a in (vs, faces) + want[:4]:
        a.setflags(write=False)
    return vs, faces, want


def check_patches(label, vs, faces, want, new_vs, new_faces, filled):
    """New faces and ``filled`` exactly, new positions finite and within ``position_bound``; returns and prints the error."""
    w_vs, w_faces, _, w_filled, _ = want
    V, F = vs.shape[0], faces.shape[0]
    assert tuple(new_vs.shape) == (w_vs.shape[0] - V, 3) and tuple(new_faces.shape) == (w_faces.shape[0] - F, 3)
    assert np.array_equal(new_faces.cpu().numpy(), w_faces[F:])
    assert np.array_equal(filled.cpu().numpy(), w_filled)
    g = new_vs.cpu().numpy()
    assert np.isfinite(g).all()
    err = float(np.abs(g.astype(np.float64) - w_vs[V:]).max()) if g.shape[0] else 0.0
    tol = position_bound(vs)
    print(f"{label}: {g.shape[0]} new vertices, {new_faces.shape[0]} new faces, max|err| {err:.3e} = {err / tol:.2f} of the "
          f"bound {tol:.3e}")
    assert err <= tol
    return err


def check_fill(name, cap):
    """``fill_holes`` without fairing against the oracle: loops the serial walk, faces, ``filled``, ``inserted`` and sizes
    exactly, the originals bit for bit, positions within the bound, and the loops that stay open exactly the unfilled ones."""
    from semigcn_amd import holes
    vs, faces, want = fan_case(name, cap)
    w_vs, w_faces, w_inserted, w_filled, loops = want
    V, F = vs.shape[0], faces.shape[0]
    out = holes.fill_holes((dev(vs), dev(faces)), max_hole_edges=cap, fair_steps=0)
    ptr, verts = HO.loops_csr(loops)
    assert np.array_equal(out.loops.ptr.cpu().numpy(), ptr) and np.array_equal(out.loops.verts.cpu().numpy(), verts)
    assert (out.num_original_vertices, out.num_original_faces) == (V, F)
    assert np.array_equal(out.faces[:F].cpu().numpy(), faces)
    assert np.array_equal(out.vs[:V].cpu().numpy().view(np.uint32), vs.view(np.uint32))
    assert np.array_equal(out.inserted.cpu().numpy(), w_inserted)
    check_patches(f"{name} cap {cap}", vs, faces, want, out.vs[V:], out.faces[F:], out.filled)
    rest = holes.boundary_loops(out.faces, out.vs.shape[0])
    open_loops = [l for l, f in zip(loops, w_filled) if not f]
    assert rest.sizes.cpu().tolist() == [len(l) for l in open_loops]
    assert np.array_equal(rest.verts.cpu().numpy(), HO.loops_csr(open_loops)[1])
    return out, want


@pytest.mark.parametrize("cap", [None, 20, 9, 3, 2])
def test_loops_that_add_nothing_between_filled_ones(cap):
    """S13: triangles (a face, no vertex, no ring table) and, under a cap, open loops (nothing at all) before, between and
    after filled loops: runs of equal entries in all three offset tables.  Cap 3 fills triangles only (faces without a ring
    table), cap 2 nothing."""
    out, want = check_fill("s13", cap)
    V, F = fan_case("s13", cap)[0].shape[0], fan_case("s13", cap)[1].shape[0]
    assert (out.vs.shape[0] - V, out.faces.shape[0] - F) == HF.S13_COUNTS[cap]
    assert out.filled.cpu().tolist() == [cap is None or n <= cap for n in HF.S13]


def test_open_loops_first_and_last():
    out, _ = check_fill("ends_open", 20)
    assert out.filled.cpu().tolist() == [False, True, True, False]


@pytest.mark.parametrize("cap", [None, 20])
def test_loops_interleaved_in_id_space(cap):
    _, (_, _, _, _, loops) = check_fill("s13_perm", cap)
    assert [len(l) for l in loops] != HF.S13 and sorted(len(l) for l in loops) == sorted(HF.S13)


def test_one_plan_through_four_caps():
    """20, 3, None, 2 on ONE FillPlan: tables that shrink to faces only, grow to everything and shrink to nothing."""
    from semigcn_amd import capi
    vs, faces = fan_case("s13", None)[:2]
    V = vs.shape[0]
    d_vs = dev(vs)
    with capi.FillPlan(dev(faces), V) as plan:
        for cap in (20, 3, None, 2):
            want = fan_case("s13", cap)[2]
            Vn, Fn = plan.plan(cap)
            assert (Vn, Fn) == HF.S13_COUNTS[cap]
            new_vs = torch.empty((Vn, 3), dtype=torch.float32, device=DEV)
            new_faces = torch.empty((Fn, 3), dtype=torch.int64, device=DEV)
            filled = plan.emit(d_vs, new_vs, new_faces)
            check_patches(f"one plan, cap {cap}", vs, faces, want, new_vs, new_faces, filled)
        torch.cuda.current_stream().synchronize()                   # the plan's buffers are freed with it


@pytest.mark.parametrize("cap", [None, 9])
@pytest.mark.parametrize("L", [255, 256, 257, 1500])
def test_many_loops_across_a_block_of_the_per_loop_kernels(L, cap):
    """One thread per loop over L + 1 entries: L = 255 is the last single block, 256 the first with a second one."""
    out, want = check_fill(f"many{L}", cap)
    assert len(out.loops) == L and int(out.filled.sum()) == sum(cap is None or n <= cap for n in cycling(L))


@pytest.mark.parametrize("n", list(HF.SINGLE_COUNTS))
def test_single_loop_at_a_chunk_and_at_a_power_of_two(n):
    """n = 256: exactly one chunk of the arc-length scan; 256, 512, 1024: the pointer jumping's ``span < nb`` round count at
    a power of two, with one less and one more."""
    out, _ = check_fill(f"single{n}", None)
    vs, faces = fan_case(f"single{n}")[:2]
    assert (out.vs.shape[0] - vs.shape[0], out.faces.shape[0] - faces.shape[0]) == HF.SINGLE_COUNTS[n]
    assert HO.half_edge_stats(out.faces.cpu().numpy()) == (1, 0)


def test_zero_length_segments_and_a_loop_of_perimeter_zero():
    out, (w_vs, _, _, _, loops) = check_fill("coincident", None)
    vs = fan_case("coincident")[0]
    V = vs.shape[0]
    first = V + sum(HO.ring_sizes(24)[1:])
    mine = out.vs[first:first + sum(HO.ring_sizes(12)[1:])].cpu().numpy()
    assert mine.shape[0] == 7 and np.array_equal(mine.view(np.uint32), np.repeat(vs[loops[1][:1]], 7, 0).view(np.uint32))
    assert bool(torch.isfinite(out.vs).all())
    # the loops near the origin on their own: their bound is 1e4 times tighter than the one the far loop sets
    near = np.arange(V, first + 7)
    tol = 2.0 ** -23 * float(np.abs(vs[loops[0] + loops[1]]).max())
    err = float(np.abs(out.vs.cpu().numpy()[near].astype(np.float64) - w_vs[near]).max())
    print(f"coincident, loops 0 and 1: max|err| {err:.3e} = {err / tol:.2f} of the bound {tol:.3e}")
    assert err <= tol


# ---- fairing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("steps", [1, 30])
def test_fairing_is_the_existing_smoothing(steps):
    """Same kernel, same inputs: bit for bit."""
    from semigcn_amd import holes, prepare
    for name in ("one_large", "planar"):
        vs, faces, _ = case(name)
        cap = 20 if name == "planar" else None
        raw = holes.fill_holes((vs, faces), max_hole_edges=cap, fair_steps=0)
        fair = holes.fill_holes((vs, faces), max_hole_edges=cap, fair_steps=steps)
        want = prepare.laplacian_smooth(raw.vs, raw.faces, steps=steps, movable=raw.inserted)
        assert torch.equal(fair.vs.view(torch.int32), want.view(torch.int32))
        assert torch.equal(fair.faces, raw.faces) and torch.equal(fair.inserted, raw.inserted)
        V = raw.num_original_vertices
        assert torch.equal(fair.vs[:V].view(torch.int32), dev(vs).view(torch.int32))
        assert not torch.equal(fair.vs[V:], raw.vs[V:])
    if steps == 30:
        assert torch.equal(holes.fill_holes((vs, faces), max_hole_edges=cap).vs, fair.vs)      # the default


def test_faired_vertices_stay_in_the_plane_and_in_the_hole():
    from semigcn_amd import holes
    vs, faces, want = case("planar")
    out = holes.fill_holes((vs, faces), max_hole_edges=20)
    V = vs.shape[0]
    new = out.vs[V:].cpu().numpy().astype(np.float64)
    assert new.shape[0] == 7
    assert np.abs(new[:, 2]).max() <= 1e-5 * diagonal(vs)
    loop = next(l for l in want[4] if len(l) == 12)
    poly = vs[loop].astype(np.float64)                                   # convex, one orientation all the way round
    edge = np.roll(poly, -1, 0) - poly
    side = edge[None, :, 0] * (new[:, None, 1] - poly[None, :, 1]) - edge[None, :, 1] * (new[:, None, 0] - poly[None, :, 0])
    assert (side > 0).all() or (side < 0).all()
    assert np.abs(side).min() > 0.25                                     # well inside, not on the border


# ---- hand-over ---------------------------------------------------------------------------------------------------------
def test_filled_mesh_feeds_prepare_inputs_and_the_network():
    from semigcn_amd import holes, prepare
    from semigcn_amd.networks import SingleScaleGCN
    vs, faces, _ = case("planar")
    out = holes.fill_holes((vs, faces), max_hole_edges=20)
    V = vs.shape[0]
    p = prepare.prepare_inputs(initial=(out.vs, out.faces), original=(vs, faces))
    mask = p.v_mask.cpu().numpy()
    assert mask[:V].all() and not mask[V:].any()
    # the first ring sits about one edge length from the border: far from eps = 0.2 edge lengths
    surf_dist = PO.scan_distances(p.initial_vs.cpu().numpy()[V:], p.original_vs.cpu().numpy(), faces)
    print(f"scale {float(p.scale):.4f}; inserted vertices: distance to the scan {surf_dist.min():.3f} .. {surf_dist.max():.3f}")
    assert surf_dist.min() > 2 * prepare.EPSILON
    assert np.array_equal(p.f_mask.cpu().numpy(), np.arange(out.faces.shape[0]) < faces.shape[0])
    batch = p.mesh_batch(dm_size=2, kn=(1,), rng=np.random.RandomState(3))
    torch.manual_seed(1)
    net = SingleScaleGCN(DEV).to(DEV)
    net.train()
    pos = net(batch.data, batch.dummy_masks[:, :1].contiguous())
    assert tuple(pos.shape) == (out.vs.shape[0], 3) and bool(torch.isfinite(pos).all())


# ---- an irregular loop -------------------------------------------------------------------------------------------------
def patch_edge_ratio(vs, faces, F, loop):
    """longest edge of the patch faces (faces[F:]) over the mean edge of the border loop"""
    vs = np.asarray(vs, np.float64)
    border = np.linalg.norm(np.roll(vs[loop], -1, 0) - vs[loop], axis=1).mean()
    return float(HO.edge_lengths(vs, faces[F:]).max() / border)


def test_irregular_loop_after_fairing():
    """The large disc on a torus with jitter 0.2: a loop of 334 edges between 0.47 and 3.68 long (mean 2.07) around a hole
    that takes most of the torus.  The ratio longest patch edge / mean border edge is not asserted against a number chosen
    in advance: the oracle's construction, faired by the float64 smoothing of tests/prepare_oracle.py, gives the value
    (4.09 here; unfaired 24.04 -- DESIGN.md section 7) and the device must agree within 1 %: the same arithmetic in float32
    and another summation order."""
    from semigcn_amd import holes
    vs, faces = one_large(jitter=0.2)
    w_vs, w_faces, w_inserted, _, loops = HO.fill_holes(vs, faces)
    assert len(loops) == 1 and len(loops[0]) >= 300
    V, F = vs.shape[0], faces.shape[0]
    out = holes.fill_holes((vs, faces))
    g_vs, g_faces = out.vs.cpu().numpy(), out.faces.cpu().numpy()
    assert np.array_equal(g_faces, w_faces)
    p = g_vs[g_faces[F:]].astype(np.float64)
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    # degenerate = an area that float32 rounding of the coordinates could produce: 1e-7 x |coordinate| (~50) on edges of ~2
    assert all(len(set(f)) == 3 for f in g_faces[F:].tolist()) and area.min() > 1e-5 * area.mean()
    want = patch_edge_ratio(PO.smooth(w_vs, w_faces, 30, movable=w_inserted), w_faces, F, loops[0])
    got = patch_edge_ratio(g_vs, g_faces, F, loops[0])
    raw = patch_edge_ratio(w_vs, w_faces, F, loops[0])
    print(f"longest patch edge / mean border edge: device {got:.4f}, oracle {want:.4f} (unfaired oracle {raw:.4f}); "
          f"smallest patch face area / mean {area.min() / area.mean():.3e}")
    assert abs(got - want) <= 0.01 * want


# ---- command line ------------------------------------------------------------------------------------------------------
def test_command_line(tmp_path, capsys):
    from semigcn_amd import holes, prepare
    from semigcn_amd.evaluate import read_obj
    vs, faces, want = case("planar")
    scan, dst = str(tmp_path / "a.obj"), str(tmp_path / "a_filled.obj")
    prepare.write_obj(scan, vs, faces)
    assert holes.main(["--scan", scan, "--out", dst, "--max-hole-edges", "20", "--fair-steps", "0"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert (rec["n_loops"], rec["n_filled"], rec["n_inserted_vertices"], rec["n_inserted_faces"]) == (2, 1, 7, 24)
    assert all(rec[k] >= 0.0 for k in ("loops_ms", "emit_ms", "fair_ms"))
    f_vs, f_faces = read_obj(dst)
    ref = holes.fill_holes((vs, faces), max_hole_edges=20, fair_steps=0)
    assert np.array_equal(f_faces, ref.faces.cpu().numpy()) and np.array_equal(f_vs.view(np.uint32), ref.vs.cpu().numpy().view(np.uint32))
    assert holes.main(["--torus", "48", "32", "--cut", "2"]) == 0
    rec = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert rec["n_loops"] == 2 and rec["n_filled"] == 2 and rec["n_inserted_vertices"] > 0 and rec["fair_steps"] == 30
    with pytest.raises(SystemExit):
        holes.main(["--out", dst])
