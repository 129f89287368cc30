"""semigcn_amd.mesh_common, and the lifetime rule of the objects the mesh stages build.

Without a device: the input check that comes before any device is asked for, the stage timer switched off, and the OBJ
writer and reader (one implementation under three names; the bytes are pinned against the format written out here).

On the device (``gpu``), on the octahedron (V = 6, F = 8) and the octahedron without one face (a hole of 3 edges): a
``Surface`` and every plan used as a context manager gives what the same calls followed by ``close()`` give, is closed
after the block, and is closed when an exception leaves the block; the stage timer's sums are recomputed from its own
events; ``refine_mesh`` measures the stages it always measured, and measuring changes nothing it returns."""
import importlib.util
import sys

import numpy as np
import pytest
import torch

import remesh_oracle as RO
from semigcn_amd import capi, evaluate, mesh_common, prepare, synth
from semigcn_amd.mesh_common import Stages, check_mesh

DEV = "cuda:0"


def octahedron(open_=False):
    vs = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
    faces = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int64)
    return vs, faces[:7] if open_ else faces


# ---- check_mesh -----------------------------------------------------------------------------------------------------------
class _Mesh:
    def __init__(self, vs, faces):
        self.vs, self.faces = vs, faces


def test_check_mesh_accepts_the_pair_and_the_object_form():
    vs, faces = octahedron()
    for v, f in ((vs, faces), (torch.from_numpy(vs), torch.from_numpy(faces)), (vs.astype(np.float64), faces.astype(np.int32))):
        for got in (check_mesh(v, f), check_mesh((v, f)), check_mesh([v, f]), check_mesh(_Mesh(v, f))):
            assert got[0] is v and got[1] is f
    with pytest.raises(TypeError, match="expected a mesh"):
        check_mesh(vs)
    with pytest.raises(TypeError, match="expected a mesh"):
        check_mesh((vs, faces, faces))


@pytest.mark.parametrize("dtypes", [True, False])
@pytest.mark.parametrize("wrap", [np.asarray, torch.from_numpy], ids=["array", "tensor"])
def test_check_mesh_rejects_a_wrong_rank_and_a_wrong_last_dimension(wrap, dtypes):
    vs, faces = octahedron()
    for bad in (vs.reshape(-1), vs[:, :2], vs.reshape(2, 3, 3), np.zeros((6, 4), np.float32)):
        with pytest.raises(ValueError, match="vs must be"):
            check_mesh(wrap(np.ascontiguousarray(bad)), wrap(faces), dtypes=dtypes)
    for bad in (faces.reshape(-1), faces[:, :2], faces.reshape(2, 4, 3), np.zeros((8, 4), np.int64)):
        with pytest.raises(ValueError, match="faces must be"):
            check_mesh((wrap(vs), wrap(np.ascontiguousarray(bad))), dtypes=dtypes)


@pytest.mark.parametrize("wrap", [np.asarray, torch.from_numpy], ids=["array", "tensor"])
def test_check_mesh_dtypes(wrap):
    vs, faces = octahedron()
    int_vs, float_faces = wrap(vs.astype(np.int64)), wrap(faces.astype(np.float32))
    with pytest.raises(ValueError, match="vs must hold floats"):
        check_mesh(int_vs, wrap(faces))
    with pytest.raises(ValueError, match="faces must hold integers"):
        check_mesh(wrap(vs), float_faces)
    with pytest.raises(ValueError, match="faces must hold integers"):
        check_mesh(_Mesh(wrap(vs), float_faces), dtypes=True)
    for got in (check_mesh(int_vs, float_faces, dtypes=False), check_mesh(_Mesh(int_vs, float_faces), dtypes=False)):
        assert got[0] is int_vs and got[1] is float_faces            # repair checks shapes only


# ---- Stages, switched off -------------------------------------------------------------------------------------------------
def test_stages_switched_off_makes_no_device_call():
    st = Stages(torch.device("cuda", 0), False)          # there may be no such device: nothing may ask for it
    for name in ("a", None, "b", "a"):
        st.mark(name)
    assert st.result() is None and st.marks == []


def test_stages_record_rounds_to_four_places():
    assert Stages.record({"a_ms": 1.23456789, "b_ms": 0.00004}) == {"a_ms": 1.2346, "b_ms": 0.0}


# ---- OBJ ------------------------------------------------------------------------------------------------------------------
def _obj_bytes(vs, faces):
    """The format both writers of the parent wrote, restated."""
    text = "".join("v %.9g %.9g %.9g\n" % (float(p[0]), float(p[1]), float(p[2])) for p in vs)
    return (text + "".join("f %d %d %d\n" % (int(t[0]) + 1, int(t[1]) + 1, int(t[2]) + 1) for t in faces)).encode()


def test_synth_module_imports_where_torch_cannot_be_imported(monkeypatch):
    """synth.py executed as a module of its own with ``import torch`` made to fail: its module level needs numpy alone
    (the writer it shares with mesh_common is looked up when called)."""
    monkeypatch.setitem(sys.modules, "torch", None)                  # ``import torch`` now raises ImportError
    with pytest.raises(ImportError):
        importlib.import_module("torch")
    spec = importlib.util.spec_from_file_location("synth_without_torch", synth.__file__)
    alone = importlib.util.module_from_spec(spec)
    monkeypatch.setitem(sys.modules, spec.name, alone)               # dataclasses look their module up by name
    spec.loader.exec_module(alone)
    m = alone.torus_mesh(6, 5, masks=False)
    assert m.vs.shape == (30, 3) and m.faces.shape == (60, 3)


def test_check_mesh_keeps_the_errors_of_a_missing_faces_argument():
    from semigcn_amd import remesh, repair
    vs, faces = octahedron()
    for fn in (lambda: remesh.split_long_edges(vs, None, 1.0), lambda: remesh.flip_edges(vs, None),
               lambda: remesh.collapse_short_edges(vs, None, 1.0), lambda: remesh.relax_project(vs, None, (vs, faces))):
        with pytest.raises(ValueError, match="faces must be"):
            fn()
    with pytest.raises(TypeError, match="expected a mesh"):           # repair: faces=None means "vs is the mesh"
        repair.self_intersections(vs)


def test_one_obj_writer_and_one_reader_under_three_names(tmp_path):
    assert prepare.write_obj is mesh_common.write_obj and evaluate.read_obj is mesh_common.read_obj
    m = synth.torus_mesh(6, 5, masks=False)
    vs32 = m.vs.astype(np.float32)
    a, b = str(tmp_path / "a.obj"), str(tmp_path / "b.obj")
    for vs in (vs32, m.vs):                                          # float32, and the float64 the golden script passes
        synth.write_obj(a, vs, m.faces)
        prepare.write_obj(b, vs, m.faces)
        want = _obj_bytes(vs, m.faces)
        assert open(a, "rb").read() == want and open(b, "rb").read() == want
    prepare.write_obj(b, torch.from_numpy(vs32), torch.from_numpy(m.faces))      # tensors write the same bytes
    assert open(b, "rb").read() == _obj_bytes(vs32, m.faces)
    synth.write_obj(a, vs32, m.faces)
    got_vs, got_faces = evaluate.read_obj(a)
    assert got_vs.dtype == np.float32 and got_vs.tobytes() == vs32.tobytes()
    assert got_faces.dtype == np.int64 and np.array_equal(got_faces, m.faces)
    for write in (synth.write_obj, prepare.write_obj):               # vertices only
        write(a, vs32[:7])
        assert open(a, "rb").read() == _obj_bytes(vs32[:7], [])
        got_vs, got_faces = mesh_common.read_obj(a)
        assert got_vs.tobytes() == vs32[:7].tobytes() and got_faces.shape == (0, 3)


# ---- on the device: the lifetime rule -------------------------------------------------------------------------------------
def _dev(x):
    return torch.from_numpy(np.array(x)).to(DEV)


_PROBES = np.array([[0.3, 0.2, 0.1], [2.0, -1.0, 0.5], [0.0, 0.0, 0.0], [-0.4, 0.4, -0.4], [1.0, 0.0, 0.0]], np.float32)


def _surface_calls(s, vs, faces):
    return s.query(_dev(_PROBES)) + s.query(_dev(_PROBES), signed=False)


def _smooth_calls(p, vs, faces):
    return (p.run(vs, 3), p.run(vs, 1, movable=torch.arange(vs.shape[0], device=DEV) % 2 == 0))


def _fill_calls(p, vs, faces):
    ptr, verts = p.loops()
    n_vs, n_faces = p.plan()
    new_vs = torch.empty((n_vs, 3), dtype=torch.float32, device=DEV)
    new_faces = torch.empty((n_faces, 3), dtype=torch.int64, device=DEV)
    return (ptr, verts, n_vs, n_faces, p.emit(vs, new_vs, new_faces), new_vs, new_faces, p.orderable, p.num_loops)


def _parts_calls(p, vs, faces):
    labels, count = p.labels()
    kept = p.select(torch.ones(p.num_components, dtype=torch.bool, device=DEV))
    return (labels, count, kept, p.largest, p.n_degenerate) + p.emit(vs)


def _remesh_calls(p, vs, faces):
    assert p.valid
    split = p.split(1.0, 4)                               # len2 = 2 of every edge is long
    return split + p.flip(4) + p.export()


#: name -> (make(vs, faces), the calls, one call that needs the object open)
OWNERS = {
    "Surface": (lambda vs, faces: evaluate.Surface(vs, faces), _surface_calls, lambda s: s.query(_dev(_PROBES))),
    "SmoothPlan": (lambda vs, faces: capi.SmoothPlan(faces, vs.shape[0]), _smooth_calls,
                   lambda p: p.run(torch.zeros((6, 3), device=DEV), 1)),
    "FillPlan": (lambda vs, faces: capi.FillPlan(faces, vs.shape[0]), _fill_calls, lambda p: p.loops()),
    "PartsPlan": (lambda vs, faces: capi.PartsPlan(faces, vs.shape[0]), _parts_calls, lambda p: p.labels()),
    "RemeshPlan": (lambda vs, faces: capi.RemeshPlan(vs, faces), _remesh_calls, lambda p: p.export()),
}


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
        else:
            assert x == y


@pytest.mark.gpu
@pytest.mark.parametrize("open_", [False, True], ids=["closed", "hole"])
@pytest.mark.parametrize("name", list(OWNERS))
def test_with_block_equals_explicit_close_and_closes(name, open_):
    make, calls, needs_open = OWNERS[name]
    vs, faces = (_dev(a) for a in octahedron(open_))
    if name == "FillPlan":
        with capi.FillPlan(faces, 6) as p:
            assert p.num_loops == (1 if open_ else 0)
    obj = make(vs, faces)
    want = calls(obj, vs, faces)
    torch.cuda.current_stream(obj.device).synchronize()
    obj.close()
    made = make(vs, faces)
    with made as obj:
        assert obj is made
        got = calls(obj, vs, faces)
    _same(got, want)
    with pytest.raises(capi.SemigcnLibraryError, match="is closed"):
        needs_open(obj)
    obj.close()                                                       # closing twice is still harmless
    with pytest.raises(KeyError, match="from inside the block"):
        with make(vs, faces) as obj:
            calls(obj, vs, faces)
            raise KeyError("from inside the block")
    with pytest.raises(capi.SemigcnLibraryError, match="is closed"):
        needs_open(obj)


def _work(n=1):
    a = torch.ones((1024, 1024), device=DEV)
    for _ in range(n):
        a = a @ a * 1e-3
    return a


@pytest.mark.gpu
def test_stages_sum_by_name_and_none_restarts_the_clock():
    st = Stages(torch.device(DEV), True)
    for name, n in (("a", 1), (None, 8), ("b", 1), ("a", 2)):
        _work(n)
        st.mark(name)
    got = st.result()
    ev = [e for _, e in st.marks]
    assert [n for n, _ in st.marks] == [None, "a", None, "b", "a"]
    assert list(got) == ["a_ms", "b_ms"]
    assert got["a_ms"] == ev[0].elapsed_time(ev[1]) + ev[3].elapsed_time(ev[4])
    assert got["b_ms"] == ev[2].elapsed_time(ev[3])
    gap = ev[1].elapsed_time(ev[2])                                  # the eight products that nobody is charged for
    assert gap > 0.0 and got["a_ms"] > 0.0 and got["b_ms"] > 0.0
    assert got["a_ms"] + got["b_ms"] == pytest.approx(ev[0].elapsed_time(ev[4]) - gap, abs=1e-3)
    assert st.result() == got                                        # asking again does not add up again


@pytest.mark.gpu
@pytest.mark.parametrize("collapse", [False, True], ids=["plain", "collapse"])
def test_refine_mesh_timings_change_nothing_but_stage_ms(collapse):
    from semigcn_amd import remesh
    vs, faces = RO.stretched_torus(12, 8)
    kw = dict(target=0.6 * RO.median_edge(vs, faces), iterations=2, collapse=collapse)
    plain = remesh.refine_mesh((vs, faces), **kw)
    timed = remesh.refine_mesh((vs, faces), timings=True, **kw)
    assert plain.stage_ms is None
    want = ["surface_ms", "report_ms", "split_ms"] + (["collapse_ms"] if collapse else []) + ["flip_ms", "relax_ms"]
    assert list(timed.stage_ms) == want
    assert all(np.isfinite(v) and v > 0.0 for v in timed.stage_ms.values())
    assert torch.equal(timed.vs, plain.vs) and torch.equal(timed.faces, plain.faces)
    assert timed.report == plain.report
    if collapse:
        assert timed.parents is None and plain.parents is None
    else:
        assert torch.equal(timed.parents, plain.parents)
