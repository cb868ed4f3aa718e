"""bdm_amd/mesh_batch.py on the host: the tail fill_holes and the two simplifiers share (the staging of the colours, the packed
outputs and their split back per mesh, the wrapping of host batches that mix files with and without colours, the walk over a tree
of mesh files).  No GPU: the device refusal is asserted as such, and where rows are wanted it is patched away."""
import numpy as np
import pytest
import torch

from bdm_amd import _lib as L
from bdm_amd import mesh_batch as MB
from bdm_amd import mesh_decimate as MD
from bdm_amd import mesh_fill as MF
from bdm_amd.ragged import first


def test_the_moved_names_are_still_those_of_the_two_modules():
    assert MF._check_colors is MD._check_colors is MB._check_colors and MF._round_uint8 is MD._round_uint8 is MB._round_uint8
    assert MF.MAX_C == MD.MAX_C == MB.MAX_C == 16


def test_staging_at_no_channel_and_at_three(monkeypatch):
    none = MB.stage_attrs(None, 0, torch.device("cpu"))   # the colours are not read at C = 0
    assert none.shape == (1, 1) and none.dtype == torch.float32 and float(none.abs().sum()) == 0.0
    cols = [torch.arange(6, dtype=torch.uint8).view(2, 3), torch.zeros(0, 3, dtype=torch.float64), torch.tensor([[0.5, -1.25, 3.0]], dtype=torch.float16)]
    with pytest.raises(L.BdmHipError):   # host tensors are refused before anything is staged
        MB.stage_attrs(cols, 3, torch.device("cpu"))
    monkeypatch.setattr(L, "ptr", lambda t: 0)
    rows = MB.stage_attrs(cols, 3, torch.device("cpu"))
    assert rows.dtype == torch.float32 and rows.is_contiguous() and rows.shape == (2 + 0 + 1 + 1, 3)   # one unread row behind them
    assert torch.equal(rows, torch.tensor([[0, 1, 2], [3, 4, 5], [0.5, -1.25, 3.0], [0, 0, 0]], dtype=torch.float32))
    monkeypatch.setattr(L, "ptr", lambda t: 0)
    alone = MB.stage_attrs([torch.zeros(0, 3)], 3, torch.device("cpu"))
    assert alone.shape == (1, 3)   # never empty


def test_outputs_are_zeroed_and_never_empty():
    v, a, f = MB.alloc_outputs(first([2, 0, 3]), first([1, 0, 0]), 3, torch.device("cpu"))
    assert (v.shape, a.shape, f.shape) == ((5, 3), (5, 3), (1, 3)) and (v.dtype, a.dtype, f.dtype) == (torch.float32, torch.float32, torch.int32)
    assert not v.any() and not a.any() and not f.any()
    v, a, f = MB.alloc_outputs(first([0]), first([0]), 0, torch.device("cpu"))
    assert (v.shape, a.shape, f.shape) == ((1, 3), (1, 1), (1, 3))


def _packed():
    """Two meshes' worth of packed outputs: 3 + 2 vertex rows, 2 + 1 face rows, three channels that need rounding and clamping."""
    verts_out = torch.arange(15, dtype=torch.float32).view(5, 3) / 4
    attrs_out = torch.tensor([[0.5, 1.5, 2.5], [254.5, 255.5, 300.0], [-3.0, float("nan"), 7.49], [1.0, 2.0, 3.0], [0.1, 0.2, 0.3]])
    faces_out = torch.tensor([[0, 1, 2], [2, 1, 0], [1, 0, 1]], dtype=torch.int32)
    return verts_out, attrs_out, faces_out, first([3, 2]), first([2, 1])


def test_split_replaces_the_rows_and_casts_the_colours_to_what_was_given():
    verts_out, attrs_out, faces_out, ovf, off = _packed()
    faces_list = [torch.zeros(4, 3, dtype=torch.int64), torch.zeros(9, 3, dtype=torch.int32)]
    for dtype in (torch.uint8, torch.float16, torch.float64):
        cols = [torch.zeros(7, 3, dtype=dtype), torch.zeros(4, 3, dtype=torch.float32)]
        out_v, out_f, out_c = MB.split_outputs(verts_out, attrs_out, faces_out, ovf, off, faces_list, cols, 3)
        assert torch.equal(out_v[0], verts_out[:3]) and torch.equal(out_v[1], verts_out[3:])
        assert [f.dtype for f in out_f] == [torch.int64, torch.int32] and torch.equal(out_f[0], faces_out[:2].long()) and torch.equal(out_f[1], faces_out[2:])
        assert out_c[0].dtype == dtype and out_c[1].dtype == torch.float32 and torch.equal(out_c[1], attrs_out[3:])
        if dtype == torch.uint8:   # to nearest, halves to even, clamped, NaN -> 0
            assert out_c[0].tolist() == [[0, 2, 2], [254, 255, 255], [0, 0, 7]]
        else:
            want = attrs_out[:3].to(dtype)
            assert torch.equal(torch.nan_to_num(out_c[0], nan=-1.0), torch.nan_to_num(want, nan=-1.0))
    assert len(MB.split_outputs(verts_out, attrs_out, faces_out, ovf, off, faces_list, None, 0)) == 2   # no colours given: none returned


def test_split_of_colours_given_without_a_channel_is_zero_width():
    verts_out, attrs_out, faces_out, ovf, off = _packed()
    faces_list = [torch.zeros(4, 3, dtype=torch.int64), torch.zeros(9, 3, dtype=torch.int64)]
    cols = [torch.zeros(7, 0, dtype=torch.uint8), torch.zeros(4, 0, dtype=torch.float64)]
    _, _, out_c = MB.split_outputs(verts_out, attrs_out[:, :1], faces_out, ovf, off, faces_list, cols, 0)
    assert [tuple(c.shape) for c in out_c] == [(3, 0), (2, 0)] and [c.dtype for c in out_c] == [torch.uint8, torch.float64]
    old = [torch.zeros(2, 3), torch.zeros(2, 3)]   # appended to two old rows each: 1 and 0 new rows
    _, _, out_c = MB.split_outputs(verts_out, attrs_out[:, :1], faces_out, ovf, off, [f[:1] for f in faces_list], [c[:2] for c in cols], 0, old_verts=old)
    assert [tuple(c.shape) for c in out_c] == [(3, 0), (2, 0)] and [c.dtype for c in out_c] == [torch.uint8, torch.float64]


def test_split_behind_old_rows_keeps_the_inputs_as_they_were_given():
    verts_out, attrs_out, faces_out, ovf, off = _packed()
    old_v = [torch.tensor([[9.0, 9, 9], [8, 8, 8]]), torch.tensor([[7.0, 7, 7]], dtype=torch.float64)]
    old_f = [torch.tensor([[2 ** 40, 0, 1]]), torch.tensor([[5, 6, 7]], dtype=torch.int32)]   # an index that does not survive int32
    old_c = [torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.uint8), torch.tensor([[0.1, 0.2, 0.3]], dtype=torch.float64)]
    out_v, out_f, out_c = MB.split_outputs(verts_out, attrs_out, faces_out, ovf, off, old_f, old_c, 3, old_verts=old_v)
    assert torch.equal(out_v[0], torch.cat([old_v[0], verts_out[2:3]])) and out_v[0].dtype == torch.float32
    assert torch.equal(out_v[1], verts_out[3:5]) and out_v[1].dtype == torch.float32   # other dtypes: the float32 rows the call wrote
    assert torch.equal(out_f[0], torch.cat([old_f[0], faces_out[1:2].long()])) and out_f[1].dtype == torch.int32 and out_f[1].shape == (1, 3)
    assert out_c[0].tolist() == [[1, 2, 3], [4, 5, 6], [0, 0, 7]]
    assert torch.equal(out_c[1], torch.cat([old_c[1], attrs_out[4:5].double()]))


def _stub(calls):
    """In place of an operator: doubles the vertices, keeps the faces, adds 1 to every colour; notes what it was given."""
    def fn(meshes, scale=2.0, colors_list=None, return_info=False, **kw):
        verts, faces = meshes
        calls.append({"colors": None if colors_list is None else [tuple(c.shape) for c in colors_list], "scale": scale, "kw": kw})
        out = ([v * scale for v in verts], list(faces))
        if colors_list is not None:
            out += ([c + 1 for c in colors_list],)
        return out + (([{"n": int(v.shape[0])} for v in verts],) if return_info else ())
    return fn


def test_a_batch_of_a_coloured_and_an_uncoloured_file_shares_one_call():
    calls = []
    verts = [torch.ones(3, 3), torch.ones(2, 3)]
    faces = [torch.tensor([[0, 1, 2]]), torch.zeros(0, 3, dtype=torch.int64)]
    colour = torch.tensor([[1, 2, 3]] * 3, dtype=torch.uint8)
    v, f, c, info = MB.run_on_host_batch(_stub(calls), verts, faces, [colour, None], "cpu", 3.0, flag=True)
    assert calls == [{"colors": [(3, 3), (2, 3)], "scale": 3.0, "kw": {"flag": True}}]   # the uncoloured file rode along at the batch's width
    assert c[1] is None and torch.equal(c[0], colour + 1) and c[0].dtype == torch.uint8
    assert torch.equal(v[0], verts[0] * 3) and torch.equal(f[0], faces[0]) and info == [{"n": 3}, {"n": 2}]
    v, f, c, info = MB.run_on_host_batch(_stub(calls), verts, faces, [None, None], "cpu")
    assert calls[-1]["colors"] is None and c == [None, None] and torch.equal(v[1], verts[1] * 2)


def test_the_batch_wrappers_are_the_shared_one_around_their_operator(monkeypatch):
    calls = []
    verts, faces, colours = [torch.ones(3, 3)], [torch.tensor([[0, 1, 2]])], [None]
    monkeypatch.setattr(MF, "fill_holes", _stub(calls))
    assert MF.fill_batch(verts, faces, colours, "cpu", 8)[3] == [{"n": 3}] and calls[-1]["scale"] == 8
    monkeypatch.setattr(MD, "simplify_vertex_clustering", lambda meshes, voxel_size=None, resolution=None, contraction="average", **kw:
                        _stub(calls)(meshes, 1.0, resolution=resolution, contraction=contraction, **kw))
    MD.decimate_batch(verts, faces, colours, "cpu", resolution=8, contraction="first")
    assert calls[-1]["kw"] == {"resolution": 8, "contraction": "first"}
    monkeypatch.setattr(MD, "simplify_quadric_decimation", lambda meshes, **kw: _stub(calls)(meshes, 1.0, **kw))
    MD.quadric_batch(verts, faces, colours, "cpu", target_fraction=0.5)
    assert calls[-1]["kw"] == {"target_number_of_triangles": None, "target_fraction": 0.5, "maximum_error": float("inf"), "boundary_weight": 1.0}


def test_mixed_widths_are_padded_and_cut_back():
    calls = []
    cols = [torch.zeros(3, 0), torch.full((2, 4), 5.0), torch.zeros(1, 0)]
    meshes = ([torch.ones(3, 3), torch.ones(2, 3), torch.ones(1, 3)], [torch.zeros(0, 3, dtype=torch.int64)] * 3)
    _, _, out, info = MB.with_padded_colors(_stub(calls), meshes, cols)
    assert calls[0]["colors"] == [(3, 4), (2, 4), (1, 4)] and [tuple(c.shape) for c in out] == [(3, 0), (2, 4), (1, 0)]
    assert torch.equal(out[1], cols[1] + 1) and len(info) == 3


def test_the_walker_sorts_chunks_and_refuses_an_empty_batch(tmp_path):
    from bdm_amd.io import load_mesh_ply, save_mesh_ply
    tri = np.array([[0, 1, 2]], dtype=np.int64)
    for rel, n in (("b/two.ply", 4), ("a/one.ply", 3), ("c.ply", 5)):
        save_mesh_ply(np.full((n, 3), float(n), dtype=np.float32), tri, tmp_path / "in" / rel,
                      colors=np.full((n, 3), 0.5, dtype=np.float32) if n == 4 else None)
    chunks, visited = [], []

    def batch_fn(verts_list, faces_list, colors_list):
        chunks.append([(int(v.shape[0]), c is not None) for v, c in zip(verts_list, colors_list)])
        return [v + 1 for v in verts_list], faces_list, colors_list, [{"k": int(v.shape[0])} for v in verts_list]
    files = MB.walk_tree(tmp_path / "in", tmp_path / "out", batch_fn, 2, lambda v_in, f_in, v, f, i: visited.append((v_in.shape[0], v.shape[0], i["k"])))
    assert files == 3 and chunks == [[(3, False), (4, True)], [(5, False)]]   # a/one.ply, b/two.ply | c.ply
    assert visited == [(3, 3, 3), (4, 4, 4), (5, 5, 5)]
    v, f, c = load_mesh_ply(tmp_path / "out" / "b" / "two.ply", with_colors=True)
    assert np.array_equal(v, np.full((4, 3), 5.0, dtype=np.float32)) and np.array_equal(f, tri) and c is not None and c.shape == (4, 3)
    assert load_mesh_ply(tmp_path / "out" / "a" / "one.ply", with_colors=True)[2] is None
    with pytest.raises(ValueError, match="batch_size must be positive"):
        MB.walk_tree(tmp_path / "in", tmp_path / "out", batch_fn, 0, lambda *a: None)
    assert len(chunks) == 2   # nothing was read
    for module in (MF, MD):
        with pytest.raises(ValueError, match="batch_size must be positive"):
            module.process_tree(tmp_path / "in", tmp_path / "out", batch_fn, batch_size=0)
