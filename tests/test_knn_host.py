"""The two-set K-nearest-neighbour rule and the attribute transfer without a GPU: the restatement tests/knn_ref.py against brute
force in float64, the mutants against the GPU test's own inputs, and everything of the Python surface that needs no device
(knn_gather, the zero-fill of knn_points, the PLY round trip with colours, the argument errors, mesh_color's tree walk, the
renderer's vert_albedo argument and main_render's coloured-mesh pass)."""
import json

import numpy as np
import pytest
import torch

import knn_ref as K


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def test_restatement_equals_brute_force_float64_on_separated_inputs():
    """Indices only.  The inputs are jittered lattices: the k + 1 nearest candidates of a query differ in d2 by far more than float32's
    error in d2 (the inputs are float32 in both; three roundings in the differences, three in the squares' sum: at most 6 * 2^-24 =
    3.6e-7 of the larger d2), so float32 and float64 must rank them alike; the gap is asserted, not assumed."""
    g = torch.Generator().manual_seed(1)
    ax = torch.arange(6, dtype=torch.float64)
    refs = torch.stack(torch.meshgrid(ax, ax * 1.37, ax * 0.61, indexing="ij"), dim=-1).reshape(-1, 3)
    refs = (refs + torch.rand(refs.shape, generator=g, dtype=torch.float64) * 0.2).float()
    queries = (torch.rand(50, 3, generator=g, dtype=torch.float64) * 5.0).float()
    k = 7
    d2 = ((refs.double()[None] - queries.double()[:, None]) ** 2).sum(-1)
    order = torch.argsort(d2, dim=1)[:, :k + 1]
    near = torch.gather(d2, 1, order)
    assert float(near.diff(dim=1).min()) > 1e-5 * float(near.max())          # 30 times the error bound
    idx, dist = K.knn(queries, refs, k)
    assert torch.equal(idx, order[:, :k])
    assert torch.allclose(dist.double(), torch.gather(d2, 1, order[:, :k]), rtol=1e-6, atol=0)
    idx64, dist64 = K.knn(queries, refs, k, dtype=torch.float64)
    assert torch.equal(idx64, idx) and dist64.dtype == torch.float64


def test_short_rows_non_finite_rows_and_overflow():
    q = torch.tensor([[0.0, 0.0, 0.0], [float("nan"), 0.0, 0.0], [1.0, 0.0, 0.0]])
    r = torch.tensor([[1.0, 0.0, 0.0], [0.0, float("inf"), 0.0], [3e19, 0.0, 0.0], [1.0, 0.0, 0.0]])
    idx, d2 = K.knn(q, r, 4)
    inf = float("inf")
    assert idx.tolist() == [[0, 3, 2, -1], [-1, -1, -1, -1], [0, 3, 2, -1]]
    assert d2.tolist() == [[1.0, 1.0, inf, inf], [inf] * 4, [0.0, 0.0, inf, inf]]
    idx, d2 = K.knn(q, torch.zeros(0, 3), 2)
    assert idx.tolist() == [[-1, -1]] * 3 and bool(torch.isinf(d2).all())
    assert K.knn(torch.zeros(0, 3), r, 2)[0].shape == (0, 2)


@pytest.mark.parametrize("mutant", K.SEARCH_MUTANTS)
def test_every_search_mutant_changes_an_output_on_a_gpu_case(mutant):
    name = K.MUTANT_CASE[mutant]
    good, bad = K.case_ref(name), K.case_ref(name, mutant)
    changed = sum(int((gi != bi).sum()) + int((K.bits(gd) != K.bits(bd)).sum()) for (gi, gd), (bi, bd) in zip(good, bad))
    print(f"{mutant} on {name}: {changed} entries differ")
    assert changed > 0


@pytest.mark.parametrize("mutant", K.INTERP_MUTANTS)
def test_every_interpolation_mutant_changes_an_output_on_the_gpu_case(mutant):
    changed = 0
    for c in K.INTERP_C:
        good, bad = K.interp_ref(c, 1, 0.5), K.interp_ref(c, 1, 0.5, mutant)
        changed += int((K.bits(good) != K.bits(bad)).sum())
    print(f"{mutant}: {changed} entries differ")
    assert changed > 0


def test_gpu_cases_hold_what_they_are_there_for():
    ties = K.case_ref("ties")[0]
    assert int((ties[1][:, 1:] == ties[1][:, :-1]).sum()) > 200                       # equal neighbouring distances: ties everywhere
    nf = K.case("nonfinite_k50")
    assert int((~torch.isfinite(nf["q"][0]).all(1)).sum()) == 16 and int((~torch.isfinite(nf["r"][0]).all(1)).sum()) == 16
    idx, d2 = K.case_ref("nonfinite_k50")[0]
    ok = torch.isfinite(nf["q"][0]).all(1)
    assert bool((idx[ok, 23] == 5).all()) and bool(torch.isinf(d2[ok, 23]).all()) and bool((idx[ok, 24:] == -1).all())   # the overflow pair
    assert bool((idx[ok, :23] >= 0).all()) and bool((idx[~ok] == -1).all())
    ragged = K.case("ragged")
    assert [(q.shape[0], r.shape[0]) for q, r in zip(ragged["q"], ragged["r"])] == [(17, 1025), (0, 40), (33, 0), (5, 2)]
    short = K.case_ref("short_k64")
    assert [int((i[0] >= 0).sum()) for i, _ in short] == [0, 1, 63, 64]
    ic = K.interp_case()
    m = ((ic["idx"] >= 0)).sum(1).tolist()
    assert m[0] == 0 and m[1] == 1 and m[4] == 4 and m[12:] == [0, 0, 0] and float(ic["d2"][2, 0]) == 0.0 and bool(torch.isinf(ic["d2"][3, 3]))


def test_interpolation_restatement():
    attr = torch.tensor([[1.0, 10.0], [3.0, 30.0], [5.0, 50.0]])
    idx = torch.tensor([[1, 0, 2], [2, -1, -1], [-1, -1, -1], [0, 1, 2]])
    inf = float("inf")
    d2 = torch.tensor([[0.0, 1.0, 4.0], [2.0, inf, inf], [inf, inf, inf], [1.0, 1.0, inf]])
    near = K.interpolate(attr, idx, d2, 0, fill=0.5)
    assert near.tolist() == [[3.0, 30.0], [5.0, 50.0], [0.5, 0.5], [1.0, 10.0]]
    idw = K.interpolate(attr, idx, d2, 1, eps=0.5, fill=0.5)
    w = [1 / 0.5, 1 / 1.5, 1 / 4.5]
    want0 = (w[0] * 3 + w[1] * 1 + w[2] * 5) / sum(w)
    assert abs(float(idw[0, 0]) - want0) < 1e-6 and idw[1].tolist() == [5.0, 50.0] and idw[2].tolist() == [0.5, 0.5]
    assert idw[3].tolist() == [2.0, 20.0]                                          # the +inf entry takes part with weight 0
    assert bool(torch.isnan(K.interpolate(attr, idx, d2, 1, fill=float("nan"))[2]).all())
    idw64 = K.interpolate(attr, idx, d2, 1, eps=0.5, fill=0.5, dtype=torch.float64)
    assert idw64.dtype == torch.float64 and abs(float(idw64[0, 0]) - want0) < 1e-12


# ---- the Python surface ---------------------------------------------------------------------------------------------------------------
def test_knn_gather():
    from bdm_amd.knn import knn_gather
    x = torch.arange(24.0).view(2, 4, 3)
    idx = torch.tensor([[[0, 3], [2, -1]], [[1, 1], [3, 0]]])
    out = knn_gather(x, idx)
    assert out.shape == (2, 2, 2, 3)
    assert out[0, 0].tolist() == [[0.0, 1.0, 2.0], [9.0, 10.0, 11.0]] and out[0, 1].tolist() == [[6.0, 7.0, 8.0], [0.0, 0.0, 0.0]]
    assert out[1, 1].tolist() == [[21.0, 22.0, 23.0], [12.0, 13.0, 14.0]]
    cut = knn_gather(x, idx, torch.tensor([4, 1]))
    assert torch.equal(cut[0], out[0]) and cut[1, :, 1].abs().sum() == 0 and torch.equal(cut[1, :, 0], out[1, :, 0])
    assert knn_gather(torch.zeros(1, 0, 3), torch.full((1, 2, 2), -1)).shape == (1, 2, 2, 3)
    with pytest.raises(ValueError):
        knn_gather(x, idx[0])
    with pytest.raises(ValueError):
        knn_gather(x, idx.float())
    with pytest.raises(ValueError):
        knn_gather(x, idx, torch.tensor([4]))


def test_knn_points_zero_fills_with_lengths(monkeypatch):
    """knn_points' padding, with the search replaced by the restatement (the kernel itself is the GPU test's business)."""
    from bdm_amd import _lib as L
    from bdm_amd import knn as KN

    def search(queries, refs, q_first, r_first, k):
        out = [K.knn(queries[q_first[i]:q_first[i + 1]], refs[r_first[i]:r_first[i + 1]], k) for i in range(q_first.numel() - 1)]
        return torch.cat([i for i, _ in out]).int(), torch.cat([d for _, d in out])
    monkeypatch.setattr(KN, "_search", search)
    monkeypatch.setattr(L, "ptr", lambda t: 0)
    p1, p2 = K.cloud(12, 1).view(2, 6, 3), K.cloud(10, 2).view(2, 5, 3)
    res = KN.knn_points(p1, p2, lengths1=torch.tensor([6, 2]), lengths2=torch.tensor([5, 2]), K=3, return_nn=True)
    assert isinstance(res, KN.KNN) and res._fields == ("dists", "idx", "knn")
    assert res.dists.shape == (2, 6, 3) and res.idx.dtype == torch.int64 and res.knn.shape == (2, 6, 3, 3)
    i0, d0 = K.knn(p1[0], p2[0], 3)
    i1, d1 = K.knn(p1[1, :2], p2[1, :2], 3)
    assert torch.equal(res.idx[0], i0) and torch.equal(res.dists[0], d0)
    assert torch.equal(res.idx[1, :2, :2], i1[:, :2]) and torch.equal(res.dists[1, :2, :2], d1[:, :2])
    assert int(res.idx[1, 2:].abs().sum()) == 0 and float(res.dists[1, 2:].abs().sum()) == 0.0          # rows past lengths1
    assert int(res.idx[1, :, 2].abs().sum()) == 0 and float(res.dists[1, :, 2].abs().sum()) == 0.0      # neighbours past lengths2
    assert torch.equal(res.knn[0], p2[0][i0]) and float(res.knn[1, :, 2].abs().sum()) == 0.0
    plain = KN.knn_points(p1, p2, K=2)
    assert plain.knn is None and torch.equal(plain.idx[1], K.knn(p1[1], p2[1], 2)[0])
    assert KN.knn_points(p1, p2, None, None, 2, 0, False, False).idx.shape == (2, 6, 2)                   # pytorch3d's argument order


def test_argument_errors_come_before_any_launch():
    """Host tensors everywhere: a ValueError means the check ran first; a well-formed call on host tensors is a BdmHipError."""
    from bdm_amd import _lib as L
    from bdm_amd.knn import knn_packed, knn_points, transfer_point_attributes
    x, y = torch.zeros(2, 5, 3), torch.zeros(2, 7, 3)
    for bad_k in (0, 65, -1, 2.5):
        with pytest.raises(ValueError, match="K="):
            knn_points(x, y, K=bad_k)
    with pytest.raises(ValueError, match="D = 3"):
        knn_points(torch.zeros(2, 5, 2), torch.zeros(2, 7, 2))
    with pytest.raises(ValueError, match="D = 3"):
        knn_points(x.long(), y)
    with pytest.raises(ValueError, match="batch dimension"):
        knn_points(x, y[:1])
    with pytest.raises(ValueError, match="lengths1"):
        knn_points(x, y, lengths1=torch.tensor([5, 6]))
    with pytest.raises(ValueError, match="lengths2"):
        knn_points(x, y, lengths2=torch.tensor([7]))
    with pytest.raises(L.BdmHipError):
        knn_points(x, y, K=2)
    with pytest.raises(ValueError, match="reference sets"):
        knn_packed([x[0]], [y[0], y[1]], 3)
    with pytest.raises(ValueError, match="D = 3"):
        knn_packed([x[0, :, :2]], [y[0]], 3)
    with pytest.raises(ValueError, match="list"):
        knn_packed(x, y, 3)
    with pytest.raises(L.BdmHipError):
        knn_packed([x[0]], [y[0]], 3)
    assert knn_packed([], [], 3) == []
    attr = torch.zeros(7, 3)
    with pytest.raises(ValueError, match="mode"):
        transfer_point_attributes([x[0]], [y[0]], [attr], mode="linear")
    with pytest.raises(ValueError, match="eps"):
        transfer_point_attributes([x[0]], [y[0]], [attr], eps=0.0)
    with pytest.raises(ValueError, match="C in 1..16"):
        transfer_point_attributes([x[0]], [y[0]], [torch.zeros(7, 17)])
    with pytest.raises(ValueError, match="attribute tensor"):
        transfer_point_attributes([x[0]], [y[0]], [torch.zeros(6, 3)])
    with pytest.raises(ValueError, match="attr_list"):
        transfer_point_attributes([x[0]], [y[0]], [])
    with pytest.raises(ValueError, match="K="):
        transfer_point_attributes([x[0]], [y[0]], [attr], K=65)
    with pytest.raises(L.BdmHipError):
        transfer_point_attributes([x[0]], [y[0]], [attr])
    assert transfer_point_attributes([], [], []) == []


# ---- files ----------------------------------------------------------------------------------------------------------------------------
TETRA_V = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
TETRA_F = np.array([[0, 2, 1], [0, 1, 3], [0, 3, 2], [1, 2, 3]], dtype=np.int64)


def _save_mesh_ply_before(verts, faces, path):
    """The bytes save_mesh_ply wrote before it had a `colors` argument, composed by hand: the header, float32 vertices, then per face
    a count byte and three little-endian int32."""
    body = b"".join(b"\x03" + np.asarray(f, dtype="<i4").tobytes() for f in faces)
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {len(verts)}\nproperty float x\nproperty float y\n"
              f"property float z\nelement face {len(faces)}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii") + np.asarray(verts, dtype="<f4").tobytes() + body)


def test_mesh_ply_round_trip_with_colours_and_byte_identity_without(tmp_path):
    from bdm_amd.io import load_mesh_ply, load_pointcloud_ply, save_mesh_ply
    save_mesh_ply(TETRA_V, TETRA_F, tmp_path / "plain.ply")
    _save_mesh_ply_before(TETRA_V, TETRA_F, tmp_path / "before.ply")
    assert (tmp_path / "plain.ply").read_bytes() == (tmp_path / "before.ply").read_bytes()
    save_mesh_ply(TETRA_V, TETRA_F, tmp_path / "none.ply", colors=None)
    assert (tmp_path / "none.ply").read_bytes() == (tmp_path / "before.ply").read_bytes()
    v, f = load_mesh_ply(tmp_path / "plain.ply")                                       # the two-tuple default
    assert np.array_equal(v, TETRA_V) and np.array_equal(f, TETRA_F)
    v, f, c = load_mesh_ply(tmp_path / "plain.ply", with_colors=True)
    assert c is None and np.array_equal(f, TETRA_F)
    colours = np.array([[0.0, 0.5, 1.0], [1.5, -0.2, 0.25], [0.1, 0.2, 0.3], [0.998, 0.002, 0.7]])
    save_mesh_ply(TETRA_V, TETRA_F, tmp_path / "col.ply", colors=colours)
    v, f, c = load_mesh_ply(tmp_path / "col.ply", with_colors=True)
    want = np.rint(np.clip(colours, 0.0, 1.0) * 255.0).astype(np.uint8)                # save_pointcloud_ply_rgb's conversion
    assert want[0].tolist() == [0, 128, 255] and want[1].tolist() == [255, 0, 64]
    assert np.array_equal(v, TETRA_V) and np.array_equal(f, TETRA_F) and c.dtype == np.float32
    assert np.array_equal(c, want.astype(np.float32) / np.float32(255.0))
    v2, f2 = load_mesh_ply(tmp_path / "col.ply")
    assert np.array_equal(v2, TETRA_V) and np.array_equal(f2, TETRA_F)
    pts, pc = load_pointcloud_ply(tmp_path / "col.ply", with_colors=True)              # the vertex element reads as a coloured cloud
    assert np.array_equal(pts, TETRA_V) and np.array_equal(pc, c)
    save_mesh_ply(v, f, tmp_path / "again.ply", colors=c)                              # uchar colours survive a second trip exactly
    assert (tmp_path / "again.ply").read_bytes() == (tmp_path / "col.ply").read_bytes()
    with pytest.raises(ValueError, match="colours"):
        save_mesh_ply(TETRA_V, TETRA_F, tmp_path / "bad.ply", colors=colours[:3])
    save_mesh_ply(np.zeros((0, 3)), np.zeros((0, 3), np.int64), tmp_path / "empty.ply", colors=np.zeros((0, 3)))
    v0, f0, c0 = load_mesh_ply(tmp_path / "empty.ply", with_colors=True)
    assert v0.shape == (0, 3) and f0.shape == (0, 3) and c0.shape == (0, 3)


def test_mesh_color_tree_walk(tmp_path):
    """process_tree with a colour function made of the restatement: which files are taken, how they are batched, what is written and
    what is counted."""
    from bdm_amd import mesh_color as MC
    from bdm_amd.io import load_mesh_ply, save_mesh_ply, save_pointcloud_ply, save_pointcloud_ply_rgb
    g = torch.Generator().manual_seed(5)
    clouds = {}
    for rel, n in (("a/one.ply", 30), ("a/two.ply", 0), ("b/three.ply", 12)):
        pts, col = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
        save_mesh_ply(TETRA_V + 0.1, TETRA_F, tmp_path / "mesh" / rel)
        save_pointcloud_ply_rgb(pts.numpy(), col.numpy(), tmp_path / "col" / rel)
        clouds[rel] = pts
    save_mesh_ply(TETRA_V, TETRA_F, tmp_path / "mesh" / "b" / "lonely.ply")            # no coloured cloud: left alone
    save_pointcloud_ply(np.zeros((3, 3)), tmp_path / "col" / "c" / "cloud_only.ply")
    calls = []

    def color_fn(verts_list, points_list, colors_list):
        calls.append([(v.shape[0], p.shape[0]) for v, p in zip(verts_list, points_list)])
        outs, near, has = [], [], []
        for v, p, c in zip(verts_list, points_list, colors_list):
            idx, d2 = K.knn(v, p, 3)
            outs.append(K.interpolate(c, idx, d2, 1, fill=MC.GREY))
            near.append(d2[:, 0])
            has.append(idx[:, 0] >= 0)
        return outs, near, has
    res = MC.process_tree(tmp_path / "mesh", tmp_path / "col", tmp_path / "out", color_fn, batch_size=2)
    assert calls == [[(4, 30), (4, 0)], [(4, 12)]]
    assert sorted(str(p.relative_to(tmp_path / "out")) for p in (tmp_path / "out").rglob("*.ply")) == ["a/one.ply", "a/two.ply", "b/three.ply"]
    near = [K.knn(torch.from_numpy(TETRA_V + 0.1), clouds[rel], 1)[1][:, 0].double().sqrt().sum() for rel in ("a/one.ply", "b/three.ply")]
    assert res == {"files": 3, "vertices": 12, "unmatched": 4, "mean_nearest_distance": float(near[0] + near[1]) / 8}
    json.dumps(res)
    v, f, c = load_mesh_ply(tmp_path / "out" / "a" / "two.ply", with_colors=True)
    assert np.array_equal(c, np.full((4, 3), np.float32(128.0) / np.float32(255.0)))   # mid-grey: rint(0.5 * 255) = 128
    v, f, c = load_mesh_ply(tmp_path / "out" / "a" / "one.ply", with_colors=True)
    assert np.array_equal(v, TETRA_V + 0.1) and np.array_equal(f, TETRA_F) and float(c.min()) >= 0.0 and float(c.std()) > 0.0
    assert MC.compose_result(0, 0, 0, 0.0)["files"] == 0 and np.isnan(MC.compose_result(2, 5, 5, 0.0)["mean_nearest_distance"])
    with pytest.raises(ValueError, match="batch_size"):
        MC.process_tree(tmp_path / "mesh", tmp_path / "col", tmp_path / "out", color_fn, batch_size=0)
    for argv in (["--k", "0"], ["--k", "65"], ["--batch-size", "0"], ["--mode", "linear"]):
        with pytest.raises(SystemExit):
            MC.parse_args(["--mesh_dir", "m", "--color_dir", "c", "--out_dir", "o"] + argv)
    args = MC.parse_args(["--mesh_dir", "m", "--color_dir", "c", "--out_dir", "o"])
    assert (args.k, args.mode, args.batch_size) == (3, "idw", 16)


# ---- the renderer's new keyword and main_render's new pass ---------------------------------------------------------------------------
def test_vert_albedo_argument_errors_come_before_any_launch():
    import mesh_render_ref as M
    from bdm_amd.cameras import Meshes, PerspectiveCameras
    from bdm_amd.render import render_mesh_batch, visualize_mesh_batch
    v, f = M.icosphere(1)
    one = Meshes([v], [f])
    cam = PerspectiveCameras(focal_length=2.0, T=torch.tensor([[0.0, 0.0, 2.0]]))
    good = torch.zeros(v.shape[0], 3)
    with pytest.raises(ValueError, match="vert_albedo"):
        render_mesh_batch(cam, one, shading="none", vert_albedo=good)
    with pytest.raises(ValueError, match="vert_albedo"):
        render_mesh_batch(cam, one, shading="smooth", vert_albedo=good[:-1])
    with pytest.raises(ValueError, match="vert_albedo"):
        render_mesh_batch(cam, one, shading="flat", vert_albedo=torch.zeros(v.shape[0], 4))
    with pytest.raises(ValueError, match="vert_albedo"):
        render_mesh_batch(cam, one, shading="smooth", vert_albedo=good.long())
    with pytest.raises(ValueError, match="vert_colors"):                               # the pin of test_mesh_render_host.py stays
        render_mesh_batch(cam, one, shading="flat", vert_colors=good)
    with pytest.raises(ValueError, match="vert_albedo"):
        visualize_mesh_batch(one, shading="none", vert_albedo=good)


def test_render_tree_draws_the_coloured_meshes_only_where_they_exist(tmp_path):
    import main_render as MR
    from bdm_amd.config import ProjectConfig, parse_overrides
    from bdm_amd.data import SyntheticShapes
    from bdm_amd.io import save_mesh_ply, save_pointcloud_ply
    assert ProjectConfig().run.render_colored_mesh_subdir == "colored_mesh"
    assert parse_overrides(["run.render_colored_mesh_subdir=cm"]).run.render_colored_mesh_subdir == "cm"
    cfg = MR.parse_args(["dataset=synthetic", f"run.render_sample_dir={tmp_path}", "dataloader.batch_size=3", "dataset.num_shapes=5",
                         "run.render_num_frames=2"])
    g = np.random.Generator(np.random.PCG64(0))
    save_pointcloud_ply(g.standard_normal((20, 3)), tmp_path / "pred" / "chair" / "synthetic_000000.ply")
    loader = SyntheticShapes(range(5), 3, image_size=32, num_points=8)
    cloud_stub = lambda cameras, points, colors: torch.zeros(len(cameras), 4, 6, 3)   # noqa: E731
    orbit_stub = lambda points, colors, path, n: [path.with_name(f"{path.stem}-{f}.png") for f in range(n)]   # noqa: E731
    calls, orbits = [], []

    def cm_stub(cameras, verts, faces, colors):
        calls.append([(v.shape[0], f.shape[0], tuple(c.shape), c.dtype) for v, f, c in zip(verts, faces, colors)])
        return torch.stack([c[:1].expand(4 * 6, 3).reshape(4, 6, 3) for c in colors])

    def cm_orbit_stub(verts, faces, colors, path, n):
        orbits.append((path.name, verts.shape[0], tuple(colors.shape), n))
        return [path.with_name(f"{path.stem}-{f}.png") for f in range(n)]

    before = MR.render_tree(cfg, loader, cloud_stub, orbit_stub)
    again = MR.render_tree(cfg, loader, cloud_stub, orbit_stub, colored_mesh_fn=cm_stub, colored_mesh_orbit_fn=cm_orbit_stub)
    assert again == before and not calls and sorted(p.name for p in (tmp_path / "renders").iterdir()) == ["pred"]
    first = {p: p.read_bytes() for p in before if p.exists()}

    col = np.tile(np.array([[1.0, 0.5, 0.0]]), (5, 1))
    save_mesh_ply(g.standard_normal((5, 3)), g.integers(0, 5, size=(4, 3)), tmp_path / "colored_mesh" / "chair" / "synthetic_000000.ply", colors=col)
    save_mesh_ply(g.standard_normal((6, 3)), g.integers(0, 6, size=(2, 3)), tmp_path / "colored_mesh" / "chair" / "synthetic_000004.ply",
                  colors=np.zeros((6, 3)))
    save_mesh_ply(g.standard_normal((4, 3)), g.integers(0, 4, size=(2, 3)), tmp_path / "colored_mesh" / "chair" / "synthetic_000001.ply")   # grey
    with pytest.raises(ValueError, match="colored_mesh_fn"):
        MR.render_tree(cfg, loader, cloud_stub, orbit_stub)
    written = MR.render_tree(cfg, loader, cloud_stub, orbit_stub, colored_mesh_fn=cm_stub, colored_mesh_orbit_fn=cm_orbit_stub)
    new = [p for p in written if p not in before]
    assert [p for p in written if p in before] == before and all(p.read_bytes() == b for p, b in first.items())
    assert sorted(str(p.relative_to(tmp_path / "renders")) for p in new) == sorted(
        [f"colored_mesh/chair/synthetic_00000{i}.png" for i in (0, 4)] + [f"colored_mesh_orbit/chair/synthetic_00000{i}-{f}.png" for i in (0, 4) for f in (0, 1)])
    assert calls == [[(5, 4, (5, 3), torch.float32)], [(6, 2, (6, 3), torch.float32)]]
    assert sorted(orbits) == [("synthetic_000000.png", 5, (5, 3), 2), ("synthetic_000004.png", 6, (6, 3), 2)]
    from PIL import Image
    px = np.asarray(Image.open(tmp_path / "renders" / "colored_mesh" / "chair" / "synthetic_000000.png"))
    assert px.shape == (4, 6, 3) and px[0, 0].tolist() == [255, 128, 0]                # the file's colours reached the draw call
    cfg.run.render_colored_mesh_subdir = "absent"
    assert MR.render_tree(cfg, loader, cloud_stub, orbit_stub) == before
