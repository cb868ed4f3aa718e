"""The Poisson mesher without a GPU: the restatement tests/surface_poisson_ref.py (section 22 of bdm_hip.h) on the clouds of DESIGN.md
section 26 -- closure, accuracy, convergence, the mutants, trimming -- and the host side of bdm_amd.surface (arguments, the resolution
snap, the command-line walk with the kernels replaced by the restatement).

Figures of the restatement at the default 12 cycles (DESIGN.md section 26 has the table):

    cloud, R, s                 V / F           volume vs analytic    largest vertex-to-surface distance
    sphere 512, 32, 2           2078 / 4152     -0.81 %               0.177 voxels
    sphere 600, 32, 2           2062 / 4120     -1.05 %               0.225
    sphere 1024, 32, 3          1686 / 3368     -0.80 %               0.089
    torus 1500, 32, 3            900 / 1800     -4.34 %               0.250
    torus 1500, 48, 2           3848 / 7696     -0.98 %               0.281
    sphere 4096, 64, 3         12224 / 24444    -0.17 %               0.120

The torus at 32^3 is the row that needs the separation passes of step 6: its tube (radius 2.43 voxels about z = 15.5) grazes the node
planes z = 13 and z = 18, the level set leaves 7 grid faces there with one diagonal inside and the other outside, and surface nets
would put four faces on the edge between the two cells on either side of each (7 open and 14 inconsistent edges in mesh_stats' count;
seeds 3211, 3212, 3213, 3300 of the same torus give 1, 2, 0, 1).  One pass takes all of them out, here and on every other cloud of the
tests; test_separation_takes_out_every_checkerboard_face shows it."""
import json
import math

import numpy as np
import pytest
import torch

import mesh_voxel_ref as MV
import surface_poisson_ref as P
import surface_ref as S

# |volume / analytic - 1| and the largest distance of a vertex from the analytic surface in voxels: the measured figure of the docstring
# plus a quarter to a half of it (the margin DESIGN.md section 16 uses)
BOUNDS = {"sphere_512_R32_s2": (0.012, 0.25), "sphere_600_R32_s2": (0.015, 0.30), "sphere_1024_R32_s3": (0.012, 0.12),
          "torus_1500_R32_s3": (0.06, 0.35), "torus_1500_R48_s2": (0.014, 0.38), "sphere_4096_R64_s3": (0.0025, 0.16)}


def _components(faces, V):
    parent = np.arange(V)

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b, c in faces.tolist():
        ra = find(a)
        parent[find(b)] = ra
        parent[find(c)] = ra
    return len({find(i) for i in range(V)})


def _closure_clouds():
    out = {name: (lambda name=name: P.closure_inputs(name)) for name in P.CLOSURE}
    out["lattice_plane_R32_s3"] = lambda: (*S.lattice_plane(32), 32, 3)
    for c in range(2):
        out[f"nonfinite_{c}_R16_s3"] = lambda c=c: (S.case_inputs("b2_n300_nonfinite_R16_s3")[0][c], S.case_inputs("b2_n300_nonfinite_R16_s3")[1][c], 16, 3)
    return out


CLOSURE_CLOUDS = _closure_clouds()
_MESHES = {}


def _mesh(name):
    if name not in _MESHES:
        pts, nrm, R, s = CLOSURE_CLOUDS[name]()
        _MESHES[name] = P.reconstruct(pts, nrm, R, s)
    return _MESHES[name]


@pytest.mark.parametrize("name", list(CLOSURE_CLOUDS))
def test_closure(name):
    from bdm_amd.surface import mesh_stats
    m = _mesh(name)
    V, F, skipped, _ = m["counts"]
    st = mesh_stats(m["verts"], m["faces"])
    print(f"{name}: V / F {V} / {F}, skipped {skipped}, border_raised {m['border_raised']}, {st}")
    assert V > 0 and F > 0 and skipped == 0
    assert MV.odd_degree_edges(m["faces"], V) == 0                                 # what step 6 of the rule proves for any input
    assert int(m["faces"].unique().numel()) == V, "a vertex no face uses"
    assert st["signed_volume"] > 0
    assert _components(m["faces"], V) == 1                                         # every cloud here is one body
    if name.startswith("lattice_plane"):
        # an open sheet: its inside is the half space below it, which reaches the border, so the lower half of the border layer (the
        # plane lies exactly between the node planes 15 and 16) is raised -- the layer that closes the sheet
        assert m["border_raised"] == (32 ** 3 - 30 ** 3) // 2
    else:
        assert m["border_raised"] == 0


@pytest.mark.parametrize("name", list(CLOSURE_CLOUDS))
def test_every_edge_has_exactly_two_faces(name):
    """`open_edges == 0` as mesh_stats counts them: no edge with one face, none with four."""
    from bdm_amd.surface import mesh_stats
    m = _mesh(name)
    st = mesh_stats(m["verts"], m["faces"])
    assert st["open_edges"] == 0, f"{st['open_edges']} edges are not shared by exactly two faces"
    assert st["inconsistent_edges"] == 0


@pytest.mark.parametrize("name", list(CLOSURE_CLOUDS))
def test_voxelisation_at_32_has_no_disagreeing_cell(name):
    """Section 25's parity rays see a closed surface along all three axes: the two sparse spheres are the rows whose grids were 'not to
    be trusted in any mode' with every tool before."""
    m = _mesh(name)
    vox = MV.voxelize(m["verts"], m["faces"], 32)
    assert vox["info"]["disagree"] == 0 and vox["info"]["faces_dropped"] == 0 and vox["info"]["occupied"] > 0


def test_separation_takes_out_every_checkerboard_face():
    """Without the passes the torus at 32^3 has 7 checkerboard faces and as many four-face edges; one pass leaves none, the second finds
    nothing to do, and only negative nodes on such faces changed."""
    from bdm_amd.surface import mesh_stats
    pts, nrm, R, s = P.closure_inputs("torus_1500_R32_s3")
    kept = P.reconstruct(pts, nrm, R, s, mutant="checkerboards_kept")
    hit, faces = P.checkerboards(kept["SU"])
    assert faces == 7 and mesh_stats(kept["verts"], kept["faces"])["open_edges"] == 7
    assert [P.separate(kept["SU"], k)[1] for k in (1, 2)] == [0, 0]
    done = _mesh("torus_1500_R32_s3")
    changed = done["SU"] != kept["SU"]
    assert torch.equal(changed, hit) and bool((done["SU"][changed] == 1).all()) and bool((kept["SU"][hit] < 0).all())
    checker = torch.tensor([[[-5, 3], [2, -7]], [[4, 4], [4, 4]]], dtype=torch.int32)          # one face, its diagonal inside
    grid = torch.full((4, 4, 4), 9, dtype=torch.int32)
    grid[1:3, 1:3, 1:3] = checker
    out, left = P.separate(grid, 1)
    assert left == 0 and out[1, 1, 1] == 1 and out[1, 2, 2] == 1 and int((out != grid).sum()) == 2


def test_forced_border():
    """A field that is negative at the border: those nodes are raised and counted, and the mesh still closes."""
    from bdm_amd.surface import mesh_stats
    R = 16
    pts, nrm = S.sphere(torch.Generator().manual_seed(3306), 200)
    splat = P.splat_of(pts, nrm, R, 2)
    idx = torch.arange(R, dtype=torch.float32)
    x, y, z = idx.view(R, 1, 1), idx.view(1, R, 1), idx.view(1, 1, R)
    phi = (4.0 - (y - 7.5).abs()).expand(R, R, R) + 0.0 * (x + z)          # a slab: inside for |y - 7.5| > 4, border included
    iso_scale = (torch.tensor(0.0), torch.tensor(1024.0))
    m = P.mesh_from_field(phi.contiguous(), splat, R, iso_scale=iso_scale)
    border = torch.ones(R, R, R, dtype=torch.bool)
    border[1:-1, 1:-1, 1:-1] = False
    want = int((border & (phi < 1.0 / 1024.0 * 0.5)).sum())
    assert m["border_raised"] == want > 0 and bool((m["SU"][border] >= 1).all())
    st = mesh_stats(m["verts"], m["faces"])
    assert m["counts"][2] == 0 and st["open_edges"] == 0 and MV.odd_degree_edges(m["faces"], m["counts"][0]) == 0 and st["signed_volume"] > 0
    kept = P.mesh_from_field(phi.contiguous(), splat, R, mutant="border_kept", iso_scale=iso_scale)
    assert kept["border_raised"] == want and mesh_stats(kept["verts"], kept["faces"])["open_edges"] > 0


@pytest.mark.parametrize("name", list(BOUNDS))
def test_accuracy(name):
    from bdm_amd.surface import mesh_stats
    m = _mesh(name)
    pts, nrm, R, s = P.closure_inputs(name)
    inv = float(P.splat_of(pts, nrm, R, s)["inv"])
    v = m["verts"].double()
    if name.startswith("sphere"):
        analytic, dist = 4.0 / 3.0 * math.pi * 0.4 ** 3, (v.norm(dim=1) - 0.4).abs().max()
    else:
        analytic = 2.0 * math.pi ** 2 * 0.35 * 0.12 ** 2
        dist = (((v[:, :2].norm(dim=1) - 0.35) ** 2 + v[:, 2] ** 2).sqrt() - 0.12).abs().max()
    dev, dist = mesh_stats(m["verts"], m["faces"])["signed_volume"] / analytic - 1.0, float(dist) * inv
    print(f"{name}: volume {dev:+.2%} of analytic, largest vertex-to-surface distance {dist:.3f} voxels")
    assert abs(dev) < BOUNDS[name][0]
    assert dist < BOUNDS[name][1]


@pytest.mark.parametrize("name", ["b1_n65_R16_s2_c3", "b1_n257_R24_s2_c3", "sphere_512_R32_s2_default", "torus_R40_s3_c3", "torus_R48_s2_c3",
                                  "sphere_4096_R64_s3_default"])
def test_float64_residual_falls_every_cycle_down_to_its_floor(name):
    """The accepted R of the GPU test up to 64 (at 128 the same run takes seconds: measured by hand, 0.24 - 0.27).  Measured factors per
    cycle: 0.22 - 0.25 at R = 16, 0.21 - 0.26 at 24, 32 and 48, 0.23 - 0.27 at 40, 0.22 - 0.26 at 64, the first cycle the smallest; no rate
    is asserted, only that every cycle reduces the residual until 1e-12 of the right-hand side."""
    pts, nrm, R, s, _ = P.case_inputs(name)
    history = []
    P.solve(P.splat_of(pts[0], nrm[0], R, s)["D"], 24, dtype=torch.float64, history=history)
    print(f"{name}: factors {[round(b / a, 3) for a, b in zip(history, history[1:]) if a > 1e-12]}")
    assert history[-1] < 1e-12
    for before, after in zip(history, history[1:]):
        assert after < before or before < 1e-12


def test_every_mutant_changes_an_output_on_its_gpu_test_input():
    assert set(P.MUTANT_CASES) == set(P.MUTANTS)
    for mutant, case in P.MUTANT_CASES.items():
        assert case in P.CASES
        changed = [P.differences(a, b) for a, b in zip(P.case_ref(case), P.case_ref(case, mutant))]
        print(f"{mutant} on {case}: {changed}")
        assert any(changed), mutant
    # the splat's rounding reaches the integer grids themselves; the solve's mutants reach phi's bits
    assert "W" in P.differences(P.case_ref("b2_n300_nonfinite_R16_s3_c2")[0], P.case_ref("b2_n300_nonfinite_R16_s3_c2", "truncate")[0])
    for mutant in ("ghost_node", "constant_prolongation", "restriction_reversed", "coarsest_one_fewer"):
        assert "phi" in P.differences(P.case_ref(P.MUTANT_CASES[mutant])[0], P.case_ref(P.MUTANT_CASES[mutant], mutant)[0])


def test_gpu_case_table_reaches_what_it_is_there_for():
    tail = lambda R: [m for m in P.sides(R) if m <= P.TAIL_SIDE]
    glob = lambda R: [m for m in P.sides(R) if m > P.TAIL_SIDE]
    assert P.sides(16) == [16, 8, 4] and glob(16) == []                            # the whole solve in the LDS kernel
    assert P.sides(24) == [24, 12, 6, 3] and glob(24) == [24]                      # an odd coarsest side
    assert glob(32) == [32] and tail(32) == [16, 8, 4]                             # one global level above the tail
    assert P.sides(48) == [48, 24, 12, 6, 3] and P.sides(40) == [40, 20, 10, 5] and tail(40) == [20, 10, 5]   # the largest tail
    assert glob(64) == [64, 32] and glob(128) == [128, 64, 32]
    assert [R for R in range(1, 300) if P.accepted(R)] == list(P.ACCEPTED)
    assert all(3 * sum(m ** 3 for m in tail(R)) <= 3 * (20 ** 3 + 10 ** 3 + 5 ** 3) and len(tail(R)) <= 3 for R in P.ACCEPTED)
    assert [P.launches(R, c) for R, c in ((16, 12), (32, 12), (64, 12), (128, 12))] == [15, 98, 170, 242]
    refs = {name: P.case_ref(name) for name in ("b2_n300_nonfinite_R16_s3_c2", "b1_n40_all_equal_R16_s2_c1", "lattice_plane_R32_s3_c4",
                                                "b3_n1025_ellipsoids_R32_s3_c4")}
    assert [r["counts"][3] for r in refs["b2_n300_nonfinite_R16_s3_c2"]] == [260, 260]                    # 40 of 300 are not valid
    empty = refs["b1_n40_all_equal_R16_s2_c1"][0]
    assert empty["counts"] == [0, 0, 0, 40] and float(empty["scale"]) == 0.0 and not bool(empty["SW"].any())
    assert refs["lattice_plane_R32_s3_c4"][0]["border_raised"] > 0
    far = refs["b3_n1025_ellipsoids_R32_s3_c4"][1]["verts"]
    assert float(far[:, 0].mean()) > 99.0                                                                  # the cloud at (100, -50, 25)
    n = 65536
    assert n * P.FIX == 2 ** 28 and 6 * n * P.FIX < 2 ** 31 and n * (2 ** 30 + 1) < 2 ** 63                  # the header's bounds


def test_density_of_the_lattice_plane_and_trimming():
    from bdm_amd.surface import mesh_stats, trim_by_density
    pts, nrm, R, s, cycles = P.case_inputs("lattice_plane_R32_s3_c4")
    m = P.case_ref("lattice_plane_R32_s3_c4")[0]
    W, cells = m["W"].long(), P.active_cells(m["SW"], m["SU"]).tolist()
    want = []
    for g in cells:                                                                                        # every vertex, in plain integers
        i, j, k = g // (R * R), (g // R) % R, g % R
        want.append(sum(int(W[i + a, j + b, k + c]) for a in (0, 1) for b in (0, 1) for c in (0, 1)))
    assert torch.equal(m["density"], torch.tensor(want, dtype=torch.int64).float() * torch.tensor(1.0 / 32768.0))
    # away from the rim: (points per voxel^2) * pi s^2 / 4 * (1 - h^2 / s^2)^4 at the corners' height h = 0.5 over the sheet
    inv = float(P.splat_of(pts[0], nrm[0], R, s)["inv"])
    per_area = (31.0 / (R - 1 - 2 * (s + 3))) ** 2
    analytic = per_area * math.pi * s * s / 4.0 * (1.0 - 0.25 / (s * s)) ** 4
    v, d = m["verts"], m["density"]
    front = (v[:, 2] - 0.25).abs() * inv < 0.5
    inner = front & (v[:, 0].abs() < 0.5 - (s + 0.5) / inv) & (v[:, 1].abs() < 0.5 - (s + 0.5) / inv)
    print(f"lattice plane: {int(front.sum())} vertices on the sheet, {int((~front).sum())} invented; density inside the rim "
          f"{float(d[inner].min()):.3f} .. {float(d[inner].max()):.3f}, analytic {analytic:.3f}; off the sheet at most {float(d[~front].max()):.3f}")
    assert int(inner.sum()) > 100 and bool(((d[inner] - analytic).abs() < 0.02 * analytic).all())
    assert float(d[~front].max()) < 0.05 * analytic
    tv, tf, td = trim_by_density(m["verts"], m["faces"], d, 0.5 * analytic)
    keep = d >= 0.5 * analytic
    assert torch.equal(tv, m["verts"][keep]) and torch.equal(td, d[keep]) and bool(front[keep].all())      # the back is gone, order kept
    old_id = torch.nonzero(keep)[:, 0]
    kept_faces = m["faces"].long()[keep[m["faces"].long()].all(dim=1)]
    assert torch.equal(old_id[tf], kept_faces) and tf.shape[0] > 0
    st = mesh_stats(tv, tf)
    assert st["open_edges"] > 0 and abs(st["area"] - 1.0) < 0.15                                           # a unit square again, open
    with pytest.raises(ValueError):
        trim_by_density(m["verts"], m["faces"], d[:-1], 1.0)
    none = trim_by_density(m["verts"], m["faces"], d, 1e9)
    assert none[0].shape == (0, 3) and none[1].shape == (0, 3)


def test_bad_arguments_and_the_resolution_snap():
    from bdm_amd import _lib as L
    from bdm_amd import surface as M
    assert M.POISSON_RESOLUTIONS == P.ACCEPTED and M.DEFAULT_CYCLES == P.DEFAULT_CYCLES
    assert all(M.nearest_poisson_resolution(R) == P.nearest_accepted(R) for R in range(1, 400))
    assert [M.nearest_poisson_resolution(R) for R in (72, 88, 104, 120, 136, 144, 208, 240, 20)] == [64, 80, 96, 112, 128, 128, 192, 224, 16]
    # the default: the accepted resolution nearest to default_resolution(n); 72 at 20000 points is not accepted
    assert [M._check_poisson(n, None, 0.0, None)[0] for n in (100, 4096, 6000, 16384, 20000, 65536)] == [16, 32, 40, 64, 64, 128]
    p, nr = torch.zeros(2, 100, 3), torch.zeros(2, 100, 3)
    for R in (72, 36, 20, 255):
        with pytest.raises(ValueError, match=f"nearest accepted one is {P.nearest_accepted(R)}"):
            M.reconstruct_surface(p, nr, method="poisson", resolution=R)
    for kw in (dict(min_weight=0.05), dict(min_weight=float("nan")), dict(cycles=0), dict(cycles=33), dict(support=5), dict(resolution=8)):
        with pytest.raises(ValueError):
            M.reconstruct_surface(p, nr, method="poisson", **kw)
    with pytest.raises(ValueError, match="min_weight"):
        M.reconstruct_surface(p, nr, method="poisson", min_weight=0.5)
    for kw in (dict(method="screened"), dict(cycles=4), dict(return_density=True), dict(return_grid="all")):
        with pytest.raises(ValueError):
            M.reconstruct_surface(p, nr, **kw)
    with pytest.raises(ValueError):
        M.reconstruct_surface(p[0], nr[0], method="poisson")
    with pytest.raises(L.BdmHipError):                                                                     # host tensors: no CPU path
        M.reconstruct_surface(p, nr, method="poisson")
    for argv in (["--method", "poisson", "--resolution", "72"], ["--cycles", "3"], ["--trim-density", "1.0"], ["--method", "poisson", "--cycles", "0"]):
        with pytest.raises(SystemExit):
            M.parse_args(["--in_dir", "a", "--out_dir", "b", *argv])
    assert M.parse_args(["--in_dir", "a", "--out_dir", "b"]).method == "imls"


def test_command_line_walk_with_the_restatement(tmp_path, monkeypatch, capsys):
    from bdm_amd import surface as M
    from bdm_amd.io import load_mesh_ply, save_pointcloud_ply_normals
    sphere, plane = S.sphere(torch.Generator().manual_seed(3305), 300), S.lattice_plane(32)
    save_pointcloud_ply_normals(sphere[0].numpy(), sphere[1].numpy(), tmp_path / "in" / "sphere.ply")
    save_pointcloud_ply_normals(plane[0].numpy(), plane[1].numpy(), tmp_path / "in" / "a" / "plane.ply")
    calls = []

    def restated(points, normals, *, resolution, support, method, cycles, return_density, return_info):
        assert method == "poisson" and return_density and return_info
        calls.append((tuple(points.shape), resolution, cycles))
        out = P.reconstruct_batch(points, normals, resolution, support, cycles)
        info = {"counts": torch.tensor([o["counts"] for o in out], dtype=torch.int32), "border_raised": torch.tensor([o["border_raised"] for o in out])}
        return [o["verts"] for o in out], [o["faces"].long() for o in out], [o["density"] for o in out], info

    monkeypatch.setattr(M, "reconstruct_surface", restated)
    base = ["--in_dir", str(tmp_path / "in"), "--method", "poisson", "--resolution", "32", "--cycles", "3"]
    res = M.main([*base, "--out_dir", str(tmp_path / "out")], device="cpu")
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == res
    want = {"sphere.ply": P.reconstruct(*sphere, 32, 3, 3), "a/plane.ply": P.reconstruct(*plane, 32, 3, 3)}
    assert sorted(calls) == [((1, 300, 3), 32, 3), ((1, 1024, 3), 32, 3)]
    for rel, ref in want.items():
        v, f = load_mesh_ply(tmp_path / "out" / rel)
        assert np.array_equal(v.view(np.int32), ref["verts"].numpy().view(np.int32)) and np.array_equal(f, ref["faces"].numpy())
    assert res["files"] == 2 and res["skipped_quads"] == 0 and res["open_edge_fraction"] == 0.0
    assert res["vertices"] == sum(r["counts"][0] for r in want.values()) and res["faces"] == sum(r["counts"][1] for r in want.values())
    assert res["border_raised"] == want["a/plane.ply"]["border_raised"] > 0 == want["sphere.ply"]["border_raised"]
    cut = 8.0
    trimmed = M.main([*base, "--out_dir", str(tmp_path / "trimmed"), "--trim-density", str(cut)], device="cpu")
    v, f = load_mesh_ply(tmp_path / "trimmed" / "a" / "plane.ply")
    keep = want["a/plane.ply"]["density"] >= cut
    assert np.array_equal(v.view(np.int32), want["a/plane.ply"]["verts"][keep].numpy().view(np.int32)) and 0 < v.shape[0] < keep.numel()
    assert trimmed["open_edge_fraction"] > 0.0 and trimmed["vertices"] < res["vertices"] and trimmed["border_raised"] == res["border_raised"]
