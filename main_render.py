"""Rendering entry point: turns the clouds a sample_* job (and main_coloring.py) wrote into pictures, each from the camera of its
dataset entry -- what the reference does inside its sample job (experiments/main.py:418-430, diffusion_utils.py:185-295).  Same
`group.key=value` overrides as the other entry points.

Reads  ${run.render_sample_dir}/{gt,pred,colored}/<category>/<name>.ply  (also <name>-<k>.ply when run.num_samples > 1; `colored`
only where main_coloring.py has written it), looks every <name> up in the dataset, and writes
${run.render_sample_dir}/renders/{gt,pred,colored}/<category>/<stem>.png.  With run.render_num_frames = F > 1 it also writes the
orbiting orthographic view of every predicted cloud (the coloured one where it exists) as renders/orbit/<category>/<stem>-<f>.png.
With run.render_shading=normals the uncoloured kinds (gt, pred, the orbit of an uncoloured prediction) are lit by their estimated
normals (bdm_amd.normals, run.render_normals_k neighbours) instead of rendering as black silhouettes; `colored` is untouched.
run.render_shading=oriented does the same with normals oriented by visibility voting and one-sided shading.
Where ${run.render_sample_dir}/${run.render_mesh_subdir} exists (the tree `python -m bdm_amd.surface` writes), every triangle mesh
<category>/<name>.ply or <name>-<k>.ply in it is drawn from its entry's camera as renders/mesh/<category>/<stem>.png
(run.render_mesh_shading = smooth | flat | none), and with run.render_num_frames > 1 its orbit as
renders/mesh_orbit/<category>/<stem>-<f>.png; a file without a face element is a cloud and is left alone.
Where ${run.render_sample_dir}/${run.render_colored_mesh_subdir} exists (the tree `python -m bdm_amd.mesh_color` writes), every mesh
in it that carries vertex colours is drawn lit, its colours as the albedo, as renders/colored_mesh/<category>/<stem>.png, and with
run.render_num_frames > 1 its orbit as renders/colored_mesh_orbit/<category>/<stem>-<f>.png.

    python main_blending.py run.job=sample_bdm_blending dataset=synthetic run.num_samples=1 dataset.max_points=1024
    python main_render.py dataset=synthetic run.render_sample_dir=<the directory the first command printed>
    python -m bdm_amd.surface --in_dir <that directory>/pred --out_dir <that directory>/pred_mesh     (then the line above again)
    python -m bdm_amd.mesh_color --mesh_dir <that directory>/pred_mesh --color_dir <that directory>/colored --out_dir <that directory>/colored_mesh
"""
import sys
from pathlib import Path

import torch

from main_blending import get_dataloader

KINDS = ("gt", "pred", "colored")
SHADINGS = ("none", "normals", "oriented")
MESH_SHADINGS = ("smooth", "flat", "none")


def parse_args(argv):
    from bdm_amd.config import parse_overrides
    cfg = parse_overrides(argv)
    if not cfg.run.render_sample_dir:
        raise ValueError("run.render_sample_dir=<directory holding pred/<category>/<name>.ply> is required")
    if cfg.run.render_num_frames < 1 or 360 % cfg.run.render_num_frames:
        raise ValueError("run.render_num_frames must divide 360")
    if cfg.run.render_shading not in SHADINGS:
        raise ValueError(f"run.render_shading={cfg.run.render_shading!r}: expected one of {SHADINGS}")
    if cfg.run.render_mesh_shading not in MESH_SHADINGS:
        raise ValueError(f"run.render_mesh_shading={cfg.run.render_mesh_shading!r}: expected one of {MESH_SHADINGS}")
    return cfg


def clouds_of(sample_dir, kind, category, name):
    """The clouds of one dataset entry under <sample_dir>/<kind>: <name>.ply and <name>-<k>.ply, sorted."""
    d = Path(sample_dir) / kind / category
    hits = [d / f"{name}.ply"] if (d / f"{name}.ply").exists() else []
    hits += sorted(p for p in d.glob(f"{name}-*.ply") if p.stem[len(name) + 1:].isdigit())
    return hits


def meshes_of(sample_dir, subdir, category, name, with_colors=False):
    """The triangle meshes of one dataset entry under <sample_dir>/<subdir>: [(path, verts (V, 3) float32, faces (F, 3) int64)] of
    <name>.ply and <name>-<k>.ply, sorted; a file without a face element is a cloud and is not among them.
    with_colors=True: [(path, verts, faces, colors (V, 3) float32)] of the meshes that carry vertex colours only."""
    from bdm_amd.io import load_mesh_ply
    out = []
    for path in clouds_of(sample_dir, subdir, category, name):
        with open(path, "rb") as f:
            head = f.read(4096).split(b"end_header")[0]
        if b"element face" in head:
            if not with_colors:
                out.append((path, *load_mesh_ply(path)))
            elif b"property uchar red" in head or b"property uint8 red" in head:
                out.append((path, *load_mesh_ply(path, with_colors=True)))
    return out


def render_tree(cfg, batches, render_fn, orbit_fn=None, device="cpu", shade_fn=None, mesh_fn=None, mesh_orbit_fn=None,
                colored_mesh_fn=None, colored_mesh_orbit_fn=None):
    """Walk the dataset, render every cloud found under the sample directory, write renders/<kind>/<category>/<stem>.png; returns
    the paths written.  render_fn(cameras (list of single cameras), points (B, n, 3), colours (B, n, 3) or None) -> images
    (B, H, W, 3) in [0, 1]: one call per batch, kind and distinct point count.  orbit_fn(points (1, n, 3), colours or None,
    path of <stem>.png, num_frames) -> the paths it wrote: called per predicted cloud when run.render_num_frames > 1.
    shade_fn(cameras, points (B, n, 3)) -> colours (B, n, 3): with run.render_shading=normals or oriented the uncoloured kinds get
    their colours from it, once per batch group (a config without the key, or "none", leaves them None as before).
    Where <sample_dir>/<run.render_mesh_subdir> exists: mesh_fn(cameras, verts_list, faces_list) -> images (B, H, W, 3), one call
    per batch, written as renders/mesh/<category>/<stem>.png; mesh_orbit_fn(verts (V, 3), faces (F, 3), path of <stem>.png,
    num_frames) -> the paths it wrote, per mesh when run.render_num_frames > 1.  Without that directory nothing changes.
    Where <sample_dir>/<run.render_colored_mesh_subdir> exists: colored_mesh_fn(cameras, verts_list, faces_list, colors_list) ->
    images, written as renders/colored_mesh/<category>/<stem>.png; colored_mesh_orbit_fn(verts, faces, colors, path, num_frames) ->
    the paths it wrote under renders/colored_mesh_orbit/.  Without that directory nothing changes either."""
    from bdm_amd.io import load_pointcloud_ply, save_image_png
    root, written = Path(cfg.run.render_sample_dir), []
    shading = getattr(cfg.run, "render_shading", "none")
    if shading not in SHADINGS:
        raise ValueError(f"run.render_shading={shading!r}: expected one of {SHADINGS}")
    if shading != "none" and shade_fn is None:
        raise ValueError(f"run.render_shading={shading} needs a shade_fn")
    mesh_subdir = getattr(cfg.run, "render_mesh_subdir", "pred_mesh")
    with_meshes = bool(mesh_subdir) and (root / mesh_subdir).is_dir()
    if with_meshes and mesh_fn is None:
        raise ValueError(f"{root / mesh_subdir} holds meshes: they need a mesh_fn")
    colored_subdir = getattr(cfg.run, "render_colored_mesh_subdir", "colored_mesh")
    with_colored = bool(colored_subdir) and (root / colored_subdir).is_dir()
    if with_colored and colored_mesh_fn is None:
        raise ValueError(f"{root / colored_subdir} holds coloured meshes: they need a colored_mesh_fn")
    for batch_idx, batch in enumerate(batches):
        if cfg.run.num_sample_batches is not None and batch_idx >= cfg.run.num_sample_batches:
            break
        batch = batch.to(device)
        cam = batch.camera   # a list of single cameras (the datasets' collation), or one batched camera
        cameras = list(cam) if isinstance(cam, (list, tuple)) else [
            type(cam)(cam.focal_length[i:i + 1], cam.principal_point[i:i + 1], cam.R[i:i + 1], cam.T[i:i + 1], device=cam.device)
            for i in range(len(cam))]
        groups = {}   # (kind, point count) -> [(row of the batch, path, points, colours or None)]
        for i, (name, cat) in enumerate(zip(batch.sequence_name, batch.sequence_category)):
            for kind in KINDS:
                for path in clouds_of(root, kind, cat, name):
                    if kind == "colored":
                        pts, col = load_pointcloud_ply(path, with_colors=True)
                        col = torch.from_numpy(col)
                    else:
                        pts, col = load_pointcloud_ply(path), None
                    groups.setdefault((kind, pts.shape[0]), []).append((i, path, torch.from_numpy(pts), col))
        for (kind, _), items in sorted(groups.items()):
            points = torch.stack([it[2] for it in items]).to(device)
            colors = torch.stack([it[3] for it in items]).to(device) if kind == "colored" else None
            cams = [cameras[it[0]] for it in items]
            if colors is None and shading != "none":
                colors = shade_fn(cams, points)
            images = render_fn(cams, points, colors)
            for (i, path, _, _), image in zip(items, images):
                out = root / "renders" / kind / batch.sequence_category[i] / f"{path.stem}.png"
                save_image_png(image.detach().cpu().permute(2, 0, 1).numpy(), out)
                written.append(out)
        if cfg.run.render_num_frames > 1 and orbit_fn is not None:
            for (kind, _), items in sorted(groups.items()):
                for i, path, pts, col in items:
                    cat = batch.sequence_category[i]
                    if kind == "gt" or (kind == "pred" and (root / "colored" / cat / path.name).exists()):
                        continue   # the orbit shows each prediction once, coloured where a coloured copy exists
                    out = root / "renders" / "orbit" / cat / f"{path.stem}.png"
                    written += [Path(p) for p in orbit_fn(pts[None].to(device), None if col is None else col[None].to(device), out,
                                                          cfg.run.render_num_frames)]
        if with_meshes:
            found = [(i, *item) for i, (name, cat) in enumerate(zip(batch.sequence_name, batch.sequence_category))
                     for item in meshes_of(root, mesh_subdir, cat, name)]
            if found:
                verts = [torch.from_numpy(v).to(device) for _, _, v, _ in found]
                faces = [torch.from_numpy(f).to(device) for _, _, _, f in found]
                images = mesh_fn([cameras[i] for i, _, _, _ in found], verts, faces)
                for (i, path, _, _), image in zip(found, images):
                    out = root / "renders" / "mesh" / batch.sequence_category[i] / f"{path.stem}.png"
                    save_image_png(image.detach().cpu().permute(2, 0, 1).numpy(), out)
                    written.append(out)
                if cfg.run.render_num_frames > 1 and mesh_orbit_fn is not None:
                    for (i, path, _, _), v, f in zip(found, verts, faces):
                        out = root / "renders" / "mesh_orbit" / batch.sequence_category[i] / f"{path.stem}.png"
                        written += [Path(p) for p in mesh_orbit_fn(v, f, out, cfg.run.render_num_frames)]
        if with_colored:
            found = [(i, *item) for i, (name, cat) in enumerate(zip(batch.sequence_name, batch.sequence_category))
                     for item in meshes_of(root, colored_subdir, cat, name, with_colors=True)]
            if found:
                verts = [torch.from_numpy(v).to(device) for _, _, v, _, _ in found]
                faces = [torch.from_numpy(f).to(device) for _, _, _, f, _ in found]
                colors = [torch.from_numpy(c).to(device) for _, _, _, _, c in found]
                images = colored_mesh_fn([cameras[it[0]] for it in found], verts, faces, colors)
                for (i, path, *_), image in zip(found, images):
                    out = root / "renders" / "colored_mesh" / batch.sequence_category[i] / f"{path.stem}.png"
                    save_image_png(image.detach().cpu().permute(2, 0, 1).numpy(), out)
                    written.append(out)
                if cfg.run.render_num_frames > 1 and colored_mesh_orbit_fn is not None:
                    for (i, path, *_), v, f, c in zip(found, verts, faces, colors):
                        out = root / "renders" / "colored_mesh_orbit" / batch.sequence_category[i] / f"{path.stem}.png"
                        written += [Path(p) for p in colored_mesh_orbit_fn(v, f, c, out, cfg.run.render_num_frames)]
    return written


def main(argv=None):
    from bdm_amd.cameras import Meshes, Pointclouds
    from bdm_amd.distributed import barrier, gpu_turn, init_from_env
    from bdm_amd.render import (render_mesh_batch, render_pointcloud_batch_pytorch3d, shade_by_normals, visualize_mesh_batch,
                                visualize_pointcloud_batch_pytorch3d)
    cfg = parse_args(sys.argv[1:] if argv is None else argv)
    rank, local_rank, world = init_from_env()
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)

    def render_fn(cameras, points, colors):
        with gpu_turn(device):
            return render_pointcloud_batch_pytorch3d(cameras, Pointclouds(points, colors)).cpu()

    oriented = cfg.run.render_shading == "oriented"   # visibility-oriented normals, lit one-sided

    def normals_of(points):
        from bdm_amd.normals import estimate_pointcloud_normals
        return estimate_pointcloud_normals(points, cfg.run.render_normals_k, "visibility" if oriented else True)

    def shade_fn(cameras, points):
        with gpu_turn(device):
            return shade_by_normals(points, normals_of(points), cameras, two_sided=not oriented)

    def orbit_fn(points, colors, path, num_frames):
        if colors is None and cfg.run.render_shading != "none":
            return shaded_orbit(points, path, num_frames)
        with gpu_turn(device):
            visualize_pointcloud_batch_pytorch3d(Pointclouds(points, colors), output_file_image=str(path), num_frames=num_frames,
                                                 scale_factor=cfg.model.scale_factor)
        return [path.with_name(f"{path.stem}-{f}.png") for f in range(num_frames)]

    def shaded_orbit(points, path, num_frames):
        """The orbit of visualize_pointcloud_batch_pytorch3d (same cameras, same file names), every frame lit from its camera."""
        from bdm_amd.cameras import OrthographicCameras, look_at_view_transform
        out = [path.with_name(f"{path.stem}-{f}.png") for f in range(num_frames)]
        with gpu_turn(device):
            normals = normals_of(points)
            R, T = look_at_view_transform(dist=10.0, elev=30, azim=list(range(0, 360, 360 // num_frames)), degrees=True, device=device)
            for f in range(num_frames):
                cam = OrthographicCameras(focal_length=0.25 * cfg.model.scale_factor, device=device, R=R[f:f + 1], T=T[f:f + 1])
                visualize_pointcloud_batch_pytorch3d(Pointclouds(points, shade_by_normals(points, normals, cam, two_sided=not oriented)),
                                                     output_file_image=str(out[f]), cameras=cam)
        return out

    def mesh_fn(cameras, verts, faces):
        with gpu_turn(device):
            return render_mesh_batch(cameras, Meshes(verts, faces), shading=cfg.run.render_mesh_shading).cpu()

    def mesh_orbit_fn(verts, faces, path, num_frames):
        with gpu_turn(device):
            visualize_mesh_batch(Meshes([verts], [faces]), output_file_image=str(path), num_frames=num_frames,
                                 scale_factor=cfg.model.scale_factor, shading=cfg.run.render_mesh_shading)
        return [path.with_name(f"{path.stem}-{f}.png") for f in range(num_frames)]

    lit = "smooth" if cfg.run.render_mesh_shading == "none" else cfg.run.render_mesh_shading   # the colours are an albedo: always lit

    def colored_mesh_fn(cameras, verts, faces, colors):
        with gpu_turn(device):
            return render_mesh_batch(cameras, Meshes(verts, faces), shading=lit, vert_albedo=torch.cat(colors)).cpu()

    def colored_mesh_orbit_fn(verts, faces, colors, path, num_frames):
        with gpu_turn(device):
            visualize_mesh_batch(Meshes([verts], [faces]), output_file_image=str(path), num_frames=num_frames,
                                 scale_factor=cfg.model.scale_factor, shading=lit, vert_albedo=colors)
        return [path.with_name(f"{path.stem}-{f}.png") for f in range(num_frames)]

    written = render_tree(cfg, get_dataloader(cfg, rank, world), render_fn, orbit_fn, device, shade_fn, mesh_fn, mesh_orbit_fn,
                          colored_mesh_fn, colored_mesh_orbit_fn)
    barrier()
    print(f"rank {rank}: rendered {len(written)} images under {(Path(cfg.run.render_sample_dir) / 'renders').absolute()}")
    return written


if __name__ == "__main__":
    main()
