"""Colouring entry point: paints the clouds a sample_* job wrote, with the PC^2 colouring model (model=coloring_model), from the
same image and camera they were reconstructed from.  Same `group.key=value` overrides as the other entry points.

Reads  ${run.coloring_sample_dir}/pred/<category>/<name>.ply  (the tree main.py / main_blending.py / main_merging.py write; also
<name>-<k>.ply when run.num_samples > 1), looks every <name> up in the dataset, and writes
${run.coloring_sample_dir}/colored/<category>/<name>.ply with uchar red / green / blue per vertex.

    python main_blending.py run.job=sample_bdm_blending dataset=synthetic run.num_samples=1 dataset.max_points=1024
    python main_coloring.py dataset=synthetic run.coloring_sample_dir=<the directory the first command printed>
"""
import sys
from pathlib import Path

import torch

from main_blending import get_dataloader


def parse_args(argv):
    """The project configuration with the colouring model group selected (model=coloring_model is the default here)."""
    from bdm_amd.config import PointCloudColoringModelConfig, ProjectConfig, parse_overrides
    cfg = ProjectConfig()
    cfg.model = PointCloudColoringModelConfig()
    cfg = parse_overrides(argv, cfg)
    if not cfg.run.coloring_sample_dir:
        raise ValueError("run.coloring_sample_dir=<directory holding pred/<category>/<name>.ply> is required")
    return cfg


def build_model(cfg, device):
    from bdm_amd.model import get_coloring_model
    from bdm_amd.utils.procedural import fill_module_
    model = get_coloring_model(cfg)
    if cfg.checkpoint.resume:
        state = torch.load(cfg.checkpoint.resume, map_location="cpu")["model"]
        state = {k.replace("module.", "", 1) if k.startswith("module.") else k: v for k, v in state.items()}
        print("load_state_dict:", model.load_state_dict(state, strict=False))
    else:
        print("checkpoint.resume not given: procedural random-init weights (benchmark mode)")
        fill_module_(model, seed=cfg.run.seed)
    return model.to(device).eval()


def predictions_of(sample_dir, category, name):
    """The clouds of one dataset entry under <sample_dir>/pred: <name>.ply and <name>-<k>.ply, sorted."""
    d = Path(sample_dir) / "pred" / category
    hits = [d / f"{name}.ply"] if (d / f"{name}.ply").exists() else []
    hits += sorted(p for p in d.glob(f"{name}-*.ply") if p.stem[len(name) + 1:].isdigit())
    return hits


def color_tree(cfg, batches, color_fn, device="cpu"):
    """Walk the dataset, colour every cloud found under the sample directory, write colored/<category>/<stem>.ply; returns the paths
    written.  color_fn(batch, points (B, n, 3)) -> colours (B, n, 3) in [0, 1].  A batch is coloured in one call per distinct
    (sample index, point count): rows of entries without such a cloud carry a copy of another entry's cloud and are not written
    (the model treats the shapes of a batch independently)."""
    from bdm_amd.io import load_pointcloud_ply, save_pointcloud_ply_rgb
    root, written = Path(cfg.run.coloring_sample_dir), []
    for batch_idx, batch in enumerate(batches):
        if cfg.run.num_sample_batches is not None and batch_idx >= cfg.run.num_sample_batches:
            break
        batch = batch.to(device)
        found = {}   # (position in the entry's list, point count) -> {row: (path, cloud)}
        for i, (name, cat) in enumerate(zip(batch.sequence_name, batch.sequence_category)):
            for k, path in enumerate(predictions_of(root, cat, name)):
                pts = torch.from_numpy(load_pointcloud_ply(path))
                found.setdefault((k, pts.shape[0]), {})[i] = (path, pts)
        for key in sorted(found):
            rows = found[key]
            filler = rows[min(rows)][1]
            points = torch.stack([rows[i][1] if i in rows else filler for i in range(len(batch.sequence_name))]).to(device)
            colors = color_fn(batch, points)
            for i, (path, pts) in sorted(rows.items()):
                out = root / "colored" / batch.sequence_category[i] / path.name
                save_pointcloud_ply_rgb(pts.numpy(), colors[i].detach().cpu().numpy(), out)
                written.append(out)
    return written


def main(argv=None):
    from bdm_amd.distributed import barrier, gpu_turn, init_from_env
    cfg = parse_args(sys.argv[1:] if argv is None else argv)
    rank, local_rank, world = init_from_env()
    device = torch.device("cuda", local_rank)
    torch.cuda.set_device(device)
    torch.manual_seed(cfg.run.seed + rank)
    model = build_model(cfg, device)

    def color_fn(batch, points):
        with gpu_turn(device):
            pc = model._forward(pc=points, camera=batch.camera, image_rgb=batch.image_rgb, mask=batch.fg_probability,
                                return_point_cloud=True, noise_std=0.0)   # (run.coloring_training_noise_std jitters the TRAINING inputs only)
        return pc.features_padded()

    written = color_tree(cfg, get_dataloader(cfg, rank, world), color_fn, device)
    barrier()
    print(f"rank {rank}: coloured {len(written)} clouds under {(Path(cfg.run.coloring_sample_dir) / 'colored').absolute()}")
    return written


if __name__ == "__main__":
    main()
