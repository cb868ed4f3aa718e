"""File output of the sample_* jobs.  The reference writes point clouds with pytorch3d.io.IO().save_pointcloud
(main_blending.py:427-445; binary little-endian PLY with float32 x, y, z -- pytorch3d's default) and the input image with
torchvision's to_pil_image(...).save(png) (main_blending.py:447-455).  Host-side, outside the timed path."""
import os

import numpy as np


def save_pointcloud_ply(points, path, binary=True):
    """float32 vertices, exact round trip in the (default) binary form."""
    pts = np.ascontiguousarray(np.asarray(points, dtype="<f4").reshape(-1, 3))
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    fmt = "binary_little_endian" if binary else "ascii"
    header = (f"ply\nformat {fmt} 1.0\nelement vertex {pts.shape[0]}\nproperty float x\nproperty float y\n"
              "property float z\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        if binary:
            f.write(pts.tobytes())
        else:
            np.savetxt(f, pts, fmt="%.9g")


def save_pointcloud_ply_rgb(points, colors, path):
    """Binary little-endian PLY with float32 x, y, z and uchar red, green, blue per vertex (what pytorch3d's save_pointcloud writes
    for a coloured cloud with colors_as_uint8=True); colours in [0, 1] are stored as round(255 c)."""
    pts = np.asarray(points, dtype="<f4").reshape(-1, 3)
    col = np.asarray(colors, dtype=np.float64).reshape(-1, 3)
    if col.shape[0] != pts.shape[0]:
        raise ValueError(f"{pts.shape[0]} points but {col.shape[0]} colours")
    rec = np.empty(pts.shape[0], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
    rec["xyz"] = pts
    rec["rgb"] = np.rint(np.clip(col, 0.0, 1.0) * 255.0).astype(np.uint8)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {pts.shape[0]}\nproperty float x\nproperty float y\n"
              "property float z\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(rec.tobytes())


def save_pointcloud_ply_normals(points, normals, path):
    """Binary little-endian PLY with float32 x, y, z, nx, ny, nz per vertex (what MeshLab and Open3D read as oriented points)."""
    pts = np.asarray(points, dtype="<f4").reshape(-1, 3)
    nrm = np.asarray(normals, dtype="<f4").reshape(-1, 3)
    if nrm.shape[0] != pts.shape[0]:
        raise ValueError(f"{pts.shape[0]} points but {nrm.shape[0]} normals")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {pts.shape[0]}\nproperty float x\nproperty float y\n"
              "property float z\nproperty float nx\nproperty float ny\nproperty float nz\nend_header\n")
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(np.ascontiguousarray(np.concatenate([pts, nrm], axis=1)).tobytes())


def _ply_normals(props, column):
    """Per-vertex normals (n, 3) float32 from the nx / ny / nz properties; column(i) as in _ply_colors."""
    names = [p[2] for p in props]
    if not all(c in names for c in ("nx", "ny", "nz")):
        raise ValueError("the PLY has no nx / ny / nz vertex properties")
    return np.stack([column(names.index(c)).astype(np.float32) for c in ("nx", "ny", "nz")], axis=1)


def _ply_colors(props, column):
    """Per-vertex colours in [0, 1] from the red / green / blue properties (uchar: / 255; float: as stored); column(i) -> the
    values of property i as a numpy array."""
    names = [p[2] for p in props]
    if not all(c in names for c in ("red", "green", "blue")):
        raise ValueError("the PLY has no red / green / blue vertex properties")
    cols = []
    for c in ("red", "green", "blue"):
        i = names.index(c)
        v = column(i).astype(np.float32)
        cols.append(v / np.float32(255.0) if props[i][1] in ("uchar", "uint8") else v)
    return np.stack(cols, axis=1)


def _ply_vertex_props(head):
    """The property lines of the vertex element (a mesh file has a face element with a list property behind it)."""
    props, element = [], None
    for l in head:
        if l.startswith("element"):
            element = l.split()[1]
        elif l.startswith("property") and element == "vertex":
            props.append(l.split())
    return props


def save_mesh_ply(verts, faces, path, colors=None):
    """Binary little-endian PLY of a triangle mesh: float32 x, y, z per vertex, then per face a uchar count (3) and three int32
    vertex indices (`property list uchar int vertex_indices`: what MeshLab, Open3D and pytorch3d read).
    colors (V, 3) in [0, 1]: uchar red, green, blue per vertex as well, under save_pointcloud_ply_rgb's conversion
    rint(clip(c, 0, 1) * 255); without colours the file is what it was before the argument existed."""
    v = np.ascontiguousarray(np.asarray(verts, dtype="<f4").reshape(-1, 3))
    f = np.asarray(faces).reshape(-1, 3)
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError(f"face indices outside 0..{v.shape[0] - 1}")
    rec = np.empty(f.shape[0], dtype=[("count", "u1"), ("idx", "<i4", 3)])
    rec["count"], rec["idx"] = 3, f
    color_props = ""
    if colors is not None:
        col = np.asarray(colors, dtype=np.float64).reshape(-1, 3)
        if col.shape[0] != v.shape[0]:
            raise ValueError(f"{v.shape[0]} vertices but {col.shape[0]} colours")
        vrec = np.empty(v.shape[0], dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)])
        vrec["xyz"] = v
        vrec["rgb"] = np.rint(np.clip(col, 0.0, 1.0) * 255.0).astype(np.uint8)
        v, color_props = vrec, "property uchar red\nproperty uchar green\nproperty uchar blue\n"
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    header = (f"ply\nformat binary_little_endian 1.0\nelement vertex {v.shape[0]}\nproperty float x\nproperty float y\n"
              f"property float z\n{color_props}element face {f.shape[0]}\nproperty list uchar int vertex_indices\nend_header\n")
    with open(path, "wb") as out:
        out.write(header.encode("ascii"))
        out.write(v.tobytes())
        out.write(rec.tobytes())


def load_mesh_ply(path, with_colors=False):
    """(verts (V, 3) float32, faces (F, 3) int64) from a binary little-endian PLY in save_mesh_ply's form: a vertex element that
    holds float x, y, z, optionally followed by uchar red, green, blue, then triangles as `property list uchar int vertex_indices`.
    with_colors=True: (verts, faces, colors), colors (V, 3) float32 in [0, 1], or None for a file that carries none."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    if [l for l in head if l.startswith("format")][0].split()[1] != "binary_little_endian":
        raise ValueError(f"{path}: only binary little-endian mesh files are read")
    props = [p[1:] for p in _ply_vertex_props(head)]
    xyz = ([["float", c] for c in "xyz"], [["float32", c] for c in "xyz"])
    rgb = ([["uchar", c] for c in ("red", "green", "blue")], [["uint8", c] for c in ("red", "green", "blue")])
    colored = len(props) == 6 and props[:3] in xyz and props[3:] in rgb
    if props not in xyz and not colored:
        raise ValueError(f"{path}: the vertex element must hold float x, y, z only, or those and uchar red, green, blue")
    faces_line = [l for l in head if l.startswith("element face")]
    if not faces_line or not any(l.split()[:4] in (["property", "list", "uchar", "int"], ["property", "list", "uint8", "int32"]) for l in head):
        raise ValueError(f"{path}: no face element with a `list uchar int` property")
    nv, nf = int([l for l in head if l.startswith("element vertex")][0].split()[-1]), int(faces_line[0].split()[-1])
    colors = None
    if colored:
        vrec = np.frombuffer(raw, dtype=[("xyz", "<f4", 3), ("rgb", "u1", 3)], count=nv, offset=end)
        verts, colors = vrec["xyz"].astype(np.float32), vrec["rgb"].astype(np.float32) / np.float32(255.0)
    else:
        verts = np.frombuffer(raw, dtype="<f4", count=3 * nv, offset=end).reshape(nv, 3).astype(np.float32)
    rec = np.frombuffer(raw, dtype=[("count", "u1"), ("idx", "<i4", 3)], count=nf, offset=end + (15 if colored else 12) * nv)
    if nf and not (rec["count"] == 3).all():
        raise ValueError(f"{path}: only triangles are read")
    faces = rec["idx"].astype(np.int64)
    return (verts, faces, colors) if with_colors else (verts, faces)


def load_pointcloud_ply(path, with_colors=False, with_normals=False):
    """(n, 3) float32 from an ASCII or binary-little-endian PLY whose vertex element starts with float x, y, z.
    with_colors=True: (points, colors), colors (n, 3) float32 in [0, 1] from its red / green / blue properties.
    with_normals=True: the normals (n, 3) float32 from its nx / ny / nz properties come last: (points, normals) or
    (points, colors, normals)."""
    def result(pts, column):
        out = (pts,) + ((_ply_colors(props, column),) if with_colors else ()) + ((_ply_normals(props, column),) if with_normals else ())
        return out if len(out) > 1 else pts
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    n = int([l for l in head if l.startswith("element vertex")][0].split()[-1])
    fmt = [l for l in head if l.startswith("format")][0].split()[1]
    props = _ply_vertex_props(head)
    if fmt == "ascii":
        rows = raw[end:].decode("ascii").split("\n")[:n]
        pts = np.array([[float(v) for v in r.split()[:3]] for r in rows], dtype=np.float32).reshape(-1, 3)
        if not (with_colors or with_normals):
            return pts
        table = np.array([[float(v) for v in r.split()] for r in rows], dtype=np.float64).reshape(n, -1)
        return result(pts, lambda i: table[:, i])
    if fmt != "binary_little_endian":
        raise ValueError(f"{path}: unsupported PLY format {fmt}")
    sizes = {"float": 4, "float32": 4, "double": 8, "float64": 8, "uchar": 1, "uint8": 1, "int": 4, "int32": 4}
    stride = sum(sizes[p[1]] for p in props)
    if [p[1] for p in props[:3]] not in (["float"] * 3, ["float32"] * 3):
        raise ValueError(f"{path}: vertex element must start with float x, y, z")
    body = np.frombuffer(raw, dtype=np.uint8, count=n * stride, offset=end).reshape(n, stride)
    pts = np.ascontiguousarray(body[:, :12]).view("<f4").reshape(n, 3).astype(np.float32)
    if not (with_colors or with_normals):
        return pts
    offs = np.cumsum([0] + [sizes[p[1]] for p in props])
    kinds = {"float": "<f4", "float32": "<f4", "double": "<f8", "float64": "<f8", "uchar": "u1", "uint8": "u1", "int": "<i4", "int32": "<i4"}

    def column(i):
        return np.ascontiguousarray(body[:, offs[i]:offs[i + 1]]).view(kinds[props[i][1]]).reshape(n)
    return result(pts, column)


def save_image_png(image_chw, path):
    """torchvision.transforms.functional.to_pil_image(float CHW in [0, 1]).save(path): pic.mul(255).byte(), mode RGB."""
    from PIL import Image
    arr = np.asarray(image_chw, dtype=np.float32)
    arr = (arr * 255.0).astype(np.uint8).transpose(1, 2, 0)  # truncation, as Tensor.byte() does
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(path)


def save_binvox(voxels, path, translate=(0.0, 0.0, 0.0), scale=1.0):
    """A (D, D, D) occupancy grid indexed [x][y][z] as a binvox file (the ShapeNetVox32 form): the header lines `#binvox 1`, `dim D D D`,
    `translate tx ty tz`, `scale s`, `data`, then (value, count) byte pairs over the linear index x D^2 + z D + y, a run of more than
    255 cells split.  The centre of cell i lies at translate + (i + 0.5) scale / D."""
    vox = np.asarray(voxels).astype(bool)
    if vox.ndim != 3 or len(set(vox.shape)) != 1 or vox.shape[0] < 1:
        raise ValueError(f"a binvox grid is cubic, got shape {vox.shape}")
    D = vox.shape[0]
    flat = np.ascontiguousarray(vox.transpose(0, 2, 1)).reshape(-1).astype(np.uint8)
    cuts = np.flatnonzero(np.diff(flat)) + 1                      # where the value changes
    starts, ends = np.concatenate([[0], cuts]), np.concatenate([cuts, [flat.size]])
    pieces = -(-(ends - starts) // 255)                           # runs of at most 255
    value = np.repeat(flat[starts], pieces)
    count = np.full(value.size, 255, dtype=np.int64)
    last = np.cumsum(pieces) - 1
    count[last] = (ends - starts) - 255 * (pieces - 1)
    t = [float(x) for x in np.asarray(translate, dtype=np.float64).reshape(3)]
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as out:
        out.write(f"#binvox 1\ndim {D} {D} {D}\ntranslate {t[0]!r} {t[1]!r} {t[2]!r}\nscale {float(scale)!r}\ndata\n".encode("ascii"))
        out.write(np.stack([value, count.astype(np.uint8)], axis=1).tobytes())


def load_binvox(path):
    """(voxels bool (D, D, D) indexed [x][y][z], translate (3,) float64, scale float) from a binvox file in save_binvox's form.  A grid
    that is not cubic, a header that is not the five lines in that order, an odd number of data bytes, a value other than 0 / 1, a
    zero count or runs that do not add up to D^3 cells raise ValueError."""
    with open(path, "rb") as f:
        raw = f.read()
    lines, at = [], 0
    for _ in range(5):
        end = raw.find(b"\n", at)
        if end < 0:
            raise ValueError(f"{path}: the binvox header ends early")
        lines.append(raw[at:end].decode("ascii", "replace").strip())
        at = end + 1
    try:
        if lines[0].split() != ["#binvox", "1"] or lines[4] != "data":
            raise ValueError("not `#binvox 1` ... `data`")
        dim, tr, sc = lines[1].split(), lines[2].split(), lines[3].split()
        if dim[0] != "dim" or tr[0] != "translate" or sc[0] != "scale" or len(dim) != 4 or len(tr) != 4 or len(sc) != 2:
            raise ValueError("expected dim, translate and scale")
        dims, translate, scale = [int(x) for x in dim[1:]], np.array([float(x) for x in tr[1:]], dtype=np.float64), float(sc[1])
    except (ValueError, IndexError) as e:
        raise ValueError(f"{path}: malformed binvox header: {e}") from None
    if len(set(dims)) != 1 or dims[0] < 1:
        raise ValueError(f"{path}: only cubic grids are read, got dim {dims}")
    D = dims[0]
    body = np.frombuffer(raw, dtype=np.uint8, offset=at)
    if body.size % 2:
        raise ValueError(f"{path}: an odd number of data bytes")
    value, count = body[0::2], body[1::2].astype(np.int64)
    if (value > 1).any() or (count == 0).any() or int(count.sum()) != D ** 3:
        raise ValueError(f"{path}: the runs do not describe {D}^3 cells of 0 / 1")
    vox = np.repeat(value.astype(bool), count).reshape(D, D, D).transpose(0, 2, 1)   # stored [x][z][y]
    return np.ascontiguousarray(vox), translate, scale
