"""Minimal stand-ins for the pytorch3d types that cross the reference's model API
(pytorch3d 0.7.x is a third-party dependency of the reference, README.md:73, not installed here):
`PerspectiveCameras` (call sites dataset/shapenet_r2n2.py:86-93, dataset/pix3d.py:152-159,
model/projection_model.py:134-140) and `Pointclouds` (main_blending.py:346).  Only the fields
the sampling path reads are kept.  Row-vector convention: X_view = X_world @ R + T;
ndc.xy = focal * X_view.xy / X_view.z + principal_point (PerspectiveCameras, in_ndc=True)."""
import math

import torch


class PerspectiveCameras:
    """in_ndc=False (screen-space intrinsics + image_size (H, W), as dataset/pix3d.py:152-159 builds them) is converted
    to NDC at construction with pytorch3d's rule (docs/notes/cameras.md, restated; unpinned: pytorch3d is absent):
        s = min(W, H);  focal_ndc = focal_screen * 2 / s;  principal_ndc = -(principal_screen - (W, H) / 2) * 2 / s"""
    orthographic = False   # (OrthographicCameras below: the same fields, projected without the division by depth)

    def __init__(self, focal_length=1.0, principal_point=((0.0, 0.0),), R=None, T=None, device="cpu", in_ndc=True,
                 image_size=None):
        def as2(v, n):
            v = torch.as_tensor(v, dtype=torch.float32)
            if v.dim() == 0:
                v = v.view(1, 1).expand(n, 2)
            elif v.dim() == 1:
                v = v.view(-1, 1).expand(-1, 2) if v.shape[0] == n and n != 2 else v.view(1, -1).expand(n, -1)
            elif v.shape[0] == 1:
                v = v.expand(n, -1)   # one row for n cameras (the default principal point with batched R, T)
            return v.contiguous()
        R = torch.eye(3)[None] if R is None else torch.as_tensor(R, dtype=torch.float32)
        T = torch.zeros(1, 3) if T is None else torch.as_tensor(T, dtype=torch.float32)
        n = max(R.shape[0], T.shape[0])
        self.R = R.expand(n, 3, 3).contiguous().to(device)
        self.T = T.expand(n, 3).contiguous().to(device)
        focal, pp = as2(focal_length, n), as2(principal_point, n)
        if not in_ndc:
            if image_size is None:
                raise ValueError("screen-space cameras (in_ndc=False) need image_size=(H, W)")
            hw = torch.as_tensor(image_size, dtype=torch.float32).reshape(-1, 2).expand(n, 2)
            wh = hw.flip(-1)
            scale = wh.min(dim=1, keepdim=True).values
            focal = focal * 2.0 / scale
            pp = -(pp - wh / 2.0) * 2.0 / scale
        self.focal_length = focal.contiguous().to(device)
        self.principal_point = pp.contiguous().to(device)

    def __len__(self):
        return self.R.shape[0]

    @property
    def device(self):
        return self.R.device

    def clone(self):
        return type(self)(self.focal_length.clone(), self.principal_point.clone(), self.R.clone(), self.T.clone(),
                          device=self.R.device)

    def to(self, device):
        return type(self)(self.focal_length, self.principal_point, self.R, self.T, device=device)

    def packed(self):
        """(n, 16) float32: R row-major, T, focal, principal point -- the layout bdm_rasterize_points takes."""
        return torch.cat([self.R.reshape(-1, 9), self.T, self.focal_length, self.principal_point], dim=1).contiguous()


class OrthographicCameras(PerspectiveCameras):
    """pytorch3d's OrthographicCameras (restated; unpinned: pytorch3d is absent): the same constructor, fields and packed() layout as
    PerspectiveCameras, without the division by the view depth: ndc.xy = focal * X_view.xy + principal_point.  Only the renderer
    (bdm_amd/render.py) takes one: the projection conditioning of the models is perspective."""
    orthographic = True


def look_at_view_transform(dist=1.0, elev=0.0, azim=0.0, degrees=True, device="cpu"):
    """R (n, 3, 3), T (n, 3) of cameras at distance `dist`, elevation `elev` and azimuth `azim` looking at the world origin with
    +Y up, by pytorch3d's construction (renderer/cameras.py look_at_view_transform, restated; unpinned: pytorch3d is absent):
        C = dist * (cos e sin a, sin e, cos e cos a);  z = normalize(-C), x = normalize(cross(up, z)), y = normalize(cross(z, x));
        R has x, y, z as COLUMNS (row-vector convention X_view = X_world R + T);  T = -R^T C.
    Scalars, lists or tensors, broadcast against each other.  Where the view direction is parallel to `up` (elev = +-90), x is
    replaced by normalize(cross(y, z)) as pytorch3d does."""
    dist, elev, azim = torch.broadcast_tensors(*[torch.as_tensor(v, dtype=torch.float32).reshape(-1) for v in (dist, elev, azim)])
    if degrees:
        elev, azim = elev * (math.pi / 180.0), azim * (math.pi / 180.0)
    C = torch.stack([dist * torch.cos(elev) * torch.sin(azim), dist * torch.sin(elev), dist * torch.cos(elev) * torch.cos(azim)], dim=1)
    normalize = lambda v: v / v.norm(dim=1, keepdim=True).clamp_min(1e-5)  # noqa: E731  (F.normalize's eps of pytorch3d's call)
    up = torch.tensor([[0.0, 1.0, 0.0]]).expand_as(C)
    z = normalize(-C)
    x = normalize(torch.cross(up, z, dim=1))
    y = normalize(torch.cross(z, x, dim=1))
    degenerate = torch.isclose(x, torch.zeros(()), atol=5e-3).all(dim=1, keepdim=True)
    x = torch.where(degenerate, normalize(torch.cross(y, z, dim=1)), x)
    R = torch.stack([x, y, z], dim=2)
    T = -torch.bmm(R.transpose(1, 2), C[:, :, None])[:, :, 0]
    return R.to(device), T.to(device)


def join_cameras(cameras):
    """The datasets collate to a python LIST of single cameras (dataset/shapenet_r2n2.py:601-612)."""
    if isinstance(cameras, (list, tuple)):
        return type(cameras[0])(torch.cat([c.focal_length for c in cameras]), torch.cat([c.principal_point for c in cameras]),
                                  torch.cat([c.R for c in cameras]), torch.cat([c.T for c in cameras]), device=cameras[0].device)
    return cameras


class Pointclouds:
    def __init__(self, points, features=None):
        self._points, self._features = points, features

    def points_padded(self):
        return self._points

    def features_padded(self):
        return self._features

    def points_list(self):
        return list(self._points)


class Meshes:
    """pytorch3d's Meshes, the list form only (restated; unpinned: pytorch3d is absent): verts a list of (V_i, 3) float tensors,
    faces a list of (F_i, 3) integer tensors of vertex indices within their own mesh -- what surface.reconstruct_surface returns.
    A mesh without vertices or without faces is legal.  Only what the mesh renderer (bdm_amd/render.py) reads is kept."""

    def __init__(self, verts, faces):
        if not isinstance(verts, (list, tuple)) or not isinstance(faces, (list, tuple)):
            raise ValueError("Meshes takes a list of (V, 3) vertex tensors and a list of (F, 3) face tensors")
        if len(verts) != len(faces):
            raise ValueError(f"{len(verts)} vertex tensors for {len(faces)} face tensors")
        for v, f in zip(verts, faces):
            if v.dim() != 2 or v.shape[1] != 3 or not v.is_floating_point():
                raise ValueError(f"vertices must be (V, 3) floating point, got {tuple(v.shape)} {v.dtype}")
            if f.dim() != 2 or f.shape[1] != 3 or f.is_floating_point() or f.dtype == torch.bool:
                raise ValueError(f"faces must be (F, 3) integers, got {tuple(f.shape)} {f.dtype}")
        self._verts, self._faces = list(verts), list(faces)

    def __len__(self):
        return len(self._verts)

    @property
    def device(self):
        return self._verts[0].device if self._verts else torch.device("cpu")

    def verts_list(self):
        return self._verts

    def faces_list(self):
        return self._faces

    def verts_packed(self):
        """(sum V, 3): the vertices of all meshes, mesh after mesh."""
        return torch.cat(self._verts) if self._verts else torch.zeros(0, 3)

    def faces_packed(self):
        """(sum F, 3) int64 indices into verts_packed() (pytorch3d's convention: each mesh's indices shifted by its first row)."""
        if not self._faces:
            return torch.zeros(0, 3, dtype=torch.int64)
        first = self.mesh_to_verts_packed_first_idx()
        return torch.cat([f.long() + int(o) for f, o in zip(self._faces, first)])

    def mesh_to_verts_packed_first_idx(self):
        """(len,) int64 on the host: the row of verts_packed() at which each mesh starts."""
        sizes = torch.tensor([v.shape[0] for v in self._verts], dtype=torch.int64)
        return torch.cumsum(sizes, 0) - sizes

    def mesh_to_faces_packed_first_idx(self):
        sizes = torch.tensor([f.shape[0] for f in self._faces], dtype=torch.int64)
        return torch.cumsum(sizes, 0) - sizes

    def faces_normals_packed(self, normalized=True):
        """(sum F, 3): (v1 - v0) x (v2 - v0) per face, of unit length unless normalized=False (then twice the area long)."""
        verts, faces = self.verts_packed(), self.faces_packed().to(self.device)
        tri = verts[faces]
        n = torch.linalg.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], dim=1)
        return n / n.norm(dim=1, keepdim=True).clamp_min(1e-12) if normalized else n

    def verts_normals_packed(self):
        """(sum V, 3): the area-weighted face normals summed over the faces around each vertex (index_add_; the order of the sum is
        not fixed) and normalised; a vertex no face uses gets zeros.  Torch code on the meshes' device: not a hot path."""
        verts, faces = self.verts_packed(), self.faces_packed().to(self.device)
        n = self.faces_normals_packed(normalized=False)
        acc = torch.zeros_like(verts)
        for k in range(3):
            acc.index_add_(0, faces[:, k], n)
        return acc / acc.norm(dim=1, keepdim=True).clamp_min(1e-12)


def r2n2_camera(azimuth, elevation, distance, focal=2.1875):
    """R2N2-style camera looking at the origin (dataset/utils.py:40-114 + shapenet_r2n2.py:46-53,86-93 with the
    identity normalisation mean=0, std=1): used for synthetic benchmark inputs."""
    az, el = -math.pi * azimuth / 180.0, -math.pi * elevation / 180.0
    sa, ca, se, ce = math.sin(az), math.cos(az), math.sin(el), math.cos(el)
    R_world2obj = torch.tensor([[ca * ce, sa * ce, -se], [-sa, ca, 0], [ca * se, sa * se, ce]], dtype=torch.float32)
    R_obj2cam = torch.tensor([[0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [1.0, 0.0, 0.0]])
    R_world2cam = R_obj2cam.mm(R_world2obj)
    T_world2cam = -(R_obj2cam.mm(torch.tensor([[distance, 0, 0]], dtype=torch.float32).t()))
    RT = torch.cat([torch.cat([R_world2cam, T_world2cam], dim=1), torch.tensor([[0.0, 0, 0, 1]])])
    rot = torch.tensor([[1.0, 0, 0, 0], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    RT = RT.mm(rot)
    s2p = torch.tensor([[-1.0, 0, 0, 0], [0, 1.0, 0, 0], [0, 0, -1.0, 0], [0, 0, 0, 1.0]])
    RT = torch.transpose(RT, 0, 1).mm(s2p)
    R, T = RT[:3, :3].clone(), RT[3, :3].clone()
    return PerspectiveCameras(focal_length=torch.tensor([[focal, focal]]), principal_point=torch.tensor([[0.0, 0.0]]),
                              R=R[None], T=T[None])


def pix3d_camera(rot_mat, trans_mat, pts_mean, pts_std, img_size_wh, bbox, focal_length_mm, out_size=224):
    """Camera of one Pix3D sample for the square crop around its bounding box (dataset/pix3d.py:104-159): the object is
    normalised to zero mean / unit std (m, s), so R_norm = R * s, t_norm = t + m R^T; OpenCV -> pytorch3d axes; the crop
    [cx - h, cx + h]^2 (h = half the longer bbox side) is resized to out_size, which composes an affine map with the
    intrinsics K = [[f, 0, w/2], [0, f, h/2]] where f = focal_mm * w / 32 (32 mm sensor width)."""
    import numpy as np
    R = np.asarray(rot_mat, dtype=np.float64).reshape(3, 3)
    t = np.asarray(trans_mat, dtype=np.float64).reshape(3)
    m = np.asarray(pts_mean, dtype=np.float64).reshape(3)
    R_norm, t_norm = R * float(pts_std), t + m @ R.T
    convert = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], dtype=np.float64)
    R_v1 = (R_norm @ convert).T
    w, h = img_size_wh
    x0, y0, x1, y1 = bbox
    cx, cy = (x0 + x1) / 2, (y0 + y1) / 2
    half_w = max(y1 - y0, x1 - x0) / 2
    x0, y0 = cx - half_w, cy - half_w
    f = focal_length_mm * w / 32
    s = out_size / (2 * half_w)
    fx, fy = s * f, s * f
    tx, ty = s * (w / 2) + s * (-x0), s * (h / 2) + s * (-y0)
    return PerspectiveCameras(focal_length=torch.tensor([[fx, fy]], dtype=torch.float32),
                              principal_point=torch.tensor([[tx, ty]], dtype=torch.float32),
                              R=torch.as_tensor(R_v1, dtype=torch.float32)[None], T=torch.as_tensor(t_norm, dtype=torch.float32)[None],
                              in_ndc=False, image_size=(out_size, out_size))
