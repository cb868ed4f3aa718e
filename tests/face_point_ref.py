"""CPU restatement of bdm_hip.h section 17 (face-to-point distance) -- TEST INFRASTRUCTURE.

Written against the header's text, not against csrc/face_point.hip: the matrix of section 14's d over (point, face) is
mesh_metrics_ref.pair_sqdist, of which the point side (mesh_metrics_ref.distance_mesh) takes the row minima; this file takes the
column minima, the lowest point index winning ties.  `dtype=torch.float64` evaluates the same formulas in float64 on the same
(float32) inputs.

Also here: the case table the two test files share, the mutants (deliberately wrong variants of the rule) that the host test
requires the cases to tell apart from the rule, and the split form's key arithmetic in integers."""
import functools
import math

import numpy as np
import torch

import mesh_metrics_ref as M

TILE = 1024          # points per LDS tile of fp_dist_kernel (FP_TILE)
THREADS = 256        # workgroup of every kernel of the file (FP_THREADS): faces per workgroup
CUS = 256            # the chooser's constant (FP_CUS)
SPLIT_BELOW, SPLIT_TARGET = 8 * CUS, 16 * CUS   # FP_SPLIT_BELOW, FP_SPLIT_TARGET
MAX_CHUNKS = 65535
KEY_NONE = (0x7F800000 << 32) | 0xFFFFFFFF   # the preset of a key: decodes to (+inf, -1)

# mutant -> what it gets wrong
MUTANTS = {"highest_on_ties": "the highest point index wins among equal distances",
           "nonfinite_eligible": "a point with a non-finite coordinate takes part (its bad coordinates read as 0)",
           "invalid_scored": "faces with nn == 0 are scored",
           "packed_index": "the index is taken in packed instead of in-cloud numbering",
           "neighbour_cloud": "mesh m reads the cloud of mesh m + 1 (cyclically)"}
# Equivalent mutant, kept for the record: the split form's key compared as a SIGNED 64-bit integer.  The key is
# (bits of d) << 32 | index and d never has its sign bit set (header, "Sign"), so bit 63 of every key that is sent -- and of the
# preset, bits(+inf) << 32 | 0xFFFFFFFF -- is clear, and signed and unsigned order agree on all of them.  No input can tell the two
# apart; what the host test asserts instead is the premise (sign bit clear on every pair of every case), that the signed minimum
# equals the unsigned one on every case, and that the two DO differ as soon as one key has bit 63 set.
EQUIVALENT_MUTANTS = {"signed_key": "a split-form key compared as signed"}


def face_point_mesh(verts, faces, points, mutant=None, dtype=torch.float32, index_offset=0):
    """One mesh and its cloud -> sqdist (F) in `dtype`, point_idx (F) int32."""
    F, P = int(faces.shape[0]), int(points.shape[0])
    best = torch.full((F,), math.inf, dtype=dtype)
    idx = torch.full((F,), -1, dtype=torch.int64)
    if F == 0 or P == 0:
        return best, idx.to(torch.int32)
    fq = M.face_quantities(verts, faces, dtype, "invalid_not_skipped" if mutant == "invalid_scored" else None)
    x = points.to(dtype)
    if mutant == "nonfinite_eligible":
        x = torch.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0)
    d = M.pair_sqdist(fq, x)   # (P, F); +inf where the face is invalid or d is NaN
    dmin = d.min(dim=0).values
    eq = d == dmin[None]
    ar = torch.arange(P)[:, None]
    if mutant == "highest_on_ties":
        pick = torch.where(eq, ar, torch.full((), -1)).max(dim=0).values
    else:
        pick = torch.where(eq, ar, torch.full((), 1 << 40)).min(dim=0).values
    ok = dmin < math.inf
    best = torch.where(ok, dmin, best)
    idx = torch.where(ok, pick + (index_offset if mutant == "packed_index" else 0), idx)
    return best, idx.to(torch.int32)


def face_point_batch(verts_list, faces_list, clouds, mutant=None, dtype=torch.float32):
    """-> {"sqdist": (sum F) in dtype, "point_idx": (sum F) int32}, packed like the face rows"""
    B = len(verts_list)
    firsts = np.cumsum([0] + [int(c.shape[0]) for c in clouds]).tolist()
    rows = []
    for m in range(B):
        src = (m + 1) % B if mutant == "neighbour_cloud" else m
        rows.append(face_point_mesh(verts_list[m], faces_list[m], clouds[src], mutant, dtype, firsts[src]))
    return {"sqdist": torch.cat([r[0] for r in rows]), "point_idx": torch.cat([r[1] for r in rows])}


def split_by_keys(verts, faces, points, chunks, signed=False):
    """The split form of one mesh in integers: every chunk of tiles sends (bits of its minimum d) << 32 | index for the faces where it
    found a finite d; the keys are combined by the integer minimum (unsigned, or signed: the equivalent mutant) with the preset and
    decoded -> sqdist (F) float32, point_idx (F) int32."""
    F, P = int(faces.shape[0]), int(points.shape[0])
    keys = np.full(F, KEY_NONE, dtype=np.uint64)
    tiles = -(-P // TILE)
    for c in range(chunks):
        lo, hi = min(P, (c * tiles // chunks) * TILE), min(P, ((c + 1) * tiles // chunks) * TILE)
        if hi <= lo or F == 0:
            continue
        sq, idx = face_point_mesh(verts, faces, points[lo:hi])
        found = (idx >= 0).numpy()
        sent = (sq.view(torch.int32).numpy().astype(np.int64).astype(np.uint64) << np.uint64(32)) | (idx.numpy().astype(np.int64) + lo).astype(np.uint64)
        sent = np.where(found, sent, keys)
        keys = np.minimum(keys.view(np.int64), sent.view(np.int64)).view(np.uint64) if signed else np.minimum(keys, sent)
    sq = torch.from_numpy((keys >> np.uint64(32)).astype(np.uint32).view(np.float32).copy())
    return sq, torch.from_numpy((keys & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32).copy())


def variant(b, sum_f, sum_p, max_p, workgroups):
    """(form, chunks) the chooser takes, from the header's text; (0, 0) outside the limits."""
    if not (0 <= b <= 65535 and 0 <= sum_f < 2 ** 31 and 0 <= sum_p < 2 ** 31 and 0 <= max_p <= sum_p and 0 <= workgroups <= sum_f):
        return 0, 0
    tiles = -(-max_p // TILE)
    if workgroups == 0 or workgroups >= SPLIT_BELOW or tiles <= 1:
        return 1, 1
    return 2, min(-(-SPLIT_TARGET // workgroups), tiles, MAX_CHUNKS)


def workgroups_of(faces_list):
    return sum(-(-int(f.shape[0]) // THREADS) for f in faces_list)


def symmetric(verts_list, faces_list, clouds):
    """point_mesh_face_distance composed in float64 from the float32 restatements of both halves (math.fsum: exactly rounded sums)
    -> (value, the largest number of terms in one of its sums)."""
    B = len(verts_list)
    fp = [face_point_mesh(v, f, c)[0] for v, f, c in zip(verts_list, faces_list, clouds)]
    pf = [M.distance_mesh(v, f, c)[0] for v, f, c in zip(verts_list, faces_list, clouds)]
    mean = lambda t: math.fsum(t.double().tolist()) / t.numel()   # noqa: E731
    return math.fsum(mean(t) for t in pf) / B + math.fsum(mean(t) for t in fp) / B, max(max(t.numel() for t in fp + pf), B)


# ---- cases ---------------------------------------------------------------------------------------------------------------------------
GRID_F = (THREADS - 1, THREADS, THREADS + 1, 2 * THREADS + 1)
GRID_P = (1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
FAR = (100.0, -50.0, 25.0)


def tie_case():
    """mesh_metrics_ref.special_points_case's mesh against a cloud of duplicated points and of points mirrored about a face: faces 0
    and 1 lie in z = 0, so (x, y, z) and (x, y, -z) are at the same d from them; faces 2 and 3 are mirror images in z = 0, faces 4
    and 5 the same triangle; every point occurs again later in the cloud."""
    verts, faces, _ = M.special_points_case()
    half = torch.tensor([[0.25, 0.25, 0.3], [0.25, 0.25, -0.3], [-0.25, 0.5, 0.125], [-0.25, 0.5, -0.125], [5.5, 0.25, 0.0],
                         [0.3, 5.3, 0.5], [0.3, 5.3, -0.5], [-4.0, 1.0, 0.75], [-4.0, 1.0, -0.75], [9.0, 9.0, 9.0]])
    return verts, faces, torch.cat([half, half.flip(0), half[:3]])


@functools.lru_cache(maxsize=None)
def case(name):
    """-> {"verts": [..], "faces": [..], "clouds": [(P_i, 3) ..]}"""
    if name.startswith("soup_"):   # soup_f<F>_p<P>: the soups and clouds of mesh_metrics_ref
        F, P = int(name.split("_")[1][1:]), int(name.split("_")[2][1:])
        v, f = M.soup(F, 100 + F)
        return {"verts": [v], "faces": [f], "clouds": [M.cloud(P, 200 + P)]}
    if name == "ragged":   # clouds of 0, TILE + 1, 1 and 1 points; an empty mesh in the middle; one mesh far from the origin
        v0, f0 = M.icosphere(1, 0.5)
        v1, f1 = M.soup(300, 11, centre=FAR)
        v2, f2 = torch.rand(4, 3, generator=torch.Generator().manual_seed(3)), torch.zeros(0, 3, dtype=torch.int64)
        v3, f3 = M.soup(THREADS + 1, 12)
        clouds = [torch.zeros(0, 3), M.cloud(TILE + 1, 22, centre=FAR), M.cloud(1, 23), M.cloud(1, 24)]
        return {"verts": [v0, v1, v2, v3], "faces": [f0, f1, f2, f3], "clouds": clouds}
    if name == "degenerate":   # invalid faces of every kind against NaN and infinite points (mesh_metrics_ref's case, its own cloud)
        c = M.dist_case("degenerate")
        return {"verts": c["verts"], "faces": c["faces"], "clouds": [c["points"][0]]}
    if name == "ties":
        v, f, pts = tie_case()
        return {"verts": [v], "faces": [f], "clouds": [pts]}
    if name == "no_valid_face":
        c = M.dist_case("no_valid_face")
        return {"verts": c["verts"], "faces": c["faces"], "clouds": [c["points"][0]]}
    raise KeyError(name)


CASES = [f"soup_f{F}_p{P}" for F in GRID_F for P in GRID_P] + ["ragged", "degenerate", "ties", "no_valid_face"]


@functools.lru_cache(maxsize=None)
def ref(name, mutant=None):
    c = case(name)
    return face_point_batch(c["verts"], c["faces"], c["clouds"], mutant)


def chunk_counts(name):
    """The chunk counts the split form is run at: 2, and as many as the largest cloud has tiles (at least 1)."""
    tiles = max(-(-int(c.shape[0]) // TILE) for c in case(name)["clouds"])
    return sorted({2, max(tiles, 1)})


bits, same = M.bits, M.same
