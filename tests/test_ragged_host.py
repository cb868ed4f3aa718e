"""bdm_amd/ragged.py without a GPU: the first-row arrays, the int32 rule for face indices, and the refusal of host tensors before
anything is allocated; and the sizes of the mesh workspaces that csrc/ragged.h's carver lays out, asked of the library (DESIGN.md
section 17.1)."""
import pytest
import torch

from bdm_amd import ragged
from bdm_amd._lib import BdmHipError


def test_first_is_the_host_int64_array_of_first_rows():
    for counts, want in (([], [0]), ([0, 3, 0, 2], [0, 0, 3, 3, 5])):
        got = ragged.first(counts)
        assert got.dtype == torch.int64 and got.device.type == "cpu" and got.tolist() == want
    assert ragged.first(n for n in (2, 1)).tolist() == [0, 2, 3]   # any iterable of counts


def test_int64_indices_outside_int32_become_minus_one():
    values = [-1, 0, 2 ** 31 - 1, 2 ** 31, 2 ** 32, 2 ** 32 + 1]
    got = ragged.faces_as_int32(torch.tensor(values, dtype=torch.int64).reshape(2, 3))
    assert got.dtype == torch.int32 and got.shape == (2, 3)
    assert got.reshape(-1).tolist() == [-1, 0, 2 ** 31 - 1, -1, -1, -1]   # the value where representable and non-negative, else -1


def test_int32_indices_pass_unchanged():
    f = torch.tensor([[0, 1, 2], [-1, 5, 2 ** 31 - 1]], dtype=torch.int32)
    got = ragged.faces_as_int32(f)
    assert got.dtype == torch.int32 and torch.equal(got, f)


def test_packers_refuse_host_tensors_before_allocating(monkeypatch):
    def allocated(*args, **kwargs):
        raise AssertionError("allocated before the host tensors were refused")
    for name in ("cat", "zeros", "empty", "tensor"):
        monkeypatch.setattr(torch, name, allocated)
    verts, faces = [torch.ones(4, 3)], [torch.ones(2, 3, dtype=torch.int64)]
    with pytest.raises(BdmHipError, match="CPU tensor"):
        ragged.pack_meshes(verts, faces)
    with pytest.raises(BdmHipError, match="CPU tensor"):
        ragged.pack_rows(verts, 3, "cuda")
    with pytest.raises(BdmHipError, match="CPU tensor"):
        ragged.pack_rows([verts[0][:0]], 3, "cuda")   # an empty side is no excuse


# (b, sum V, sum F): zero sums, b of 1, 33 and 65535, sums either side of multiples of 1024 (the scan's partial sums), the largest
# accepted sums, and from (-1, 10, 10) on sizes that an operator refuses
WORKSPACE_ROWS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 0, 1), (1, 3, 1), (1, 1022, 340), (1, 1023, 341), (1, 1024, 342), (1, 1025, 2047), (1, 2047, 2048),
                  (1, 2048, 2049), (33, 0, 0), (33, 4914, 6576), (33, 262210, 87400), (65535, 0, 0), (65535, 65535, 65535), (65535, 1048575, 2097151),
                  (65535, 1048576, 2097152), (1, 2 ** 31 - 2, 0), (1, 0, 357913941), (3, 1789569705, 357913941), (3, 1789569706, 357913941),
                  (-1, 10, 10), (65536, 10, 10), (1, -1, 1), (1, 1, -1), (1, 2 ** 31 - 1, 0), (1, 2 ** 31, 1), (1, 10, 357913942)]
# The values the library returned before the workspaces were laid out by ragged.h's carver (commit 2a90d23 built and asked): the
# layouts are part of no interface, but a layout that moved would show here first.  components and taubin take (b, sum V) only.
WORKSPACE_BYTES = {
    "adjacency": [64, 80, 80, 112, 112, 16400, 16432, 16480, 57408, 65584, 65648, 592, 197728, 4196880, 1048624, 3145968, 59772912, 59772976,
                  17188257824, 8589934672, 22913482832, 22913482832, 0, 0, 0, 0, 0, 0, 0],
    "components": [48, 64, 96, 64, 96, 12336, 12336, 12352, 12384, 24624, 24640, 576, 59568, 3148128, 1048608, 1835264, 13635584, 13635616,
                   25778192416, 64, 21481827072, 21481827072, 0, 0, 0, 96, 0, 0, 192],
    "taubin": [16, 32, 64, 32, 128, 32736, 32768, 32800, 32832, 65536, 65568, 544, 157792, 8391264, 1048576, 3145696, 34602976, 34603008,
               68719476704, 32, 57266230624, 57266230656, 0, 0, 0, 64, 0, 0, 352],
    "fill": [128, 176, 176, 384, 384, 77696, 77904, 78160, 426048, 434336, 434576, 1456, 1382320, 19929744, 2621536, 16515760, 438853552,
             438853728, 17188257920, 73018638432, 87337992352, 0, 0, 0, 0, 0, 0, 0, 0],
}


@pytest.mark.parametrize("name", list(WORKSPACE_BYTES))
def test_mesh_workspace_sizes_are_what_they_were(name):
    from bdm_amd import _lib as L
    fn = getattr(L.lib(), f"bdm_mesh_{name}_workspace_bytes")
    nargs = 3 if name in ("adjacency", "fill") else 2
    assert [fn(*row[:nargs]) for row in WORKSPACE_ROWS] == WORKSPACE_BYTES[name]


# (b, sum V, sum F, h, w) for the mesh rasteriser, whose workspace is keys (8 b h w bytes, padded to 16), records (16 sum V), offsets:
# b of 0, 1 and 33, an odd pixel count (the padding), sums either side of multiples of 4, 224 x 224 and 1 x 1, the largest accepted
# sizes, and from (-1, 10, 10, 16, 16) on the sizes that the operator refuses
RENDER_WORKSPACE_ROWS = [(0, 0, 0, 1, 1), (0, 7, 9, 224, 224), (1, 0, 0, 1, 1), (1, 3, 1, 1, 1), (1, 3, 5, 224, 224), (1, 4, 3, 224, 224), (1, 5, 4, 3, 3),
                         (1, 1023, 2047, 5, 7), (33, 0, 0, 1, 1), (33, 4911, 6575, 1, 1), (33, 4912, 6576, 3, 5), (33, 4913, 6577, 224, 224),
                         (16, 100000, 200000, 224, 224), (1, 2 ** 31 - 1, 2 ** 31 - 1, 4096, 4096), (127, 3, 1, 4096, 4096),
                         (-1, 10, 10, 16, 16), (1, 2 ** 31, 10, 16, 16), (1, 10, 2 ** 31, 16, 16), (1, -1, 10, 16, 16), (1, 10, -1, 16, 16),
                         (1, 10, 10, 4097, 16), (1, 10, 10, 16, 4097), (1, 10, 10, 0, 16), (1, 10, 10, 16, 0), (128, 10, 10, 4096, 4096)]
# The values the library returned before mesh_render.hip laid its workspace out with the carver (commit dfe440f built and asked).
RENDER_WORKSPACE_BYTES = [16, 128, 48, 96, 401488, 401504, 192, 16688, 816, 79392, 83104, 13325616, 8022800, 34493956112, 17045653552,
                          0, 0, 0, 0, 0, 0, 0, 0, 0, 0]


def test_render_workspace_sizes_are_what_they_were():
    from bdm_amd import _lib as L
    fn = L.lib().bdm_render_meshes_workspace_bytes
    assert [fn(*row) for row in RENDER_WORKSPACE_ROWS] == RENDER_WORKSPACE_BYTES
