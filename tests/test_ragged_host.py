"""bdm_amd/ragged.py without a GPU: the first-row arrays, the int32 rule for face indices, and the refusal of host tensors before
anything is allocated."""
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
