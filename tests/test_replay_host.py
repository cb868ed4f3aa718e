"""bdm_amd/replay.py without a device: the order of the replayed-step sequence (first step eager, second recorded, later ones
replayed, every k-th probed eagerly), a broken recording, the probe weight's restore, the cache record's identity and what its key
is sensitive to.  The recorder is a fake (`record=`); `denoise` logs where it ran."""
import contextlib

import pytest
import torch

from bdm_amd import _lib as L
from bdm_amd import ops, profiling, replay


class _FakeTape:
    def __init__(self, broken=None):
        self.broken, self.replays = broken, 0

    def replay(self):
        self.replays += 1


def _recorder(broken=None):
    made = []

    @contextlib.contextmanager
    def record():
        made.append(_FakeTape(broken))
        yield made[-1]
    return record, made


def _record():
    return dict(key=None, tape=None, warm=False, off=None, eps=None, steps=-1)


def _denoise(log):
    def denoise():
        log.append((ops._static_epoch != 0, profiling.PROBE_WEIGHT[0]))
        return object()
    return denoise


def test_order_eager_record_replay_probe():
    g, log = _record(), []
    record, made = _recorder()
    out = [replay.run_step(g, _denoise(log), probe=3, record=record) for _ in range(9)]
    # steps 0 (eager), 1 (recorded inside static_step), 2, 5, 8 (probes, weight 3) ran denoise; 3, 4, 6, 7 replayed
    assert log == [(False, 1), (True, 1), (False, 3), (False, 3), (False, 3)]
    assert g["steps"] == 8 and g["warm"] and g["off"] is None
    assert len(made) == 1 and g["tape"] is made[0] and made[0].replays == 4
    assert g["eps"] is out[1]
    assert all(out[i] is g["eps"] for i in (3, 4, 6, 7))
    assert len({id(out[i]) for i in (0, 1, 2, 5, 8)}) == 5
    assert ops._static_epoch == 0 and profiling.PROBE_WEIGHT[0] == 1


def test_without_probe_every_later_step_replays():
    g, log = _record(), []
    record, made = _recorder()
    for _ in range(6):
        replay.run_step(g, _denoise(log), record=record)
    assert log == [(False, 1), (True, 1)] and made[0].replays == 4 and g["steps"] == 5


def test_broken_recording_parks_the_loop_on_the_eager_path():
    g, log = _record(), []
    record, made = _recorder(broken="aten::item: host <-> device traffic inside the step")
    out = [replay.run_step(g, _denoise(log), probe=2, record=record) for _ in range(6)]
    assert g["off"] == "aten::item: host <-> device traffic inside the step" and g["tape"] is None and g["eps"] is None
    assert len(made) == 1 and made[0].replays == 0  # no second recording, nothing replayed
    assert log == [(False, 1), (True, 1)] + [(False, 1)] * 4  # later steps: eager, outside static_step, never a probe
    assert len({id(o) for o in out}) == 6 and g["steps"] == 5


def test_probe_weight_restored_when_the_probed_step_raises():
    g, log = _record(), []
    record, _ = _recorder()
    for _ in range(2):
        replay.run_step(g, _denoise(log), probe=3, record=record)

    def failing():
        assert profiling.PROBE_WEIGHT[0] == 3
        raise RuntimeError("kernel failed")
    with pytest.raises(RuntimeError, match="kernel failed"):
        replay.run_step(g, failing, probe=3, record=record)
    assert profiling.PROBE_WEIGHT[0] == 1 and g["steps"] == 2


def test_step_record_identity():
    class Owner:
        pass
    owner, like = Owner(), torch.zeros(2, 5, 3).transpose(1, 2)
    assert not like.is_contiguous()
    g = replay.step_record(owner, ("a", 1), like, feat="f")
    assert owner._tape_cache is g and type(g) is dict
    assert set(g) == {"key", "tape", "warm", "off", "eps", "x", "t", "steps", "feat"}
    assert (g["key"], g["tape"], g["warm"], g["off"], g["eps"], g["steps"], g["feat"]) == (("a", 1), None, False, None, None, -1, "f")
    assert g["x"].shape == like.shape and g["x"].dtype == like.dtype and g["x"].is_contiguous()
    assert g["t"].dtype == torch.int64 and g["t"].tolist() == [0, 0]
    g["steps"] = 7
    assert replay.step_record(owner, ("a", 1), like, feat="f") is g and g["steps"] == 7
    assert replay.step_record(owner, ("a", 1), like, valid=lambda r: r["feat"] == "f", feat="f") is g
    other = replay.step_record(owner, ("a", 1), like, valid=lambda r: r["feat"] == "h", feat="h")  # same key, not valid
    assert other is not g and owner._tape_cache is other and other["feat"] == "h"
    fresh = replay.step_record(owner, ("a", 2), like)
    assert fresh is not other and owner._tape_cache is fresh and fresh["steps"] == -1 and fresh["tape"] is None
    assert fresh["x"].data_ptr() != g["x"].data_ptr() and "feat" not in fresh
    owner._tape_cache = None  # how tests and tools reset it
    assert replay.step_record(owner, ("a", 2), like) is not fresh


def test_wanted():
    assert replay.wanted("1", 1 << 30, 1 << 20)
    assert replay.wanted("auto", 1 << 20, 1 << 20) and not replay.wanted("auto", (1 << 20) + 1, 1 << 20)
    assert not replay.wanted("0", 1, 1 << 20)


def test_key_sensitivity(monkeypatch):
    net = torch.nn.Sequential(torch.nn.Linear(4, 4), torch.nn.Linear(4, 2))
    sig = replay.weights_signature(net)
    assert replay.weights_signature(net) == sig
    with torch.no_grad():
        net[0].weight.mul_(1.25)  # rewritten in place: same address, new version
    sig2 = replay.weights_signature(net)
    assert sig2 != sig
    net[1].bias = torch.nn.Parameter(torch.zeros(2))  # replaced
    assert replay.weights_signature(net) != sig2

    if not torch.cuda.is_available():
        monkeypatch.setattr(L, "stream", lambda: 0)
    cam = object()
    key = replay.step_key(net, torch.Size([2, 8, 3]), torch.device("cpu"), id(cam))
    assert key == replay.step_key(net, (2, 8, 3), torch.device("cpu"), id(cam))
    assert key[0] == (2, 8, 3) and key[-1] == id(cam) and replay.weights_signature(net) in key and ops.saturation_epoch() in key
    assert key != replay.step_key(net, (2, 8, 3), torch.device("cpu"), id(object()))
    assert key != replay.step_key(net, (2, 9, 3), torch.device("cpu"), id(cam))
    monkeypatch.setattr(ops, "_sat_epoch", ops._sat_epoch + 1)  # poll_h2_saturation re-routed a layer
    assert key != replay.step_key(net, (2, 8, 3), torch.device("cpu"), id(cam))
    assert replay.step_key(net, (2, 8, 3), torch.device("cpu")) != replay.step_key(net, (2, 8, 3), torch.device("cpu"), stream=False)
    if torch.cuda.is_available():
        dev = torch.device("cuda")
        here = replay.step_key(net, (2, 8, 3), dev)
        with torch.cuda.stream(torch.cuda.Stream()):
            there, there_graph = replay.step_key(net, (2, 8, 3), dev), replay.step_key(net, (2, 8, 3), dev, stream=False)
        assert here != there and L.stream() in here                       # a tape belongs to the stream it was recorded on
        assert there_graph == replay.step_key(net, (2, 8, 3), dev, stream=False)  # a graph's key has no stream
