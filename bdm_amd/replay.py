"""One recorded-and-replayed step for the reverse loops (model._denoise_loop_tape, pvd.Model._gen_samples_tape).

A loop keeps its state and its denoiser input in static buffers g["x"], g["t"]; per timestep it fills g["t"], calls
run_step() for eps and does its own scheduler arithmetic eagerly (one launch: its scalars and its noise draw change per
step).  run_step runs the first step on those buffers eagerly, so that every lazy cache (weight packs, workspaces, kernel
attributes) exists; RECORDS the second one while it runs (tape.py) and REPLAYS the flat list of C-ABI calls for every
later step -- of this call, of later segments, of later trajectories: ~11 us of host time per launch instead of 15-20,
and recorded inside a private memory pool the replay costs the GPU what the eager step costs.  A recording the recorder
could not finish parks the loop on the eager path for good and leaves the reason in g["off"].

A recording holds addresses and kernel routes, so it lives exactly as long as its key: step_key() has every ingredient a
stale replay was once traced to, and step_record() drops the record when the key moves.
"""
import torch

from . import _lib as L
from . import ops, profiling, tape


def weights_signature(module):
    """Changes whenever a parameter is rewritten or replaced: a recorded step (graph or tape) holds the addresses of the
    weight packs derived from them, so it must not outlive the weights it was recorded with."""
    return hash(tuple((p.data_ptr(), p._version) for p in module.parameters()))


def step_key(module, shape, device, *extra, stream=True):
    """What a recorded step of `module` on buffers of `shape` is keyed by: the weights, the kernel routes
    (ops.saturation_epoch) and the stream it was recorded on (stream=False: a hipGraph replays on any stream), then `extra`."""
    return (tuple(shape), str(device), L.stream() if stream else None, weights_signature(module), ops.saturation_epoch()) + extra


def wanted(mode, n_points, max_points):
    """BDM_TAPE: "1" always, "auto" up to max_points (= B * N), anything else never."""
    return mode == "1" or (mode == "auto" and n_points <= max_points)


def step_record(owner, key, like, valid=None, **hold):
    """owner._tape_cache if it was made for `key` (and `valid(record)` holds), else a fresh one in its place: static buffers
    x (like `like`, contiguous) and t (int64 per batch entry), no tape yet; `hold` keeps objects alive whose id() is in the key."""
    g = getattr(owner, "_tape_cache", None)
    if g is None or g["key"] != key or (valid is not None and not valid(g)):
        g = dict(hold, key=key, tape=None, warm=False, off=None, eps=None, steps=-1,
                 x=torch.empty_like(like, memory_format=torch.contiguous_format),
                 t=torch.zeros(like.shape[0], dtype=torch.int64, device=like.device))
        owner._tape_cache = g
    return g


def run_step(g, denoise, probe=0, record=tape.record):
    """eps of one step on g's static buffers.  probe = k (bench.py's eager_probe_every): once a tape exists every k-th step
    runs eagerly through the kernel-class profiler, each profiled launch standing for k.  `record` is replaceable so that
    the sequence can be driven without a device."""
    g["steps"] = i = g["steps"] + 1  # counted across calls: the samplers run the loops in segments
    if g["tape"] is not None and probe and i % probe == probe - 1:
        profiling.PROBE_WEIGHT[0] = probe
        try:
            return denoise()
        finally:
            profiling.PROBE_WEIGHT[0] = 1
    if g["tape"] is not None:
        g["tape"].replay()
        return g["eps"]
    if g["warm"] and g["off"] is None:
        with ops.static_step(), record() as tp:
            eps = denoise()
        if tp.broken:
            g["off"] = tp.broken  # stay eager (on the static buffers) and say why
        else:
            g["tape"], g["eps"] = tp, eps
        return eps
    eps = denoise()
    g["warm"] = True
    return eps
