"""tools/gen_golden_simple.py -- goldens of the reference's simple point denoiser and PVCNN++ (build container only).

Imports the reference's own Python read-only through oracle.gen_golden._install_reference (the PVCNN plugin replaced by the
CPU restatement of its ops) and builds SimplePointModel and PVCNN2PlusPlus directly (point_cloud_model.py imports diffusers).
Weights are procedural (fill_module_, seeded), after which the PositionalEncoding buffer is set back to its constructed value
2 ** linspace(1, 9, 10), so that the sin / cos arguments reach |512 x| as in a trained checkpoint.  No output-head rescale
(head scale 1).  Each file holds the seeds, shapes, t, state-dict keys and the reference's outputs only.

    python tools/gen_golden_simple.py      # from the repo root
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.gen_golden import OUT, _install_reference, point_cloud_inputs  # noqa: E402

S, E, B = 387, 64, 2
CASES = [("simple", 1024, 21, 31, [17, 905]), ("simple", 1100, 22, 32, [500, 3]),
         ("pvcnnpp", 1024, 23, 33, [250, 999]), ("pvcnnpp", 1100, 24, 34, [640, 41])]


def build(kind, weight_seed):
    from bdm_amd.utils.procedural import fill_module_
    from model.simple.simple_model import SimplePointModel
    from model.pvcnn.pvcnn_plus_plus import PVCNN2PlusPlus
    if kind == "simple":
        net = SimplePointModel(embed_dim=E, num_classes=3, extra_feature_channels=S)
        pe = [net.positional_encoding]
    else:
        net = PVCNN2PlusPlus(embed_dim=E, num_classes=3, extra_feature_channels=S)
        pe = [net.simple_point_model.positional_encoding]
    net = fill_module_(net.eval(), seed=weight_seed)
    for m in pe:
        m.freq_bands.copy_(2 ** torch.linspace(1, 9, 10))
    return net


def main():
    _install_reference()
    torch.set_grad_enabled(False)
    torch.set_num_threads(1)
    for kind, N, wseed, iseed, ts in CASES:
        net = build(kind, wseed)
        x = point_cloud_inputs(B, 3 + S, N, seed=iseed)
        t = torch.tensor(ts)
        y = net(x, t)
        sd = net.state_dict()
        path = os.path.join(OUT, f"{kind}_full_n{N}.npz")
        np.savez_compressed(path, B=B, S=S, N=N, weight_seed=wseed, input_seed=iseed, t=t.numpy(), out=y.numpy(),
                            keys=np.array(list(sd.keys())), shapes=np.array([str(tuple(v.shape)) for v in sd.values()]))
        print(f"{path}: out {tuple(y.shape)} |out| {float(y.norm()):.4f}, {len(sd)} keys")


if __name__ == "__main__":
    main()
