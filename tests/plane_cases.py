"""What the GPU tests of the plane generator and of its attention layer share: the committed fixtures
(tests/golden/plane_decoder_*.npz), the small configuration they were recorded with, and one forward + backward of a module."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SMALL = dict(in_channels=8, out_channels=16, up_block_types=("TimeUpDecoderBlock2D",) * 4, block_out_channels=(16,) * 4, norm_num_groups=4,
             layers_per_block=1)


def load(name):
    z = np.load(os.path.join(GOLDEN, f"plane_decoder_{name}.npz"))
    return {k: torch.as_tensor(z[k].astype(np.float32) if z[k].dtype == np.float16 else z[k]) for k in z.files}


def params_of(z):
    return {k[len("param/"):]: v for k, v in z.items() if k.startswith("param/")}


def run_module(net, noise, probe, frame_id=None):
    net.zero_grad()
    out = net(noise, frame_id=frame_id)
    (out * probe).sum().backward()
    return out.detach(), {n: p.grad.detach().clone() for n, p in net.named_parameters() if p.grad is not None}
