"""What the flow head of the deform network costs on an MI355X on its two paths: path="torch" (PyTorch ops, `PointLinear`
branches: the default) against path="fused" (csrc/flow_head.hip).

    python tools/flow_head_bench.py --out profiles/flow_head_bench.json
        one process.  (a) The head alone, for each of the seven flow models: N = 100 k points, W = 128, forward + backward of
        sum(means3D . probe) with gradients for hidden, pts and every parameter (nothing reads `flow`, as in the training loop).
        (b) The 4-D network step of tools/deform_step_profile.py (decoder-free tri-plane sampler, n_frames = 50,
        composition_rank = 10, 100 k points) with flow_model = "se3" and the head on either path.  In each comparison both sides
        are warmed up, then five alternations torch / fused, every window timed with device events over at least --min-window
        seconds; then a few iterations of either side under torch.profiler for the launches per iteration, and the library's
        own count (sr_profile_collect).  Writes the JSON and prints it.  The "torch" side is the baseline; the exit status is 0
        whichever side is faster (the fused path is opt-in).

Needs a HIP device; there is no CPU fallback."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tools import benchkit  # noqa: E402


def head_steps(dev, model, n, width, n_basis, seed=5):
    from splatfields_amd.deform_field import FlowHead
    torch.manual_seed(seed)
    heads = {}
    for path in ("torch", "fused"):
        head = FlowHead(W=width, flow_model=model, num_basis=n_basis, n_frames=50, path=path)
        if heads:
            head.load_state_dict(heads["torch"].state_dict())
        else:
            with torch.no_grad():                       # branch_coeff starts at zero: give every branch a value
                for name, p in head.named_parameters():
                    if name.startswith("branch_") or name.startswith("gaussian_warp"):
                        p.normal_(0.0, 0.5 if name.endswith("bias") else 1.0 / width ** 0.5)
        heads[path] = head.to(dev)
    hidden = torch.randn(n, width, device=dev).requires_grad_(True)
    pts = (torch.rand(n, 3, device=dev) * 2 - 1).requires_grad_(True)
    probe = torch.randn(n, 3, device=dev)
    time_step, frame_id = torch.tensor(0.37, device=dev), torch.tensor(18, device=dev)

    def step(path):
        head = heads[path]
        params = list(head.parameters())

        def fn():
            for p in params:
                p.grad = None
            hidden.grad, pts.grad = None, None
            _, means = head(hidden, pts, time_step=time_step, frame_id=frame_id)
            (means * probe).sum().backward()
        return fn

    return {"torch": step("torch"), "fused": step("fused")}


def network_steps(dev, n, seed=0):
    from splatfields_amd.deform_field import SplatFields
    xyz = (torch.rand(n, 3, device=dev) * 2 - 1).requires_grad_(True)
    t_emb = torch.full((n, 1), 0.37, device=dev)
    nets = {}
    for path in ("torch", "fused"):
        torch.manual_seed(seed)
        nets[path] = SplatFields(n_frames=50, composition_rank=10, encoder=None, flow_model="se3", flow_head=path).to(dev)
    nets["fused"].load_state_dict(nets["torch"].state_dict())

    def step(path):
        net = nets[path]
        params = list(net.parameters())

        def fn():
            for p in params:
                p.grad = None
            xyz.grad = None
            out = net(xyz, t_emb)
            sum((v * v).mean() for k, v in out.items() if torch.is_tensor(v) and k != "flow").backward()
        return fn

    return {"torch": step("torch"), "fused": step("fused")}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--out", default=None)
    p.add_argument("--points", type=int, default=100_000)
    p.add_argument("--width", type=int, default=128)
    p.add_argument("--basis", type=int, default=4)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--min-window", type=float, default=0.3, help="seconds per timed window")
    p.add_argument("--profiled-iterations", type=int, default=3)
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("flow_head_bench needs a HIP device: there is no CPU fallback")
    dev = torch.device("cuda:0")
    from splatfields_amd.build import source_hash
    from splatfields_amd.deform_field import FLOW_MODELS
    from splatfields_amd.flow_head import FLOW_HEAD_LAUNCHES
    doc = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "_source_hash": source_hash(),
           "workload": f"head alone: {a.points} points, W = {a.width}, K = {a.basis}, forward + backward of sum(means3D . probe), gradients for "
                       "hidden, pts and every parameter; network step: tools/deform_step_profile.py's network with flow_model = 'se3'",
           "protocol": f"one process; per comparison both sides warmed up ({a.warmup} iterations), then {a.repeats} alternations torch / fused, windows "
                       f">= {a.min_window} s between device events; launches from torch.profiler ({a.profiled_iterations} iterations per side) and from "
                       "sr_profile_collect (one iteration); 'torch' is the default path and the baseline",
           "flow_head_launches": list(FLOW_HEAD_LAUNCHES), "head": {}}
    for model in FLOW_MODELS:
        doc["head"][model] = benchkit.compare(head_steps(dev, model, a.points, a.width, a.basis), a)
    doc["network_step_se3"] = benchkit.compare(network_steps(dev, a.points), a)
    benchkit.write_doc(doc, a.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
