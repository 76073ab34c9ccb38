"""Records what the reference's `FlowHead` (utils/time_utils.py:194-304) computes for each of its seven flow models:

  flow_head_keys.json    {model: [state-dict keys]}
  flow_head_cases.npz    per model m and precision p in (f32, f64):  m/param/<key> (float32: the master values of both precisions),
                         m/hidden, m/pts, m/probe_flow, m/probe_means, m/frame_id, m/time_step, and
                         m/p/flow, m/p/means3D, m/p/grad/hidden, m/p/grad/pts, m/p/grad/<key>  of  sum(probe . output)

Run where the reference checkout exists:  python tests/golden/make_flow_head_golden.py /path/to/reference
The float64 evaluation runs under torch.set_default_dtype(torch.float64): the reference builds its identity matrices and
bottom rows with the default dtype.  The branch weights and `branch_coeff` are randomised (the reference's zero initialisation
of `branch_coeff` would pin nothing); every master value is rounded to float32 first, so both precisions see the same numbers."""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = ("offset", "se3", "se3Affine", "se3Scaled", "affine", "dct", "dct_siren")
N, W, K, N_FRAMES, FRAME_ID, TIME_STEP = 97, 32, 4, 6, 3, 0.625


def import_time_utils(ref):
    """utils/time_utils.py with scene.tripFields masked out: the flow head does not use it, and its own imports do not exist here"""
    sys.path.insert(0, ref)
    scene_pkg = types.ModuleType("scene")
    scene_pkg.__path__ = []
    masked = types.ModuleType("scene.tripFields")
    for name in ["TriPlaneEncoder", "VarTriPlaneEncoder", "HexPlaneEncoder", "VarHexPlaneEncoder", "GridEncoder", "VarGridEncoder",
                 "LaplaceDensity", "BellDensity"]:
        setattr(masked, name, object)
    saved = {k: sys.modules.get(k) for k in ("scene", "scene.tripFields")}
    sys.modules["scene"], sys.modules["scene.tripFields"] = scene_pkg, masked
    try:
        from utils import time_utils
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return time_utils


def evaluate(FlowHead, model, state, inputs, dtype):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        head = FlowHead(W=W, flow_model=model, num_basis=K, n_frames=N_FRAMES)
        head.load_state_dict({k: v.to(dtype) for k, v in state.items()}, strict=True)
        hidden = inputs["hidden"].to(dtype).requires_grad_()
        pts = inputs["pts"].to(dtype).requires_grad_()
        flow, means = head(hidden, pts, time_step=torch.tensor(TIME_STEP, dtype=dtype), frame_id=torch.tensor(FRAME_ID))
        ((flow * inputs["probe_flow"].to(dtype)).sum() + (means * inputs["probe_means"].to(dtype)).sum()).backward()
        out = {"flow": flow.detach(), "means3D": means.detach(), "grad/hidden": hidden.grad, "grad/pts": pts.grad}
        for k, p in head.named_parameters():
            out["grad/" + k] = p.grad if p.grad is not None else torch.zeros_like(p)
        return {k: v.numpy() for k, v in out.items()}
    finally:
        torch.set_default_dtype(prev)


def main(ref):
    FlowHead = import_time_utils(ref).FlowHead
    keys, data = {}, {}
    for idx, model in enumerate(MODELS):
        torch.manual_seed(700 + idx)
        head = FlowHead(W=W, flow_model=model, num_basis=K, n_frames=N_FRAMES)
        with torch.no_grad():
            for k, p in head.named_parameters():
                if k.startswith("branch_") or k.startswith("gaussian_warp"):
                    p.copy_(torch.randn(p.shape) * (0.5 if k.endswith("bias") else 1.0 / W ** 0.5))
        state = {k: v.detach().clone().float().double() for k, v in head.state_dict().items()}
        keys[model] = list(state)
        flow_shape = (N, 4, 4) if model == "se3" else (N, 3)
        inputs = {"hidden": torch.randn(N, W), "pts": torch.rand(N, 3) * 2 - 1, "probe_flow": torch.randn(flow_shape),
                  "probe_means": torch.randn(N, 3)}
        inputs = {k: v.float().double() for k, v in inputs.items()}
        for k, v in state.items():
            data[f"{model}/param/{k}"] = v.numpy().astype(np.float32)
        for k, v in inputs.items():
            data[f"{model}/{k}"] = v.numpy().astype(np.float32)
        data[f"{model}/frame_id"], data[f"{model}/time_step"] = np.array(FRAME_ID), np.array(TIME_STEP)
        for tag, dtype in (("f32", torch.float32), ("f64", torch.float64)):
            for k, v in evaluate(FlowHead, model, state, inputs, dtype).items():
                data[f"{model}/{tag}/{k}"] = v
    with open(os.path.join(HERE, "flow_head_keys.json"), "w") as f:
        json.dump(keys, f, indent=1)
        f.write("\n")
    np.savez_compressed(os.path.join(HERE, "flow_head_cases.npz"), **data)
    print("wrote", len(data), "arrays for", len(keys), "models")


if __name__ == "__main__":
    main(sys.argv[1])
