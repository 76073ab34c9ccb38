"""Writes tests/golden/moran_cases.npz: the reference's own Moran's I regulariser (extract_geo.py `query_nn`,
`morans_measure`, `morans_loss`, summed as train.py:203-215 does) on small inputs, evaluated in float64 AND in float32.  Run
on a CPU where a reference checkout exists:

    python tests/golden/make_moran_golden.py /path/to/reference

`pytorch3d.ops.knn.knn_points`, which `query_nn` imports, does not exist here: a stand-in module supplies the exact k-NN of
the float64 points through scipy.spatial.cKDTree, ordered by (distance, index).  The other imports of extract_geo.py (the
training stack) are empty stand-ins; only the three functions run.  Numeric arrays only travel.  Per case `<name>`:
    <name>/points [N,3], /feature_<t> [N,F_t]        float32 inputs;   /k, /eps;   /nn_ix [N,K] int32
    <name>/f64/{weights [N,K,K], terms [T], means [T], total, d_feature_<t>, d_points}   and the same under /f32
and `free_pair`: /weight [B,n,n], /feature [B,n,F] that did not come from query_nn, /f64|f32/{loss, measure, d_weight,
d_feature} with d_* the gradients of `morans_loss`.  The float32 evaluation is the reference's own rounding error: the
tolerance of the HIP kernels is derived from its distance to the float64 one (tests/test_gpu_moran.py).

Every case is checked here: the K-th and (K+1)-th squared neighbour distances of every point differ by more than 1e-4
relative (the neighbour SETS are unambiguous in float32), and every mean meant to be interior lies in [0.05, 0.95]."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from moran_reference import REFERENCE_WIDTHS, ambiguous_share, cloud, exact_knn, smooth_features  # noqa: E402  (inputs and the k-NN only)


def import_reference(ref_dir):
    def knn_points(p1, p2, K, return_sorted=True):
        assert p1.shape[0] == 1 and p1.data_ptr() == p2.data_ptr() or torch.equal(p1, p2)
        idx, d2 = exact_knn(p1[0], K)
        return d2[:, :K].to(p1.dtype)[None], idx[None], None

    stand_ins = {"pytorch3d": {}, "pytorch3d.ops": {}, "pytorch3d.ops.knn": {"knn_points": knn_points},
                 "scene": {"Scene": object, "SplatFieldsModel": object},
                 "arguments": dict.fromkeys(["ModelParams", "PipelineParams", "get_combined_args", "ModelHiddenParams", "OptimizationParams"], object),
                 "gaussian_renderer": {"GaussianModel": object}, "plyfile": {"PlyData": object, "PlyElement": object},
                 "utils": {}, "utils.sh_utils": dict.fromkeys(["SH2RGB", "RGB2SH", "eval_sh"], object),
                 "utils.general_utils": dict.fromkeys(["strip_symmetric", "build_scaling_rotation"], object)}
    for name, attrs in stand_ins.items():
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m
    sys.path.insert(0, ref_dir)
    import extract_geo
    return extract_geo


def reference_eval(ref, points, features, k, eps, dtype):
    pts = points.to(dtype).clone().requires_grad_(True)
    feats = [f.to(dtype).clone().requires_grad_(True) for f in features]
    weights, nn_ix = ref.query_nn(pts, n_neighbors=k, eps=eps)
    terms = [ref.morans_loss(weights, f[nn_ix]) for f in feats]                  # train.py:204-210
    means = [ref.morans_measure(weights, f[nn_ix]) for f in feats]
    total = sum(terms)
    total.backward()
    out = {"weights": weights, "terms": torch.stack(terms), "means": torch.stack(means), "total": total,
           "d_points": pts.grad if pts.grad is not None else torch.zeros_like(pts)}
    for t, f in enumerate(feats):
        out[f"d_feature_{t}"] = f.grad if f.grad is not None else torch.zeros_like(f)
    return {key: v.detach().numpy().copy() for key, v in out.items()}, nn_ix


def with_duplicates(points, pairs, seed):
    gen = torch.Generator().manual_seed(seed)
    perm = torch.randperm(points.shape[0], generator=gen)
    points = points.clone()
    points[perm[:pairs]] = points[perm[pairs:2 * pairs]]
    return points


def cases():
    """name -> (points, features, k, eps, kind).  kind "interior": every mean must lie in [0.05, 0.95]; "negative": every mean
    must lie below -0.01 (the noise's seed was chosen for that: the mean of pure noise is near 0 with either sign); the
    duplicates' seed is the first that leaves no point with one twin inside and the other outside its neighbourhood."""
    rand = lambda seed, *s: torch.rand(*s, generator=torch.Generator().manual_seed(seed))
    out = {}
    p = cloud("uniform", 200, 1)
    out["smooth4"] = (p, smooth_features(p, REFERENCE_WIDTHS, 0.5, 11), 5, 1e-5, "interior")
    p = cloud("uniform", 150, 2)
    out["noise"] = (p, [torch.randn(150, w, generator=torch.Generator().manual_seed(13 + w)) for w in (3, 4)], 5, 1e-5, "negative")
    p = cloud("uniform", 100, 3)
    out["constant"] = (p, [torch.full((100, 3), 0.05), torch.full((100, 1), -0.05)], 5, 1e-5, "")
    p = with_duplicates(cloud("uniform", 120, 4), 5, 11)
    out["duplicates"] = (p, smooth_features(p, (3, 4, 1), 0.5, 14), 5, 1e-5, "interior")
    p = cloud("planar", 150, 5)
    out["planar"] = (p, smooth_features(p, (3, 1), 0.5, 15), 5, 1e-5, "interior")
    p = cloud("clustered", 200, 7)
    out["clustered"] = (p, smooth_features(p, (4,), 0.5, 16, wavelength=0.02), 5, 1e-5, "")
    p = cloud("uniform", 100, 27)
    out["k3"] = (p, smooth_features(p, (3, 1), 0.5, 17), 3, 1e-5, "interior")
    p = cloud("uniform", 100, 8)
    out["k8"] = (p, smooth_features(p, (4, 1), 0.5, 18), 8, 1e-5, "interior")
    p = cloud("uniform", 5, 9)
    out["n_equals_k"] = (p, [rand(19, 5, 3) + 0.5, rand(20, 5, 1) - 0.5], 5, 1e-5, "")
    return out


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = import_reference(sys.argv[1])
    torch.set_num_threads(1)
    arrays = {}
    for name, (points, features, k, eps, kind) in cases().items():
        points = points.float().contiguous()
        _, d2 = exact_knn(points, k)
        assert ambiguous_share(d2, 1e-4) == 0.0, (name, "a k-th / (k+1)-th neighbour distance within 1e-4 relative")
        arrays[f"{name}/points"] = points.numpy()
        arrays[f"{name}/k"], arrays[f"{name}/eps"] = np.array(k, dtype=np.int64), np.array(eps, dtype=np.float64)
        for t, f in enumerate(features):
            arrays[f"{name}/feature_{t}"] = f.float().contiguous().numpy()
        for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
            res, nn_ix = reference_eval(ref, points, [f.float() for f in features], k, eps, dtype)
            for key, v in res.items():
                arrays[f"{name}/{tag}/{key}"] = v
            arrays[f"{name}/nn_ix"] = nn_ix.numpy().astype(np.int32)
        means = arrays[f"{name}/f64/means"]
        print(name, "means", means, "terms", arrays[f"{name}/f64/terms"])
        if kind == "interior":
            assert ((means >= 0.05) & (means <= 0.95)).all(), (name, means)
        if kind == "negative":
            assert (means < -0.01).all() and (arrays[f"{name}/f64/terms"] == 1.0).all(), (name, means)
    # a weight / feature pair that did not come from query_nn: any non-negative matrix, not symmetric, B x n x n
    gen = torch.Generator().manual_seed(31)
    weight = torch.rand(40, 6, 6, generator=gen) + 0.05
    base = torch.randn(40, 1, 7, generator=gen)
    feature = base + 0.4 * torch.randn(40, 6, 7, generator=gen)
    arrays["free_pair/weight"], arrays["free_pair/feature"] = weight.numpy(), feature.numpy()
    for tag, dtype in (("f64", torch.float64), ("f32", torch.float32)):
        w = weight.to(dtype).clone().requires_grad_(True)
        x = feature.to(dtype).clone().requires_grad_(True)
        loss = ref.morans_loss(w, x)
        loss.backward()
        measure = ref.morans_measure(w.detach(), x.detach())
        for key, v in (("loss", loss), ("measure", measure), ("d_weight", w.grad), ("d_feature", x.grad)):
            arrays[f"free_pair/{tag}/{key}"] = v.detach().numpy().copy()
    m = arrays["free_pair/f64/measure"]
    print("free_pair measure", m)
    assert 0.05 <= m <= 0.95
    path = os.path.join(HERE, "moran_cases.npz")
    np.savez_compressed(path, **arrays)
    print(path, os.path.getsize(path), "bytes,", len(arrays), "arrays")


if __name__ == "__main__":
    main()
