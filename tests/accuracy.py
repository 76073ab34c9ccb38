"""The suite's accuracy rule, stated once.

A kernel is one more float32 evaluation of a formula whose float64 evaluation is the reference.  Per tensor, its deviation
d = max |ours - float64 reference| over EVERY element may be FACTOR times r, where r is the deviation of another float32 evaluation
of the same formula (the restatement in float32, or the reference's own float32 run) from the same float64 reference, floored
at one float32 ulp of the tensor's largest magnitude.  Every check prints its ratios d / (FACTOR r) before it asserts (run
pytest with -s).  Imports numpy and torch only."""
import numpy as np
import torch

FACTOR = 4.0


def ulp32(x: float) -> float:
    """the spacing of float32 at |x|"""
    return float(np.spacing(np.float32(abs(x))))


def bound(ref64, *approximations, floor=True):
    """FACTOR x the largest error of the given approximations of ref64, floored at one float32 ulp of the tensor's maximum"""
    errors = [(a.detach().double().cpu() - ref64).abs().max().item() for a in approximations]
    return FACTOR * max(errors + ([ulp32(ref64.abs().max().item())] if floor else []))


def within(label, tag, got, ref64, ref32, show=6):
    """got / ref64 / ref32: {name: tensor}.  Asserts d <= FACTOR r for every name of ref64, with r from ref32, and returns the worst
    ratio d / (FACTOR r).  got[k] is reshaped to the reference's shape and must be finite; an empty tensor has d = 0.  Prints the
    `show` worst ratios (None: all of them)."""
    lines, bad = [], []
    for k, w in ref64.items():
        assert k in got, (label, tag, k, "missing")
        g = got[k].detach().double().cpu().reshape(w.shape)
        assert torch.isfinite(g).all(), (label, tag, k, "not finite")
        top = w.abs().max().item() if w.numel() else 0.0
        r = max((ref32[k].double().reshape(w.shape) - w).abs().max().item() if w.numel() else 0.0, ulp32(top))
        d = (g - w).abs().max().item() if w.numel() else 0.0
        lines.append((d / (FACTOR * r), k, d, r))
        if not d <= FACTOR * r:
            bad.append((k, d, FACTOR * r))
    worst = max(lines)
    print(f"[{label}] {tag}: {len(lines)} tensors, worst d/4r {worst[0]:.3f} ({worst[1]})  " +
          "  ".join(f"{k} {q:.3f}" for q, k, _, _ in sorted(lines, reverse=True)[:show]))
    assert not bad, (label, tag, bad)
    return worst[0]


def assert_deviations(label, tag, d, r, keys):
    """d, r: {key: number}, r precomputed by the caller.  Asserts d[k] <= FACTOR r[k] for every key, printing the ratios first."""
    print(f"[{label}] {tag}: " + "  ".join(f"{k} {d[k]:.3e}/{FACTOR * r[k]:.3e}" + (f" = {d[k] / (FACTOR * r[k]):.2f}" if r[k] > 0 else "")
                                            for k in keys))
    for k in keys:
        assert d[k] <= FACTOR * r[k], (label, tag, k, d[k], FACTOR * r[k])


def same_bits(a: dict, b: dict, keys=None) -> bool:
    """torch.equal for every key (None: the two dicts must hold the same keys, and every one of them is compared)"""
    if keys is None:
        if a.keys() != b.keys():
            return False
        keys = a.keys()
    return all(torch.equal(a[k], b[k]) for k in keys)
