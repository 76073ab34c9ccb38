"""The float64 restatement of the visual-hull test (tests/hull_reference.py) against the reference's own survivor sets
(tests/golden/hull_cases.npz, written by tests/golden/make_hull_golden.py from calls of the reference's functions).

Where the reference computed in float64 the sets must be equal.  Its Blender branches compute in float32: there a voxel may be
decided the other way only if it lies within delta32 of a rounding boundary, and at most 1e-3 of the survivors
may.  Observed when the fixtures were written: no voxel differs in any case."""
import numpy as np
import pytest

from tests import hull_reference as R

CASES = R.golden_cases()


def restated(c):
    if "points" in c:
        alive, margin = R.hull_points(c["points"], c["masks"], c["matrices"], c["convention"], c["outside"])
        return np.nonzero(alive)[0].astype(np.int32), margin
    return R.hull_grid(c["masks"], c["matrices"], c["aabb"], c["G"], c["convention"], c["outside"])


def test_fixture_inventory():
    assert sorted(CASES) == ["blender_hull", "blender_load", "samples_krt", "samples_list"]
    assert CASES["samples_krt"]["G"] == 32 and CASES["samples_list"]["G"] == 32 and CASES["blender_hull"]["G"] == 256
    assert len({m.shape for m in CASES["samples_list"]["masks"]}) > 1                    # ragged
    assert [CASES[k]["float32"] for k in sorted(CASES)] == [True, True, False, False]
    for c in CASES.values():
        assert c["indices"].dtype == np.int32 and len(c["indices"]) > 100 and np.all(np.diff(c["indices"]) > 0)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_the_reference(name):
    c = CASES[name]
    got, margin = restated(c)
    want = c["indices"]
    differ = np.setxor1d(got, want)
    print(f"{name}: {len(want)} survivors in the reference, {len(got)} restated, {len(differ)} differ"
          + (f", largest margin of a differing item {margin[differ].max():.3e} px" if len(differ) else ""))
    if not c["float32"]:
        assert np.array_equal(got, want)
        return
    size = c["masks"][0].shape[0]
    assert all(m.shape == (size, size) for m in c["masks"])       # the "ndc" mapping equals the reference for square images
    assert len(differ) <= 1e-3 * len(want)
    assert np.all(margin[differ] < R.delta32(size))


def test_margin_statistics():
    """the share of voxels near a rounding boundary (what the GPU tests' 1e-9 px requirement rests on)"""
    c = CASES["samples_krt"]
    _, margin = restated(c)
    near = margin[np.isfinite(margin)]
    print(f"samples_krt: {np.mean(near < 1e-3):.4f} of the voxels within 1e-3 px of a boundary, smallest margin {near.min():.3e} px")
    assert near.min() > 1e-9 and np.mean(near < 1e-3) < 0.05


def test_restatement_edge_rules():
    """half to even in both directions, no sign test on h2, non-finite carved under both policies, `keep` keeps the outside"""
    M = np.array([[[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0]]])       # u = x / z, v = y / z
    mask = np.zeros((1, 5, 5), np.uint8)
    mask[0, 2, 2] = mask[0, 2, 0] = 1
    pts = np.array([[1.5, 2.0, 1.0],      # px = 1.5 -> 2 (even): hit
                    [2.5, 2.0, 1.0],      # px = 2.5 -> 2 (even): hit
                    [0.5, 2.0, 1.0],      # px = 0.5 -> 0: hit (mask[2, 0])
                    [3.5, 2.0, 1.0],      # px = 3.5 -> 4: miss
                    [-2.0, -2.0, -1.0],   # behind the camera, projects to (2, 2): survives
                    [1.0, 1.0, 0.0],      # h2 = 0: infinite
                    [0.0, 0.0, 0.0],      # 0 / 0
                    [9.0, 2.0, 1.0]])     # outside the image
    for outside, want in (("carve", [1, 1, 1, 0, 1, 0, 0, 0]), ("keep", [1, 1, 1, 0, 1, 0, 0, 1])):
        alive, _ = R.hull_points(pts, mask, M, "krt", outside)
        assert alive.tolist() == [bool(w) for w in want], outside
