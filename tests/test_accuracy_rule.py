"""tests/accuracy.py on known answers: two-element tensors whose d and r are powers of two, so every ratio is exact.  No GPU."""
import math

import pytest
import torch

from tests.accuracy import FACTOR, assert_deviations, bound, same_bits, ulp32, within

T = lambda *v: torch.tensor(v, dtype=torch.float64)
E = 2.0 ** -20


def run(got, ref64, ref32):
    return within("rule", "case", {"x": got}, {"x": ref64}, {"x": ref32})


def test_r_comes_from_the_float32_evaluation():
    ref64 = T(1.0, 2.0)
    ref32 = ref64 + T(E, 0.0)
    assert FACTOR == 4.0
    assert run(ref64 + T(4 * E, 0.0), ref64, ref32) == 1.0
    assert run(ref32, ref64, ref32) == 0.25
    with pytest.raises(AssertionError):
        run(ref64 + T(5 * E, 0.0), ref64, ref32)


def test_r_is_floored_at_one_ulp_of_the_largest_magnitude():
    ref64 = T(1.0, -3.0)
    u = 2.0 ** -22                                        # float32 spacing in [2, 4)
    assert run(ref64 + T(4 * u, 0.0), ref64, ref64) == 1.0
    assert run(ref64 + T(0.0, -2 * u), ref64, ref64) == 0.5
    with pytest.raises(AssertionError):
        run(ref64 + T(5 * u, 0.0), ref64, ref64)


@pytest.mark.parametrize("bad", (float("nan"), float("inf"), float("-inf")))
def test_non_finite_values_fail_wherever_they_are(bad):
    ref64 = T(0.0, 1.0)
    with pytest.raises(AssertionError):
        run(T(bad, 1.0), ref64, ref64)
    with pytest.raises(AssertionError):
        run(T(0.0, bad), ref64, ref64)


def test_names_shapes_and_empty_tensors():
    ref64 = T(1.0, 2.0)
    with pytest.raises(AssertionError):
        within("rule", "missing name", {"y": ref64}, {"x": ref64}, {"x": ref64})
    assert within("rule", "another name more", {"x": ref64, "y": ref64 + 1.0}, {"x": ref64}, {"x": ref64}) == 0.0
    empty = torch.zeros(0, 3, dtype=torch.float64)
    assert within("rule", "empty", {"x": empty.float()}, {"x": empty}, {"x": empty.float()}) == 0.0
    ref = torch.arange(6, dtype=torch.float64).reshape(2, 3)
    assert within("rule", "reshaped", {"x": ref.float().reshape(3, 2)}, {"x": ref}, {"x": ref.float().reshape(6)}) == 0.0
    with pytest.raises(RuntimeError):
        within("rule", "another element count", {"x": torch.zeros(5)}, {"x": ref}, {"x": ref})
    moved = ref.clone()                                   # the same values at other places are another tensor
    moved[0, 1], moved[1, 0] = ref[1, 0], ref[0, 1]
    with pytest.raises(AssertionError):
        within("rule", "transposed", {"x": moved}, {"x": ref}, {"x": ref})


def test_the_worst_tensor_is_returned_and_every_tensor_is_held(capsys):
    ref64 = {"a": T(1.0, 2.0), "b": T(1.0, 2.0)}
    ref32 = {k: v + T(E, 0.0) for k, v in ref64.items()}
    got = {"a": ref64["a"] + T(2 * E, 0.0), "b": ref64["b"] + T(0.0, 3 * E)}
    assert within("rule", "two tensors", got, ref64, ref32) == 0.75
    assert "[rule] two tensors: 2 tensors, worst d/4r 0.750 (b)  b 0.750  a 0.500" in capsys.readouterr().out
    assert within("rule", "two tensors", got, ref64, ref32, show=1) == 0.75
    assert capsys.readouterr().out.rstrip().endswith("(b)  b 0.750")
    within("rule", "all", got, ref64, ref32, show=None)
    assert capsys.readouterr().out.rstrip().endswith("(b)  b 0.750  a 0.500")
    got["a"] = ref64["a"] + T(5 * E, 0.0)
    with pytest.raises(AssertionError):
        within("rule", "one of two fails", got, ref64, ref32)
    assert "a 1.250" in capsys.readouterr().out, "the ratios are printed before the assertion"


@pytest.mark.parametrize("x", (1e-30, 0.5, 0.99999997, 1.0, 1.5, 2.0, 3.0, 1e10, 3.4e38))
def test_ulp32_is_the_spacing_of_the_binade(x):
    x32 = float(torch.tensor(x, dtype=torch.float32))     # 0.99999997 rounds to 1 - 2^-24, the last float32 below 1
    assert ulp32(x) == ulp32(-x) == 2.0 ** (math.frexp(x32)[1] - 24)


def test_ulp32_of_zero_is_the_smallest_subnormal():
    assert ulp32(0.0) == 2.0 ** -149


def test_bound_takes_the_largest_error_of_the_approximations():
    ref64 = T(1.0, 3.0)
    assert bound(ref64, ref64 + T(E, 0.0), ref64 + T(0.0, 2 * E)) == 4.0 * 2 * E
    assert bound(ref64, ref64.float()) == 4.0 * 2.0 ** -22                       # the floor: one ulp at 3
    assert bound(ref64, ref64 + T(2.0 ** -30, 0.0), floor=False) == 4.0 * 2.0 ** -30


def test_assert_deviations_holds_every_key_to_four_r(capsys):
    r = {"a": 1.0, "b": 0.25}
    assert_deviations("rule", "at the bound", {"a": 4.0, "b": 1.0}, r, ("a", "b"))
    assert "a 4.000e+00/4.000e+00 = 1.00" in capsys.readouterr().out
    assert_deviations("rule", "a key that is not asked for", {"a": 4.0, "b": 9.0}, r, ("a",))
    with pytest.raises(AssertionError):
        assert_deviations("rule", "above", {"a": 4.0, "b": 1.0 + 2.0 ** -50}, r, ("a", "b"))
    assert "b 1.000e+00/1.000e+00" in capsys.readouterr().out, "the ratios are printed before the assertion"
    assert_deviations("rule", "nothing allowed, nothing there", {"a": 0.0}, {"a": 0.0}, ("a",))
    with pytest.raises(AssertionError):
        assert_deviations("rule", "not a number", {"a": float("nan")}, r, ("a",))


def test_same_bits_is_torch_equal_per_key():
    a = {"x": torch.tensor([1.0, 2.0]), "y": torch.tensor([3])}
    assert same_bits(a, {k: v.clone() for k, v in a.items()})
    assert not same_bits(a, {"x": a["x"]}) and not same_bits({"x": a["x"]}, a)                   # other keys
    assert same_bits(a, {"x": a["x"], "y": torch.tensor([4])}, keys=("x",))
    assert not same_bits(a, {"x": a["x"], "y": torch.tensor([4])})
    assert not same_bits(a, {"x": torch.tensor([1.0, 2.0 + 2.0 ** -22]), "y": a["y"]})
    # as torch.equal has it: the two zeros compare equal, NaN equals nothing
    zeros = same_bits({"x": torch.tensor([0.0])}, {"x": torch.tensor([-0.0])})
    assert zeros == torch.equal(torch.tensor([0.0]), torch.tensor([-0.0])) and zeros is True
    assert not same_bits({"x": torch.tensor([float("nan")])}, {"x": torch.tensor([float("nan")])})
