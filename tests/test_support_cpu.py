"""The truth table of tests/support.py's comparisons: what "bit for bit" accepts and refuses, in both modes."""
import numpy as np
import pytest
import torch

from support import same_bits, same_values, twice, words

f32 = np.float32
MODES = (True, False)  # nan_payload


def nan32(sign, payload):
    return np.array([(sign << 31) | 0x7F800000 | payload], np.uint32).view(f32)[0]


def refuses(got, want, *what, **kw):
    with pytest.raises(AssertionError) as err:
        same_bits(got, want, *what, **kw)
    return str(err.value)


@pytest.mark.parametrize("nan_payload", MODES)
def test_equal_arrays_pass_and_one_bit_fails(nan_payload):
    a = np.linspace(-3, 7, 15, dtype=f32).reshape(3, 5)
    same_bits(a.copy(), a, nan_payload=nan_payload)
    b = a.copy()
    b.view(np.uint32)[1, 2] ^= 1  # the last mantissa bit of one element
    refuses(b, a, nan_payload=nan_payload)
    refuses(np.array([-0.0], f32), np.array([0.0], f32), nan_payload=nan_payload)
    refuses(np.array([np.nan], f32), np.array([1.0], f32), nan_payload=nan_payload)
    refuses(np.array([1.0], f32), np.array([np.nan], f32), nan_payload=nan_payload)


def test_nan_payload_and_sign_count_only_in_exact_mode():
    a = np.array([1.0, nan32(0, 0x400000), 2.0, nan32(1, 0x1234)], f32)
    b = np.array([1.0, nan32(1, 0x000001), 2.0, nan32(0, 0x400000)], f32)
    assert np.isnan(a[[1, 3]]).all() and np.isnan(b[[1, 3]]).all() and a.tobytes() != b.tobytes()
    same_bits(a, a.copy())
    refuses(a, b)
    same_bits(a, b, nan_payload=False)
    with np.errstate(invalid="ignore"):  # widening a signalling NaN
        same_bits(a.astype(np.float64), b.astype(np.float64), nan_payload=False)
    same_bits(float("nan"), -float("nan"), nan_payload=False)


@pytest.mark.parametrize("nan_payload", MODES)
def test_dtype_and_shape_are_compared_first(nan_payload):
    refuses(np.ones(4, f32), np.ones(4, np.float64), nan_payload=nan_payload)
    assert "dtype" in refuses(np.ones(4, f32).view(np.int32), np.ones(4, f32), nan_payload=nan_payload)  # equal bytes
    assert "shape" in refuses(np.ones((2, 3), f32), np.ones((3, 2), f32), nan_payload=nan_payload)
    refuses(np.zeros((0,), f32), np.zeros((0, 3), f32), nan_payload=nan_payload)
    same_bits(np.zeros((0, 3), f32), np.zeros((0, 3), f32), nan_payload=nan_payload)


@pytest.mark.parametrize("nan_payload", MODES)
def test_lists_tuples_and_none(nan_payload):
    a, b = np.arange(3, dtype=np.int32), np.ones(2, f32)
    same_bits([a, (b, None)], (a.copy(), [b.copy(), None]), nan_payload=nan_payload)
    refuses([a, [b, b]], [a, [b]], nan_payload=nan_payload)
    refuses([a], [a, a], nan_payload=nan_payload)
    refuses(None, a, nan_payload=nan_payload)
    refuses(a, None, nan_payload=nan_payload)
    refuses([a], a, nan_payload=nan_payload)
    same_bits(None, None, nan_payload=nan_payload)


@pytest.mark.parametrize("nan_payload", MODES)
@pytest.mark.parametrize("dtype", [np.int8, np.uint8, np.bool_, np.int32, np.int64, np.float32, np.float64])
def test_every_dtype_in_both_modes(dtype, nan_payload):
    a = (np.arange(10) % 2).astype(dtype)
    same_bits(a, a.copy(), nan_payload=nan_payload)
    same_bits(torch.from_numpy(a), a, nan_payload=nan_payload)  # a tensor against an array
    same_bits(a[3], a[5], nan_payload=nan_payload)              # scalars
    b = a.copy()
    b[7] = 1 - b[7]
    assert "1 of 10" in refuses(b, a, nan_payload=nan_payload)


def test_a_view_compares_by_its_elements():
    base = np.arange(24, dtype=f32).reshape(4, 6)
    got = base[:, ::2]
    assert not got.flags.c_contiguous
    same_bits(got, got.copy())
    same_bits(torch.from_numpy(base)[:, ::2], got.copy())
    same_bits(base.T, np.ascontiguousarray(base.T), nan_payload=False)
    refuses(got, base[:, 1::2])


def test_the_message_says_where_and_how_many():
    want = np.zeros((3, 4), f32)
    got = want.copy()
    got[1, 2], got[2, 0], got[2, 3] = 0.5, np.inf, -0.0
    text = refuses(got, want, "depth of view 2")
    assert "depth of view 2" in text and "3 of 12 elements differ" in text and "first at (1, 2)" in text
    assert "0.5 (0000003f)" in text and "0.0 (00000000)" in text  # both values there, with their bytes
    assert "largest |difference| over the finite elements 5.000e-01" in text
    assert "list[1]" in refuses([want, got], [want, want], "list")


def test_twice_runs_over_the_exact_mode():
    results = iter([np.array([1.0, 2.0], f32), np.array([1.0, np.nextafter(f32(2), f32(3))], f32)])
    with pytest.raises(AssertionError, match="second run"):
        twice(lambda: (next(results), None))
    calls = []
    out = twice(lambda: calls.append(1) or [np.arange(3), (np.ones(2, f32), None)])
    assert len(calls) == 2 and out[0].tolist() == [0, 1, 2]
    nans = iter([np.array([nan32(0, 1)], f32), np.array([nan32(1, 1)], f32)])
    with pytest.raises(AssertionError):
        twice(lambda: next(nans))  # another NaN is another result


def test_same_values_is_the_comparison_by_value():
    same_values(np.array([-0.0, 1.0], f32), np.array([0.0, 1.0], f32))
    same_values([np.arange(3)], [np.arange(3)])
    for got, want in ((np.array([np.nan], f32), np.array([np.nan], f32)), (np.ones(2, f32), np.ones(2, np.float64)),
                      (np.ones(2, f32), np.ones((2, 1), f32)), (np.array([1, 2]), np.array([1, 3])), ([np.ones(1)], [np.ones(1)] * 2)):
        with pytest.raises(AssertionError):
            same_values(got, want)


def test_words_are_the_float32_bits():
    a = np.array([[1.0, -0.0], [np.inf, 2.0 ** -149]], f32)
    assert words(a).dtype == np.uint32 and words(a).tolist() == [[0x3F800000, 0x80000000], [0x7F800000, 1]]
    assert words(a[:, 1]).tolist() == [0x80000000, 1] and words(f32(1.0)).tolist() == [0x3F800000]
    with pytest.raises(AssertionError):
        words(a.astype(np.float64))
