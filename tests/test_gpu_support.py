"""The transfers of tests/support.py on the device: what goes up comes back with the same bytes."""
import numpy as np
import pytest
import torch

from support import DEV, dev, devs, host, hosts, same_bits

f32 = np.float32


def special_floats(n):
    """NaNs of both signs with non-default payloads, infinities, denormals, both zeros, repeated to n values."""
    bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFABCDEF, 0x7FD55555, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF,
                     0x80000000, 0x00000000, 0x3F800000, 0xC2F6E979], np.uint32)
    return np.resize(bits, n).view(f32)


@pytest.mark.gpu
def test_a_round_trip_keeps_every_byte():
    rng = np.random.default_rng(3)
    for n in (0, 1, 65):
        arrays = [rng.standard_normal(n), rng.standard_normal(n).astype(f32), rng.integers(-128, 128, n).astype(np.int8),
                  rng.integers(0, 256, n).astype(np.uint8), rng.random(n) < 0.5, rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32),
                  rng.integers(-2 ** 63, 2 ** 63, n), special_floats(n)]
        for a in arrays:
            t = dev(a)
            assert t.device == DEV and t.is_contiguous() and tuple(t.shape) == a.shape
            back = host(t)
            assert back.dtype == a.dtype and back.shape == a.shape and back.tobytes() == a.tobytes(), (n, a.dtype)
        same_bits(hosts(devs(arrays)), arrays, f"n = {n}")
    grid = special_floats(65 * 6).reshape(65, 6)
    for view in (grid[:, ::2], grid.T, grid[::-1]):
        assert not view.flags.c_contiguous
        assert dev(view).is_contiguous() and host(dev(view)).tobytes() == np.ascontiguousarray(view).tobytes()
    assert dev(None) is None and dev(np.arange(3), torch.float32).dtype == torch.float32
    assert host([1.5, 2.5]).dtype == np.float64 and host(torch.ones(2, requires_grad=True)).tolist() == [1.0, 1.0]
