"""tests/checksum_model.py, the host restatement of wafer_diag_checksum that tests/test_gpu_checksum.py holds the kernel to:
the vectorised numpy form against a cell-by-cell sum in Python integers, and the properties every use of the checksum relies
on -- additive over planes, sensitive to one bit of one cell and to where a value sits."""
import numpy as np
import pytest

from tests.checksum_model import DTYPES, MASK, hash64, model, model_slow, stored_bits


def _cells(shape, seed, dtype):
    c = np.random.default_rng(seed).standard_normal(shape)
    return c if dtype == "f64" else c.astype(np.float32).astype(np.float64)


def test_hash_is_the_documented_mixer():
    """h(0) = 0 (every stage maps 0 to 0), and h(1) by hand from the two constants"""
    z = 1
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & MASK
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & MASK
    z ^= z >> 31
    got = hash64(np.array([0, 1], dtype=np.uint64))
    assert int(got[0]) == 0 and int(got[1]) == z


@pytest.mark.parametrize("shape,z_first,dtype", [((130, 9, 7), 0, "f64"), ((7, 5, 3), 11, "f32"), ((66, 3, 2), 2 ** 20, "f32fast")])
def test_vectorised_model_equals_the_python_int_loop(shape, z_first, dtype):
    cells = _cells(shape, 5, dtype)
    cells[0, 0, 0], cells[-1, -1, -1], cells[1, 2, 1] = -0.0, np.inf, -np.inf
    got = model(cells, z_first, dtype)
    assert isinstance(got, int) and 0 <= got <= MASK
    assert got == model_slow(cells, z_first, dtype)


def test_float_dtypes_take_32_zero_extended_bits():
    cells = _cells((5, 4, 3), 6, "f32")
    bits = stored_bits(cells, "f32")
    assert bits.dtype == np.uint64 and int(bits.max()) < 2 ** 32
    assert np.array_equal(bits, cells.astype(np.float32).view(np.uint32))
    assert model(cells, 0, "f32") == model(cells, 0, "f32fast") != model(cells, 0, "f64")
    with pytest.raises(ValueError):      # as stored: a value a float does not hold is the caller's mistake
        model(np.full((1, 1, 1), 0.1), 0, "f32")


@pytest.mark.parametrize("dtype", DTYPES)
def test_additive_over_a_partition_of_the_planes(dtype):
    cells = _cells((33, 6, 12), 7, dtype)
    whole = model(cells, 0, dtype)
    for cuts in ([0, 12], [0, 1, 12], [0, 5, 6, 11, 12], list(range(13))):
        parts = [model(cells[:, :, a:b], a, dtype) for a, b in zip(cuts, cuts[1:])]
        assert sum(parts) & MASK == whole
    assert model(cells[:, :, 4:4], 4, dtype) == 0
    # the planes are GLOBAL: the same values on other planes are another sum
    assert model(cells[:, :, 3:7], 3, dtype) != model(cells[:, :, 3:7], 4, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_one_ulp_of_one_cell_changes_the_sum(dtype):
    cells = _cells((65, 5, 4), 8, dtype)
    base = model(cells, 0, dtype)
    for at in [(0, 0, 0), (64, 4, 3), (63, 2, 1)]:
        c = cells.copy()
        if dtype == "f64":
            c[at] = np.nextafter(c[at], np.inf)
        else:
            c[at] = np.nextafter(np.float32(c[at]), np.float32(np.inf))
        assert c[at] != cells[at]
        assert model(c, 0, dtype) != base


@pytest.mark.parametrize("dtype", DTYPES)
def test_swapping_two_unequal_cells_changes_the_sum(dtype):
    cells = _cells((65, 5, 4), 9, dtype)
    base = model(cells, 0, dtype)
    for a, b in [((0, 0, 0), (1, 0, 0)), ((3, 1, 2), (3, 2, 2)), ((10, 4, 0), (10, 4, 3)), ((63, 2, 1), (64, 2, 1))]:
        assert cells[a] != cells[b]
        c = cells.copy()
        c[a], c[b] = cells[b], cells[a]
        assert model(c, 0, dtype) != base


@pytest.mark.parametrize("dtype", DTYPES)
def test_signed_zeros_differ(dtype):
    plus, minus = np.zeros((3, 2, 2)), np.zeros((3, 2, 2))
    minus[1, 1, 0] = -0.0
    assert np.array_equal(plus, minus)
    assert model(plus, 0, dtype) != model(minus, 0, dtype)
    assert model(minus, 0, dtype) == model_slow(minus, 0, dtype)
