"""A host restatement of wafer_diag_checksum, written from the definition in include/wafer_hip.h (not from the kernel), for
tests/test_checksum_model.py (CPU) and tests/test_gpu_checksum.py (GPU).

Over the work cells (x, y, k) counted, k the GLOBAL work plane, all arithmetic mod 2^64:

    h(z):  z = (z ^ z >> 30) * 0xbf58476d1ce4e5b9;  z = (z ^ z >> 27) * 0x94d049bb133111eb;  return z ^ z >> 31
    lin  = (k * ny + y) * nx + x
    term = h(bits ^ h(lin + 0x9e3779b97f4a7c15))
    sum  = the sum of the terms

bits is the 64 bits of the stored double on dtype "f64", and the 32 bits of the stored float, zero-extended, on "f32" and
"f32fast".  model() takes the cells AS STORED: on the float dtypes the caller passes values a float holds exactly (what
download_phi returns), and a value that a float does not hold is an error of the caller, not something to round here.

np.uint64 arrays wrap silently on * and +, which is the arithmetic wanted; model_slow() is the same sum in Python integers with
every reduction mod 2^64 written out, for the CPU test that holds the two together."""
import struct

import numpy as np

M1 = 0xbf58476d1ce4e5b9
M2 = 0x94d049bb133111eb
GOLDEN = 0x9e3779b97f4a7c15
MASK = (1 << 64) - 1
DTYPES = ("f64", "f32", "f32fast")


def hash64(z):
    """h() on a uint64 array"""
    z = np.asarray(z, dtype=np.uint64)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(M1)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(M2)
    return z ^ (z >> np.uint64(31))


def stored_bits(work_cells, dtype):
    """the bits of every cell in its storage type, as uint64 (the float dtypes zero-extended)"""
    if dtype not in DTYPES:
        raise ValueError(f"dtype {dtype!r}")
    cells = np.ascontiguousarray(work_cells, dtype=np.float64)
    if dtype == "f64":
        return cells.view(np.uint64)
    with np.errstate(over="ignore", invalid="ignore"):
        narrow = cells.astype(np.float32)
    same = narrow.astype(np.float64).view(np.uint64) == cells.view(np.uint64)
    if not np.all(same | np.isnan(cells)):
        raise ValueError("cells that a float does not hold: pass the values as stored")
    return narrow.view(np.uint32).astype(np.uint64)


def model(work_cells, z_first=0, dtype="f64"):
    """the checksum of the (nx, ny, nplanes) work cells of global work planes [z_first, z_first + nplanes), as a Python int;
    an array without planes sums to 0"""
    cells = np.asarray(work_cells)
    if cells.ndim != 3:
        raise ValueError("work cells are (nx, ny, nplanes)")
    nx, ny, nplanes = cells.shape
    if cells.size == 0:
        return 0
    bits = stored_bits(cells, dtype)
    x = np.arange(nx, dtype=np.uint64)[:, None, None]
    y = np.arange(ny, dtype=np.uint64)[None, :, None]
    k = (np.uint64(z_first) + np.arange(nplanes, dtype=np.uint64))[None, None, :]
    with np.errstate(over="ignore"):
        lin = (k * np.uint64(ny) + y) * np.uint64(nx) + x
        terms = hash64(bits ^ hash64(lin + np.uint64(GOLDEN)))
        return int(np.sum(terms, dtype=np.uint64))


def _hash64_int(z):
    z = ((z ^ (z >> 30)) * M1) & MASK
    z = ((z ^ (z >> 27)) * M2) & MASK
    return z ^ (z >> 31)


def model_slow(work_cells, z_first=0, dtype="f64"):
    """model() cell by cell in Python integers (small arrays only)"""
    cells = np.asarray(work_cells, dtype=np.float64)
    nx, ny, nplanes = cells.shape
    total = 0
    for x in range(nx):
        for y in range(ny):
            for kl in range(nplanes):
                v = float(cells[x, y, kl])
                if dtype == "f64":
                    bits = struct.unpack("<Q", struct.pack("<d", v))[0]
                else:
                    bits = struct.unpack("<I", struct.pack("<f", v))[0]
                lin = ((z_first + kl) * ny + y) * nx + x
                total = (total + _hash64_int(bits ^ _hash64_int((lin + GOLDEN) & MASK))) & MASK
    return total
