"""The histogram behind the load pipeline's radix select, in NumPy (TEST INFRASTRUCTURE).

``histogram`` is the specification of ``sushi_hip_load_histogram`` (csrc/sushi_load.hip: side_key, radix_hist_kernel):
  side 0: the samples >= 0, key = the float32's bit pattern;
  side 1: the samples <= 0, key = the bit pattern of -x;
  +0.0 and -0.0 -> key 0 on both sides (NumPy compares them equal); NaN belongs to neither side;
  of the keys with (key & mask) == prefix, bin (key >> shift) & 255 is counted.
``StandInLib`` puts it where ``sushi_amd.load._median`` / ``_select`` expect the library, so their bucket walk runs on the
CPU (tests/test_load_select_host.py); tests/test_load_scale_gpu.py compares the kernel with the same function.
``POPULATIONS`` are the crafted sample sets both files walk."""
import numpy as np
import torch


def side_keys(x, side):
    """uint32 keys of the members of one side of `x` (a float32 array), in `x`'s order."""
    x = np.ascontiguousarray(x, np.float32).reshape(-1)
    if side == 0:
        member = x >= 0
        bits = x[member].view(np.uint32)
    else:
        member = x <= 0
        bits = (-x[member]).view(np.uint32)
    return np.where(x[member] == 0, np.uint32(0), bits).astype(np.uint32)


def histogram(x, side, prefix, mask, shift):
    """int64[256]: what sushi_hip_load_histogram(x, len(x), side, prefix, mask, shift) leaves in `hist`."""
    keys = side_keys(x, side)
    keys = keys[(keys & np.uint32(mask)) == np.uint32(prefix)]
    return np.bincount(((keys >> np.uint32(shift)) & np.uint32(255)).astype(np.int64), minlength=256).astype(np.int64)


def median_key(x, side):
    """Key of the upper middle member of one side (0 for an empty side): a prefix whose filtered set is not empty."""
    keys = np.sort(side_keys(x, side))
    return int(keys[keys.shape[0] // 2]) if keys.shape[0] else 0


def levels(key):
    """The four (prefix, mask, shift) of the radix walk towards `key`."""
    return [(0, 0, 24), (key & 0xFF000000, 0xFF000000, 16), (key & 0xFFFF0000, 0xFFFF0000, 8),
            (key & 0xFFFFFF00, 0xFFFFFF00, 0)]


class StandInLib(object):
    """sushi_hip_load_histogram over a host array: `data` and `hist` are CPU tensors whose pointers the call must name."""

    def __init__(self, x):
        self.x = np.ascontiguousarray(x, np.float32).reshape(-1)
        self.data = torch.from_numpy(self.x)
        self.hist = torch.zeros(256, dtype=torch.int64)
        self.calls = []

    def sushi_hip_load_histogram(self, data_ptr, n, side, prefix, mask, shift, hist_ptr, stream):
        assert data_ptr == self.data.data_ptr() and hist_ptr == self.hist.data_ptr() and n == self.x.shape[0]
        assert side in (0, 1) and shift in (24, 16, 8, 0) and prefix & ~mask == 0
        self.calls.append((side, prefix, mask, shift))
        self.hist.copy_(torch.from_numpy(histogram(self.x, side, prefix, mask, shift)))
        return 0


def _random_thirds():
    rng = np.random.default_rng(20261018)
    return rng.integers(-30000, 30001, 100000).astype(np.float32) / np.float32(3)


def _low_byte_only():
    k = np.arange(200)
    v = (1000.0 + k * 2.0 ** -14).astype(np.float32)          # 200 consecutive float32 values: one ulp of 1000 is 2^-14
    return np.where(k % 2 == 0, v, -v).astype(np.float32)


# (id, builder of a float32 array); every one has at least one sample on each side of zero
POPULATIONS = [
    ("even-different-middles", lambda: np.array([1, 2, 3, 4.5, -1, -2, -3.25, -7], np.float32)),
    ("random-thirds", _random_thirds),
    ("signed-zeros-subnormals", lambda: np.array([-0.0, 0.0, -0.0, 5, -5, 1e-40, -1e-40], np.float32)),
    ("subnormal-runs", lambda: np.array([1e-41] * 50 + [-3e-42] * 50 + [1, -1], np.float32)),
    ("low-byte-only", _low_byte_only),
    ("tie-run-across-rank", lambda: np.array([7] * 1000 + [9] * 999 + [-2] * 500 + [-4] * 500, np.float32)),
    ("two", lambda: np.array([3, -4], np.float32)),
    ("one-zero", lambda: np.array([0], np.float32)),
]
POPULATION_IDS = [p[0] for p in POPULATIONS]


def expected_medians(x):
    """(np.median of the samples >= 0, np.median of the samples <= 0) as Python floats: what wav.py:145-146 computes."""
    return float(np.median(x[x >= 0])), float(np.median(x[x <= 0]))
