"""The bucket walk of the load pipeline's radix select (sushi_amd/load.py: _median, _select) on the CPU: the library's
histogram call is replaced by its NumPy specification (tests/load_select_ref.py), so what is tested here is the walk --
which bucket holds the rank, what rank is left inside it, which two order statistics an even count needs, and how a
side's key turns back into a sample.  Exact: ``==`` against np.median of each side of zero (wav.py:145-146)."""
import numpy as np
import pytest

import load_select_ref as ref
from sushi_amd import SushiError, load


@pytest.mark.parametrize("name,make", ref.POPULATIONS, ids=ref.POPULATION_IDS)
def test_median_walk_equals_numpy_median(name, make):
    x = make()
    want = ref.expected_medians(x)
    lib = ref.StandInLib(x)
    for side in (0, 1):
        got = load._median(lib, lib.data, x.shape[0], side, lib.hist, None)
        assert isinstance(got, float)
        assert got == want[side], (name, side, got, want[side])
    # after the count of a side, every select walks all four levels, top byte first, each under the prefix chosen above it
    walks = [c for c in lib.calls if c[0] == 1][1:]
    assert len(walks) % 4 == 0 and [c[3] for c in walks[:4]] == [24, 16, 8, 0]
    assert all(a[1] == b[1] & a[2] for a, b in zip(walks[:3], walks[1:4]))


def test_select_returns_the_key_of_every_rank():
    """_select against a sort of the side's keys, at every rank of a population with ties, zeros of both signs and keys that
    share their upper bytes."""
    x = np.concatenate([ref._low_byte_only(), np.array([0.0, -0.0, 7, 7, 7, -7, -7, 1e-41, -1e-41, 65536.0, -0.5], np.float32)])
    lib = ref.StandInLib(x)
    for side in (0, 1):
        keys = np.sort(ref.side_keys(x, side))
        got = [load._select(lib, lib.data, x.shape[0], side, r, lib.hist, None) for r in range(keys.shape[0])]
        assert got == [int(k) for k in keys], side
        with pytest.raises(SushiError):
            load._select(lib, lib.data, x.shape[0], side, keys.shape[0], lib.hist, None)


def test_one_sided_population_raises_for_the_empty_side():
    x = np.array([1, 2, 3], np.float32)
    lib = ref.StandInLib(x)
    assert load._median(lib, lib.data, 3, 0, lib.hist, None) == 2.0
    with pytest.raises(SushiError):
        load._median(lib, lib.data, 3, 1, lib.hist, None)


def test_stand_in_histogram_is_the_stated_key_rule():
    """The specification itself, on values whose keys are known by hand."""
    x = np.array([0.0, -0.0, 1.0, -1.0, 2.0, np.nan, 1e-45, -1e-45], np.float32)
    assert list(ref.side_keys(x, 0)) == [0, 0, 0x3F800000, 0x40000000, 1]
    assert list(ref.side_keys(x, 1)) == [0, 0, 0x3F800000, 1]
    h = ref.histogram(x, 0, 0, 0, 24)
    assert h.sum() == 5 and h[0] == 3 and h[0x3F] == 1 and h[0x40] == 1
    h = ref.histogram(x, 1, 0x3F800000, 0xFFFF0000, 8)
    assert h.sum() == 1 and h[0] == 1
    assert ref.histogram(x, 0, 0, 0xFFFFFF00, 0)[1] == 1 and ref.histogram(x, 0, 0, 0xFFFFFF00, 0)[0] == 2
    assert ref.levels(0x12345678) == [(0, 0, 24), (0x12000000, 0xFF000000, 16), (0x12340000, 0xFFFF0000, 8),
                                      (0x12345600, 0xFFFFFF00, 0)]
