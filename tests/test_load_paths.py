"""Every way a WavStream comes into being -- WavStream(path), downmix=, load_mixes, from_samples, from_channels, retimed -- against
tests/golden/load_paths.json, the digests of what the NumPy load path made of the same inputs when the file was generated
(tests/golden/gen_load_paths_golden.py; inputs and constructors: tests/load_paths_cases.py).  Without a GPU on the NumPy path;
with one on the device path too, every file in several uploads, where the row left in HBM must hold the same bytes."""
import json
import os

import pytest

import load_paths_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "load_paths.json")) as _f:
    GOLDEN = json.load(_f)["cases"]


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("load_paths")
    return dict((name, cases.write_input(d, name)) for name in cases.INPUTS)


def test_golden_file_covers_the_cross_product():
    want = set(cases.key(n, t, r, h) for n in cases.INPUTS for t in cases.SAMPLE_TYPES for r in cases.RESAMPLE_MODES
               for h in cases.CONSTRUCTORS)
    assert set(GOLDEN) == want and len(want) == 4 * 4 * 7
    # only the mono file's side mixes are errors
    assert sorted(k for k, g in GOLDEN.items() if "error" in g) == sorted(
        k for k in want if k.startswith("mono16-12k/") and k.rsplit("/", 1)[1] in ("init-side", "load_mixes"))


def _check(inputs, name, sample_type, resample, on_device):
    path, top, rate = inputs[name]
    for how in cases.CONSTRUCTORS:
        where = cases.key(name, sample_type, resample, how)
        got, streams = cases.outcome(how, path, top, rate, sample_type, resample)
        assert got == GOLDEN[where], where
        for s in streams:
            if on_device:
                assert s._dev_row is not None and s._dev_row.is_cuda, where
                assert s._dev_row.cpu().numpy().tobytes() == s.data.tobytes(), where
            else:
                assert s._dev_row is None, where


@pytest.mark.parametrize("resample", cases.RESAMPLE_MODES)
@pytest.mark.parametrize("sample_type", cases.SAMPLE_TYPES)
@pytest.mark.parametrize("name", sorted(cases.INPUTS))
def test_host_path_builds_what_the_golden_file_holds(monkeypatch, inputs, name, sample_type, resample):
    monkeypatch.setenv("SUSHI_HIP_LOAD", "host")
    _check(inputs, name, sample_type, resample, on_device=False)


@pytest.mark.gpu
@pytest.mark.parametrize("resample", cases.RESAMPLE_MODES)
@pytest.mark.parametrize("sample_type", cases.SAMPLE_TYPES)
@pytest.mark.parametrize("name", sorted(cases.INPUTS))
def test_device_path_builds_what_the_golden_file_holds(monkeypatch, inputs, name, sample_type, resample):
    from sushi_amd import load
    monkeypatch.setenv("SUSHI_HIP_LOAD", "auto")
    monkeypatch.setattr(load, "UPLOAD_CHUNK_BYTES", cases.UPLOAD_BYTES)
    _check(inputs, name, sample_type, resample, on_device=True)
