"""What a batch handle holds about its requests, on the CPU: sushi_amd/csrc/batch_core.hpp (host only) built with g++ into
tests/host_batch_check.cpp, which checks what a staged batch must be over the table of cases of tests/batch_cases.hpp; its --dump
against the recorded images (tests/golden/batch_stage.json); and, on the GPU, the bytes the library really uploads against the
images the check writes -- the library and the check are the same code."""
import json
import os
import subprocess

import numpy as np
import pytest

from host_checks import build_check

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    return build_check("host_batch_check", tmp_path_factory.mktemp("batch_check"))


def test_every_staged_case_passes_its_checks(check_exe):
    r = subprocess.run([check_exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_dump_equals_the_recorded_images(check_exe):
    with open(os.path.join(HERE, "golden", "batch_stage.json")) as f:
        want = f.read()
    got = subprocess.check_output([check_exe, "--dump"], text=True)
    assert got == want                                            # byte for byte
    cases = [json.loads(line) for line in got.splitlines()]
    with open(os.path.join(HERE, "golden", "plan_cases.json")) as f:
        plans = json.load(f)["cases"]
    # the same table as the plans', refused where they are, sized as they are
    assert [c["name"] for c in cases] == [p["name"] for p in plans]
    for c, p in zip(cases, plans):
        assert (c["rc"], c.get("total", 0)) == (p["rc"], p["total"]), c["name"]
        assert (c.get("whole") is not None) == bool(p.get("whole_wanted")), c["name"]


def test_checks_are_clean_under_address_and_undefined_sanitizers(tmp_path):
    """The same program with its own sanitizer runtime, run stand-alone (no environment, no preload): exit 0, nothing on stderr."""
    exe = build_check("host_batch_check", tmp_path, sanitize=True)
    for args in ([], ["--dump"]):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 0 and r.stderr == "", r.stdout[-2000:] + r.stderr


@pytest.mark.gpu
def test_device_memory_holds_the_staged_images(check_exe, tmp_path, monkeypatch):
    """Three cases of the table on float32 noise just long enough for their requests: what lies in a batch's memory from its
    descriptors on is, byte for byte, the image the host check stages -- after create, after a reset to other requests, and (a plan
    on lanes) in the two regions the first whole-row run uploads the one-sub-batch cut into; that run's results are those of the
    same requests without lanes."""
    import torch
    from sushi_amd import _native
    from sushi_amd.device import DeviceStream, SearchBatch
    with open(os.path.join(HERE, "golden", "plan_cases.json")) as f:
        plans = {p["name"]: p for p in json.load(f)["cases"]}
    with open(os.path.join(HERE, "golden", "batch_stage.json")) as f:
        staged = {c["name"]: c for c in map(json.loads, f)}
    images = tmp_path / "images"
    images.mkdir()
    subprocess.check_call([check_exe, "--image", str(images)])
    rng = np.random.default_rng(20261019)

    def requests(name):
        req = np.fromfile(images / (name + ".req"), _native.REQUEST_DTYPE)
        assert len(req) == plans[name]["n"]
        return req

    def streams(req):
        dst_len = int((req["win_start"] + req["n_pos"] + req["tmpl_len"] - 1).max())
        src_len = int((req["tmpl_off"] + req["tmpl_len"]).max())
        return DeviceStream(rng.random(dst_len, dtype=np.float32)), DeviceStream(rng.random(src_len, dtype=np.float32))

    def batch(D, S, req, name, **kw):
        b = SearchBatch(D, S, req["tmpl_off"], req["tmpl_len"], req["win_start"], req["n_pos"], path="fft", workspace_bytes=plans[name]["cap"], **kw)
        torch.cuda.synchronize()
        return b

    def device_bytes(b, off, nbytes):
        return b._mem[off:off + nbytes].cpu().numpy().tobytes()

    def holds_image(b, name, image):
        return device_bytes(b, plans[name]["layout"]["desc"], len(image)) == image

    def image_of(name):
        with open(images / (name + ".img"), "rb") as f:
            image = f.read()
        assert len(image) == staged[name]["image_bytes"]
        return image

    # one sub-batch; then the same handle for a permutation of its requests
    monkeypatch.delenv("SUSHI_HIP_LANES", raising=False)
    name = "b_four_cap0"
    req = requests(name)
    D, S = streams(req)
    b = batch(D, S, req, name)
    assert b.sub_batches == 1 and holds_image(b, name, image_of(name))
    perm = req[[2, 0, 3, 1]]
    assert b.reset(perm["tmpl_off"], perm["tmpl_len"], perm["win_start"], perm["n_pos"])
    torch.cuda.synchronize()
    perm.tofile(os.path.join(tmp_path, "perm.req"))
    subprocess.check_call([check_exe, "--stage", os.path.join(tmp_path, "perm.req"), str(plans[name]["cap"]), "", os.path.join(tmp_path, "perm.img")])
    with open(os.path.join(tmp_path, "perm.img"), "rb") as f:
        perm_image = f.read()
    assert perm_image != image_of(name) and holds_image(b, name, perm_image)

    # a greedy cut into two, every multiply-accumulate class, patterns beyond 30 segments
    name = "d_mixed_halfway"
    req = requests(name)
    D2, S2 = streams(req)
    b = batch(D2, S2, req, name)
    assert b.sub_batches == 2 and holds_image(b, name, image_of(name))
    del b, D2, S2

    # four parts on two lanes with a pending whole cut: the first run without the exclusion makes and uploads it
    name = "b_four_4x2_cap0"
    req = requests(name)
    monkeypatch.setenv("SUSHI_HIP_LANES", "4:2")
    b = batch(D, S, req, name, exclusion="never")
    assert (b.sub_batches, b.lanes) == (4, 2) and holds_image(b, name, image_of(name))
    b.run()
    idx, score = b.results()
    torch.cuda.synchronize()
    assert holds_image(b, name, image_of(name)[:staged[name]["whole"][0][0]])        # (what lies in front of the whole cut: untouched)
    for k, (off, nbytes, _fnv) in enumerate(staged[name]["whole"]):
        with open(images / ("%s.whole%d" % (name, k)), "rb") as f:
            want = f.read()
        assert len(want) == nbytes and image_of(name)[off:off + nbytes] != want
        assert device_bytes(b, off, nbytes) == want, k
    monkeypatch.setenv("SUSHI_HIP_LANES", "1:1")
    one = batch(D, S, req, "b_four_1x1", exclusion="never")
    assert (one.sub_batches, one.lanes) == (1, 1)
    one.run()
    idx1, score1 = one.results()
    assert (idx == idx1).all() and (score.view(np.uint32) == score1.view(np.uint32)).all()
