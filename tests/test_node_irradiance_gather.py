"""node/gather_irradiance.js: irradiance gathers driven from JavaScript (WebGPURenderer.gatherIrradiance of node/index.js)
equal the Python binding's on the same points, and the reference model."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import gather_util as gu
import parity_util as pu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(REPO, "webgpu-raytracer_amd", "node")
node = shutil.which("node")


@pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")
@pytest.mark.gpu
def test_javascript_irradiance_gathers_match_python(W, tmp_path):
    from webgpu_raytracer_amd import renderer as R
    W._build.build_rt()
    assert W._build.build_node_addon()
    b = pu.bridge_for(W, "cornell")
    m = gu.model_for(W, b)
    points = gu.scene_points(m, b)
    r = W.WebGPURenderer(0)
    try:
        W.upload_scene(r, b, 16, 16)
        want, st = r.gatherIrradiance(points, 4, 8, gu.SEED, stats=True)
    finally:
        r.destroy()
    ref, _, counts = m.gatherIrradiance(points, 4, 8, gu.SEED)
    gu.check_against_model(want, ref, "python")
    points_path, out_path = tmp_path / "points.bin", tmp_path / "out.f32"
    points.tofile(str(points_path))
    out = subprocess.run([node, os.path.join(NODE_DIR, "gather_irradiance.js"), "cornell", str(points_path), str(out_path), "4",
                          "8", str(gu.SEED)], check=True, capture_output=True, text=True, timeout=300).stdout
    info = json.loads(out.strip().splitlines()[-1])
    got = np.fromfile(str(out_path), dtype=R.IRRADIANCE_DTYPE)
    assert got.shape[0] == points.shape[0] == info["points"]
    assert np.array_equal(gu.result_words(got), gu.result_words(want))
    for name in ("rays", "samples") + gu.COUNT_NAMES + ("lds",):
        assert info["stats"][name] == st[name], name
    gu.check_counts(info["stats"], counts, points.shape[0], 8, "node")
