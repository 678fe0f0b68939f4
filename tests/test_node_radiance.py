"""node/trace_radiance.js: radiance queries driven from JavaScript (WebGPURenderer.traceRadiance of node/index.js) equal the
Python binding's on the same rays, and the reference model."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import parity_util as pu
import radiance_util as ru
import ray_query_util as rq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(REPO, "webgpu-raytracer_amd", "node")
node = shutil.which("node")


@pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")
@pytest.mark.gpu
def test_javascript_radiance_queries_match_python(W, tmp_path):
    from webgpu_raytracer_amd import renderer as R
    W._build.build_rt()
    assert W._build.build_node_addon()
    b = pu.bridge_for(W, "cornell")
    rays = ru.with_pads(rq.to_rt_rays(rq.scene_rays(b, False, 2500, 1500)))
    r = W.WebGPURenderer(0)
    try:
        W.upload_scene(r, b, 16, 16)
        want, st = r.traceRadiance(rays, 4, 2, ru.SEED, stats=True)
    finally:
        r.destroy()
    ref, counts = ru.model_for(W, b).traceRadiance(rays, 4, 2, ru.SEED)
    ru.check_against_model(want, ref, "python")
    rays_path, out_path = tmp_path / "rays.bin", tmp_path / "out.f32"
    rays.tofile(str(rays_path))
    out = subprocess.run([node, os.path.join(NODE_DIR, "trace_radiance.js"), "cornell", str(rays_path), str(out_path), "4", "2",
                          str(ru.SEED)], check=True, capture_output=True, text=True, timeout=300).stdout
    info = json.loads(out.strip().splitlines()[-1])
    got = np.fromfile(str(out_path), dtype=R.RADIANCE_DTYPE)
    assert got.shape[0] == rays.shape[0] == info["rays"]
    assert np.array_equal(ru.result_words(got), ru.result_words(want))
    for name in ("rays", "samples") + ru.COUNT_NAMES + ("lds",):
        assert info["stats"][name] == st[name], name
    ru.check_counts(info["stats"], counts, rays.shape[0], 2, "node")
