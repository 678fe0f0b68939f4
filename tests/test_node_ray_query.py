"""node/trace_rays.js: ray queries driven from JavaScript (WebGPURenderer.traceRays of node/index.js) equal the oracle."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import parity_util as pu
import ray_query_util as rq

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(REPO, "webgpu-raytracer_amd", "node")
node = shutil.which("node")


@pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")
@pytest.mark.gpu
@pytest.mark.parametrize("shadow", [False, True])
def test_javascript_ray_queries_match_the_oracle(W, oracle_lib, tmp_path, shadow):
    from webgpu_raytracer_amd import renderer as R
    W._build.build_rt()
    assert W._build.build_node_addon()
    b = pu.bridge_for(W, "cornell")
    cpu = rq.oracle_for(W, oracle_lib, b)
    rays = rq.scene_rays(b, shadow, 3000, 1000)
    ref, counts = cpu.traceRays(rays, any_hit=shadow)
    rays_path, hits_path = tmp_path / "rays.f32", tmp_path / "hits.bin"
    rq.to_rt_rays(rays).tofile(str(rays_path))
    out = subprocess.run([node, os.path.join(NODE_DIR, "trace_rays.js"), "cornell", str(rays_path), str(hits_path),
                          "1" if shadow else "0", repr(rq.T_MIN)], check=True, capture_output=True, text=True, timeout=300).stdout
    info = json.loads(out.strip().splitlines()[-1])
    hits = np.fromfile(str(hits_path), dtype=R.RAY_HIT_DTYPE)
    assert hits.shape[0] == rays.shape[0] == info["rays"]
    if shadow:
        rq.check_any(hits, ref, "node any")
    else:
        rq.check_closest(hits, rays, ref, "node closest")
    assert info["stats"]["rays"] == rays.shape[0]
    assert info["stats"]["nodes_visited"] == int(counts[:, 0].sum()) and info["stats"]["tris_tested"] == int(counts[:, 1].sum())
