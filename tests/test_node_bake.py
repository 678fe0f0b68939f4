"""node/index.js bakeIrradiance / bakePoints: a lightmap bake driven from JavaScript equals the Python binding's on the same
scene, word for word, and node/bake_lightmap.js writes its PNG."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import parity_util as pu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(REPO, "webgpu-raytracer_amd", "node")
node = shutil.which("node")

SCRIPT = """
const fs = require('fs');
const { WebGPURenderer, WorldBridge } = require(%r);
(async () => {
  const bridge = new WorldBridge();
  await bridge.initWasm();
  await bridge.loadScene('cornell');
  const r = new WebGPURenderer(0);
  await r.init();
  await r.loadTexturesFromWorld(bridge);
  r.updateCombinedGeometry(bridge.vertices, bridge.normals, bridge.uvs);
  r.updateCombinedBVH(bridge.tlas, bridge.blas);
  r.updateBuffer('topology', bridge.mesh_topology);
  r.updateBuffer('instance', bridge.instances);
  r.updateBuffer('lights', bridge.lights);
  r.updateBuffer('draw_commands', bridge.draw_commands);
  bridge.updateCamera(16, 16);
  r.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount);
  const bake = r.bakeIrradiance(0, 32, 32, 4, 8, { seed: 5, stats: true });
  const pts = r.bakePoints(0, 32, 32, { owner: true });
  fs.writeFileSync(process.argv[2], Buffer.from(bake.data.buffer));
  fs.writeFileSync(process.argv[3], Buffer.from(pts.points.buffer, pts.points.byteOffset, pts.points.byteLength));
  console.log(JSON.stringify({ covered: bake.covered, n: pts.n, stats: bake.stats }));
  r.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
"""


@pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")
@pytest.mark.gpu
def test_javascript_bake_matches_python(W, tmp_path):
    import json
    from webgpu_raytracer_amd import renderer as R
    W._build.build_rt()
    assert W._build.build_node_addon()
    b = pu.bridge_for(W, "cornell")
    r = W.WebGPURenderer(0)
    try:
        W.upload_scene(r, b, 16, 16)
        want, n, st = r.bakeIrradiance(0, 32, 32, 4, 8, 5, stats=True)
        points, texels = r.bakePoints(0, 32, 32)
    finally:
        r.destroy()
    script, atlas_path, points_path = tmp_path / "bake.js", tmp_path / "atlas.f32", tmp_path / "points.bin"
    script.write_text(SCRIPT % os.path.join(NODE_DIR, "index.js"))
    out = subprocess.run([node, str(script), str(atlas_path), str(points_path)], check=True, capture_output=True, text=True,
                         timeout=300).stdout
    info = json.loads(out.strip().splitlines()[-1])
    got = np.fromfile(str(atlas_path), dtype=R.IRRADIANCE_DTYPE).reshape(32, 32)
    assert info["covered"] == n == info["n"] and n > 100
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.fromfile(str(points_path), dtype=np.uint32), points.view(np.uint32).ravel())
    for name in ("rays", "samples", "extension_rays", "shadow_rays", "shaded_hits", "nodes_visited", "tris_tested", "lds"):
        assert info["stats"][name] == st[name], name
    # the example: bakes and writes a PNG through the addon's writer
    png = tmp_path / "bake.png"
    out = subprocess.run([node, os.path.join(NODE_DIR, "bake_lightmap.js"), "32", str(png), "4", "8"], check=True,
                         capture_output=True, text=True, timeout=300).stdout
    info = json.loads(out.strip().splitlines()[-1])
    assert info["floorTriangles"] == 2 and info["covered"] == 32 * 32      # the floor quad fills its chart
    assert info["lit"] > 512                                               # ... and is lit from above, not gathered from below
    assert png.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
