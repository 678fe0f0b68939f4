"""node/index.js bakeAtlasIrradiance / bakeAtlasPoints: the small composition case of the atlas-bake tests on cornell, driven
from JavaScript, equals the Python binding's word for word, and node/bake_atlas.js writes its PNG."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import atlas_bake_util as au
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
  const entries = %s;
  const raw = fs.readFileSync(process.argv[2]);
  const atlasUv = new Float32Array(raw.buffer, raw.byteOffset, raw.byteLength / 4);
  const opts = { atlasUv, tMax: 5, padBase: 1000 };
  const bake = r.bakeAtlasIrradiance(entries, %d, %d, 4, 8, Object.assign({ seed: 5, stats: true }, opts));
  const pts = r.bakeAtlasPoints(entries, %d, %d, Object.assign({ owner: true }, opts));
  fs.writeFileSync(process.argv[3], Buffer.from(bake.data.buffer));
  fs.writeFileSync(process.argv[4], Buffer.from(pts.points.buffer, pts.points.byteOffset, pts.points.byteLength));
  fs.writeFileSync(process.argv[5], Buffer.from(pts.owner.buffer));
  console.log(JSON.stringify({ covered: bake.covered, n: pts.n, stats: bake.stats, texels: Array.from(pts.texels) }));
  r.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
"""


@pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")
@pytest.mark.gpu
def test_javascript_atlas_bake_matches_python(W, tmp_path):
    from webgpu_raytracer_amd import renderer as R
    W._build.build_rt()
    assert W._build.build_node_addon()
    b = pu.bridge_for(W, "cornell")
    entries = au.small_entries(au.instance_count(b))
    uv = au.merged_grid_uv(b, [e[0] for e in entries])
    width, height = au.SMALL_W, au.SMALL_H
    r = W.WebGPURenderer(0)
    try:
        W.upload_scene(r, b, 16, 16)
        want, n, st = r.bakeAtlasIrradiance(entries, width, height, 4, 8, 5, t_max=5.0, pad_base=1000, atlas_uv=uv, stats=True)
        points, texels, owner = r.bakeAtlasPoints(entries, width, height, t_max=5.0, pad_base=1000, atlas_uv=uv, owner=True)
    finally:
        r.destroy()
    script, uv_path = tmp_path / "bake.js", tmp_path / "uv.f32"
    atlas_path, points_path, owner_path = tmp_path / "atlas.f32", tmp_path / "points.bin", tmp_path / "owner.i32"
    uv.astype(np.float32).tofile(str(uv_path))
    script.write_text(SCRIPT % (os.path.join(NODE_DIR, "index.js"), json.dumps([list(map(int, e)) for e in entries]), width, height,
                                width, height))
    out = subprocess.run([node, str(script), str(uv_path), str(atlas_path), str(points_path), str(owner_path)], check=True,
                         capture_output=True, text=True, timeout=300).stdout
    info = json.loads(out.strip().splitlines()[-1])
    got = np.fromfile(str(atlas_path), dtype=R.IRRADIANCE_DTYPE).reshape(height, width)
    assert info["covered"] == n == info["n"] and n > 0.1 * width * height
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(np.fromfile(str(points_path), dtype=np.uint32), points.view(np.uint32).ravel())
    assert np.array_equal(np.fromfile(str(owner_path), dtype=np.int32), owner.ravel())
    assert info["texels"] == texels.tolist()
    for name in ("rays", "samples", "extension_rays", "shadow_rays", "shaded_hits", "nodes_visited", "tris_tested", "lds"):
        assert info["stats"][name] == st[name], name
    # the example: sixteen instances of instanced1000 on a 4 x 4 grid of 16 x 16 rectangles, written through the addon's writer
    png = tmp_path / "atlas.png"
    out = subprocess.run([node, os.path.join(NODE_DIR, "bake_atlas.js"), "instanced1000", "16", "16", str(png), "4", "8"],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    info = json.loads(out.strip().splitlines()[-1])
    assert info["entries"] == 16 and info["size"] == 64 and info["geometries"] == 4
    assert info["covered"] > 0.1 * 64 * 64 and info["lit"] > 0
    assert png.read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
