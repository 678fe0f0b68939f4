"""The one-call lightmap driven from JavaScript (WebGPURenderer.bakeAtlasLightmap / encodeAtlas of node/index.js): one small
Cornell atlas, filtered, guttered and encoded as RGBE8 through the addon, holds the words of the Python call; its f32 form
encoded by the addon's encodeAtlas gives the same words again, and the counts agree."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import bake_util as bu
import denoise_util as du
import parity_util as pu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(REPO, "webgpu-raytracer_amd", "node")
node = shutil.which("node")

SCRIPT = """
const fs = require('fs');
const { WebGPURenderer, WorldBridge } = require(process.argv[1] + '/index.js');
const [uvPath, rgbePath, againPath, width, height, depth, spp, seed] = process.argv.slice(2);
(async () => {
  const b = fs.readFileSync(uvPath);
  const atlasUv = new Float32Array(Uint8Array.from(b).buffer);
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
  const opts = { atlasUv, seed: +seed, tMax: 5.0, padBase: 1000, dilate: 3,
    denoise: { planeEps: 0.02, maxDist: 0.5, normalCos: 0.9, passes: 2, step: 1 } };
  const entries = [[0, 0, 0, +width, +height]];
  const rgbe = r.bakeAtlasLightmap(entries, +width, +height, +depth, +spp, { ...opts, format: 'rgbe', stats: true });
  const f32 = r.bakeAtlasLightmap(entries, +width, +height, +depth, +spp, { ...opts, format: 'f32' });
  const again = r.encodeAtlas(f32.data, +width, +height, 'rgbe');
  r.destroy();
  fs.writeFileSync(rgbePath, Buffer.from(rgbe.data.buffer));
  fs.writeFileSync(againPath, Buffer.from(again.data.buffer));
  console.log(JSON.stringify({ width: rgbe.width, height: rgbe.height, format: rgbe.format, covered: rgbe.covered,
    filled: rgbe.filled, rays: rgbe.stats.rays, f32Covered: f32.covered, f32Filled: f32.filled, kind: again.data.constructor.name }));
})().catch((e) => { console.error(e); process.exit(1); });
"""


@pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")
@pytest.mark.gpu
def test_javascript_lightmap_has_the_words_of_the_python_call(W, tmp_path):
    W._build.build_rt()
    assert W._build.build_node_addon()
    width, height, depth, spp = 33, 31, 2, 4
    b = pu.bridge_for(W, "cornell")
    uv = bu.grid_uv(b, 0)
    r = W.WebGPURenderer(0)
    try:
        W.upload_scene(r, b, 16, 16)
        want, n, filled, _ = r.bakeAtlasLightmap([(0, 0, 0, width, height)], width, height, depth, spp, bu.SEED, t_max=5.0,
                                                 pad_base=1000, atlas_uv=uv, denoise=dict(du.PARAMS, passes=2, step=1), dilate=3,
                                                 format="rgbe", stats=True)
    finally:
        r.destroy()
    assert n > 0 and filled > 0 and (want != 0).sum() > 50
    paths = [tmp_path / name for name in ("uv.f32", "rgbe.u32", "again.u32")]
    uv.tofile(str(paths[0]))
    out = subprocess.run([node, "-e", SCRIPT, NODE_DIR] + [str(x) for x in paths] +
                         [str(v) for v in (width, height, depth, spp, bu.SEED)],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    info = json.loads(out.strip().splitlines()[-1])
    assert info == {"width": width, "height": height, "format": "rgbe", "covered": n, "filled": filled, "rays": n,
                    "f32Covered": n, "f32Filled": filled, "kind": "Uint32Array"}
    for path in paths[1:]:
        got = np.fromfile(str(path), dtype=np.uint32).reshape(height, width)
        assert np.array_equal(got, want), path
