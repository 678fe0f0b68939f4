"""Directional gathers and the one-call directional lightmap driven from JavaScript (WebGPURenderer.gatherDirectional /
bakeAtlasDirectionalLightmap of node/index.js): the gather on the points of a small Cornell atlas and the four filtered,
guttered f16 layers hold the words of the Python calls, and the counts agree."""
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
const [uvPath, pointsPath, gatherPath, layersPath, width, height, depth, spp, seed] = process.argv.slice(2);
(async () => {
  const atlasUv = new Float32Array(Uint8Array.from(fs.readFileSync(uvPath)).buffer);
  const points = new Float32Array(Uint8Array.from(fs.readFileSync(pointsPath)).buffer);
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
  const g = r.gatherDirectional(points, +depth, +spp, { seed: +seed, stats: true });
  const opts = { atlasUv, seed: +seed, tMax: 5.0, padBase: 1000, dilate: 3, format: 'f16', stats: true,
    denoise: { planeEps: 0.02, maxDist: 0.5, normalCos: 0.9, passes: 2, step: 1 } };
  const lm = r.bakeAtlasDirectionalLightmap([[0, 0, 0, +width, +height]], +width, +height, +depth, +spp, opts);
  let refused = '';
  try { r.bakeAtlasDirectionalLightmap([[0, 0, 0, +width, +height]], +width, +height, +depth, +spp, { ...opts, format: 'rgbe' }); }
  catch (e) { refused = String(e.message); }
  r.destroy();
  fs.writeFileSync(gatherPath, Buffer.from(g.data.buffer));
  fs.writeFileSync(layersPath, Buffer.from(lm.data.buffer));
  console.log(JSON.stringify({ n: g.n, rays: g.stats.rays, samples: g.stats.samples, width: lm.width, height: lm.height,
    layers: lm.layers, format: lm.format, covered: lm.covered, filled: lm.filled, lmRays: lm.stats.rays,
    kind: lm.data.constructor.name, refused: refused.includes('directional lightmap') }));
})().catch((e) => { console.error(e); process.exit(1); });
"""


@pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")
@pytest.mark.gpu
def test_javascript_directional_calls_have_the_words_of_the_python_calls(W, tmp_path):
    W._build.build_rt()
    assert W._build.build_node_addon()
    width, height, depth, spp = 33, 31, 2, 4
    b = pu.bridge_for(W, "cornell")
    uv = bu.grid_uv(b, 0)
    entries = [(0, 0, 0, width, height)]
    r = W.WebGPURenderer(0)
    try:
        W.upload_scene(r, b, 16, 16)
        points, texels = r.bakeAtlasPoints(entries, width, height, t_max=5.0, pad_base=1000, atlas_uv=uv)
        want_g = r.gatherDirectional(points, depth, spp, bu.SEED)
        want, n, filled, _ = r.bakeAtlasDirectionalLightmap(entries, width, height, depth, spp, bu.SEED, t_max=5.0, pad_base=1000,
                                                            atlas_uv=uv, denoise=dict(du.PARAMS, passes=2, step=1), dilate=3,
                                                            format="f16", stats=True)
    finally:
        r.destroy()
    assert n == len(texels) > 0 and filled > 0 and want.shape == (4, height, width, 4)
    assert (want_g["layer"][:, 1:, :3] != 0).any() and (want[1:, :, :, :3] != 0).any()     # band 1 is there
    paths = [tmp_path / name for name in ("uv.f32", "points.f32", "gather.f32", "layers.f16")]
    uv.tofile(str(paths[0]))
    np.ascontiguousarray(points, np.float32).tofile(str(paths[1]))
    out = subprocess.run([node, "-e", SCRIPT, NODE_DIR] + [str(x) for x in paths] +
                         [str(v) for v in (width, height, depth, spp, bu.SEED)],
                         check=True, capture_output=True, text=True, timeout=300).stdout
    info = json.loads(out.strip().splitlines()[-1])
    assert info == {"n": n, "rays": n, "samples": n * spp, "width": width, "height": height, "layers": 4, "format": "f16",
                    "covered": n, "filled": filled, "lmRays": n, "kind": "Uint16Array", "refused": True}
    got_g = np.fromfile(str(paths[2]), dtype=np.uint32).reshape(n, 16)
    assert np.array_equal(got_g, np.ascontiguousarray(want_g).view(np.uint32).reshape(n, 16))
    got = np.fromfile(str(paths[3]), dtype=np.uint16).reshape(4, height, width, 4)
    assert np.array_equal(got, want.view(np.uint16))
