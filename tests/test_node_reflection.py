"""Reflection probes driven from JavaScript (WebGPURenderer.bakeReflection / filterReflection / encodeReflection of
node/index.js) equal the Python binding's words on one small case, and node/bake_reflection.js writes, level by level, the
Radiance pictures Python's encodeReflection gives for the descriptor and probe it reports."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import parity_util as pu
import probe_util as prb
import reflection_util as rf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE_DIR = os.path.join(REPO, "webgpu-raytracer_amd", "node")
node = shutil.which("node")
needs_node = pytest.mark.skipif(node is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / node_api.h not present")

JS = """
const fs = require('fs');
const { WebGPURenderer, WorldBridge } = require(process.argv[1] + '/index.js');
const f32 = (p) => { const b = fs.readFileSync(p); return new Float32Array(b.buffer.slice(b.byteOffset, b.byteOffset + b.length)); };
(async () => {
  const [dir, probesPath, bakePath, filterPath, encPath] = process.argv.slice(1);
  const bridge = new WorldBridge();
  await bridge.initWasm();
  await bridge.loadScene('cornell');
  const renderer = new WebGPURenderer(0);
  await renderer.init();
  await renderer.loadTexturesFromWorld(bridge);
  renderer.updateCombinedGeometry(bridge.vertices, bridge.normals, bridge.uvs);
  renderer.updateCombinedBVH(bridge.tlas, bridge.blas);
  renderer.updateBuffer('topology', bridge.mesh_topology);
  renderer.updateBuffer('instance', bridge.instances);
  renderer.updateBuffer('lights', bridge.lights);
  bridge.updateCamera(16, 16);
  renderer.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount);
  const desc = WebGPURenderer.reflectionDesc({ size: 16, levels: 3, spt: 3, filterSamples: 128 });
  const bake = renderer.bakeReflection(desc, f32(probesPath), 4, { seed: 5, stats: true });
  const maps = new Float32Array(bake.n * 256 * 4);
  for (let p = 0; p < bake.n; p++) maps.set(bake.data.subarray(p * bake.chainTexels * 4, p * bake.chainTexels * 4 + 1024), p * 1024);
  const again = renderer.filterReflection(desc, maps);
  const enc = renderer.encodeReflection(desc, bake.data.slice(0, bake.chainTexels * 4), 'rgbe');
  fs.writeFileSync(bakePath, Buffer.from(bake.data.buffer));
  fs.writeFileSync(filterPath, Buffer.from(again.data.buffer));
  fs.writeFileSync(encPath, Buffer.concat(enc.map((l) => Buffer.from(l.data.buffer))));
  console.log(JSON.stringify({ n: bake.n, chainTexels: bake.chainTexels, offsets: bake.offsets, stats: bake.stats, made: Array.from(desc),
    sides: enc.map((l) => l.width) }));
  renderer.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
"""


@needs_node
def test_node_addon_exports_the_bindings(W):
    W._build.build_scene()
    W._build.build_tex()
    W._build.build_rt()
    path = W._build.build_node_addon(force=True)
    assert path and os.path.exists(path)
    node_dir = os.path.dirname(path)
    js = ("const m=require('%s/index.js');const P=m.WebGPURenderer.prototype;console.log(typeof m.native.rtBakeReflection,"
          "typeof m.native.rtFilterReflection,typeof m.WebGPURenderer.reflectionDesc,typeof P.bakeReflection,"
          "typeof P.filterReflection,typeof P.encodeReflection)" % node_dir)
    out = subprocess.run([node, "-e", js], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split() == ["function"] * 6
    assert os.path.exists(os.path.join(node_dir, "bake_reflection.js"))
    dts = open(os.path.join(node_dir, "index.d.ts")).read()
    for m in ("reflectionDesc(", "bakeReflection(", "filterReflection(", "encodeReflection("):
        assert m in dts, m


@needs_node
@pytest.mark.gpu
def test_javascript_reflection_probes_match_python(W, tmp_path):
    from webgpu_raytracer_amd import renderer as R
    W._build.build_rt()
    assert W._build.build_node_addon()
    b = pu.bridge_for(W, "cornell")
    lo, hi = prb.scene_bounds(b)
    probes = prb.make_probes(np.stack([0.5 * (lo + hi), lo + 0.25 * (hi - lo)]), pad_first=17)
    d = R.reflection_desc(16, 3, 3, 128)
    r = W.WebGPURenderer(0)
    try:
        W.upload_scene(r, b, 16, 16)
        bake, st = r.bakeReflection(d, probes, 4, 5, stats=True)
        assert (bake[..., :3] > 0).mean() > 0.25 and (bake[..., 3] > 0).mean() > 0.5
        paths = [str(tmp_path / n) for n in ("probes.f32", "bake.f32", "filter.f32", "enc.u32")]
        probes.tofile(paths[0])
        out = subprocess.run([node, "-e", JS, NODE_DIR] + paths, check=True, capture_output=True, text=True, timeout=300).stdout
        info = json.loads(out.strip().splitlines()[-1])
        assert info["n"] == 2 and info["chainTexels"] == 336 and info["offsets"] == [0, 256, 320, 336] and info["sides"] == [16, 8, 4]
        assert bytes(info["made"]) == d.tobytes()
        assert np.array_equal(np.fromfile(paths[1], np.uint32), bake.view(np.uint32).reshape(-1))
        assert np.array_equal(np.fromfile(paths[2], np.uint32), bake.view(np.uint32).reshape(-1))     # the filter of its level 0
        want = np.concatenate([l.reshape(-1) for l in r.encodeReflection(d, bake[0], "rgbe")])
        assert np.array_equal(np.fromfile(paths[3], np.uint32), want)
        for name in ("rays", "samples") + prb.COUNT_NAMES + ("lds",):
            assert info["stats"][name] == st[name], name
        # the tool: one probe in the middle of the scene, a Radiance picture per level and a JSON descriptor
        prefix = str(tmp_path / "probe")
        subprocess.run([node, os.path.join(NODE_DIR, "bake_reflection.js"), "cornell", prefix, "8", "2", "2", "64", "1", "4"],
                       check=True, capture_output=True, text=True, timeout=300)
        j = json.load(open(prefix + ".json"))
        assert j["sides"] == [8, 4] and j["stats"]["samples"] == 64 * 2
        dj = R.reflection_desc(j["size"], j["levels"], j["spt"], j["filterSamples"])
        probe = prb.make_probes(np.array([j["position"]], np.float32), pad_first=0)
        py = r.encodeReflection(dj, r.bakeReflection(dj, probe, j["maxDepth"], j["seed"])[0], "rgbe")
        for m, level in enumerate(py):
            blob = open("%s_%d.hdr" % (prefix, m), "rb").read()
            head = ("#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (8 >> m, 8 >> m)).encode("latin1")
            assert blob.startswith(head) and blob[len(head):] == level.tobytes(), m
    finally:
        r.destroy()
