'use strict';
// Headless probe gathers against a built-in scene (WebGPURenderer.gatherProbes):
// usage: node gather_probes.js <scene> <probes.bin> <out.f32> [maxDepth] [spp] [seed]
//   probes.bin raw little-endian, 8 words per probe {position, tMax, 3 unused words (float32), pad (uint32: the RNG stream id)}
//   out.f32    written: 112 bytes per probe {sh[9][3], hitFraction} (float32): the SH9 radiance coefficients
// prints one JSON line with the probe count and the gather's stats
const fs = require('fs');
const { WebGPURenderer, WorldBridge } = require('./index.js');

(async () => {
  const [scene = 'cornell', probesPath, outPath, depth = '4', spp = '1', seed = '0'] = process.argv.slice(2);
  if (!probesPath || !outPath) throw new Error('usage: node gather_probes.js <scene> <probes.bin> <out.f32> [maxDepth] [spp] [seed]');
  const raw = fs.readFileSync(probesPath);
  const probes = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length));
  const bridge = new WorldBridge();
  await bridge.initWasm();
  await bridge.loadScene(scene);
  const renderer = new WebGPURenderer(0);
  await renderer.init();
  await renderer.loadTexturesFromWorld(bridge);
  renderer.updateCombinedGeometry(bridge.vertices, bridge.normals, bridge.uvs);
  renderer.updateCombinedBVH(bridge.tlas, bridge.blas);
  renderer.updateBuffer('topology', bridge.mesh_topology);
  renderer.updateBuffer('instance', bridge.instances);
  renderer.updateBuffer('lights', bridge.lights);
  bridge.updateCamera(16, 16);
  renderer.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount);   // the light count of the shading
  const out = renderer.gatherProbes(probes, parseInt(depth, 10), parseInt(spp, 10), { seed: parseInt(seed, 10), stats: true });
  fs.writeFileSync(outPath, Buffer.from(out.data.buffer));
  console.log(JSON.stringify({ scene, probes: out.n, stats: out.stats }));
  renderer.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
