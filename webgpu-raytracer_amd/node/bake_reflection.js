'use strict';
// Headless reflection-probe bake against a built-in scene (WebGPURenderer.bakeReflection / encodeReflection):
// usage: node bake_reflection.js <scene> <outPrefix> [size] [levels] [spt] [filterSamples] [maxDepth] [seed] [x y z]
//   the probe sits at (x, y, z), by default the middle of the scene's bounds (the TLAS root's box)
//   <outPrefix>_<m>.hdr   written per level m: a flat Radiance picture of (size >> m)^2 shared-exponent texels in octahedral
//                         layout, row 0 first; level m is filtered with the GGX lobe of the roughness m / (levels - 1)
//   <outPrefix>.json      written: the descriptor, the probe and the bake's stats
// prints one JSON line with the level sizes and the bake's stats
const fs = require('fs');
const { WebGPURenderer, WorldBridge } = require('./index.js');

(async () => {
  const [scene = 'cornell', prefix, size = '64', levels = '5', spt = '64', filterSamples = '256', depth = '4', seed = '0', px, py, pz] = process.argv.slice(2);
  if (!prefix) throw new Error('usage: node bake_reflection.js <scene> <outPrefix> [size] [levels] [spt] [filterSamples] [maxDepth] [seed] [x y z]');
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
  const root = new Float32Array(bridge.tlas.buffer, bridge.tlas.byteOffset, 8);   // {min, skip, max, data} of node 0
  const position = pz === undefined ? [0, 1, 2].map((a) => 0.5 * (root[a] + root[4 + a])) : [px, py, pz].map(parseFloat);
  const d = { size: parseInt(size, 10), levels: parseInt(levels, 10), spt: parseInt(spt, 10), filterSamples: parseInt(filterSamples, 10) };
  const desc = WebGPURenderer.reflectionDesc(d);
  const probe = new Float32Array(8);
  probe.set(position);
  probe[3] = 1e30;                                                         // tMax; pad stays 0
  const baked = renderer.bakeReflection(desc, probe, parseInt(depth, 10), { seed: parseInt(seed, 10), stats: true });
  const encoded = renderer.encodeReflection(desc, baked.data, 'rgbe');
  const sides = [];
  encoded.forEach((level, m) => {
    const texels = Buffer.from(level.data.buffer, level.data.byteOffset, level.data.byteLength);
    fs.writeFileSync(`${prefix}_${m}.hdr`, Buffer.concat([Buffer.from(`#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y ${level.height} +X ${level.width}\n`, 'latin1'), texels]));
    sides.push(level.width);
  });
  fs.writeFileSync(`${prefix}.json`, JSON.stringify(Object.assign({ scene, format: 'rgbe', position, maxDepth: parseInt(depth, 10),
    seed: parseInt(seed, 10), sides }, d, { stats: baked.stats })));
  console.log(JSON.stringify({ scene, sides, stats: baked.stats }));
  renderer.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
