'use strict';
// Headless irradiance-volume bake against a built-in scene (WebGPURenderer.bakeVolume / encodeVolume):
// usage: node bake_volume.js <scene> <out.f16> <out.json> [nx] [ny] [nz] [maxDepth] [spp] [seed] [windowWidth]
//        [--visibility SIZE --spt N]
//   the grid spans the scene's bounds (the TLAS root's box), its outer probes half a cell inside them
//   out.f16    written: seven layers of nx * ny * nz texels of four half floats, layer j holding the floats 4 j .. 4 j + 3 of
//              every probe's record {sh'[9][3], hitFraction}: irradiance coefficients, ready for a 3D-texture upload
//   out.json   written: the descriptor {origin, step, dims, window, tMax, padFirst, maxHitFraction} and the bake's stats
//   windowWidth  of the Hanning window against ringing, (1 + cos(pi l / w)) / 2 per band l; 0 (the default) = none
//   --visibility SIZE  also bakes the probes' visibility maps (WebGPURenderer.bakeVolumeVisibility) of SIZE x SIZE texels at
//              --spt N samples per texel (64), rays as long as a cell's diagonal, and writes them beside out.f16 as
//              <out.f16>.visibility: one image of bordered tiles of two half floats per texel {mean distance, mean squared
//              distance}, probe (x, y, z) at tile (x, z * ny + y); out.json then carries the descriptor under "visibility"
// prints one JSON line with the probe count and the bake's stats
const fs = require('fs');
const { WebGPURenderer, WorldBridge } = require('./index.js');

(async () => {
  const argv = process.argv.slice(2), flags = {};
  for (const name of ['--visibility', '--spt']) {
    const at = argv.indexOf(name);
    if (at >= 0) flags[name] = parseInt(argv.splice(at, 2)[1], 10);
  }
  const [scene = 'cornell', outPath, jsonPath, nx = '8', ny = '8', nz = '8', depth = '4', spp = '256', seed = '0', width = '0'] = argv;
  if (!outPath || !jsonPath) throw new Error('usage: node bake_volume.js <scene> <out.f16> <out.json> [nx] [ny] [nz] [maxDepth] [spp] [seed] [windowWidth]');
  const dims = [nx, ny, nz].map((v) => parseInt(v, 10));
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
  const step = [0, 1, 2].map((a) => (root[4 + a] - root[a]) / dims[a]);
  const origin = [0, 1, 2].map((a) => root[a] + 0.5 * step[a]);
  const w = parseFloat(width);
  const window = w > 0 ? [0, 1, 2].map((l) => (1 + Math.cos(Math.PI * l / w)) / 2) : [1, 1, 1];
  const d = { origin, step, dims, window, tMax: 1e30, padFirst: 0, maxHitFraction: 1 };
  const desc = WebGPURenderer.volumeDesc(d);
  const baked = renderer.bakeVolume(desc, parseInt(depth, 10), parseInt(spp, 10), { seed: parseInt(seed, 10), stats: true });
  const layers = renderer.encodeVolume(desc, baked.data, 'f16');
  fs.writeFileSync(outPath, Buffer.from(layers.data.buffer));
  let visibility;
  if (flags['--visibility']) {
    visibility = { size: flags['--visibility'], spt: flags['--spt'] || 64, maxDistance: Math.hypot(step[0], step[1], step[2]) };
    const vis = WebGPURenderer.volumeVisibilityDesc(visibility);
    const maps = renderer.bakeVolumeVisibility(desc, vis, { seed: parseInt(seed, 10), stats: true });
    const tiles = renderer.encodeVolumeVisibility(desc, vis, maps.data, 'f16');
    fs.writeFileSync(outPath + '.visibility', Buffer.from(tiles.data.buffer));
    Object.assign(visibility, { format: 'f16', width: tiles.width, height: tiles.height, tile: tiles.tile, stats: maps.stats });
  }
  fs.writeFileSync(jsonPath, JSON.stringify(Object.assign({ scene, format: 'f16', layers: 7 }, d, { stats: baked.stats }, visibility ? { visibility } : {})));
  console.log(JSON.stringify({ scene, probes: baked.n, stats: baked.stats }));
  renderer.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
