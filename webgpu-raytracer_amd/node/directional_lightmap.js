'use strict';
// Bake the finished DIRECTIONAL lightmap of the first N instances of a scene in ONE call: four layers of spherical-harmonic
// radiance coefficients (bands 0 .. 1, world space) per texel, for renderers that light normal-mapped surfaces from a lightmap.
// usage: node directional_lightmap.js [scene] [N] [cell] [maxDepth] [spp] [seed] [--format f16|f32] [--out FILE]
//        [--denoise PASSES --plane-eps E --max-dist D [--normal-cos C]] [--dilate R]
// defaults: instanced1000, 64, 32, 4, 16, 0, f16, directional.f16 / directional.f32, no filter, no gutter
// The atlas and the chart layout are those of lightmap.js.  bakeAtlasDirectionalLightmap runs the point pass, the directional
// gather, the scatter and then, per layer, the filter, the gutter fill and the encode back to back on the device; what comes
// back is the four encoded layers, once.  The file holds them layer-major as raw little-endian texels {sh[k].r, sh[k].g,
// sh[k].b, w}, row 0 first: layer 0 is Y0, layers 1 .. 3 the y, z and x harmonics of band 1; w >= 0 = covered, -2 = gutter, -1 =
// no surface.  The irradiance at a unit normal n is pi * 0.282094792 * c0 + (2 pi / 3) * 0.488602512 * (c1 n.y + c2 n.z + c3
// n.x).  'rgbe' is refused: band-1 coefficients are signed.  Prints one JSON line.
const fs = require('fs');
const { WebGPURenderer, WorldBridge } = require('./index.js');

(async () => {
  const argv = process.argv.slice(2);
  const flag = (name, parse, none) => {
    const at = argv.indexOf(name);
    return at >= 0 ? parse(argv.splice(at, 2)[1]) : none;
  };
  const format = flag('--format', String, 'f16');
  const dilate = flag('--dilate', (v) => parseInt(v, 10), 0);
  const passes = flag('--denoise', (v) => parseInt(v, 10), 0);
  const planeEps = flag('--plane-eps', parseFloat), maxDist = flag('--max-dist', parseFloat);
  const normalCos = flag('--normal-cos', parseFloat, 0.9);
  if (passes > 0 && (planeEps === undefined || maxDist === undefined)) throw new Error('--denoise needs --plane-eps E and --max-dist D');
  const outPath = flag('--out', String, 'directional.' + format);
  const [scene = 'instanced1000', count = '64', cellSize = '32', depth = '4', spp = '16', seed = '0'] = argv;
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
  renderer.updateBuffer('draw_commands', bridge.draw_commands);   // the bake takes each instance's triangle range from these
  bridge.updateCamera(16, 16);
  renderer.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount);
  const draw = bridge.draw_commands, topo = bridge.mesh_topology;
  const nInst = draw.length / 4, nVerts = bridge.uvs.length / 2, nTris = topo.length / 20;
  const n = Math.min(parseInt(count, 10), nInst), cell = parseInt(cellSize, 10);
  const side = Math.ceil(Math.sqrt(n));
  const entries = [], geometries = new Set();
  const atlasUv = new Float32Array(nVerts * 2).fill(-1);
  const corner = [[0.11, 0.13], [0.89, 0.12], [0.12, 0.87]];
  for (let e = 0; e < n; e++) {
    entries.push([e, (e % side) * cell, Math.floor(e / side) * cell, cell, cell]);
    const first = Math.floor(draw[4 * e + 2] / 3), tris = Math.floor(draw[4 * e] / 3);
    if (geometries.has(first)) continue;
    geometries.add(first);
    const g = Math.max(1, Math.ceil(Math.sqrt(tris)));
    for (let j = 0; j < tris && first + j < nTris; j++)
      for (let c = 0; c < 3; c++) {
        const v = topo[20 * (first + j) + c];
        atlasUv[2 * v] = (j % g + corner[c][0]) / g;
        atlasUv[2 * v + 1] = (Math.floor(j / g) + corner[c][1]) / g;
      }
  }
  const size = side * cell;
  const t0 = process.hrtime.bigint();
  const bake = renderer.bakeAtlasDirectionalLightmap(entries, size, size, parseInt(depth, 10), parseInt(spp, 10), {
    atlasUv, seed: parseInt(seed, 10), stats: true, format, dilate,
    denoise: passes > 0 ? { passes, planeEps, maxDist, normalCos } : null });
  const ms = Number(process.hrtime.bigint() - t0) / 1e6;
  const texels = Buffer.from(bake.data.buffer, bake.data.byteOffset, bake.data.byteLength);
  fs.writeFileSync(outPath, texels);
  console.log(JSON.stringify({ scene, entries: n, geometries: geometries.size, size, layers: bake.layers, format: bake.format, bytes: texels.length,
    covered: bake.covered, ms, out: outPath, ...(passes > 0 ? { denoise: passes, planeEps, maxDist, normalCos } : {}),
    ...(dilate > 0 ? { dilate, filled: bake.filled } : {}), stats: bake.stats }));
  renderer.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
