'use strict';
// Bake the lightmap of the first N instances of a scene into ONE atlas and write it as a PNG:
// usage: node bake_atlas.js [scene] [N] [cell] [out.png] [maxDepth] [spp] [seed] [--denoise PASSES --plane-eps E --max-dist D
//        [--normal-cos C]] [--dilate R]
// defaults: instanced1000, 64, 32, atlas.png, 4, 16, 0, no denoising, no dilation
// The atlas is a square grid of ceil(sqrt(N)) x ceil(sqrt(N)) rectangles of cell x cell texels, instance e in rectangle e.
// Instances of one geometry share their vertices and so their chart: the rectangle is what tells their texels apart.  The
// chart itself is an override layout made here - triangle k of a geometry gets cell k of a ceil(sqrt(n)) grid of the unit
// square, as the triangle (0.11, 0.13) (0.89, 0.12) (0.12, 0.87) of its cell - one layout per distinct geometry, merged into
// one array (for meshes whose triangles share no vertices across geometries).  One bakeAtlasIrradiance call bakes them all:
// one point pass, one gather, one scatter.  The picture shows pi * (E / pi) * albedo with albedo = 0.8 and gamma 2.2; texels
// without a surface are transparent.  --dilate R (1 .. 24) puts a gutter of R texels of copied colour around every chart
// (dilateAtlas); its texels are drawn like covered ones.  --denoise PASSES (1 .. 3) filters the atlas before that (denoiseAtlas,
// guided by one more point pass, bakeAtlasPoints: taps count within E of a texel's tangent plane and within D of it, world
// units, where the normals' dot product is at least C, default 0.9).  Prints one JSON line.
const fs = require('fs');
const { WebGPURenderer, WorldBridge, encodePng } = require('./index.js');

(async () => {
  const argv = process.argv.slice(2);
  const flag = (name, parse, none) => {
    const at = argv.indexOf(name);
    return at >= 0 ? parse(argv.splice(at, 2)[1]) : none;
  };
  const dilate = flag('--dilate', (v) => parseInt(v, 10), 0);
  const denoise = flag('--denoise', (v) => parseInt(v, 10), 0);
  const planeEps = flag('--plane-eps', parseFloat), maxDist = flag('--max-dist', parseFloat);
  const normalCos = flag('--normal-cos', parseFloat, 0.9);
  if (denoise > 0 && (planeEps === undefined || maxDist === undefined)) throw new Error('--denoise needs --plane-eps E and --max-dist D');
  const [scene = 'instanced1000', count = '64', cellSize = '32', outPath = 'atlas.png', depth = '4', spp = '16', seed = '0'] =
    argv;
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
  // the entries, and one chart layout per distinct geometry among them
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
  const bake = renderer.bakeAtlasIrradiance(entries, size, size, parseInt(depth, 10), parseInt(spp, 10),
    { atlasUv, seed: parseInt(seed, 10), stats: true });
  if (denoise > 0) {
    const pts = renderer.bakeAtlasPoints(entries, size, size, { atlasUv });
    bake.data = renderer.denoiseAtlas(bake.data, size, size, pts.points, pts.texels, { passes: denoise, planeEps, maxDist, normalCos }).data;
  }
  let filled = 0;
  if (dilate > 0) ({ data: bake.data, filled } = renderer.dilateAtlas(bake.data, size, size, dilate));
  const rgba = new Uint8Array(size * size * 4);
  const albedo = 0.8;
  let lit = 0;
  for (let i = 0; i < size * size; i++) {
    if (bake.data[4 * i + 3] < 0 && bake.data[4 * i + 3] !== -2) continue;   // no surface, no copied colour
    for (let c = 0; c < 3; c++) {
      const v = Math.PI * bake.data[4 * i + c] * albedo;
      rgba[4 * i + c] = Math.round(255 * Math.pow(Math.min(Math.max(v, 0), 1), 1 / 2.2));
    }
    rgba[4 * i + 3] = 255;
    if (bake.data[4 * i] > 0 && bake.data[4 * i + 3] >= 0) lit++;   // covered texels only, not the gutter
  }
  fs.writeFileSync(outPath, Buffer.from(encodePng(rgba, size, size)));
  console.log(JSON.stringify({ scene, entries: n, geometries: geometries.size, size, covered: bake.covered, lit, out: outPath,
    ...(denoise > 0 ? { denoise, planeEps, maxDist, normalCos } : {}), ...(dilate > 0 ? { dilate, filled } : {}), stats: bake.stats }));
  renderer.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
