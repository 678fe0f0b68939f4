'use strict';
// Bake a lightmap of the floor of the Cornell box and write it as a PNG:
// usage: node bake_lightmap.js [size] [out.png] [maxDepth] [spp] [seed] [--denoise PASSES --plane-eps E --max-dist D [--normal-cos C]]
//        [--dilate R]     defaults: 256, bake.png, 4, 64, 0, no denoising, no dilation
// The box is one instance whose quads all carry the uvs (0,0) .. (1,1), so the scene's own uvs would lay every quad over the
// whole atlas.  The example therefore supplies an override layout: the floor - the two largest triangles in the plane
// y = min y - gets u = (x - min x) / (max x - min x), v = (z - min z) / (max z - min z); every other vertex goes to (-1, -1),
// where its triangles have no area and cover nothing.  (The quads of this scene share no vertices.)
// A bake point carries the mesh's normal as stored, and this floor's normals point out of the room, so bakeIrradiance would
// gather below the floor and return black.  The example shows the three steps instead: bakePoints, the normals turned
// towards the middle of the room on the host, gatherIrradiance, and the scatter by texel index.
// The gather returns E / pi per point; the picture shows pi * (E / pi) * albedo with albedo = 0.8 and gamma 2.2: the floor seen
// from above, dark where the two boxes stand and in their shadows.  --dilate R (1 .. 24) puts a gutter of R texels of copied
// colour around the chart (dilateAtlas); its texels are drawn like covered ones.  --denoise PASSES (1 .. 3) filters the atlas
// before that (denoiseAtlas, guided by the points of step 1 with their normals as turned: taps count within E of a texel's
// tangent plane and within D of it, world units, where the normals' dot product is at least C, default 0.9).  Prints one JSON line.
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
  const [size = '256', outPath = 'bake.png', depth = '4', spp = '64', seed = '0'] = argv;
  const scene = 'cornell', inst = 0;
  const n = parseInt(size, 10);
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
  renderer.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount);   // the light count of the shading
  // the floor's own chart
  const pos = bridge.vertices, topo = bridge.mesh_topology;
  const nVerts = pos.length / 4, nTris = topo.length / 20;
  let minY = Infinity;
  const lo3 = [Infinity, Infinity, Infinity], hi3 = [-Infinity, -Infinity, -Infinity];
  for (let v = 0; v < nVerts; v++) {
    minY = Math.min(minY, pos[4 * v + 1]);
    for (let c = 0; c < 3; c++) { lo3[c] = Math.min(lo3[c], pos[4 * v + c]); hi3[c] = Math.max(hi3[c], pos[4 * v + c]); }
  }
  const inPlane = [];
  for (let k = 0; k < nTris; k++) {
    const ids = [topo[20 * k], topo[20 * k + 1], topo[20 * k + 2]];
    if (!ids.every((v) => Math.abs(pos[4 * v + 1] - minY) < 1e-4)) continue;
    const [a, b, c] = ids.map((v) => [pos[4 * v], pos[4 * v + 2]]);
    inPlane.push({ ids, area: Math.abs((b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])) });
  }
  const largest = Math.max(...inPlane.map((t) => t.area));
  const floor = inPlane.filter((t) => t.area > largest - 1e-6).map((t) => t.ids);
  let lo = [Infinity, Infinity], hi = [-Infinity, -Infinity];
  for (const ids of floor) for (const v of ids) {
    lo = [Math.min(lo[0], pos[4 * v]), Math.min(lo[1], pos[4 * v + 2])];
    hi = [Math.max(hi[0], pos[4 * v]), Math.max(hi[1], pos[4 * v + 2])];
  }
  const atlasUv = new Float32Array(nVerts * 2).fill(-1);
  for (const ids of floor) for (const v of ids) {
    atlasUv[2 * v] = (pos[4 * v] - lo[0]) / (hi[0] - lo[0]);
    atlasUv[2 * v + 1] = (pos[4 * v + 2] - lo[1]) / (hi[1] - lo[1]);
  }
  // 1. points   2. normals towards the middle of the room   3. gather   4. scatter
  const pts = renderer.bakePoints(inst, n, n, { atlasUv });
  const mid = [0, 1, 2].map((c) => 0.5 * (lo3[c] + hi3[c]));
  for (let j = 0; j < pts.n; j++) {
    let d = 0;
    for (let c = 0; c < 3; c++) d += pts.points[8 * j + 4 + c] * (mid[c] - pts.points[8 * j + c]);
    if (d < 0) for (let c = 0; c < 3; c++) pts.points[8 * j + 4 + c] = -pts.points[8 * j + 4 + c];
  }
  const res = renderer.gatherIrradiance(pts.points, parseInt(depth, 10), parseInt(spp, 10), { seed: parseInt(seed, 10), stats: true });
  const bake = { data: new Float32Array(n * n * 4), covered: pts.n, stats: res.stats };
  for (let i = 0; i < n * n; i++) bake.data[4 * i + 3] = -1;   // no surface
  for (let j = 0; j < pts.n; j++) bake.data.set(res.data.subarray(4 * j, 4 * j + 4), 4 * pts.texels[j]);
  if (denoise > 0) bake.data = renderer.denoiseAtlas(bake.data, n, n, pts.points, pts.texels, { passes: denoise, planeEps, maxDist, normalCos }).data;
  let filled = 0;
  if (dilate > 0) ({ data: bake.data, filled } = renderer.dilateAtlas(bake.data, n, n, dilate));
  const rgba = new Uint8Array(n * n * 4);
  const albedo = 0.8;
  let lit = 0;
  for (let i = 0; i < n * n; i++) {
    if (bake.data[4 * i + 3] < 0 && bake.data[4 * i + 3] !== -2) continue;   // no surface, no copied colour
    for (let c = 0; c < 3; c++) {
      const v = Math.PI * bake.data[4 * i + c] * albedo;
      rgba[4 * i + c] = Math.round(255 * Math.pow(Math.min(Math.max(v, 0), 1), 1 / 2.2));
    }
    rgba[4 * i + 3] = 255;
    if (bake.data[4 * i] > 0 && bake.data[4 * i + 3] >= 0) lit++;   // covered texels only, not the gutter
  }
  fs.writeFileSync(outPath, Buffer.from(encodePng(rgba, n, n)));
  console.log(JSON.stringify({ scene, inst, size: n, floorTriangles: floor.length, covered: bake.covered, lit, out: outPath,
    ...(denoise > 0 ? { denoise, planeEps, maxDist, normalCos } : {}), ...(dilate > 0 ? { dilate, filled } : {}), stats: bake.stats }));
  renderer.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
