'use strict';
// Headless ray queries against a built-in scene (WebGPURenderer.traceRays):
// usage: node trace_rays.js <scene> <rays.f32> <hits.bin> [any] [tMin]
//   rays.f32   raw little-endian float32, 8 per ray {origin, tMax, direction, -}
//   hits.bin   written: 16 bytes per ray {t (float32), tri (int32), inst (int32), hit (uint32)}
// prints one JSON line with the ray count and the query's stats
const fs = require('fs');
const { WebGPURenderer, WorldBridge } = require('./index.js');

(async () => {
  const [scene = 'cornell', raysPath, hitsPath, any = '0', tMin = '0.001'] = process.argv.slice(2);
  if (!raysPath || !hitsPath) throw new Error('usage: node trace_rays.js <scene> <rays.f32> <hits.bin> [any] [tMin]');
  const raw = fs.readFileSync(raysPath);
  const rays = new Float32Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length));
  const bridge = new WorldBridge();
  await bridge.initWasm();
  await bridge.loadScene(scene);
  const renderer = new WebGPURenderer(0);
  await renderer.init();
  renderer.updateCombinedGeometry(bridge.vertices, bridge.normals, bridge.uvs);
  renderer.updateCombinedBVH(bridge.tlas, bridge.blas);
  renderer.updateBuffer('topology', bridge.mesh_topology);
  renderer.updateBuffer('instance', bridge.instances);
  renderer.updateBuffer('lights', bridge.lights);
  const out = renderer.traceRays(rays, { anyHit: any === '1', tMin: parseFloat(tMin), stats: true });
  fs.writeFileSync(hitsPath, Buffer.from(out.words.buffer));
  console.log(JSON.stringify({ scene, rays: rays.length / 8, stats: out.stats }));
  renderer.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
