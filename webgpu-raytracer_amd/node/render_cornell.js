'use strict';
// Headless driver reproducing the reference's call sequence (src/main.ts:51-116,119-181):
// load scene -> upload buffers -> resolution -> N x { compute(frame); present() } -> captureFrame.
// usage: node render_cornell.js [scene] [width] [height] [frames] [depth] [--denoise PASSES [--plane-eps E] [--temporal MAX_HISTORY]]
//   -> prints one JSON line
// --denoise PASSES (1 .. 5): every present() filters the frame first (setPresentDenoise: the G-buffer-guided a-trous filter,
// demodulated, planeEps E = 0.02 unless given), and the line also carries the sha256 of denoiseFrame()'s image of the last frame.
// --temporal MAX_HISTORY (1 .. 256), with --denoise: the filter reprojects last frame's history first (setFrameTemporal, planeEps E).
const crypto = require('crypto');
const { WebGPURenderer, WorldBridge } = require('./index.js');

(async () => {
  const argv = process.argv.slice(2);
  const flag = (name, parse, dflt) => {
    const i = argv.indexOf(name);
    if (i < 0) return dflt;
    const v = parse(argv[i + 1]);
    argv.splice(i, 2);
    return v;
  };
  const denoise = flag('--denoise', (v) => parseInt(v, 10), 0);
  const planeEps = flag('--plane-eps', parseFloat, 0.02);
  const temporal = flag('--temporal', (v) => parseInt(v, 10), 0);
  if (temporal > 0 && !(denoise > 0)) throw new Error('--temporal needs --denoise');
  const [scene = 'cornell', w = '96', h = '96', frames = '3', depth = '4'] = argv;
  const width = parseInt(w, 10), height = parseInt(h, 10);
  const bridge = new WorldBridge();
  await bridge.initWasm();
  await bridge.loadScene(scene);
  const renderer = new WebGPURenderer(0);
  await renderer.init();
  renderer.buildPipeline(parseInt(depth, 10), 1);
  if (process.env.RT_NODE_GPU_BLAS) {  // rebuild the scene's BLASes with the GPU builder (same arrays, byte for byte)
    bridge.setBlasBuilder(renderer);
    bridge.update(0);
  }
  await renderer.loadTexturesFromWorld(bridge);
  renderer.updateCombinedGeometry(bridge.vertices, bridge.normals, bridge.uvs);
  renderer.updateCombinedBVH(bridge.tlas, bridge.blas);
  renderer.updateBuffer('topology', bridge.mesh_topology);
  renderer.updateBuffer('instance', bridge.instances);
  renderer.updateBuffer('lights', bridge.lights);
  renderer.updateBuffer('draw_commands', bridge.draw_commands);
  renderer.updateScreenSize(width, height);
  bridge.updateCamera(width, height);
  renderer.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount);
  renderer.recreateBindGroup();
  renderer.resetAccumulation();
  const desc = denoise > 0 ? WebGPURenderer.frameDenoiseDesc({ passes: denoise, planeEps }) : null;
  if (desc) renderer.setPresentDenoise(desc);
  if (temporal > 0) renderer.setFrameTemporal(WebGPURenderer.frameTemporalDesc({ maxHistory: temporal, planeEps }));
  for (let f = 1; f <= parseInt(frames, 10); f++) { renderer.compute(f); renderer.present(); }
  if (process.env.RT_NODE_BATCH) {  // extra frames through the batched entry point
    const n = parseInt(process.env.RT_NODE_BATCH, 10), first = parseInt(frames, 10) + 1;
    renderer.computeBatch(Array.from({ length: n }, (_, i) => first + i));
    renderer.present();
  }
  await renderer.device.queue.onSubmittedWorkDone();
  const frame = await renderer.captureFrame();
  const acc = renderer.readAccum();
  const sha = (buf) => crypto.createHash('sha256').update(Buffer.from(buf)).digest('hex');
  console.log(JSON.stringify({ scene, width, height, frames: parseInt(frames, 10),
    rgba_sha256: sha(frame.data), accum_sha256: sha(acc.buffer), counters: renderer.getCounters(),
    ...(temporal > 0 ? { temporal } : {}),
    ...(desc ? { denoise, planeEps, denoised_sha256: sha(renderer.denoiseFrame(desc).data.buffer) } : {}) }));
  renderer.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
