'use strict';
// Headless live loop over an animated glTF (src/main.ts:119-181): load GLB -> upload -> N x renderFrame with the world
// advanced every `interval` frames (GPU BLAS builder behind update(t)) -> hashes of the accumulation buffer and the frame.
// usage: node animate_glb.js model.glb [width] [height] [frames] [interval] [depth] [--denoise PASSES [--plane-eps E]
//          [--temporal MAX_HISTORY [--motion]]]   -> prints one JSON line
// --denoise PASSES: every present() filters the frame first (setPresentDenoise, planeEps E = 0.02 unless given); --temporal
// MAX_HISTORY: the filter reprojects last frame's history first; --motion: and follows the animated surface (frame motion,
// normalCos 0.8: the shading normal is not carried).  The line then carries the sha256 of denoiseFrame()'s image too, and
// with --motion how many pixels of the last frame were carried as moved.
const crypto = require('crypto');
const fs = require('fs');
const { WebGPURenderer, WorldBridge, LiveLoop } = require('./index.js');

(async () => {
  const argv = process.argv.slice(2);
  const flag = (name, parse, dflt) => {
    const i = argv.indexOf(name);
    if (i < 0) return dflt;
    const v = parse ? parse(argv[i + 1]) : true;
    argv.splice(i, parse ? 2 : 1);
    return v;
  };
  const denoise = flag('--denoise', (v) => parseInt(v, 10), 0);
  const planeEps = flag('--plane-eps', parseFloat, 0.02);
  const temporal = flag('--temporal', (v) => parseInt(v, 10), 0);
  const motion = flag('--motion', null, false);
  if (temporal > 0 && !(denoise > 0)) throw new Error('--temporal needs --denoise');
  if (motion && !(temporal > 0)) throw new Error('--motion needs --temporal');
  const [file, w = '96', h = '64', frames = '6', interval = '2', depth = '5'] = argv;
  const width = parseInt(w, 10), height = parseInt(h, 10);
  const renderer = new WebGPURenderer(0);
  await renderer.init();
  renderer.buildPipeline(parseInt(depth, 10), 1);
  const bridge = new WorldBridge();
  await bridge.initWasm();
  if (process.env.RT_NODE_GPU_BLAS) bridge.setBlasBuilder(renderer);
  if (process.env.RT_NODE_DEVICE_UPDATE) bridge.setDeviceUpdater(renderer);   // update(t) inside the renderer (rt_world_update)
  await bridge.loadScene('viewer', undefined, new Uint8Array(fs.readFileSync(file)));
  await renderer.loadTexturesFromWorld(bridge);
  renderer.updateScreenSize(width, height);
  const loop = new LiveLoop(renderer, bridge, width, height, parseInt(interval, 10));
  const desc = denoise > 0 ? WebGPURenderer.frameDenoiseDesc({ passes: denoise, planeEps }) : null;
  for (let f = 0; f < parseInt(frames, 10); f++) {
    loop.renderFrame();
    if (f === 0 && desc) {   // the first frame has uploaded the scene, which the motion flag needs
      renderer.setPresentDenoise(desc);
      if (temporal > 0) renderer.setFrameTemporal(WebGPURenderer.frameTemporalDesc({ maxHistory: temporal, planeEps, motion, normalCos: motion ? 0.8 : 0.9 }));
    }
  }
  await renderer.device.queue.onSubmittedWorkDone();
  const acc = renderer.readAccum();
  const frame = await renderer.captureFrame();
  const sha = (buf) => crypto.createHash('sha256').update(Buffer.from(buf)).digest('hex');
  console.log(JSON.stringify({ frames: parseInt(frames, 10), animations: bridge.getAnimationList(), frameCount: loop.frameCount,
    accum_sha256: sha(acc.buffer), rgba_sha256: sha(frame.data), deviceResident: !!bridge.deviceResident,
    ...(desc ? { denoise, planeEps, denoised_sha256: sha(renderer.denoiseFrame(desc).data.buffer) } : {}),
    ...(temporal > 0 ? { temporal } : {}),
    ...(motion ? { motion: true, moved: new Uint32Array(renderer.readFrameMotion().data.buffer).filter((v, i) => i % 8 === 3 && v === 3).length } : {}) }));
  renderer.destroy();
})().catch((e) => { console.error(e); process.exit(1); });
