'use strict';
// Headless driver: ONE image rendered as `world` ranks of a sharded image (rt_dist_*, include/mi355rt.h) — the replacement of
// the reference's worker distribution (src/main.ts:278-290, src/distributed/DistributedHost.ts:90-140) for one picture.
// Same call sequence per rank as render_cornell.js; after every frame the stripes are gathered on rank 0, which presents.
// usage: node render_sharded.js [scene] [width] [height] [frames] [depth] [world]   -> prints one JSON line
//   (accum_sha256 / rgba_sha256 of the assembled image, counters summed over the ranks: what render_cornell.js prints for
//   the same frames on one context)
// Fewer devices than ranks: the ranks are contexts of this process on device 0 and the blocks go through the host
// (readBlock / writeBlock).  Enough devices: one forked child per GPU, the RCCL unique id handed round over the IPC
// channel, gatherStripes().  RT_NODE_SHARDED_MODE=contexts|fork forces one of the two.
const crypto = require('crypto');
const path = require('path');
const childProcess = require('child_process');

const STRIPE_ROWS = 8;
const CHILD_LIMIT_MS = 300000;
const sha = (buf) => crypto.createHash('sha256').update(Buffer.from(buf)).digest('hex');

function parseArgs(argv) {
  const [scene = 'cornell', w = '96', h = '96', frames = '3', depth = '4', world = '2'] = argv;
  return { scene, width: parseInt(w, 10), height: parseInt(h, 10), frames: parseInt(frames, 10), depth: parseInt(depth, 10),
    world: parseInt(world, 10) };
}

async function makeRank(a, device) {
  const { WebGPURenderer, WorldBridge } = require('./index.js');
  const bridge = new WorldBridge();
  await bridge.initWasm();
  await bridge.loadScene(a.scene);
  const renderer = new WebGPURenderer(device);
  await renderer.init();
  renderer.buildPipeline(a.depth, 1);
  await renderer.loadTexturesFromWorld(bridge);
  renderer.updateCombinedGeometry(bridge.vertices, bridge.normals, bridge.uvs);
  renderer.updateCombinedBVH(bridge.tlas, bridge.blas);
  renderer.updateBuffer('topology', bridge.mesh_topology);
  renderer.updateBuffer('instance', bridge.instances);
  renderer.updateBuffer('lights', bridge.lights);
  renderer.updateBuffer('draw_commands', bridge.draw_commands);
  renderer.updateScreenSize(a.width, a.height);
  bridge.updateCamera(a.width, a.height);
  renderer.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount);
  renderer.recreateBindGroup();
  renderer.resetAccumulation();
  return renderer;
}

function sumCounters(list) {
  const out = {};
  for (const c of list) for (const k of Object.keys(c)) out[k] = (out[k] || 0) + c[k];
  return out;
}

async function result(a, mode, rank0, counters) {
  await rank0.device.queue.onSubmittedWorkDone();
  const frame = await rank0.captureFrame();
  return { scene: a.scene, width: a.width, height: a.height, frames: a.frames, world: a.world, mode,
    rgba_sha256: sha(frame.data), accum_sha256: sha(rank0.readDisplay().buffer), counters };
}

// the ranks as contexts of this process; the host carries the blocks
async function runContexts(a) {
  const ranks = [];
  for (let k = 0; k < a.world; k++) {
    const r = await makeRank(a, 0);
    r.distInit(k, a.world, STRIPE_ROWS, null);
    ranks.push(r);
  }
  for (let f = 1; f <= a.frames; f++) {
    for (const r of ranks) { r.compute(f); r.packStripes(); }
    ranks.forEach((r, k) => ranks[0].writeBlock(k, r.readBlock()));
    ranks[0].unpackStripes();
    ranks[0].present();
  }
  const out = await result(a, 'contexts', ranks[0], sumCounters(ranks.map((r) => r.getCounters())));
  for (const r of ranks) r.destroy();
  return out;
}

// one rank in a forked child: device = rank, RCCL gather
async function runChild(a, rank) {
  const { WebGPURenderer } = require('./index.js');
  process.on('disconnect', () => process.exit(1));   // the parent is gone: no rank outlives it
  const id = await new Promise((resolve) => {
    if (rank === 0) {
      const made = WebGPURenderer.distUniqueId();
      process.send({ id: Array.from(made) });
      resolve(made);
    } else {
      process.once('message', (m) => resolve(Uint8Array.from(m.id)));
      process.send({ ready: rank });   // the parent forwards the id only to a rank that is listening
    }
  });
  const r = await makeRank(a, rank);
  r.distInit(rank, a.world, STRIPE_ROWS, id);
  for (let f = 1; f <= a.frames; f++) {
    r.compute(f);
    r.gatherStripes();
    if (rank === 0) r.present();
  }
  await r.device.queue.onSubmittedWorkDone();
  const msg = { rank, counters: r.getCounters() };
  if (rank === 0) msg.result = await result(a, 'fork', r, null);
  r.destroy();
  await new Promise((resolve) => process.send(msg, resolve));
  process.removeAllListeners('disconnect');
  process.disconnect();   // the IPC channel would keep the child alive
}

// parent of the forked mode: never touches the GPU; every child has a time limit and is killed on expiry or on a failure
function runFork(a, argv) {
  return new Promise((resolve, reject) => {
    const kids = [], done = [];
    let rank0 = null, failed = false, id = null;
    const ready = [];
    const stop = (why) => {
      if (failed) return;
      failed = true;
      clearTimeout(timer);
      for (const k of kids) k.kill('SIGKILL');
      reject(new Error(why));
    };
    const timer = setTimeout(() => stop(`a rank did not finish within ${CHILD_LIMIT_MS / 1000} s`), CHILD_LIMIT_MS);
    for (let k = 0; k < a.world; k++) {
      // dmabuf IPC for RCCL across processes (bench.py sets the same for its ranks), unless the caller has chosen
      const kid = childProcess.fork(__filename, argv.concat(['--rank', String(k)]),
        { env: Object.assign({ HSA_ENABLE_IPC_MODE_LEGACY: '0' }, process.env) });
      kids.push(kid);
      kid.on('message', (m) => {
        if (m.id || m.ready !== undefined) {   // rank 0's unique id goes to every other rank once that rank listens
          if (m.id) id = m.id; else ready.push(m.ready);
          if (id) for (const j of ready.splice(0)) kids[j].send({ id });
          return;
        }
        done.push(m.counters);
        if (m.result) rank0 = m.result;
      });
      kid.on('exit', (code) => {
        if (code !== 0) return stop(`rank ${k} exited with ${code}`);
        if (kids.every((o) => o.exitCode === 0)) {
          clearTimeout(timer);
          if (!rank0 || done.length !== a.world) return stop('a rank ended without its result');
          rank0.counters = sumCounters(done);
          resolve(rank0);
        }
      });
    }
  });
}

// device count asked in a short-lived process of its own: this one must not have touched the GPU when it forks
function deviceCount() {
  const out = childProcess.spawnSync(process.execPath, ['-e',
    `console.log(require(${JSON.stringify(path.join(__dirname, 'index.js'))}).WebGPURenderer.deviceCount())`],
  { encoding: 'utf8', timeout: 60000 });
  const n = parseInt((out.stdout || '').trim().split('\n').pop(), 10);
  return Number.isFinite(n) ? n : 0;
}

(async () => {
  const argv = process.argv.slice(2);
  const at = argv.indexOf('--rank');
  if (at >= 0) return runChild(parseArgs(argv.slice(0, at)), parseInt(argv[at + 1], 10));
  const a = parseArgs(argv);
  if (!(a.world >= 1)) throw new Error('world must be >= 1');
  const mode = process.env.RT_NODE_SHARDED_MODE || (deviceCount() >= a.world && a.world > 1 ? 'fork' : 'contexts');
  const out = mode === 'fork' ? await runFork(a, argv) : await runContexts(a);
  console.log(JSON.stringify(out));
})().catch((e) => { console.error(e); process.exit(1); });
