'use strict';
// index.js — Node host: the reference's WebGPURenderer / WorldBridge class surface
// (src/renderer/WebGPURenderer.ts:7-138, src/world-bridge.ts:4-216) over the N-API addon.
// Plain CommonJS so that the Node 12 in this image runs it; index.d.ts carries the TypeScript
// signatures of the reference classes.
const path = require('path');
const native = require(path.join(__dirname, 'mi355rt.node'));

const KIND = { topology: 0, instance: 1, lights: 2, draw_commands: 3 };
const RT_REALLOCATED = 1;

// PNG container (colour type 6, filter 0) around zlib — stands in for the encoded images a glTF would carry
const zlib = require('zlib');
const CRC_TABLE = (() => {
  const t = new Uint32Array(256);
  for (let i = 0; i < 256; i++) {
    let c = i;
    for (let k = 0; k < 8; k++) c = (c & 1) ? (0xedb88320 ^ (c >>> 1)) : (c >>> 1);
    t[i] = c >>> 0;
  }
  return t;
})();
function crc32(buf) {
  let c = 0xffffffff;
  for (let i = 0; i < buf.length; i++) c = CRC_TABLE[(c ^ buf[i]) & 255] ^ (c >>> 8);
  return (c ^ 0xffffffff) >>> 0;
}
function pngChunk(tag, data) {
  const out = Buffer.alloc(12 + data.length);
  out.writeUInt32BE(data.length, 0);
  out.write(tag, 4, 'latin1');
  Buffer.from(data.buffer, data.byteOffset, data.length).copy(out, 8);
  out.writeUInt32BE(crc32(out.subarray(4, 8 + data.length)), 8 + data.length);
  return out;
}
function encodePng(rgba, width, height) {
  const rows = Buffer.alloc(height * (1 + width * 4));
  for (let y = 0; y < height; y++)
    Buffer.from(rgba.buffer, rgba.byteOffset + y * width * 4, width * 4).copy(rows, y * (1 + width * 4) + 1);
  const ihdr = Buffer.alloc(13);
  ihdr.writeUInt32BE(width, 0);
  ihdr.writeUInt32BE(height, 4);
  ihdr[8] = 8; ihdr[9] = 6;
  return new Uint8Array(Buffer.concat([Buffer.from([0x89, 0x50, 0x4e, 0x47, 0x0d, 0x0a, 0x1a, 0x0a]), pngChunk('IHDR', ihdr),
    pngChunk('IDAT', zlib.deflateSync(rows, { level: 1 })), pngChunk('IEND', Buffer.alloc(0))]));
}

class WebGPURenderer {
  // `new WebGPURenderer(canvas)`: the canvas becomes a device ordinal (there is no swap chain).
  constructor(device = 0) {
    this._device = device;
    this._ctx = null;
    this.width = 0;
    this.height = 0;
    this._capture = null;
  }
  // only init() throws in the reference (WebGPUContext.ts:15,19)
  async init() {
    this._ctx = native.rtCreate(this._device);
  }
  get device() {
    const self = this;
    return { queue: { onSubmittedWorkDone: async () => { self._check(native.rtSync(self._ctx), 'sync'); } } };
  }
  _check(rc, what) {
    if (rc < 0) throw new Error(`${what} failed (${rc}): ${native.rtLastError(this._ctx)}`);
    return rc;
  }
  buildPipeline(depth, spp) { this._check(native.rtSetPipeline(this._ctx, depth, spp), 'buildPipeline'); }
  updateScreenSize(width, height) {
    this.width = width;
    this.height = height;
    this._check(native.rtResize(this._ctx, width, height), 'updateScreenSize');
  }
  resetAccumulation() { this._check(native.rtResetAccum(this._ctx), 'resetAccumulation'); }
  // ResourceManager.ts:153-198: encoded image per texture -> decode (host) -> 1024x1024 layer (GPU resize);
  // an image that is missing or does not decode becomes the white fallback bitmap and a warning (:169-175)
  async loadTexturesFromWorld(bridge) {
    const n = bridge.textureCount;
    if (n === 0) { this._check(native.rtUploadTextures(this._ctx, null, 0), 'loadTexturesFromWorld'); return; }
    this._check(native.rtAllocTextureLayers(this._ctx, n), 'loadTexturesFromWorld');
    this.textureWarnings = [];
    for (let i = 0; i < n; i++) {
      const data = bridge.getTexture(i);
      let img = null;
      if (data) {
        try { img = native.mtDecode(data); } catch (e) { this.textureWarnings.push(`Failed tex ${i}: ${e.message}`); }
      }
      this._check(native.rtUploadTextureImage(this._ctx, i, img ? img.data : null, img ? img.width : 0, img ? img.height : 0),
        'loadTexturesFromWorld');
    }
  }
  updateBuffer(type, data) {
    return this._check(native.rtUpload(this._ctx, KIND[type], data), `updateBuffer(${type})`) === RT_REALLOCATED;
  }
  updateCombinedGeometry(v, n, uv) {
    return this._check(native.rtUploadGeometry(this._ctx, v, n, uv), 'updateCombinedGeometry') === RT_REALLOCATED;
  }
  updateCombinedBVH(tlas, blas) {
    return this._check(native.rtUploadBVH(this._ctx, tlas, blas), 'updateCombinedBVH') === RT_REALLOCATED;
  }
  updateSceneUniforms(cameraData, frameCount, lightCount) {
    this._check(native.rtSetScene(this._ctx, cameraData, frameCount, lightCount), 'updateSceneUniforms');
  }
  recreateBindGroup() {}
  compute(frameCount) { this._check(native.rtCompute(this._ctx, frameCount), 'compute'); }
  // the recorder's `for (k < batch) compute(samplesDone + k)` as one dispatch per kernel (bit-identical)
  computeBatch(frameCounts) { this._check(native.rtComputeBatch(this._ctx, Uint32Array.from(frameCounts)), 'computeBatch'); }
  present() { this._check(native.rtPresent(this._ctx), 'present'); }
  async captureFrame() {
    if (!this.width) throw new Error('No render target');
    const n = this.width * this.height * 4;
    if (!this._capture || this._capture.length !== n) this._capture = new Uint8Array(n);  // reused between calls
    this._check(native.rtCapture(this._ctx, this._capture), 'captureFrame');
    return { data: this._capture.buffer, width: this.width, height: this.height };
  }
  // additions
  readAccum() {
    const out = new Float32Array(this.width * this.height * 4);
    this._check(native.rtReadAccum(this._ctx, out), 'readAccum');
    return out;
  }
  getCounters() {
    const c = native.rtGetCounters(this._ctx);
    return { primary_rays: c[0], extension_rays: c[1], shadow_rays: c[2], nodes_visited: c[3], tris_tested: c[4], shaded_hits: c[5] };
  }
  // interleaved row stripes: compute() traces only rows y with floor(y / stripeRows) % count === rank (rt_set_stripes)
  setStripes(stripeRows, rank, count) { this._check(native.rtSetStripes(this._ctx, stripeRows, rank, count), 'setStripes'); }
  // ---- the sharded image (rt_dist_*): this context as rank `rank` of `world`; the image is assembled on rank 0 ----
  // uniqueId: the Uint8Array(128) of WebGPURenderer.distUniqueId() -> RCCL gather (gatherStripes); null / undefined -> the host
  // moves the blocks itself (packStripes + readBlock on every rank, writeBlock + unpackStripes on rank 0)
  static distUniqueId() { return native.rtDistUniqueId(); }
  static deviceCount() { return native.rtDeviceCount(); }
  distInit(rank, world, stripeRows = 8, uniqueId = null) {
    this._check(native.rtDistInit(this._ctx, rank, world, stripeRows, uniqueId || null), 'distInit');
  }
  distShutdown() { this._check(native.rtDistShutdown(this._ctx), 'distShutdown'); }
  distBlockBytes() { return native.rtDistBlockBytes(this._ctx); }
  packStripes() { this._check(native.rtPackStripes(this._ctx), 'packStripes'); }
  readBlock() {
    const out = new Float32Array(this.distBlockBytes() / 4);
    this._check(native.rtDistReadBlock(this._ctx, out), 'readBlock');
    return out;
  }
  writeBlock(fromRank, block) { this._check(native.rtDistWriteBlock(this._ctx, fromRank, block), 'writeBlock'); }
  unpackStripes() { this._check(native.rtUnpackStripes(this._ctx), 'unpackStripes'); }
  gatherStripes() { this._check(native.rtGatherStripes(this._ctx), 'gatherStripes'); }
  readDisplay() {
    const out = new Float32Array(this.width * this.height * 4);
    this._check(native.rtReadDisplay(this._ctx, out), 'readDisplay');
    return out;
  }
  // ---- ray queries against the uploaded scene (rt_trace_rays): rays = 8 floats per ray {origin, tMax, direction, -};
  // opts: {anyHit = false, tMin = 0.001, stats = false}.  Closest hit: {t, tri, inst, hit} per ray, a miss is
  // {the ray's tMax, -1, -1, 0}; any hit: {0, -1, -1, occluded}.  With stats the result also carries .stats.
  traceRays(rays, opts = {}) {
    if (!(rays instanceof Float32Array) || rays.length % 8 !== 0) throw new TypeError('traceRays: a Float32Array of 8 floats per ray');
    const n = rays.length / 8;
    const words = new Uint32Array(n * 4);
    const r = native.rtTraceRays(this._ctx, rays, opts.anyHit ? 1 : 0, opts.tMin === undefined ? 0.001 : opts.tMin, words, !!opts.stats);
    if (typeof r === 'number') this._check(r, 'traceRays');
    const asF = new Float32Array(words.buffer), asI = new Int32Array(words.buffer);
    const out = { t: new Float32Array(n), tri: new Int32Array(n), inst: new Int32Array(n), hit: new Uint32Array(n) };
    for (let i = 0; i < n; i++) {
      out.t[i] = asF[4 * i]; out.tri[i] = asI[4 * i + 1]; out.inst[i] = asI[4 * i + 2]; out.hit[i] = words[4 * i + 3];
    }
    out.words = words;   // the raw rt_ray_hit records (t as its bit pattern)
    if (typeof r === 'object' && r) out.stats = r;
    return out;
  }
  rayQueryStats() {
    const r = native.rtRayQueryStats(this._ctx);
    if (typeof r === 'number') this._check(r, 'rayQueryStats');
    return r;
  }
  // ---- radiance queries (rt_trace_radiance): the path tracer's radiance along the caller's rays.  rays = 8 words per ray
  // {origin, tMax, direction, pad}; pad holds the bits of a uint32, the ray's RNG stream id (write it through a Uint32Array
  // on the same buffer).  opts: {seed = 0, stats = false}.  Result: 4 floats per ray {r, g, b, t} in .data; a miss is
  // {0, 0, 0, the ray's tMax}.  With stats the result also carries .stats.
  traceRadiance(rays, maxDepth, spp, opts = {}) {
    if (!(rays instanceof Float32Array) || rays.length % 8 !== 0) throw new TypeError('traceRadiance: a Float32Array of 8 floats per ray');
    const n = rays.length / 8;
    const data = new Float32Array(n * 4);
    const r = native.rtTraceRadiance(this._ctx, rays, maxDepth >>> 0, spp >>> 0, (opts.seed || 0) >>> 0, data, !!opts.stats);
    if (typeof r === 'number') this._check(r, 'traceRadiance');
    const out = { data, n };
    if (typeof r === 'object' && r) out.stats = r;
    return out;
  }
  // ---- irradiance gathers (rt_gather_irradiance): the cosine-weighted mean radiance arriving at the caller's surface
  // points, over spp hemisphere directions drawn on the device.  points = 8 words per point {position, tMax, normal, pad}; pad
  // holds the bits of a uint32 below 2^31, the point's RNG stream id.  opts: {seed = 0, stats = false}.  Result: 4 floats per
  // point {r, g, b, hitFraction} in .data (rgb is E / pi: multiply by pi for irradiance).  With stats the result also
  // carries .stats.
  gatherIrradiance(points, maxDepth, spp, opts = {}) {
    if (!(points instanceof Float32Array) || points.length % 8 !== 0) throw new TypeError('gatherIrradiance: a Float32Array of 8 floats per point');
    const n = points.length / 8;
    const data = new Float32Array(n * 4);
    const r = native.rtGatherIrradiance(this._ctx, points, maxDepth >>> 0, spp >>> 0, (opts.seed || 0) >>> 0, data, !!opts.stats);
    if (typeof r === 'number') this._check(r, 'gatherIrradiance');
    const out = { data, n };
    if (typeof r === 'object' && r) out.stats = r;
    return out;
  }
  // ---- probe gathers (rt_gather_probes): the radiance arriving at points in space, over spp directions drawn uniformly on
  // the sphere on the device, projected onto the nine real spherical harmonics of bands 0 .. 2.  probes = 8 words per probe
  // {position, tMax, 3 unused words (0), pad}; pad holds the bits of a uint32 below 2^31, the probe's RNG stream id.  opts:
  // {seed = 0, stats = false}.  Result: 28 floats per probe in .data: sh[k][c] at 3 k + c (coefficient-major, rgb inside),
  // then hitFraction.  With stats the result also carries .stats.
  gatherProbes(probes, maxDepth, spp, opts = {}) {
    if (!(probes instanceof Float32Array) || probes.length % 8 !== 0) throw new TypeError('gatherProbes: a Float32Array of 8 floats per probe');
    const n = probes.length / 8;
    const data = new Float32Array(n * 28);
    const r = native.rtGatherProbes(this._ctx, probes, maxDepth >>> 0, spp >>> 0, (opts.seed || 0) >>> 0, data, !!opts.stats);
    if (typeof r === 'number') this._check(r, 'gatherProbes');
    const out = { data, n };
    if (typeof r === 'object' && r) out.stats = r;
    return out;
  }
  // ---- irradiance volumes (rt_bake_volume, rt_sample_volume, rt_encode_volume): a probe grid baked into windowed irradiance
  // coefficients, sampled trilinearly and exported as texel layers, all on the device.  A descriptor is the 64 bytes of an
  // rt_volume_desc, made by WebGPURenderer.volumeDesc({origin, step, dims: [nx, ny, nz], window = [1, 1, 1], tMax = 1e30,
  // padFirst = 0, maxHitFraction = 1}); probe (x, y, z) is record (z * ny + y) * nx + x.
  static volumeDesc(o) {
    const buf = new ArrayBuffer(64), f = new Float32Array(buf), u = new Uint32Array(buf);
    const window = o.window || [1, 1, 1];
    for (let a = 0; a < 3; a++) { f[a] = o.origin[a]; f[4 + a] = o.step[a]; f[8 + a] = window[a]; u[3 + 4 * a] = o.dims[a] >>> 0; }
    f[12] = o.tMax === undefined ? 1e30 : o.tMax;
    u[13] = (o.padFirst || 0) >>> 0;
    f[14] = o.maxHitFraction === undefined ? 1 : o.maxHitFraction;
    return new Uint8Array(buf);
  }
  static _volumeProbes(desc) { const u = new Uint32Array(desc.buffer, desc.byteOffset, 16); return u[3] * u[7] * u[11]; }
  // Result: 28 floats per probe in .data (irradiance coefficients sh'[k][c] at 3 k + c, then hitFraction), .n probes; opts:
  // {seed = 0, stats = false}; the stats are the probe gather's.
  bakeVolume(desc, maxDepth, spp, opts = {}) {
    const n = WebGPURenderer._volumeProbes(desc);
    const data = new Float32Array(n * 28);
    const r = native.rtBakeVolume(this._ctx, desc, maxDepth >>> 0, spp >>> 0, (opts.seed || 0) >>> 0, data, !!opts.stats);
    if (typeof r === 'number') this._check(r, 'bakeVolume');
    const out = { data, n };
    if (typeof r === 'object' && r) out.stats = r;
    return out;
  }
  // volume: the .data of a bake; points: 8 words per point {position, -, normal, -}.  Result: 4 floats per point in .data {r, g,
  // b, W}: the irradiance at the normal and the valid share of the interpolation weight.  Needs no scene.
  sampleVolume(desc, volume, points) {
    if (!(volume instanceof Float32Array) || volume.length !== WebGPURenderer._volumeProbes(desc) * 28) throw new TypeError('sampleVolume: a Float32Array of 28 floats per probe');
    if (!(points instanceof Float32Array) || points.length % 8 !== 0) throw new TypeError('sampleVolume: a Float32Array of 8 floats per point');
    const n = points.length / 8;
    const data = new Float32Array(n * 4);
    this._check(native.rtSampleVolume(this._ctx, desc, volume, points, data), 'sampleVolume');
    return { data, n };
  }
  // The volume as seven layers of n texels, layer j holding the floats 4 j .. 4 j + 3 of every record: format 'f32' or 'f16'
  // ('rgbe' is refused: coefficients are signed).  Result: {data, layers: 7, n, format}.
  encodeVolume(desc, volume, format) {
    const n = WebGPURenderer._volumeProbes(desc);
    if (!(volume instanceof Float32Array) || volume.length !== n * 28) throw new TypeError('encodeVolume: a Float32Array of 28 floats per probe');
    const f = WebGPURenderer._lightmapFormat(format);
    const data = WebGPURenderer._lightmapArray(7 * n, f);
    this._check(native.rtEncodeVolume(this._ctx, desc, f, volume, data), 'encodeVolume');
    return { data, layers: 7, n, format: ['f32', 'f16', 'rgbe'][f] };
  }
  // ---- probe visibility maps (rt_bake_volume_visibility, rt_sample_volume_visible, rt_encode_volume_visibility): per probe of
  // a volume an octahedral map of size x size texels {mean distance, mean squared distance}, and the sampler that weights every
  // corner probe by its visibility of the point, so that a probe behind a wall does not light the room in front of it.  A
  // descriptor is the 32 bytes of an rt_volume_visibility_desc, made by WebGPURenderer.volumeVisibilityDesc({size,
  // maxDistance, spt = 64, normalBias = 0, minVisibility = 0, crushThreshold = 0, backface = false}).
  static volumeVisibilityDesc(o) {
    const buf = new ArrayBuffer(32), f = new Float32Array(buf), u = new Uint32Array(buf);
    u[0] = o.size >>> 0;
    u[1] = (o.spt === undefined ? 64 : o.spt) >>> 0;
    f[2] = o.maxDistance;
    f[3] = o.normalBias || 0;
    f[4] = o.minVisibility || 0;
    f[5] = o.crushThreshold || 0;
    u[6] = o.backface ? 1 : 0;
    return new Uint8Array(buf);
  }
  static _visibilityTexels(desc, vis) {
    const size = new Uint32Array(vis.buffer, vis.byteOffset, 8)[0];
    return WebGPURenderer._volumeProbes(desc) * size * size;
  }
  // Result: 2 floats per texel in .data, probe-major, texel (i, j) of a map at j * size + i; .n probes, .size; opts: {seed = 0,
  // stats = false}; the stats are a ray query's, summed over the batches.
  bakeVolumeVisibility(desc, vis, opts = {}) {
    const data = new Float32Array(WebGPURenderer._visibilityTexels(desc, vis) * 2);
    const r = native.rtBakeVolumeVisibility(this._ctx, desc, vis, (opts.seed || 0) >>> 0, data, !!opts.stats);
    if (typeof r === 'number') this._check(r, 'bakeVolumeVisibility');
    const out = { data, n: WebGPURenderer._volumeProbes(desc), size: new Uint32Array(vis.buffer, vis.byteOffset, 8)[0] };
    if (typeof r === 'object' && r) out.stats = r;
    return out;
  }
  // sampleVolume with the visibility weight: volume and points as there, visibility the .data of a bakeVolumeVisibility.
  sampleVolumeVisible(desc, vis, volume, visibility, points) {
    if (!(volume instanceof Float32Array) || volume.length !== WebGPURenderer._volumeProbes(desc) * 28) throw new TypeError('sampleVolumeVisible: a Float32Array of 28 floats per probe');
    if (!(visibility instanceof Float32Array) || visibility.length !== WebGPURenderer._visibilityTexels(desc, vis) * 2) throw new TypeError('sampleVolumeVisible: a Float32Array of 2 floats per texel of every map');
    if (!(points instanceof Float32Array) || points.length % 8 !== 0) throw new TypeError('sampleVolumeVisible: a Float32Array of 8 floats per point');
    const n = points.length / 8;
    const data = new Float32Array(n * 4);
    this._check(native.rtSampleVolumeVisible(this._ctx, desc, vis, volume, visibility, points, data), 'sampleVolumeVisible');
    return { data, n };
  }
  // The maps as one image of bordered tiles, probe (x, y, z) at tile (x, z * ny + y), each (size + 2)^2 texels with the wrapped
  // neighbours as its border: format 'f32' or 'f16' ('rgbe' is refused).  Result: {data, width, height, tile, format}.
  encodeVolumeVisibility(desc, vis, visibility, format) {
    if (!(visibility instanceof Float32Array) || visibility.length !== WebGPURenderer._visibilityTexels(desc, vis) * 2) throw new TypeError('encodeVolumeVisibility: a Float32Array of 2 floats per texel of every map');
    const f = WebGPURenderer._lightmapFormat(format);
    const u = new Uint32Array(desc.buffer, desc.byteOffset, 16), tile = new Uint32Array(vis.buffer, vis.byteOffset, 8)[0] + 2;
    const width = u[3] * tile, height = u[7] * u[11] * tile;
    const data = f === 1 ? new Uint16Array(width * height * 2) : new Float32Array(width * height * 2);
    this._check(native.rtEncodeVolumeVisibility(this._ctx, desc, vis, f, visibility, data), 'encodeVolumeVisibility');
    return { data, width, height, tile, format: ['f32', 'f16', 'rgbe'][f] };
  }
  // ---- reflection probes (rt_bake_reflection, rt_filter_reflection): octahedral radiance maps of size x size texels {r, g, b,
  // hitFraction} and their GGX-filtered chains, level m of side size >> m at the roughness m / (levels - 1).  A descriptor is
  // the 32 bytes of an rt_reflection_desc, made by WebGPURenderer.reflectionDesc({size, levels, spt = 1, filterSamples = 256}).
  static reflectionDesc(o) {
    return new Uint8Array(Uint32Array.of(o.size >>> 0, o.levels >>> 0, (o.spt === undefined ? 1 : o.spt) >>> 0,
      (o.filterSamples === undefined ? 256 : o.filterSamples) >>> 0, 0, 0, 0, 0).buffer);
  }
  // levels + 1 texel offsets: level m of a chain is the texels [offsets[m], offsets[m + 1]); the last is the length of a chain
  static reflectionLevelOffsets(desc) {
    const u = new Uint32Array(desc.buffer, desc.byteOffset, 8), off = [0];
    if (u[1] > 32) throw new RangeError('reflection: levels');
    for (let m = 0; m < u[1]; m++) off.push(off[m] + (u[0] >>> m) * (u[0] >>> m));
    return off;
  }
  // probes as for gatherProbes.  opts: {seed = 0, stats = false}.  Result: .data holds a chain per probe, 4 floats per texel; .n
  // probes, .chainTexels, .offsets; with stats the capture's .stats (rays = texels).
  bakeReflection(desc, probes, maxDepth, opts = {}) {
    if (!(probes instanceof Float32Array) || probes.length % 8 !== 0) throw new TypeError('bakeReflection: a Float32Array of 8 floats per probe');
    const n = probes.length / 8, offsets = WebGPURenderer.reflectionLevelOffsets(desc), chainTexels = offsets[offsets.length - 1];
    const data = new Float32Array(n * chainTexels * 4);
    const r = native.rtBakeReflection(this._ctx, desc, probes, maxDepth >>> 0, (opts.seed || 0) >>> 0, data, !!opts.stats);
    if (typeof r === 'number') this._check(r, 'bakeReflection');
    const out = { data, n, chainTexels, offsets };
    if (typeof r === 'object' && r) out.stats = r;
    return out;
  }
  // maps: size * size texels of 4 floats per probe.  Result as for bakeReflection, level 0 the map word for word.  Needs no scene.
  filterReflection(desc, maps) {
    const offsets = WebGPURenderer.reflectionLevelOffsets(desc), chainTexels = offsets[offsets.length - 1], map = offsets[1] * 4;
    if (!(maps instanceof Float32Array) || maps.length % map !== 0) throw new TypeError('filterReflection: a Float32Array of size * size * 4 floats per probe');
    const n = maps.length / map;
    const data = new Float32Array(n * chainTexels * 4);
    this._check(native.rtFilterReflection(this._ctx, desc, maps, data), 'filterReflection');
    return { data, n, chainTexels, offsets };
  }
  // chain: the floats of ONE chain.  Result: one encodeAtlas result per level, in 'f32', 'f16' or 'rgbe' (radiance is not
  // signed, so the shared-exponent format applies).
  encodeReflection(desc, chain, format) {
    const offsets = WebGPURenderer.reflectionLevelOffsets(desc), size = new Uint32Array(desc.buffer, desc.byteOffset, 8)[0];
    if (!(chain instanceof Float32Array) || chain.length !== offsets[offsets.length - 1] * 4) throw new TypeError('encodeReflection: the floats of one chain');
    const out = [];
    for (let m = 0; m + 1 < offsets.length; m++) out.push(this.encodeAtlas(chain.slice(offsets[m] * 4, offsets[m + 1] * 4), size >>> m, size >>> m, format));
    return out;
  }
  // ---- the reflection sampler (rt_sample_reflection): baked chains read on the device at a direction and a roughness, with a
  // bilinear fetch that follows the octahedral map across its seams and, with parallax, the direction bent to where it leaves
  // the probe's box.  A descriptor is the 32 bytes of an rt_reflection_sample_desc.
  static reflectionSampleDesc(o) {
    return new Uint8Array(Uint32Array.of(o.size >>> 0, o.levels >>> 0, o.parallax ? 1 : 0, 0, 0, 0, 0, 0).buffer);
  }
  // chains: whole chains as bakeReflection's .data holds them; queries: 8 floats per query {position, probe index as the bits
  // of a u32, direction, roughness}; opts: {probes, boxes}, 8 floats per chain each ({position, tMax, -, pad} and {lo, -, hi, -}),
  // read with parallax only.  Result: .data holds 4 floats {r, g, b, hitFraction} per query.  Needs no scene.
  sampleReflection(desc, chains, queries, opts = {}) {
    if (!(chains instanceof Float32Array)) throw new TypeError('sampleReflection: the chains are a Float32Array');
    if (!(queries instanceof Float32Array) || queries.length % 8 !== 0) throw new TypeError('sampleReflection: a Float32Array of 8 floats per query');
    const n = queries.length / 8;
    const data = new Float32Array(n * 4);
    this._check(native.rtSampleReflection(this._ctx, desc, chains, opts.probes || null, opts.boxes || null, queries, data), 'sampleReflection');
    return { data, n };
  }
  // ---- directional gathers (rt_gather_directional): the radiance arriving at the caller's surface points, over spp directions
  // drawn uniformly on the hemisphere of the normal on the device, projected onto the four real spherical harmonics of bands 0
  // .. 1 in world space.  points as for gatherIrradiance.  opts: {seed = 0, stats = false}.  Result: 16 floats per point in
  // .data, four rows {sh[k].r, sh[k].g, sh[k].b, hitFraction}, k = 0 .. 3 (Y0, then the y, z and x of band 1): row k is the texel
  // of atlas layer k.  With stats the result also carries .stats.
  gatherDirectional(points, maxDepth, spp, opts = {}) {
    if (!(points instanceof Float32Array) || points.length % 8 !== 0) throw new TypeError('gatherDirectional: a Float32Array of 8 floats per point');
    const n = points.length / 8;
    const data = new Float32Array(n * 16);
    const r = native.rtGatherDirectional(this._ctx, points, maxDepth >>> 0, spp >>> 0, (opts.seed || 0) >>> 0, data, !!opts.stats);
    if (typeof r === 'number') this._check(r, 'gatherDirectional');
    const out = { data, n };
    if (typeof r === 'object' && r) out.stats = r;
    return out;
  }
  // ---- lightmap bakes (rt_bake_points, rt_bake_irradiance): the covered texels of TLAS-order instance `inst`'s width x height
  // atlas as gather points, by the texel rule of include/mi355rt.h.  opts: {tMax = 1e30, padBase = 0, atlasUv = null (a
  // Float32Array of 2 floats per scene vertex overriding the scene's uvs), owner = false}.  Result: {n, points (8 words per
  // point), texels (Uint32Array, ascending)} and with owner the Int32Array owner map (global triangle index, -1 = uncovered).
  bakePoints(inst, width, height, opts = {}) {
    const texels = new Uint32Array(width * height), points = new Float32Array(width * height * 8);
    const owner = opts.owner ? new Int32Array(width * height) : null;
    const n = native.rtBakePoints(this._ctx, inst >>> 0, width >>> 0, height >>> 0, (opts.padBase || 0) >>> 0,
      opts.tMax === undefined ? 1e30 : opts.tMax, opts.atlasUv || null, points, texels, owner);
    this._check(n, 'bakePoints');
    const out = { n, points: points.subarray(0, n * 8), texels: texels.subarray(0, n) };
    if (owner) out.owner = owner;
    return out;
  }
  // The whole bake: points, the irradiance gather on them, scatter.  opts as above plus {seed = 0, stats = false}.  Result:
  // {data (4 floats per texel {r, g, b, hitFraction}, row 0 first; uncovered texels are {0, 0, 0, -1}), width, height, covered}
  // and with stats the gather's .stats.  rgb is E / pi: multiply by pi * albedo for the outgoing radiance of a Lambert texel.
  bakeIrradiance(inst, width, height, maxDepth, spp, opts = {}) {
    const data = new Float32Array(width * height * 4);
    const r = native.rtBakeIrradiance(this._ctx, inst >>> 0, width >>> 0, height >>> 0, (opts.padBase || 0) >>> 0,
      opts.tMax === undefined ? 1e30 : opts.tMax, opts.atlasUv || null, maxDepth >>> 0, spp >>> 0, (opts.seed || 0) >>> 0, data,
      !!opts.stats);
    if (typeof r === 'number') this._check(r, 'bakeIrradiance');
    const out = { data, width, height, covered: r.covered };
    if (r.stats) out.stats = r.stats;
    return out;
  }
  // ---- atlas bakes (rt_bake_atlas_points, rt_bake_atlas_irradiance): entries = an array of [inst, x, y, w, h] (or a
  // Uint32Array of 5 words per entry): TLAS-order instance `inst` baked at w x h texels into the rectangle at (x, y) of one
  // width x height atlas, by the atlas rule of include/mi355rt.h; the lowest entry owns a texel several cover.  opts as for
  // bakePoints.  Result: {n, points, texels (atlas texel indices, ascending)} and with owner the Int32Array owner map of 2
  // words per texel {entry, global triangle index}, {-1, -1} = uncovered.
  static _atlasEntries(entries) {
    const flat = entries instanceof Uint32Array ? entries : Uint32Array.from(entries.flat());
    if (flat.length % 5 !== 0) throw new TypeError('atlas bake: entries are [inst, x, y, w, h]');
    const rects = new Uint32Array(flat.length / 5 * 8);
    for (let e = 0; e < flat.length / 5; e++) rects.set(flat.subarray(5 * e, 5 * e + 5), 8 * e);
    return rects;
  }
  bakeAtlasPoints(entries, width, height, opts = {}) {
    const texels = new Uint32Array(width * height), points = new Float32Array(width * height * 8);
    const owner = opts.owner ? new Int32Array(width * height * 2) : null;
    const n = native.rtBakeAtlasPoints(this._ctx, width >>> 0, height >>> 0, (opts.padBase || 0) >>> 0,
      opts.tMax === undefined ? 1e30 : opts.tMax, WebGPURenderer._atlasEntries(entries), opts.atlasUv || null, points, texels, owner);
    this._check(n, 'bakeAtlasPoints');
    const out = { n, points: points.subarray(0, n * 8), texels: texels.subarray(0, n) };
    if (owner) out.owner = owner;
    return out;
  }
  // The whole atlas bake: the points of all entries, ONE irradiance gather on them, scatter.  Result as bakeIrradiance's.
  bakeAtlasIrradiance(entries, width, height, maxDepth, spp, opts = {}) {
    const data = new Float32Array(width * height * 4);
    const r = native.rtBakeAtlasIrradiance(this._ctx, width >>> 0, height >>> 0, (opts.padBase || 0) >>> 0,
      opts.tMax === undefined ? 1e30 : opts.tMax, WebGPURenderer._atlasEntries(entries), opts.atlasUv || null, maxDepth >>> 0,
      spp >>> 0, (opts.seed || 0) >>> 0, data, !!opts.stats);
    if (typeof r === 'number') this._check(r, 'bakeAtlasIrradiance');
    const out = { data, width, height, covered: r.covered };
    if (r.stats) out.stats = r.stats;
    return out;
  }
  // ---- atlas dilation (rt_dilate_atlas): a gutter of copied colour around the charts of a baked atlas.  atlas = 4 floats per
  // texel, covered where the fourth is >= 0 (as the bakes return it).  Every uncovered texel within `radius` (0 .. 24) texels
  // of a covered one receives the first three words of the nearest covered texel - the lowest texel index among equally near
  // ones - and -2 as its fourth, by the dilation rule of include/mi355rt.h.  opts: {src = false}.  Result: {data (a new
  // Float32Array), width, height, filled} and with src the Uint32Array source map (own index in covered texels, the source's
  // in filled ones, 0xffffffff elsewhere).
  dilateAtlas(atlas, width, height, radius, opts = {}) {
    if (!(atlas instanceof Float32Array) || atlas.length !== width * height * 4) throw new TypeError('dilateAtlas: a Float32Array of 4 floats per texel');
    const data = atlas.slice();   // a copy of the bytes: NaN payloads stay
    const src = opts.src ? new Uint32Array(width * height) : null;
    const filled = native.rtDilateAtlas(this._ctx, width >>> 0, height >>> 0, radius >>> 0, data, src);
    this._check(filled, 'dilateAtlas');
    const out = { data, width, height, filled };
    if (src) out.src = src;
    return out;
  }
  // ---- frame denoise (rt_denoise_frame): the G-buffer-guided a-trous filter of the frame of the last compute(), by the frame
  // denoise rule of include/mi355rt.h.  frameDenoiseDesc({passes = 4, step = 1, planeEps, normalCos = 0.9, sigmaLum = 4,
  // demodulate = true, sameInstance = false}) -> the descriptor both calls take.  denoiseFrame(desc) -> {data: a Float32Array of
  // 4 per pixel in the accumulator's format (rgb = radiance, a = 1 where the accumulation weight was > 0), width, height}.
  // setPresentDenoise(desc | null): present() filters the frame first; null restores the plain path.
  static frameDenoiseDesc(opts = {}) {
    if (opts.planeEps === undefined) throw new TypeError('frameDenoiseDesc: opts.planeEps is required');
    const flags = ((opts.demodulate === undefined || opts.demodulate) ? 1 : 0) | (opts.sameInstance ? 2 : 0);
    return Float64Array.of(opts.passes === undefined ? 4 : opts.passes, opts.step === undefined ? 1 : opts.step, flags,
      opts.normalCos === undefined ? 0.9 : opts.normalCos, opts.planeEps, opts.sigmaLum === undefined ? 4 : opts.sigmaLum);
  }
  static _frameDenoiseDesc(desc, what) {
    const d = desc instanceof Float64Array ? desc : WebGPURenderer.frameDenoiseDesc(desc);
    if (d.length !== 6) throw new TypeError(what + ': a descriptor of frameDenoiseDesc()');
    return d;
  }
  denoiseFrame(desc) {
    const data = new Float32Array(this.width * this.height * 4);
    this._check(native.rtDenoiseFrame(this._ctx, WebGPURenderer._frameDenoiseDesc(desc, 'denoiseFrame'), data), 'denoiseFrame');
    return { data, width: this.width, height: this.height };
  }
  setPresentDenoise(desc) {
    const d = (desc === null || desc === undefined) ? null : WebGPURenderer._frameDenoiseDesc(desc, 'setPresentDenoise');
    this._check(native.rtSetPresentDenoise(this._ctx, d), 'setPresentDenoise');
  }
  // ---- frame temporal (rt_set_frame_temporal): the optional stage of the frame denoiser that reprojects last frame's history
  // ahead of the first pass, by the frame temporal rule of include/mi355rt.h.  frameTemporalDesc({maxHistory = 32, varHistory =
  // 4, planeEps, normalCos = 0.9, sameInstance = false}) -> the descriptor.  setFrameTemporal(desc | null): denoiseFrame and a
  // filtered present() run the stage; null restores the plain path; any call drops the history.  resetFrameHistory(): the next
  // frame is a first frame (for a caller who swaps the whole scene).
  static frameTemporalDesc(opts = {}) {
    if (opts.planeEps === undefined) throw new TypeError('frameTemporalDesc: opts.planeEps is required');
    return Float64Array.of((opts.sameInstance ? 1 : 0) | (opts.motion ? 2 : 0), opts.maxHistory === undefined ? 32 : opts.maxHistory,
      opts.varHistory === undefined ? 4 : opts.varHistory, opts.normalCos === undefined ? 0.9 : opts.normalCos, opts.planeEps);
  }
  setFrameTemporal(desc) {
    let d = null;
    if (desc !== null && desc !== undefined) {
      d = desc instanceof Float64Array ? desc : WebGPURenderer.frameTemporalDesc(desc);
      if (d.length !== 5) throw new TypeError('setFrameTemporal: a descriptor of frameTemporalDesc()');
    }
    this._check(native.rtSetFrameTemporal(this._ctx, d), 'setFrameTemporal');
  }
  resetFrameHistory() {
    this._check(native.rtResetFrameHistory(this._ctx), 'resetFrameHistory');
  }
  // ---- frame motion (frameTemporalDesc({..., motion: true}), RT_FRAME_TEMPORAL_MOTION): the temporal stage follows moving
  // instances and skinned surfaces, by the frame motion rule of include/mi355rt.h; set it once a scene is uploaded.
  // setFrameMotionIds(ids): on the upload path, the stable id of the instance at each position of the instance array now
  // uploaded, a permutation of 0 .. n - 1 (the identity after every instance upload; a device-resident world update supplies
  // its own).  readFrameMotion() -> {data: a Float32Array of 8 per pixel {P'.xyz, bits(status)} {N'.xyz, bits(stable id)},
  // width, height}: where every pixel's surface point was in the previous frame.
  setFrameMotionIds(ids) {
    const a = ids instanceof Uint32Array ? ids : Uint32Array.from(ids);
    this._check(native.rtSetFrameMotionIds(this._ctx, a), 'setFrameMotionIds');
  }
  readFrameMotion() {
    const data = new Float32Array(this.width * this.height * 8);
    this._check(native.rtReadFrameMotion(this._ctx, data), 'readFrameMotion');
    return { data, width: this.width, height: this.height };
  }
  // ---- atlas denoise (rt_denoise_atlas): the edge-stopped a-trous filter of a baked atlas.  atlas = 4 floats per texel;
  // points (8 floats each) and texels as bakePoints / bakeAtlasPoints return them for the same atlas.  opts: {planeEps,
  // maxDist (both required, world units), normalCos = 0.9, passes = 3, step = 1}: `passes` passes of the 5 x 5 kernel at tap
  // spacings step, 2 * step, ... (at most 4); a tap counts only where its guide's normal has a dot product >= normalCos with
  // the texel's and its guide's position lies within planeEps of the texel's tangent plane and within maxDist of its position,
  // by the denoise rule of include/mi355rt.h.  Texels without a point are copied.  Result: {data (a new Float32Array), width,
  // height}.
  denoiseAtlas(atlas, width, height, points, texels, opts = {}) {
    if (!(atlas instanceof Float32Array) || atlas.length !== width * height * 4) throw new TypeError('denoiseAtlas: a Float32Array of 4 floats per texel');
    if (!(opts.planeEps !== undefined && opts.maxDist !== undefined)) throw new TypeError('denoiseAtlas: opts.planeEps and opts.maxDist are required');
    const n = texels ? texels.length : 0;
    if (n && (!(points instanceof Float32Array) || !(texels instanceof Uint32Array) || points.length !== 8 * n)) throw new TypeError('denoiseAtlas: points of 8 floats per texel index');
    const data = new Float32Array(width * height * 4);
    this._check(native.rtDenoiseAtlas(this._ctx, width >>> 0, height >>> 0, (opts.step === undefined ? 1 : opts.step) >>> 0,
      (opts.passes === undefined ? 3 : opts.passes) >>> 0, opts.normalCos === undefined ? 0.9 : opts.normalCos, opts.planeEps,
      opts.maxDist, atlas, n ? points : null, n ? texels : null, data), 'denoiseAtlas');
    return { data, width, height };
  }
  // ---- lightmaps (rt_bake_atlas_lightmap, rt_encode_atlas): the finished lightmap in one call - the atlas bake, the filter on
  // the guides the bake already holds on the device, the gutter fill and the encode, with one copy back.  opts as for
  // bakeAtlasIrradiance plus {denoise: null or {planeEps, maxDist, normalCos = 0.9, passes = 3, step = 1}, dilate = 0, format =
  // 'f32'}.  Result: {data, width, height, format, covered, filled} and with stats the gather's .stats.  data is a Float32Array
  // of 4 per texel ('f32': word for word bakeAtlasIrradiance, then denoiseAtlas, then dilateAtlas), a Uint16Array of 4 halves per
  // texel ('f16') or a Uint32Array of one Radiance pixel R | G << 8 | B << 16 | E << 24 per texel ('rgbe').
  static _lightmapFormat(format) {
    const f = { f32: 0, f16: 1, rgbe: 2, rgbe8: 2 }[String(format === undefined ? 'f32' : format).toLowerCase()];
    if (f === undefined) throw new TypeError("lightmap format must be 'f32', 'f16' or 'rgbe'");
    return f;
  }
  static _lightmapArray(texels, f) {
    return f === 1 ? new Uint16Array(texels * 4) : f === 2 ? new Uint32Array(texels) : new Float32Array(texels * 4);
  }
  _bakeLightmap(what, call, layers, entries, width, height, maxDepth, spp, opts) {
    const f = WebGPURenderer._lightmapFormat(opts.format), dn = opts.denoise || null;
    if (dn && !(dn.planeEps !== undefined && dn.maxDist !== undefined)) throw new TypeError(what + ': denoise.planeEps and denoise.maxDist are required');
    const stages = dn ? Float64Array.of(dn.passes === undefined ? 3 : dn.passes, dn.step === undefined ? 1 : dn.step,
      dn.normalCos === undefined ? 0.9 : dn.normalCos, dn.planeEps, dn.maxDist, opts.dilate || 0, f)
      : Float64Array.of(0, 0, 0, 0, 0, opts.dilate || 0, f);
    const data = WebGPURenderer._lightmapArray(layers * width * height, f);
    const r = call(this._ctx, width >>> 0, height >>> 0, (opts.padBase || 0) >>> 0,
      opts.tMax === undefined ? 1e30 : opts.tMax, WebGPURenderer._atlasEntries(entries), opts.atlasUv || null, maxDepth >>> 0,
      spp >>> 0, (opts.seed || 0) >>> 0, stages, data, !!opts.stats);
    if (typeof r === 'number') this._check(r, what);
    const out = { data, width, height, format: ['f32', 'f16', 'rgbe'][f], covered: r.covered, filled: r.filled };
    if (r.stats) out.stats = r.stats;
    return out;
  }
  bakeAtlasLightmap(entries, width, height, maxDepth, spp, opts = {}) {
    return this._bakeLightmap('bakeAtlasLightmap', native.rtBakeAtlasLightmap, 1, entries, width, height, maxDepth, spp, opts);
  }
  // ---- directional lightmaps (rt_bake_atlas_directional_lightmap): the same call around the directional gather.  Result as
  // bakeAtlasLightmap's plus layers = 4: data holds four layers of width * height texels, layer-major; layer k is {sh[k].r,
  // sh[k].g, sh[k].b, w} with the coverage word w of the flat lightmap.  format 'f32' or 'f16'; 'rgbe' is refused (band-1
  // coefficients are signed).  filled is the count of one layer.
  bakeAtlasDirectionalLightmap(entries, width, height, maxDepth, spp, opts = {}) {
    const out = this._bakeLightmap('bakeAtlasDirectionalLightmap', native.rtBakeAtlasDirectionalLightmap, 4, entries, width, height,
      maxDepth, spp, opts);
    out.layers = 4;
    return out;
  }
  // The encode stage alone: atlas = 4 floats per texel, e.g. what dilateAtlas returned.  Result: {data, width, height, format}.
  encodeAtlas(atlas, width, height, format) {
    if (!(atlas instanceof Float32Array) || atlas.length !== width * height * 4) throw new TypeError('encodeAtlas: a Float32Array of 4 floats per texel');
    const f = WebGPURenderer._lightmapFormat(format);
    const data = WebGPURenderer._lightmapArray(width * height, f);
    this._check(native.rtEncodeAtlas(this._ctx, width >>> 0, height >>> 0, f, atlas, data), 'encodeAtlas');
    return { data, width, height, format: ['f32', 'f16', 'rgbe'][f] };
  }
  destroy() { if (this._ctx) { native.rtDestroy(this._ctx); this._ctx = null; } }
}

class WorldBridge {
  constructor() { this._w = null; this._cache = {}; this.hasNewData = false; this.hasNewGeometry = false; this._wh = [-1, -1]; }
  async initWasm() {}
  // world-bridge.ts:109-130; glbData: Uint8Array of a .glb (or .gltf JSON with data URIs)
  async loadScene(sceneName, objSource, glbData) {
    if (this._w) native.msDestroy(this._w);
    this._w = native.msCreate(sceneName, objSource === undefined ? null : objSource, glbData || null);
    // a GLB that does not parse leaves the procedural scene alone (lib.rs:57-67 ignores the error); keep the reason
    this.loadWarning = glbData ? native.msLastError() : '';
    if (this._blasRenderer) native.msSetBlasBuilder(this._w, this._blasRenderer._ctx);
    if (this._deviceRenderer) native.msSetDeviceUpdater(this._w, this._deviceRenderer._ctx);
    this.deviceResident = false;
    this._wh = [-1, -1];
    this._refresh();
    this.hasNewData = true;
    this.hasNewGeometry = true;
  }
  update(time) {
    if (this._blasRenderer && !this._blasRenderer._ctx) throw new Error('the renderer set with setBlasBuilder() has been destroyed');
    if (this._deviceRenderer && !this._deviceRenderer._ctx) throw new Error('the renderer set with setDeviceUpdater() has been destroyed');
    native.msUpdate(this._w, time);
    this.deviceResident = !!native.msDeviceResident(this._w);
    this.deviceWarning = (this._deviceRenderer && !this.deviceResident) ? native.msLastError() : '';
    if (!this._deviceRenderer && this._blasRenderer) {
      const err = native.msLastError();
      if (err) throw new Error(err);   // the GPU builder failed: no silent CPU result
    }
    if (!this.deviceResident) this._refresh();   // a device-resident update leaves the host arrays alone
    this.hasNewData = true; this.hasNewGeometry = true;
  }
  // run the whole per-frame half of update(t) on the GPU, inside `renderer`'s buffers (rt_world_update): skinning, BLAS
  // builds, topology / light / draw-command packing, TLAS, instances; syncWorld() then uploads nothing.  null = host path
  setDeviceUpdater(renderer) {
    this._deviceRenderer = renderer || null;
    if (this._w) native.msSetDeviceUpdater(this._w, renderer ? renderer._ctx : null);
    if (!renderer) this.deviceResident = false;
  }
  // build the BLASes of update(t) on the GPU (rt_build_blas: the CPU builder's tree, byte for byte); null = CPU builder
  setBlasBuilder(renderer) {
    this._blasRenderer = renderer || null;
    if (this._w) native.msSetBlasBuilder(this._w, renderer ? renderer._ctx : null);
  }
  updateCamera(width, height) {
    if (this._wh[0] === width && this._wh[1] === height) return;
    this._wh = [width, height];
    native.msUpdateCamera(this._w, width, height);
    this._cache.camera = native.msGet(this._w, 'camera');
  }
  _refresh() {
    for (const k of ['vertices', 'normals', 'uvs', 'mesh_topology', 'tlas', 'blas', 'instances', 'lights', 'draw_commands', 'camera'])
      this._cache[k] = native.msGet(this._w, k);
  }
  get vertices() { return this._cache.vertices; }
  get normals() { return this._cache.normals; }
  get uvs() { return this._cache.uvs; }
  get mesh_topology() { return this._cache.mesh_topology; }
  get tlas() { return this._cache.tlas; }
  get blas() { return this._cache.blas; }
  get instances() { return this._cache.instances; }
  get lights() { return this._cache.lights; }
  get lightCount() { return this._cache.lights.length / 2; }
  get draw_commands() { return this._cache.draw_commands; }
  get cameraData() { return this._cache.camera; }
  get textureCount() {
    if (!this._w) return 0;
    return native.msEncodedTextureCount(this._w) || native.msTextureCount(this._w);
  }
  // world-bridge.ts:98-99, 161-170
  getAnimationList() { return this._w ? native.msAnimationNames(this._w) : []; }
  loadAnimation(data) { return native.msLoadAnimation(this._w, data); }
  setAnimation(index) { native.msSetAnimation(this._w, index); }
  get hasWorld() { return !!this._w && this._cache.vertices.length > 0; }
  getTextureRGBA(i) { return native.msTexture(this._w, i); }
  // world-bridge.ts:101-106 hands out ENCODED images; the synthetic scenes hold raw texels, so encode them as PNG
  getTexture(i) {
    if (native.msEncodedTextureCount(this._w)) return native.msEncodedTexture(this._w, i);   // glTF input
    const rgba = this.getTextureRGBA(i);
    return rgba ? encodePng(rgba, 1024, 1024) : undefined;
  }
}

// src/main.ts:133-163: the per-frame scene sync of the live loop. Returns true when something was uploaded.
function syncWorld(renderer, bridge, width, height) {
  if (!bridge.hasNewData) return false;
  let rebind = false;
  if (bridge.deviceResident) {   // update(t) ran inside the renderer: only the camera uniforms and the restart remain
    bridge.hasNewGeometry = false;
    bridge.updateCamera(width, height);
    renderer.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount);
    renderer.resetAccumulation();
    bridge.hasNewData = false;
    return true;
  }
  rebind = renderer.updateCombinedBVH(bridge.tlas, bridge.blas) || rebind;
  rebind = renderer.updateBuffer('instance', bridge.instances) || rebind;
  rebind = renderer.updateBuffer('draw_commands', bridge.draw_commands) || rebind;
  if (bridge.hasNewGeometry) {
    rebind = renderer.updateCombinedGeometry(bridge.vertices, bridge.normals, bridge.uvs) || rebind;
    rebind = renderer.updateBuffer('topology', bridge.mesh_topology) || rebind;
    rebind = renderer.updateBuffer('lights', bridge.lights) || rebind;
    bridge.hasNewGeometry = false;
  }
  bridge.updateCamera(width, height);
  renderer.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount);
  if (rebind) renderer.recreateBindGroup();
  renderer.resetAccumulation();
  bridge.hasNewData = false;
  return true;
}

// `renderFrame` of src/main.ts:119-181 without requestAnimationFrame: every updateInterval frames the world advances to
// t = totalFrameCount / updateInterval / 60, the scene is re-synced and the accumulation restarts; each call traces and presents
class LiveLoop {
  constructor(renderer, bridge, width, height, updateInterval = 0) {
    Object.assign(this, { renderer, bridge, width, height, updateInterval, frameCount: 0, totalFrameCount: 0 });
  }
  renderFrame() {
    if (this.updateInterval > 0 && this.frameCount >= this.updateInterval)
      this.bridge.update(this.totalFrameCount / (this.updateInterval || 1) / 60);
    if (syncWorld(this.renderer, this.bridge, this.width, this.height)) this.frameCount = 0;
    this.frameCount++;
    this.totalFrameCount++;
    this.renderer.compute(this.frameCount);
    this.renderer.present();
  }
}

module.exports = { WebGPURenderer, WorldBridge, LiveLoop, syncWorld, encodePng, native };
