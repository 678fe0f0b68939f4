// TypeScript view of index.js: the method surface of the reference classes
// (src/renderer/WebGPURenderer.ts:7-138, src/world-bridge.ts:4-216).
export interface RayQueryStats {
  rays: number; nodes_visited: number; tris_tested: number; walk: number; lds: number; rayreg: number; workgroups: number; kernel_ms: number;
}
export interface RadianceQueryStats {
  rays: number; samples: number; extension_rays: number; shadow_rays: number; shaded_hits: number; nodes_visited: number;
  tris_tested: number; lds: number; workgroups: number; kernel_ms: number;
}

export class WebGPURenderer {
  constructor(device?: number);
  readonly device: { queue: { onSubmittedWorkDone(): Promise<void> } };
  init(): Promise<void>;
  buildPipeline(depth: number, spp: number): void;
  updateScreenSize(width: number, height: number): void;
  resetAccumulation(): void;
  loadTexturesFromWorld(bridge: WorldBridge): Promise<void>;
  updateBuffer(type: "topology" | "instance" | "lights" | "draw_commands", data: Uint32Array | Float32Array): boolean;
  updateCombinedGeometry(v: Float32Array, n: Float32Array, uv: Float32Array): boolean;
  updateCombinedBVH(tlas: Float32Array, blas: Float32Array): boolean;
  updateSceneUniforms(cameraData: Float32Array, frameCount: number, lightCount: number): void;
  recreateBindGroup(): void;
  compute(frameCount: number): void;
  computeBatch(frameCounts: ArrayLike<number>): void;
  present(): void;
  captureFrame(): Promise<{ data: ArrayBufferLike; width: number; height: number }>;
  readAccum(): Float32Array;
  getCounters(): Record<string, number>;
  /** compute() traces only rows y with floor(y / stripeRows) % count === rank */
  setStripes(stripeRows: number, rank: number, count: number): void;
  /** ncclGetUniqueId: rank 0 makes the 128 bytes and the host hands them to the other ranks */
  static distUniqueId(): Uint8Array;
  static deviceCount(): number;
  /** become rank `rank` of `world` of one sharded image; uniqueId given: RCCL gather, else the host moves the blocks */
  distInit(rank: number, world: number, stripeRows?: number, uniqueId?: Uint8Array | null): void;
  distShutdown(): void;
  /** bytes of one rank's compact block at the current size */
  distBlockBytes(): number;
  /** enqueue: accumulator -> this rank's compact block */
  packStripes(): void;
  /** this rank's packed block (blocking) */
  readBlock(): Float32Array;
  /** rank 0: the block of `fromRank` into its receive slot */
  writeBlock(fromRank: number, block: Float32Array | Uint8Array): void;
  /** rank 0, enqueue: all receive blocks -> the display buffer present() reads */
  unpackStripes(): void;
  /** pack -> RCCL gather to rank 0 -> unpack on the context's stream; collective */
  gatherStripes(): void;
  /** rank 0: the assembled float4 image (blocking) */
  readDisplay(): Float32Array;
  /** Ray casts against the uploaded scene (rt_trace_rays): 8 floats per ray {origin, tMax, direction, -}.  Closest hit: a miss
   *  is {the ray's tMax, -1, -1, 0}; anyHit: {0, -1, -1, occluded}.  `words` are the raw 16-byte hit records. */
  traceRays(rays: Float32Array, opts?: { anyHit?: boolean; tMin?: number; stats?: boolean }):
    { t: Float32Array; tri: Int32Array; inst: Int32Array; hit: Uint32Array; words: Uint32Array; stats?: RayQueryStats };
  rayQueryStats(): RayQueryStats;
  /** The path tracer's radiance along the caller's rays (rt_trace_radiance): 8 words per ray {origin, tMax, direction, pad},
   *  pad = the bits of a uint32, the ray's RNG stream id.  `data` holds 4 floats per ray {r, g, b, t}; a miss is
   *  {0, 0, 0, the ray's tMax}. */
  traceRadiance(rays: Float32Array, maxDepth: number, spp: number, opts?: { seed?: number; stats?: boolean }):
    { data: Float32Array; n: number; stats?: RadianceQueryStats };
  /** Irradiance gathers at the caller's surface points (rt_gather_irradiance): 8 words per point {position, tMax, normal, pad},
   *  pad = the bits of a uint32 below 2^31, the point's RNG stream id.  `data` holds 4 floats per point {r, g, b, hitFraction}:
   *  the cosine-weighted mean incoming radiance (E / pi) over spp directions drawn on the device, and the fraction of them
   *  that hit something within tMax.  The stats are a radiance query's with rays = points. */
  gatherIrradiance(points: Float32Array, maxDepth: number, spp: number, opts?: { seed?: number; stats?: boolean }):
    { data: Float32Array; n: number; stats?: RadianceQueryStats };
  /** Probe gathers (rt_gather_probes): 8 words per probe {position, tMax, 3 unused words, pad}, pad = the bits of a uint32
   *  below 2^31, the probe's RNG stream id.  `data` holds 28 floats per probe: the SH9 projection of the radiance arriving
   *  over spp uniform sphere directions drawn on the device, sh[k][c] at 3 k + c, then hitFraction.  The stats are a radiance
   *  query's with rays = probes; kernel_ms counts the radiance launches only. */
  gatherProbes(probes: Float32Array, maxDepth: number, spp: number, opts?: { seed?: number; stats?: boolean }):
    { data: Float32Array; n: number; stats?: RadianceQueryStats };
  /** Irradiance volumes (rt_bake_volume / rt_sample_volume / rt_encode_volume).  A descriptor is the 64 bytes of an
   *  rt_volume_desc; probe (x, y, z) of the dims grid sits at origin + (x, y, z) * step and is record (z * ny + y) * nx + x. */
  static volumeDesc(o: { origin: number[]; step: number[]; dims: number[]; window?: number[]; tMax?: number; padFirst?: number;
    maxHitFraction?: number }): Uint8Array;
  /** `data` holds 28 floats per probe: irradiance coefficients (the probe gather times the cosine-lobe band factors and the
   *  window), then hitFraction.  The stats are the probe gather's. */
  bakeVolume(desc: Uint8Array, maxDepth: number, spp: number, opts?: { seed?: number; stats?: boolean }):
    { data: Float32Array; n: number; stats?: RadianceQueryStats };
  /** points: 8 words per point {position, -, normal, -}.  `data` holds 4 floats per point {r, g, b, W}: the irradiance at the
   *  normal from the eight surrounding valid probes and the valid share of the interpolation weight.  Needs no scene. */
  sampleVolume(desc: Uint8Array, volume: Float32Array, points: Float32Array): { data: Float32Array; n: number };
  /** Seven layers of n texels, layer j holding the floats 4 j .. 4 j + 3 of every record; 'rgbe' is refused. */
  encodeVolume(desc: Uint8Array, volume: Float32Array, format: 'f32' | 'f16'):
    { data: Float32Array | Uint16Array; layers: 7; n: number; format: string };
  /** Probe visibility maps (rt_bake_volume_visibility / rt_sample_volume_visible / rt_encode_volume_visibility).  A descriptor
   *  is the 32 bytes of an rt_volume_visibility_desc: maps of size x size octahedral texels {mean distance, mean squared
   *  distance} per probe of a volume, spt samples per texel, maxDistance the length of every visibility ray. */
  static volumeVisibilityDesc(o: { size: number; maxDistance: number; spt?: number; normalBias?: number; minVisibility?: number;
    crushThreshold?: number; backface?: boolean }): Uint8Array;
  /** `data` holds 2 floats per texel, probe-major, texel (i, j) of a map at j * size + i.  The stats are a ray query's, summed
   *  over the batches. */
  bakeVolumeVisibility(desc: Uint8Array, vis: Uint8Array, opts?: { seed?: number; stats?: boolean }):
    { data: Float32Array; n: number; size: number; stats?: RayQueryStats };
  /** sampleVolume with every corner probe's weight multiplied by its visibility of the point.  Needs no scene. */
  sampleVolumeVisible(desc: Uint8Array, vis: Uint8Array, volume: Float32Array, visibility: Float32Array, points: Float32Array):
    { data: Float32Array; n: number };
  /** One image of bordered tiles, probe (x, y, z) at tile (x, z * ny + y), 2 channels per texel; 'rgbe' is refused. */
  encodeVolumeVisibility(desc: Uint8Array, vis: Uint8Array, visibility: Float32Array, format: 'f32' | 'f16'):
    { data: Float32Array | Uint16Array; width: number; height: number; tile: number; format: string };
  /** Reflection probes (rt_bake_reflection / rt_filter_reflection).  A descriptor is the 32 bytes of an rt_reflection_desc:
   *  level 0 of size x size octahedral texels {r, g, b, hitFraction}, `levels` levels with level m of side size >> m,
   *  GGX-filtered at the roughness m / (levels - 1); spt samples per texel of a capture, filterSamples lobe samples per texel. */
  static reflectionDesc(o: { size: number; levels: number; spt?: number; filterSamples?: number }): Uint8Array;
  /** levels + 1 texel offsets of a chain's levels; the last is the length of a chain. */
  static reflectionLevelOffsets(desc: Uint8Array): number[];
  /** `data` holds a chain per probe, 4 floats per texel.  The stats are a radiance query's with rays = texels. */
  bakeReflection(desc: Uint8Array, probes: Float32Array, maxDepth: number, opts?: { seed?: number; stats?: boolean }):
    { data: Float32Array; n: number; chainTexels: number; offsets: number[]; stats?: RadianceQueryStats };
  /** maps: size * size texels of 4 floats per probe; level 0 of each chain is its map word for word.  Needs no scene. */
  filterReflection(desc: Uint8Array, maps: Float32Array): { data: Float32Array; n: number; chainTexels: number; offsets: number[] };
  /** One encodeAtlas result per level of ONE chain; all three formats apply. */
  encodeReflection(desc: Uint8Array, chain: Float32Array, format: 'f32' | 'f16' | 'rgbe'):
    { data: Float32Array | Uint16Array | Uint32Array; width: number; height: number; format: string }[];
  /** The reflection sampler (rt_sample_reflection).  A descriptor is the 32 bytes of an rt_reflection_sample_desc: the size
   *  and levels of the chains, and whether directions are bent to where they leave the probe's box. */
  static reflectionSampleDesc(o: { size: number; levels: number; parallax?: boolean }): Uint8Array;
  /** chains: whole chains, 4 floats per texel; queries: 8 floats per query {position, probe index as u32 bits, direction,
   *  roughness}; probes and boxes: 8 floats per chain, read with parallax only.  `data` holds 4 floats {r, g, b, hitFraction}
   *  per query: the seam-aware bilinear fetch from the two levels around roughness * (levels - 1).  Needs no scene. */
  sampleReflection(desc: Uint8Array, chains: Float32Array, queries: Float32Array, opts?: { probes?: Float32Array; boxes?: Float32Array }):
    { data: Float32Array; n: number };
  /** Directional gathers (rt_gather_directional): points as for gatherIrradiance.  `data` holds 16 floats per point, four rows
   *  {sh[k].r, sh[k].g, sh[k].b, hitFraction}: the projection of the radiance arriving over spp uniform directions on the
   *  hemisphere of the normal onto Y0 and the y, z, x harmonics of band 1, in world space; row k is the texel of atlas layer k.
   *  The stats are a radiance query's with rays = points; kernel_ms counts the radiance launches only. */
  gatherDirectional(points: Float32Array, maxDepth: number, spp: number, opts?: { seed?: number; stats?: boolean }):
    { data: Float32Array; n: number; stats?: RadianceQueryStats };
  /** Lightmap bakes (rt_bake_points): the covered texels of TLAS-order instance `inst`'s width x height atlas as gather points,
   *  in ascending texel index; pad = padBase + texel index.  atlasUv: 2 floats per scene vertex, overriding the scene's uvs.
   *  owner: the Int32Array owner map (global triangle index, -1 = uncovered). */
  bakePoints(inst: number, width: number, height: number,
             opts?: { tMax?: number; padBase?: number; atlasUv?: Float32Array | null; owner?: boolean }):
    { n: number; points: Float32Array; texels: Uint32Array; owner?: Int32Array };
  /** The whole bake (rt_bake_irradiance): points, the irradiance gather on them, scatter.  `data` holds 4 floats per texel
   *  {r, g, b, hitFraction}, row 0 first; rgb is E / pi (multiply by pi * albedo), uncovered texels are {0, 0, 0, -1}. */
  bakeIrradiance(inst: number, width: number, height: number, maxDepth: number, spp: number,
                 opts?: { tMax?: number; padBase?: number; atlasUv?: Float32Array | null; seed?: number; stats?: boolean }):
    { data: Float32Array; width: number; height: number; covered: number; stats?: RadianceQueryStats };
  /** Atlas bakes (rt_bake_atlas_points): every entry [inst, x, y, w, h] bakes TLAS-order instance `inst` at w x h texels
   *  into the rectangle at (x, y) of one width x height atlas; the lowest entry owns a texel several cover.  texels are atlas
   *  texel indices, ascending; pad = padBase + atlas texel index.  owner: 2 words per texel {entry, global triangle index},
   *  {-1, -1} = uncovered. */
  bakeAtlasPoints(entries: number[][] | Uint32Array, width: number, height: number,
                  opts?: { tMax?: number; padBase?: number; atlasUv?: Float32Array | null; owner?: boolean }):
    { n: number; points: Float32Array; texels: Uint32Array; owner?: Int32Array };
  /** The whole atlas bake (rt_bake_atlas_irradiance): the points of all entries, one irradiance gather, scatter. */
  bakeAtlasIrradiance(entries: number[][] | Uint32Array, width: number, height: number, maxDepth: number, spp: number,
                      opts?: { tMax?: number; padBase?: number; atlasUv?: Float32Array | null; seed?: number; stats?: boolean }):
    { data: Float32Array; width: number; height: number; covered: number; stats?: RadianceQueryStats };
  /** Atlas dilation (rt_dilate_atlas): every uncovered texel (fourth float < 0 or NaN) within `radius` (0 .. 24) texels of a
   *  covered one receives the first three words of the nearest covered texel, the lowest texel index among equally near
   *  ones, and -2 as its fourth.  `data` is a new array; `src` the source map (own index in covered texels, the source's in
   *  filled ones, 0xffffffff elsewhere). */
  dilateAtlas(atlas: Float32Array, width: number, height: number, radius: number, opts?: { src?: boolean }):
    { data: Float32Array; width: number; height: number; filled: number; src?: Uint32Array };
  /** Frame denoise (rt_denoise_frame): the descriptor of denoiseFrame / setPresentDenoise - `passes` passes (1 .. 5) of the
   *  5 x 5 a-trous kernel at tap spacings step, 2 * step, ... (at most 16), taps accepted by normal (normalCos), tangent plane
   *  (planeEps, world units) and - sigmaLum > 0 - luminance; demodulate filters radiance / albedo. */
  static frameDenoiseDesc(opts: { planeEps: number; passes?: number; step?: number; normalCos?: number; sigmaLum?: number;
                                  demodulate?: boolean; sameInstance?: boolean }): Float64Array;
  /** The filtered frame of the last compute(): 4 floats per pixel, rgb = radiance, a = 1 where the accumulation weight was > 0. */
  denoiseFrame(desc: Float64Array | object): { data: Float32Array; width: number; height: number };
  /** present() filters the frame first (null: the plain path). */
  setPresentDenoise(desc: Float64Array | object | null): void;
  /** Frame temporal (rt_set_frame_temporal): the descriptor of setFrameTemporal - a pixel's history grows to maxHistory frames
   *  (1 .. 256), the variance is the temporal one from varHistory frames on, history taps are accepted by normal (normalCos) and
   *  tangent plane (planeEps, world units). */
  static frameTemporalDesc(opts: { planeEps: number; maxHistory?: number; varHistory?: number; normalCos?: number;
                                   sameInstance?: boolean; motion?: boolean }): Float64Array;
  /** denoiseFrame and a filtered present() reproject and blend last frame's history first (null: the plain path). */
  setFrameTemporal(desc: Float64Array | object | null): void;
  /** Drop the temporal stage's history: the next frame is a first frame. */
  resetFrameHistory(): void;
  /** Frame motion (frameTemporalDesc({motion: true})): the stable id of the instance at each position of the uploaded instance
   *  array, a permutation of 0 .. n - 1; the identity after every instance upload. */
  setFrameMotionIds(ids: Uint32Array | number[]): void;
  /** The carry plane of the last run of the motion stage: 8 floats per pixel, {P'.xyz, bits(status)} {N'.xyz, bits(stable id)}. */
  readFrameMotion(): { data: Float32Array; width: number; height: number };
  /** Atlas denoise (rt_denoise_atlas): `passes` passes of the 5 x 5 a-trous kernel at tap spacings step, 2 * step, ... (at
   *  most 4), guided by the points of bakePoints / bakeAtlasPoints for the same atlas: a tap counts only where its normal has
   *  a dot product >= normalCos with the texel's and its position lies within planeEps of the texel's tangent plane and
   *  within maxDist of its position.  Texels without a point are copied.  `data` is a new array. */
  denoiseAtlas(atlas: Float32Array, width: number, height: number, points: Float32Array | null, texels: Uint32Array | null,
               opts: { planeEps: number; maxDist: number; normalCos?: number; passes?: number; step?: number }):
    { data: Float32Array; width: number; height: number };
  /** The finished lightmap in one call (rt_bake_atlas_lightmap): the atlas bake, the filter on the guides the bake already
   *  holds on the device, the gutter fill and the encode, with one copy back.  'f32': 4 floats per texel, word for word
   *  bakeAtlasIrradiance -> denoiseAtlas -> dilateAtlas; 'f16': 4 halves per texel; 'rgbe': one Radiance pixel R | G << 8 |
   *  B << 16 | E << 24 per texel, 0 where there is no surface and nothing was filled. */
  bakeAtlasLightmap(entries: number[][] | Uint32Array, width: number, height: number, maxDepth: number, spp: number,
                    opts?: { tMax?: number; padBase?: number; atlasUv?: Float32Array | null; seed?: number; stats?: boolean;
                             denoise?: { planeEps: number; maxDist: number; normalCos?: number; passes?: number; step?: number } | null;
                             dilate?: number; format?: 'f32' | 'f16' | 'rgbe' }):
    { data: Float32Array | Uint16Array | Uint32Array; width: number; height: number; format: 'f32' | 'f16' | 'rgbe';
      covered: number; filled: number; stats?: RadianceQueryStats };
  /** The finished directional lightmap in one call (rt_bake_atlas_directional_lightmap): as bakeAtlasLightmap around the
   *  directional gather.  `data` holds four layers of width * height texels, layer-major; layer k is {sh[k].r, sh[k].g,
   *  sh[k].b, w}, filtered, gutter-filled and encoded like a flat lightmap.  'rgbe' is refused: band-1 coefficients are signed.
   *  `filled` is the count of one layer (all four are equal). */
  bakeAtlasDirectionalLightmap(entries: number[][] | Uint32Array, width: number, height: number, maxDepth: number, spp: number,
                    opts?: { tMax?: number; padBase?: number; atlasUv?: Float32Array | null; seed?: number; stats?: boolean;
                             denoise?: { planeEps: number; maxDist: number; normalCos?: number; passes?: number; step?: number } | null;
                             dilate?: number; format?: 'f32' | 'f16' }):
    { data: Float32Array | Uint16Array; width: number; height: number; layers: 4; format: 'f32' | 'f16';
      covered: number; filled: number; stats?: RadianceQueryStats };
  /** The encode stage alone (rt_encode_atlas) on any atlas of 4 floats per texel.  `data` is a new array. */
  encodeAtlas(atlas: Float32Array, width: number, height: number, format: 'f32' | 'f16' | 'rgbe'):
    { data: Float32Array | Uint16Array | Uint32Array; width: number; height: number; format: 'f32' | 'f16' | 'rgbe' };
  destroy(): void;
}
export class WorldBridge {
  hasNewData: boolean;
  hasNewGeometry: boolean;
  initWasm(): Promise<void>;
  loadScene(sceneName: string, objSource?: string, glbData?: Uint8Array): Promise<void>;
  update(time: number): void;
  updateCamera(width: number, height: number): void;
  readonly vertices: Float32Array;
  readonly normals: Float32Array;
  readonly uvs: Float32Array;
  readonly mesh_topology: Uint32Array;
  readonly tlas: Float32Array;
  readonly blas: Float32Array;
  readonly instances: Float32Array;
  readonly lights: Uint32Array;
  readonly lightCount: number;
  readonly draw_commands: Uint32Array;
  readonly cameraData: Float32Array;
  readonly textureCount: number;
  readonly hasWorld: boolean;
  getTextureRGBA(index: number): Uint8Array | undefined;
  /** build the BLASes of update(t) on the GPU with this renderer (same tree as the CPU builder); null restores the CPU builder */
  setBlasBuilder(renderer: WebGPURenderer | null): void;
  /** the whole per-frame half of update(t) on the GPU (rt_world_update); the host arrays are then not refreshed */
  setDeviceUpdater(renderer: WebGPURenderer | null): void;
  deviceResident: boolean;
  deviceWarning: string;
  getAnimationList(): string[];
  loadAnimation(data: Uint8Array): number;
  setAnimation(index: number): void;
  /** why a GLB passed to loadScene was ignored ('' when it loaded) */
  loadWarning: string;
  /** encoded image bytes (PNG / JPEG), as world-bridge.ts:101-106 hands them out */
  getTexture(index: number): Uint8Array | undefined;
}

/** src/main.ts:133-163 — re-upload what the bridge marks as new, reset the accumulation; true when something was uploaded */
export function syncWorld(renderer: WebGPURenderer, bridge: WorldBridge, width: number, height: number): boolean;
/** RGBA8 rows, top first -> the bytes of a PNG file (colour type 6). */
export function encodePng(rgba: Uint8Array, width: number, height: number): Uint8Array;
/** `renderFrame` of src/main.ts:119-181 */
export class LiveLoop {
  constructor(renderer: WebGPURenderer, bridge: WorldBridge, width: number, height: number, updateInterval?: number);
  frameCount: number;
  totalFrameCount: number;
  renderFrame(): void;
}
