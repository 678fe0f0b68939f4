// The persistent path-trace kernel, written once and compiled under five names (k_pathtrace.hip.h includes this file five
// times, inside namespace rtk): RT_PT_KERNEL is the kernel's name, RT_PT_WAVES its waves per workgroup, RT_PT_SIMD_WAVES the
// waves per SIMD of its launch bounds (an expression that may use the template parameters) and RT_PT_PLAIN whether it is the
// form for scenes of plain materials.  RT_PT_SWEEP: whether the walks sweep the BLAS leaves (k_traverse.hip.h traverse_leaves);
// such a form takes RT_PT_SWEEP_PARAMS behind the common parameters, the leaf and node records and their numbers, and RT_PT_SWEEP_ARG
// makes the walk's LeafSweep of them (the other forms define both empty, and keep their parameter list).  No include guard.
// ONE_INST (LDS form only): the scene's TLAS is a single leaf (k_traverse.hip.h traverse<.., ONE_INST>).  Every hit is then in
// the one instance, and what a trip would compute from (instance, triangle) alone is read from the per-triangle world
// records the host built at upload time behind the shading records (k_prepare_world_tris: Sg.tri_shade + 8 * n_tris).
template <bool DETAIL, bool LDS, bool ONE_INST = false>
__global__ __launch_bounds__(64 * RT_PT_WAVES, RT_PT_SIMD_WAVES) void RT_PT_KERNEL(DevScene Sg, DevFrame F, rt_scene_uniforms U,
                                                              uint32_t* __restrict__ ticket, uint32_t n_nodes_total,
                                                              uint32_t n_tris_total, uint32_t n_inst_total,
                                                              uint32_t n_verts_total,
                                                              const DevFrameSlot* __restrict__ slots, uint32_t n_slots,
                                                              LdsPlan plan RT_PT_SWEEP_PARAMS) {
  // Batched dispatch (rt_compute_batch): the launch covers n_slots consecutive compute() frames. The work item is
  // one (frame, pixel): tickets enumerate (frame, tile) pairs, so a launch has n_slots times as many tickets and the
  // persistent waves stay fed and balanced even when a rank owns 1/8 of the image. With n_slots > 1 every item
  // writes its frame colour to F.frame_col and k_accumulate_frames adds the frames in frame order afterwards, which
  // makes the result bit-identical to n_slots separate dispatches; with n_slots == 1 the item accumulates directly.
  // LEAN: the one-leaf form runs at RT_PT_ONE_INST_WAVES = 5 waves per SIMD, 96 VGPRs (the other forms keep their code).
  // The wave-uniform ticket is read into a scalar register, and the sizes the trip divides by are taken as new values where
  // they are used (rt_fresh), so that the compiler does not compute their conversions and reciprocals once before the loop
  // and carry them, wave-uniform, in a dozen VGPRs through the whole kernel.
  constexpr bool LEAN = ONE_INST;
  // SLIM: the 8-wave form runs at RT_PT_WIDE_WAVES = 6 waves per SIMD, 80 VGPRs.  Two values of the path live outside
  // registers between the moments they are used: the sample sum p.col, read and written once per sample, sits in LDS
  // behind the wave queues (col_park), and the pixel index p.pixel is recomputed from pixel_xy.
  constexpr uint32_t WAVES = RT_PT_WAVES;   // per workgroup; they share one staged scene
  constexpr bool SLIM = WAVES == 8;
  // ONE_PASS: one surface-frame pass per trip, at the head of the shade section, for the lanes that have just started a
  // sample and the lanes whose extension ray of the last trip found a hit together; neither start_sample nor the code behind
  // the extension walk makes a frame.  The camera is read as new where a sample starts (fresh_camera_basis).
  constexpr bool ONE_PASS = ONE_INST;
  // PLAIN (RT_PT_PLAIN, the includer's): surface frame and bounce without the materials the host has seen the scene not to
  // have (setup_surface, shade_bounce).  The product one-leaf form only.
  constexpr bool PLAIN = RT_PT_PLAIN;
  static_assert(!PLAIN || (ONE_INST && LDS && !DETAIL), "the plain form is a product one-leaf form");
  // SWEEP (RT_PT_SWEEP, the includer's): the host has seen that the BLAS is sweepable (scene_facts.h walk_facts); both walks
  // of a trip test its leaves alone.  A product one-leaf form only.
  constexpr bool SWEEP = RT_PT_SWEEP;
  static_assert(!SWEEP || (ONE_INST && LDS && !DETAIL), "a sweep form is a product one-leaf form");
  extern __shared__ f4 s_scene[];
  // per-wave triangle work queue at the start of LDS, staged scene after it
  // (LEAN: the wave's index in a scalar register, and so the addresses of its queue)
  const uint32_t wave = LEAN ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6;
  WaveWork WW;
  {
    wave_work_at(WW, reinterpret_cast<char*>(s_scene) + wave * RT_WORK_BYTES_PER_WAVE);
  }
  // first slot behind the wave queues (SLIM: and the parked sample sums)
  const uint32_t rec0 = (WAVES * (RT_WORK_BYTES_PER_WAVE + (SLIM ? RT_PT_COL_BYTES_PER_WAVE : 0u))) / 16;
  TravMem M;
  DevScene S = Sg;
  const float4* wrec = nullptr;   // ONE_INST: the staged world records
  if (LDS) {
    // Small scene: the whole scene (traversal records AND the arrays shading reads) lives in LDS,
    // staged once per workgroup; only textures, the G-buffer and the accumulation buffer stay in HBM.
    // (The non-ONE_INST layout is that of stage_whole_scene, k_pathtrace.hip.h: keep the two in step.)
    uint32_t slot = rec0;
    auto stage = [&](const void* src, size_t n) {
      f4* base = s_scene + slot;
      lds_stage(base, src, n);
      slot += (uint32_t)n;
      if (LEAN) slot = __builtin_amdgcn_readfirstlane(slot);   // else the compiler carries the LDS addresses of S in VGPRs
      return base;
    };
    M.gnodes = M.gtri = M.ginst = nullptr;
    M.groot = nullptr;
    M.k_lds = n_nodes_total;
    M.t_min = RT_T_MIN;
    M.l_nodes = slot;
    f4* ln = stage(Sg.tnodes, (size_t)2 * n_nodes_total);
    M.l_tri = slot;
    f4* lt = stage(Sg.tri_geom, (size_t)RT_TRI_STRIDE * n_tris_total);
    M.l_inst = slot;
    f4* li = stage(Sg.inst_trav, (size_t)4 * n_inst_total);
    M.l_root = slot;
    stage(Sg.inst_root, ((size_t)n_inst_total + 3) / 4);
    // ONE_INST: the two slots of world record per triangle lie behind the shading records, and come along
    S.tri_shade = reinterpret_cast<const float4*>(stage(Sg.tri_shade, (size_t)(ONE_INST ? 10 : 8) * n_tris_total));
    if constexpr (ONE_INST) {
      // topo, pos, uv and inst have no reader in these forms: light_pdf takes the world record, sample_light the shading
      // record (one_leaf_lds_slots, launch_plan.h)
      wrec = S.tri_shade + 8 * n_tris_total;
    } else {
      S.topo = reinterpret_cast<const float4*>(stage(Sg.topo, (size_t)5 * n_tris_total));
      S.pos = reinterpret_cast<const float4*>(stage(Sg.pos, n_verts_total));   // S.nrm stays in global memory: no reader left here
      // uv (8 B/vertex) and lights (8 B each): the device buffers are allocated with >= 16-byte slack
      S.uv = reinterpret_cast<const float2*>(stage(Sg.uv, ((size_t)n_verts_total + 1) / 2));
      S.inst = reinterpret_cast<const float4*>(stage(Sg.inst, (size_t)9 * n_inst_total));
    }
    S.lights = reinterpret_cast<const uint2*>(stage(Sg.lights, ((size_t)Sg.n_lights + 1) / 2));
    S.light_rec = reinterpret_cast<const float4*>(stage(Sg.light_rec, (size_t)4 * Sg.n_lights));
    __syncthreads();
    S.tnodes = reinterpret_cast<const float4*>(ln);
    S.tri_geom = reinterpret_cast<const float4*>(lt);
    S.inst_trav = reinterpret_cast<const float4*>(li);
  } else {
    trav_stage_mixed(M, s_scene, rec0, Sg, plan, n_tris_total, n_inst_total);
    __syncthreads();
  }
  constexpr int MODE = LDS ? RT_TRAV_LDS : RT_TRAV_MIXED;

#ifdef RT_CLOCK_STAMP
  const unsigned long long stamp_c0 = __builtin_amdgcn_s_memtime(), stamp_r0 = __builtin_amdgcn_s_memrealtime();
#endif
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t tiles_x = (U.width + 7u) / 8u;
  // tickets enumerate only the tile rows this rank owns when the stripes are tile-aligned
  const uint32_t n_tiles = tiles_x * (F.own_period ? F.own_tile_rows : (U.height + 7u) / 8u);
  const CameraBasis cam = camera_basis(U);

  // wave-uniform work cursor: pixels [tile_pos, 64) of the wave's tile are still unassigned; the tile's origin and frame are
  // worked out once per ticket (two divisions by run-time values, 20 instructions each: not once per regenerated lane)
  uint32_t tile_pos = 64u, tile_x0 = 0u, tile_y0 = 0u, tile_slot = 0u;
  // PREPASS (the wide one-leaf form): the cursor is a lane mask instead, bit i set while slot i of the wave's tile is a pixel
  // with a path to trace that no lane has taken yet (part (a) below).  The 256-thread one-leaf forms hold their registers
  // with it too, but a single-frame dispatch has 1.3 tickets per wave and the Cornell live loop without lookahead did not
  // gain (0.874 -> 0.880 ms per frame, one run each): they keep the cursor.
  constexpr bool PREPASS = LEAN && SLIM;
  unsigned long long tile_live = 0ull;
  uint32_t tile_xy0 = 0u;   // PREPASS: the tile's origin, x0 | y0 << 16
  uint32_t ticket_next = 0xffffffffu;   // PREPASS: the second ticket of the pair the wave drew, or none
  bool work_left = true;

  PathState p = idle_path();
  uint32_t item_slot = 0u;  // frame of the batch the lane's current (frame, pixel) item belongs to
  uint32_t pixel_xy = 0u;   // x | y << 16 of p.pixel
  bool alive = false;       // lane owns a running path
  bool have_pixel = false;  // lane owns a pixel whose samples are not all done
  // cnt_ext, cnt_shadow: rays of the whole wave, wave-uniform (scalar registers); the others count per lane
  uint32_t cnt_ext = 0, cnt_shadow = 0, cnt_nodes = 0, cnt_tris = 0, cnt_shaded = 0;

#ifdef RT_PT_STAMPS
  unsigned long long pt_cyc[6] = {0, 0, 0, 0, 0, 0}, pt_trips = 0;
#endif
  for (;;) {
#ifdef RT_PT_STAMPS
    const unsigned long long ps0 = __builtin_amdgcn_s_memtime();
#endif
    // ------------------------------------------------------------ regenerate
    // (a) wave-wide: every lane without a pixel takes the next unassigned one of the wave's tile.
    //     All lanes execute this loop (busy lanes with need = false) so that the wave-uniform cursor
    //     (tile, tile_pos, work_left) stays identical in every lane.
    //     A lane keeps a pixel only if the pixel has a path to trace.  It reads the pixel's G-buffer depth here; a
    //     background pixel (or every pixel, when MAX_DEPTH = 0: start_sample's test) is finished at once with colour +0,
    //     and the lane takes the next slot in the same refill instead of sitting out a whole trip; so does a lane whose
    //     slot is outside the image or the rank's rows.  A background sample draws no random number, traces nothing and
    //     counts nothing, and +0 summed over the samples is +0, so the pixel gets the bits it got from a lane trip per
    //     sample.
    //     PREPASS: the depth test is made once per ticket for the whole tile, not once per refill for the slots the refill
    //     reaches.  When the wave takes a ticket, lane i stands for slot i of the tile: it reads its own pixel's depth (one
    //     coalesced load per tile row), finishes the pixel there if it is background, and the wave keeps the ballot of the
    //     others in tile_live.  A refill hands the r-th set bit of tile_live to the r-th needy lane and clears the bits it
    //     handed out; it issues no global load and goes round the loop only when a tile runs out while lanes are needy.
    //     The image cannot change: which lane traces a pixel has no effect on the result (the RNG is seeded from pixel,
    //     frame and sample; the parked sums are private to a lane; the counters are sums); a background pixel draws
    //     nothing, traces nothing, counts nothing and gets the same {+0, +0, +0, 1} at the same address whichever lane
    //     stores it; a batched dispatch writes frame_col, a single one adds +0 to accum or overwrites it: both per pixel.
    if constexpr (PREPASS) {
      bool need = !alive && !have_pixel;
      for (;;) {
        const unsigned long long mask = __ballot(need);
        if (mask == 0ull || !work_left) break;
        if (tile_live == 0ull) {
          // tickets are drawn two at a time, half the atomic round trips: the second waits in ticket_next and is range-checked
          // like the first when its turn comes (a launch has far fewer than 2^32 - 1 tickets, the value that says "none")
          uint32_t t = ticket_next;
          ticket_next = 0xffffffffu;
          if (t == 0xffffffffu) {
            const int leader = __builtin_ctzll(mask);
            if (lane == (uint32_t)leader) t = atomicAdd(ticket, 2u);
            t = __builtin_amdgcn_readlane(t, leader);
            ticket_next = t + 1u;
          }
          if (t >= n_tiles * n_slots) {
            work_left = false;
            break;
          }
          // frame-major ticket: frame = t / n_tiles, tile = t % n_tiles
          tile_slot = t / n_tiles;
          const uint32_t tile_in_frame = t - tile_slot * n_tiles;
          uint32_t trow = tile_in_frame / tiles_x;
          const uint32_t tx0 = (tile_in_frame - trow * tiles_x) * 8u;
          if (F.own_period) trow = (trow / F.own_run) * F.own_period + F.own_first + (trow % F.own_run);
          // the origin as x0 | y0 << 16, one scalar register (width, height <= 65535: rt_resize refuses more; x0 + 7 and
          // y0 + 7 stay below 65536, so a slot's offset adds to the pair without a carry between the halves)
          tile_xy0 = tx0 | (trow * 8u) << 16;
          // the tile's prepass: lane i looks at slot i (the lane number taken as new: what is computed from it here is not
          // carried in registers through the trip)
          uint32_t slot_of_lane = lane;
          asm volatile("" : "+v"(slot_of_lane));
          const uint32_t xy = tile_xy0 + ((slot_of_lane & 7u) | (slot_of_lane >> 3) << 16);
          const uint32_t x = xy & 0xffffu, y = xy >> 16;
          bool live = false;
          if (x < U.width && y < U.height && owns_row(fresh_stripes(F), y)) {
            const uint32_t pixel = y * rt_fresh(U.width) + x;
            // (MAX_DEPTH taken as new and the depth plane named global memory, as in the cursor form below)
            const float gdepth = __builtin_bit_cast(float, ld_g32(reinterpret_cast<const uint32_t*>(slots[tile_slot].depth), pixel));
            if (!(gdepth >= 1.0f) && rt_fresh(F.max_depth) != 0u) {   // (this form of the test: a NaN depth is live)
              live = true;
            } else {
              finish_black_pixel(F, U, slots, tile_slot, pixel);
            }
          }
          tile_live = __ballot(live);
          if (tile_live == 0ull) continue;   // nothing to trace in this tile: the next ticket
        }
        // The r-th needy lane takes the r-th live slot.  The live slots' numbers go through the start of the wave's triangle
        // queue (WW.items), which is idle outside the walks: the lane that stands for the j-th set bit of tile_live writes
        // its number to word j, the needy lane of rank r reads word r.  (The LDS executes a wave's instructions in order.)
        const uint32_t rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        const uint32_t ord =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(tile_live >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)tile_live, 0u));
        const uint32_t n_live = (uint32_t)__builtin_popcountll(tile_live);
        __builtin_amdgcn_wave_barrier();
        if (__builtin_amdgcn_inverse_ballot_w64(tile_live)) ((rt_lptr32_ordered)WW.items)[ord] = lane;
        // the lowest min(needy lanes, live slots) set bits are handed out (a lane without a live slot clears no bit)
        tile_live &= ~__ballot(ord < (uint32_t)__builtin_popcountll(mask));
        __builtin_amdgcn_wave_barrier();
        if (need && rank < n_live) {
          const uint32_t slot = ld_l32(WW.items, rank);
          need = false;
          have_pixel = true;
          pixel_xy = tile_xy0 + ((slot & 7u) | (slot >> 3) << 16);
          if constexpr (!SLIM) p.pixel = (pixel_xy >> 16) * U.width + (pixel_xy & 0xffffu);
          p.sample = 0u;
          item_slot = tile_slot;
          if constexpr (SLIM) {
            col_park_clear<WAVES>(s_scene);
          } else {
            p.col = rt3_splat(0.0f);
          }
        }
        __builtin_amdgcn_wave_barrier();
      }
    } else {
      bool need = !alive && !have_pixel;
      for (;;) {
        const unsigned long long mask = __ballot(need);
        if (mask == 0ull || !work_left) break;
        if (tile_pos >= 64u) {
          const int leader = __builtin_ctzll(mask);
          uint32_t t = 0;
          if (lane == (uint32_t)leader) t = atomicAdd(ticket, 1u);
          t = LEAN ? __builtin_amdgcn_readlane(t, leader) : __shfl(t, leader, 64);
          if (t >= n_tiles * n_slots) {
            work_left = false;
            break;
          }
          // frame-major ticket: frame = t / n_tiles, tile = t % n_tiles
          tile_slot = t / n_tiles;
          const uint32_t tile_in_frame = t - tile_slot * n_tiles;
          uint32_t trow = tile_in_frame / tiles_x;
          tile_x0 = (tile_in_frame - trow * tiles_x) * 8u;
          if (F.own_period) trow = (trow / F.own_run) * F.own_period + F.own_first + (trow % F.own_run);
          tile_y0 = trow * 8u;
          tile_pos = 0u;
        }
        // rank of this lane among the needy lanes
        const uint32_t rank =
            __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
        const uint32_t slot = tile_pos + rank;
        if (need && slot < 64u) {
          const uint32_t x = tile_x0 + (slot & 7u);
          const uint32_t y = tile_y0 + (slot >> 3);
          if (x < U.width && y < U.height && (LEAN ? owns_row(fresh_stripes(F), y) : owns_row(F, y))) {
            const uint32_t pixel = y * (LEAN ? rt_fresh(U.width) : U.width) + x;
            // (LEAN: MAX_DEPTH taken as new here, or its test is carried through the trip as a lane mask in two SGPRs)
            // (LEAN: the depth plane named global memory, as the G-buffer loads of start_sample)
            const float gdepth = LEAN ? __builtin_bit_cast(float, ld_g32(reinterpret_cast<const uint32_t*>(slots[tile_slot].depth), pixel))
                                      : slots[tile_slot].depth[pixel];
            if (!(gdepth >= 1.0f) && (LEAN ? rt_fresh(F.max_depth) : F.max_depth) != 0u) {
              need = false;
              have_pixel = true;
              if constexpr (!SLIM) p.pixel = y * U.width + x;
              pixel_xy = x | (y << 16);   // width, height <= 65535: rt_resize refuses more
              p.sample = 0u;
              item_slot = tile_slot;
              if constexpr (SLIM) {
                col_park_clear<WAVES>(s_scene);
              } else {
                p.col = rt3_splat(0.0f);
              }
            } else {
              finish_black_pixel(F, U, slots, tile_slot, pixel);
            }
          }
        }
        tile_pos += (uint32_t)__builtin_popcountll(mask);
      }
    }
    // (b) start the next sample of the owned pixel: camera ray + depth-0 surface from the G-buffer (the pixel is not
    //     background: the sample always starts).  ONE_PASS: camera ray and the pixel's G-buffer words; the surface frame is
    //     made below, with the frames of the lanes whose extension ray found a hit in the last trip.
    RT_LSTAT(6, !alive && have_pixel);
    GbufSurface gs = {0.0f, 0.0f, 0u};
    bool started = false;   // ONE_PASS: the lane has just started a sample, its surface frame comes from the G-buffer words
    if (!alive && have_pixel) {
      const uint32_t x = pixel_xy & 0xffffu, y = pixel_xy >> 16;
      const DevFrameSlot slot = slots[item_slot];
      if constexpr (SLIM) p.pixel = y * rt_fresh(U.width) + x;
      if constexpr (ONE_PASS) {
        // (the camera read as new: thirteen scalar registers the rest of the trip can use)
        alive = started = start_sample<true, true, true>(S, F, fresh_size(U), fresh_camera_basis(), slot, x, y, p, wrec, &gs);
      } else {
        alive = LEAN ? start_sample<true, ONE_INST>(S, F, fresh_size(U), cam, slot, x, y, p, wrec)
                     : start_sample<true>(S, F, U, cam, slot, x, y, p);
      }
    }
    const bool running = alive;
    bool path_done = false;
#ifdef RT_PT_STAMPS
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned long long ps0b = __builtin_amdgcn_s_memtime();
    unsigned long long ps1 = ps0b;
#endif

    // ------------------------------------------------------------ surface frame (ONE_PASS) and shade one bounce
    bool want_shadow = false, want_extend = false;
    bool nee_valid = false;
    rt3 sh_o = rt3_splat(0.0f), sh_d = rt3_splat(0.0f), nee = rt3_splat(0.0f);
    float sh_tmax = 0.0f;
    RT_LSTAT(0, running);
    RT_LSTAT(8, ONE_PASS && running);
    if (running) {
      // ONE_PASS: a lane that is alive here and has not just started a sample came through the last trip without ending, so
      // its extension ray of that trip found a hit (shade_bounce asks for the ray or ends the path, and a miss ends it): every
      // running lane needs a surface frame, and no other lane does.  One pass makes it for both kinds: instance rows, local
      // ray, triangle records and barycentrics once; the lane condition `started` picks the tail (normal and albedo of the
      // G-buffer and hit_t of the primary ray, or interpolated vertex normals and the material).  Per lane the functions and
      // their inputs are those of the two separate calls: a new hit's ray, triangle and distance are not touched between the
      // walk that found it and this point.  The frame (normal, geometric normal, albedo, texture coordinates) lives from here
      // to the end of the bounce only.
      if constexpr (ONE_PASS) {
        // every hit, the primary pass's too, is in the one instance the TLAS leaf names: its index is read here, as traverse()
        // reads it, and p.inst is not carried through the walks
        p.inst = __builtin_amdgcn_readfirstlane(rt_f2u(ld_l(s_scene, M.l_nodes + 1u).w) >> 3);
        setup_surface<true, PLAIN>(S, p, started, gs.nx, gs.ny, gs.albedo, wrec);
#ifdef RT_PT_STAMPS
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        ps1 = __builtin_amdgcn_s_memtime();
#endif
      }
      if (DETAIL) cnt_shaded++;
      BounceOut bo;
      shade_bounce<ONE_INST, PLAIN>(S, LEAN ? rt_fresh(U.light_count) : U.light_count, LEAN ? rt_fresh(F.max_depth) : F.max_depth, p,
                             bo, wrec);
      want_shadow = bo.want_shadow;
      want_extend = bo.want_extend;
      nee_valid = bo.nee_valid;
      sh_o = bo.sh_o;
      sh_d = bo.sh_d;
      sh_tmax = bo.sh_tmax;
      nee = bo.nee;
      const bool ended = bo.ended;
      if (ended) path_done = true;
    }

#ifdef RT_PT_STAMPS
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned long long ps2 = __builtin_amdgcn_s_memtime();
#endif
    // ------------------------------------------------------------ shadow rays (any hit)
    const unsigned long long shadow_mask = __ballot(want_shadow);
    if (shadow_mask != 0ull) {
      cnt_shadow += (uint32_t)__builtin_popcountll(shadow_mask);
      float t_;
      int32_t a_, b_;
      bool occluded;
      if constexpr (SWEEP) {
        traverse_leaves<true, MODE, !PLAIN>(M, s_scene, WW, LeafSweep{RT_PT_SWEEP_ARG}, U.blas_base_idx, want_shadow, sh_o, sh_d, sh_tmax,
                                    t_, a_, b_, occluded);
      } else {
        traverse<true, DETAIL, MODE, ONE_INST>(M, s_scene, WW, U.blas_base_idx, want_shadow, sh_o, sh_d, sh_tmax, t_, a_, b_,
                                     occluded, cnt_nodes, cnt_tris);
      }
      if (want_shadow) {
        if (!occluded && nee_valid) p.radiance = p.radiance + nee;  // nothing is added when bsdf_pdf <= 0
      }
    }

#ifdef RT_PT_STAMPS
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned long long ps3 = __builtin_amdgcn_s_memtime();
#endif
    // ------------------------------------------------------------ extension rays (closest hit)
    const unsigned long long extend_mask = __ballot(want_extend);
    if (extend_mask != 0ull) {
      cnt_ext += (uint32_t)__builtin_popcountll(extend_mask);
      float t_;
      int32_t tri_, inst_;
      bool any_;
      if constexpr (SWEEP) {
        traverse_leaves<false, MODE, !PLAIN>(M, s_scene, WW, LeafSweep{RT_PT_SWEEP_ARG}, U.blas_base_idx, want_extend, p.ro, p.rd, RT_T_MAX,
                                     t_, tri_, inst_, any_);
      } else {
        traverse<false, DETAIL, MODE, ONE_INST>(M, s_scene, WW, U.blas_base_idx, want_extend, p.ro, p.rd, RT_T_MAX, t_, tri_,
                                      inst_, any_, cnt_nodes, cnt_tris);
      }
      RT_LSTAT(5, want_extend && inst_ >= 0);
      if (want_extend) {
        if (inst_ < 0) {
          path_done = true;
        } else {
          p.hit_t = t_;
          p.tri = (uint32_t)tri_;
          p.inst = (uint32_t)inst_;
          // (ONE_PASS: the hit's surface frame is made at the start of the next trip)
          if constexpr (!ONE_PASS) setup_surface<ONE_INST>(S, p, false, 0.0f, 0.0f, 0u, wrec);
          p.depth++;
        }
      }
    }

#ifdef RT_PT_STAMPS
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    const unsigned long long ps4 = __builtin_amdgcn_s_memtime();
#endif
    // ------------------------------------------------------------ sample / pixel finished
    RT_LSTAT(7, path_done);
    if (path_done) {
      alive = false;
      if constexpr (SLIM) {
        p.col = col_park_add<WAVES>(s_scene, p.radiance);
        p.pixel = (pixel_xy >> 16) * rt_fresh(U.width) + (pixel_xy & 0xffffu);
      } else {
        p.col = p.col + p.radiance;
      }
      p.sample++;
      if (p.sample >= (LEAN ? rt_fresh(F.spp) : F.spp)) {  // the item's last sample
        if (LEAN) {
          finish_pixel(fresh_spp(F), U, slots, item_slot, p.pixel, p.col);
        } else {
          finish_pixel(F, U, slots, item_slot, p.pixel, p.col);
        }
        have_pixel = false;
      }
    }
#ifdef RT_PT_STAMPS
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    {
      const unsigned long long ps5 = __builtin_amdgcn_s_memtime();
      pt_cyc[0] += ps0b - ps0; pt_cyc[5] += ps1 - ps0b; pt_cyc[1] += ps2 - ps1;
      pt_cyc[2] += ps3 - ps2; pt_cyc[3] += ps4 - ps3; pt_cyc[4] += ps5 - ps4;
      pt_trips++;
    }
#endif
    if (!work_left && __ballot(alive || have_pixel) == 0ull) break;
  }
#ifdef RT_PT_STAMPS
  if (lane == 0u) {
    for (int k = 0; k < 5; k++) atomicAdd(&g_pt_sections[k], pt_cyc[k]);
    atomicAdd(&g_pt_sections[5], pt_trips);
    atomicAdd(&g_pt_sections[6], 1ull);
    atomicAdd(&g_pt_sections[7], pt_cyc[5]);
  }
#endif

#ifdef RT_CLOCK_STAMP
  if (threadIdx.x == 0 && blockIdx.x < RT_CLOCK_STAMP_SLOTS) {
    g_clock_stamps[2 * blockIdx.x] = __builtin_amdgcn_s_memtime() - stamp_c0;
    g_clock_stamps[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime() - stamp_r0;
  }
#endif
  // counters: one flush per persistent wave
  LaneCounters c;
  c.primary = 0;
  c.extension = lane == 0u ? cnt_ext : 0u;   // the wave's count, once
  c.shadow = lane == 0u ? cnt_shadow : 0u;
  c.nodes = cnt_nodes;
  c.tris = cnt_tris;
  c.shaded = cnt_shaded;
  flush_counters<DETAIL>(c, F.counters, blockIdx.x * WAVES + wave);
}
