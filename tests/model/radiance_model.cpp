// radiance_model.cpp — TEST INFRASTRUCTURE: the reference of the radiance queries (rt_trace_radiance, mi355rt.h).
// The oracle restates ray_color (Raytracer.wgsl:607-783) with the depth-0 surface read from its G-buffer; a radiance query
// takes the depth-0 surface from the traced hit instead, the way every later depth does (:738-779).  This file includes the
// oracle as its translation unit - the result is a self-contained oracle library plus two entry points - and restates the
// bounce loop ONCE on the oracle's own helpers (intersect_tlas, intersect_tlas_shadow, sample_light_source, get_light_pdf,
// eval_ggx, sample_*, sample_tex, power_heuristic), with ONE surface-frame function used for depth 0 and for every bounce,
// and a switch:
//   gbuffer_depth0 = 0   the semantics of rt_trace_radiance;
//   gbuffer_depth0 = 1   (tri, inst), normal, albedo and the background test of stream id `pad` come from the oracle's
//                        G-buffer and t is recomputed: the oracle's ray_color to the letter.  It exists only to tie the
//                        restated loop to the oracle (tests/test_radiance_model.py: bit for bit the oracle's frame).
// build: the flags of oracle/Makefile (tests/radiance_util.py does it).  With -DRADIANCE_MODEL_MAIN the file is a stand-alone
// program that renders frames and traces radiance queries on scene arrays read from files (for a sanitizer build on the CPU;
// tests/test_hostile_records_model.py writes the files).
#include "../../oracle/rt_oracle.cpp"

namespace {

struct Surface {
  uint32_t tri_idx;
  int32_t inst_idx;
  float hit_t;
  rt2 tex_uv;
  rt3 normal, albedo, world_geom_n;
};

// The surface frame of the hit (tri_idx, inst_idx) of `ray`.  gn / ga = the pixel's G-buffer words: depth 0 of the oracle's
// ray_color (Raytracer.wgsl:617-655: t recomputed, octahedral normal, unorm8 albedo); null: a traced hit at distance
// traced_t (:738-779).
void surface_frame(const Oracle& o, const Ray& ray, uint32_t tri_idx, int32_t inst_idx, float traced_t, const float* gn,
                   const uint8_t* ga, Surface& sf) {
  const rt_topology* tri = &o.topology[tri_idx];
  const rt_instance* inst = &o.instances[inst_idx];
  const float* inv = inst->inverse;
  rt3 v0_pos = o.get_pos(tri->v0), v1_pos = o.get_pos(tri->v1), v2_pos = o.get_pos(tri->v2);

  Ray r_local = make_ray(rt_mat_mul_point(inv, ray.origin), rt_mat_mul_dir(inv, ray.direction));
  rt3 s = r_local.origin - v0_pos;
  rt3 e1 = v1_pos - v0_pos;
  rt3 e2 = v2_pos - v0_pos;
  rt3 h_val = rt_cross(r_local.direction, e2);
  float f_val = 1.0f / rt_dot(e1, h_val);
  float u_bar = f_val * rt_dot(s, h_val);
  rt3 q = rt_cross(s, e1);
  float v_bar = f_val * rt_dot(r_local.direction, q);
  float w_bar = 1.0f - u_bar - v_bar;

  rt2 uv0 = o.get_uv(tri->v0), uv1 = o.get_uv(tri->v1), uv2 = o.get_uv(tri->v2);
  sf.tri_idx = tri_idx;
  sf.inst_idx = inst_idx;
  sf.tex_uv = uv0 * w_bar + uv1 * u_bar + uv2 * v_bar;

  if (gn) {
    sf.hit_t = f_val * rt_dot(e2, q);
    sf.normal = Oracle::unpack_normal(rt2_make(gn[0], gn[1]));
    sf.albedo = rt3_make(rt_from_unorm8(ga[0]), rt_from_unorm8(ga[1]), rt_from_unorm8(ga[2]));
  } else {
    sf.hit_t = traced_t;
    rt3 n0 = o.get_normal(tri->v0), n1 = o.get_normal(tri->v1), n2 = o.get_normal(tri->v2);
    rt3 ln = rt_normalize(n0 * w_bar + n1 * u_bar + n2 * v_bar);
    sf.normal = rt_normalize(rt_vec_mul_mat_dir(ln, inv));

    sf.albedo = rt3_make(tri->data0[0], tri->data0[1], tri->data0[2]);
    if (tri->data2[0] > -0.5f) sf.albedo = sf.albedo * o.sample_tex(sf.tex_uv, rt_f2i32_sat(tri->data2[0]));

    if (tri->data2[2] > -0.5f) {
      rt3 n_map = o.sample_tex(sf.tex_uv, rt_f2i32_sat(tri->data2[2])) * 2.0f - rt3_splat(1.0f);
      rt3 T = rt_normalize(e1);
      rt3 B = rt_normalize(rt_cross(ln, T));
      rt3 ln_mapped = rt_normalize(T * n_map.x + B * n_map.y + ln * n_map.z);
      sf.normal = rt_normalize(rt_vec_mul_mat_dir(ln_mapped, inv));
    }
  }
  rt3 local_geom_n = rt_normalize(rt_cross(e1, e2));
  sf.world_geom_n = rt_normalize(rt_vec_mul_mat_dir(local_geom_n, inv));
}

// The bounce loop of ray_color (Raytracer.wgsl:656-783) for a path whose depth-0 surface is `sf`
rt3 bounce_loop(const Oracle& o, Ray ray, uint32_t* rng, Surface sf, uint32_t max_depth, Counters& c) {
  rt3 throughput = rt3_splat(1.0f);
  rt3 radiance = rt3_splat(0.0f);
  float prev_bsdf_pdf = 0.0f;
  bool specular_bounce = true;

  for (uint32_t depth = 0u; depth < max_depth; depth++) {
    c.shaded_hits++;
    const rt_topology* tri = &o.topology[sf.tri_idx];
    uint32_t mat_type = rt_f2u32_sat(tri->data0[3] + 0.5f);
    rt3 hit_p = ray.origin + ray.direction * sf.hit_t;

    sf.normal = (rt_dot(ray.direction, sf.normal) < 0.0f) ? sf.normal : -sf.normal;
    sf.world_geom_n = (rt_dot(ray.direction, sf.world_geom_n) < 0.0f) ? sf.world_geom_n : -sf.world_geom_n;
    const rt3 normal = sf.normal, albedo = sf.albedo, world_geom_n = sf.world_geom_n;

    float metallic = tri->data1[0];
    float roughness = tri->data1[1];
    if (tri->data2[1] > -0.5f) {
      rt3 mr = o.sample_tex(sf.tex_uv, rt_f2i32_sat(tri->data2[1]));
      metallic *= mr.z;
      roughness *= mr.y;
    }
    roughness = rt_max(roughness, 0.005f);

    rt3 emissive = rt3_make(tri->data3[0], tri->data3[1], tri->data3[2]);
    if (tri->data2[3] > -0.5f) emissive = emissive * o.sample_tex(sf.tex_uv, rt_f2i32_sat(tri->data2[3]));

    rt3 f0 = rt_mix3(rt3_splat(0.04f), albedo, metallic);

    // --- emissive / light ---
    if (mat_type == 3u || rt_length(emissive) > 1e-4f) {
      rt3 em_val = (mat_type == 3u) ? albedo : emissive;
      if (specular_bounce) {
        radiance = radiance + throughput * em_val;
      } else {
        radiance = radiance + throughput * em_val *
                                  Oracle::power_heuristic(prev_bsdf_pdf, o.get_light_pdf(sf.tri_idx, (uint32_t)sf.inst_idx,
                                                                                         sf.hit_t, ray.direction));
      }
      if (mat_type == 3u) break;
    }

    // --- next event estimation ---
    if (mat_type != 2u) {
      LightSample light_s = o.sample_light_source(hit_p, rng);
      if (light_s.pdf > 0.0f) {
        c.shadow_rays++;
        if (!o.intersect_tlas_shadow(make_ray(hit_p + world_geom_n * 1e-4f, light_s.dir), T_MIN, light_s.dist - 2e-4f, c)) {
          rt3 bsdf_val = rt3_splat(0.0f);
          float bsdf_pdf_val = 0.0f;
          if (mat_type == 0u) {
            bsdf_val = Oracle::eval_diffuse(albedo);
            bsdf_pdf_val = rt_max(rt_dot(normal, light_s.dir), 0.0f) / PI;
          } else if (mat_type == 1u) {
            bsdf_val = Oracle::eval_ggx(normal, -ray.direction, light_s.dir, roughness, f0);
            rt3 H = rt_normalize(-ray.direction + light_s.dir);
            bsdf_pdf_val = (Oracle::ggx_d(rt_dot(normal, H), roughness * roughness) * rt_max(rt_dot(normal, H), 0.0f)) /
                           (4.0f * rt_max(rt_dot(-ray.direction, H), 0.0f));
          }
          if (bsdf_pdf_val > 0.0f) {
            radiance = radiance + throughput * bsdf_val * light_s.L * Oracle::power_heuristic(light_s.pdf, bsdf_pdf_val) *
                                      rt_max(rt_dot(normal, light_s.dir), 0.0f) / light_s.pdf;
          }
        }
      }
    }

    ScatterResult scatter;
    if (mat_type == 0u) {
      scatter = Oracle::sample_diffuse(normal, albedo, rng);
    } else if (mat_type == 1u) {
      scatter = Oracle::sample_ggx(normal, -ray.direction, roughness, f0, rng);
    } else {
      scatter = Oracle::sample_dielectric(ray.direction, normal, tri->data1[2], albedo, rng);
    }

    if (mat_type != 2u && rt_dot(scatter.dir, world_geom_n) <= 0.0f) {
      scatter.pdf = 0.0f;
      scatter.throughput = rt3_splat(0.0f);
    }
    if (scatter.pdf <= 0.0f || rt_length(scatter.throughput) <= 0.0f) break;

    throughput = throughput * scatter.throughput;

    rt3 ray_offset_normal = (rt_dot(scatter.dir, world_geom_n) > 0.0f) ? world_geom_n : -world_geom_n;
    ray = make_ray(hit_p + ray_offset_normal * 1e-4f, scatter.dir);

    prev_bsdf_pdf = scatter.pdf;
    specular_bounce = scatter.is_specular;

    if (depth > 3u) {
      float p = rt_max(throughput.x, rt_max(throughput.y, throughput.z));
      if (Oracle::rand_pcg(rng) > p) break;
      throughput = throughput / p;
    }

    // --- next intersection ---
    if (depth < max_depth - 1u) {
      c.extension_rays++;
      HitResult hit = o.intersect_tlas(ray, T_MIN, T_MAX, c);
      if (hit.inst_idx < 0) break;
      surface_frame(o, ray, rt_f2u32_sat(hit.tri_idx), hit.inst_idx, hit.t, nullptr, nullptr, sf);
    }
  }
  return radiance;
}

}  // namespace

extern "C" {

// rays: n x rt_ray {o, t_max, d, pad}.  out: n x 4 f32 {r, g, b, t}.  counts: n x 5 u64 {extension_rays, shadow_rays,
// shaded_hits, nodes_visited, tris_tested} of each ray (may be null).  gbuffer_depth0: see the head of this file.
void radiance_model_trace(oracle_ctx* ctx, const rt_ray* rays, uint32_t n, uint32_t max_depth, uint32_t spp, uint32_t seed,
                          int gbuffer_depth0, float* out, uint64_t* counts) {
  const Oracle& o = ctx->o;
  for (uint32_t i = 0; i < n; i++) {
    const rt_ray& q = rays[i];
    const Ray ray = make_ray(rt3_make(q.origin[0], q.origin[1], q.origin[2]), rt3_make(q.dir[0], q.dir[1], q.dir[2]));
    Counters cn;
    rt3 col = rt3_splat(0.0f);
    float t = q.t_max;
    // depth 0: where the path starts
    bool shade = false;
    uint32_t tri_idx = 0u;
    int32_t inst_idx = -1;
    const float* gn = nullptr;
    const uint8_t* ga = nullptr;
    if (gbuffer_depth0) {
      const uint32_t pixel_idx = q.pad;
      if (!(o.g_depth[pixel_idx] >= 1.0f)) {
        gn = &o.g_normal[(size_t)pixel_idx * 4];
        ga = &o.render_target[(size_t)pixel_idx * 4];
        tri_idx = rt_f2u(gn[2]);
        inst_idx = (int32_t)rt_f2u(gn[3]);
        shade = true;
      }
    } else {
      // the first segment does not depend on the sample: traced once per ray, one extension ray
      cn.extension_rays++;
      HitResult hit = o.intersect_tlas(ray, T_MIN, q.t_max, cn);
      t = hit.t;   // a miss: the bound it was given
      if (hit.inst_idx >= 0) {
        tri_idx = rt_f2u32_sat(hit.tri_idx);
        inst_idx = hit.inst_idx;
        shade = max_depth != 0u;
      }
    }
    if (shade) {
      for (uint32_t s = 0u; s < spp; s++) {
        uint32_t rng = Oracle::init_rng(q.pad, seed * spp + s);
        Surface sf;
        surface_frame(o, ray, tri_idx, inst_idx, t, gn, ga, sf);
        if (gbuffer_depth0) t = sf.hit_t;
        col = col + bounce_loop(o, ray, &rng, sf, max_depth, cn);
      }
      col = col / (float)spp;
    }
    float* w = out + (size_t)i * 4;
    w[0] = col.x;
    w[1] = col.y;
    w[2] = col.z;
    w[3] = t;
    if (counts) {
      uint64_t* k = counts + (size_t)i * 5;
      k[0] = cn.extension_rays;
      k[1] = cn.shadow_rays;
      k[2] = cn.shaded_hits;
      k[3] = cn.nodes_visited;
      k[4] = cn.tris_tested;
    }
  }
}

// The pinhole rays of the frame the oracle computed last (trace_pixel's u, v, d; Raytracer.wgsl:806-809 without the lens
// offset): width x height rt_ray in pixel order, pad = pixel index, t_max = 1e30.
void radiance_model_camera_rays(oracle_ctx* ctx, rt_ray* out) {
  const Oracle& o = ctx->o;
  const rt_scene_uniforms& scene = o.scene;
  const rt_camera& cam = scene.camera;
  rt3 cam_o = rt3_make(cam.origin[0], cam.origin[1], cam.origin[2]);
  rt3 cam_ll = rt3_make(cam.lower_left[0], cam.lower_left[1], cam.lower_left[2]);
  rt3 cam_h = rt3_make(cam.horizontal[0], cam.horizontal[1], cam.horizontal[2]);
  rt3 cam_v = rt3_make(cam.vertical[0], cam.vertical[1], cam.vertical[2]);
  for (uint32_t y = 0; y < scene.height; y++) {
    for (uint32_t x = 0; x < scene.width; x++) {
      const uint32_t p_idx = y * scene.width + x;
      rt3 off = rt3_splat(0.0f);
      float u = ((float)x + 0.5f + scene.jitter[0] * (float)scene.width) / (float)scene.width;
      float v = 1.0f - ((float)y + 0.5f + scene.jitter[1] * (float)scene.height) / (float)scene.height;
      rt3 d = cam_ll + u * cam_h + v * cam_v - cam_o - off;
      rt3 org = cam_o + off;
      rt_ray& r = out[p_idx];
      r.origin[0] = org.x; r.origin[1] = org.y; r.origin[2] = org.z;
      r.t_max = 1e30f;
      r.dir[0] = d.x; r.dir[1] = d.y; r.dir[2] = d.z;
      r.pad = p_idx;
    }
  }
}

}  // extern "C"

#ifdef RADIANCE_MODEL_MAIN
// ---- the oracle's frames and the radiance queries on a scene read from files, as a program of its own
#include <cstdio>
#include <cstdlib>
#include <string>

namespace {

template <class T>
std::vector<T> read_file(const std::string& path) {
  std::vector<T> v;
  FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) {
    std::printf("cannot open %s\n", path.c_str());
    std::exit(2);
  }
  std::fseek(f, 0, SEEK_END);
  const long bytes = std::ftell(f);
  std::fseek(f, 0, SEEK_SET);
  v.resize((size_t)bytes / sizeof(T));
  if (bytes && std::fread(v.data(), 1, (size_t)bytes, f) != (size_t)bytes) std::exit(2);
  std::fclose(f);
  return v;
}

}  // namespace

// usage: <textures.u8 or -> <width> <height> <max_depth> <scene directory>...
// A scene directory holds vertices.f32, normals.f32, uvs.f32, topology.u32, tlas.f32, blas.f32, instances.f32, lights.u32,
// draw_commands.u32, camera.f32 and rays.f32 (rt_ray records).  Every scene is uploaded in the order of upload_scene, three
// frames are computed and presented, and the rays are traced as a radiance query with 2 samples.
int main(int argc, char** argv) {
  if (argc < 6) return 2;
  const std::string tex_path = argv[1];
  const uint32_t width = (uint32_t)std::atoi(argv[2]), height = (uint32_t)std::atoi(argv[3]), depth = (uint32_t)std::atoi(argv[4]);
  std::vector<uint8_t> tex;
  if (tex_path != "-") tex = read_file<uint8_t>(tex_path);
  for (int a = 5; a < argc; a++) {
    const std::string dir = std::string(argv[a]) + "/";
    auto pos = read_file<float>(dir + "vertices.f32"), nrm = read_file<float>(dir + "normals.f32"), uv = read_file<float>(dir + "uvs.f32");
    auto topo = read_file<uint32_t>(dir + "topology.u32"), lights = read_file<uint32_t>(dir + "lights.u32");
    auto draw = read_file<uint32_t>(dir + "draw_commands.u32");
    auto tlas = read_file<float>(dir + "tlas.f32"), blas = read_file<float>(dir + "blas.f32"), inst = read_file<float>(dir + "instances.f32");
    auto cam = read_file<float>(dir + "camera.f32");
    auto rays = read_file<float>(dir + "rays.f32");
    if (cam.size() != 24 || pos.size() % 4 || nrm.size() != pos.size() || uv.size() * 2 != pos.size()) return 2;
    oracle_ctx* c = oracle_create();
    oracle_set_threads(c, 1);
    oracle_build_pipeline(c, depth, 1);
    if (!tex.empty()) oracle_upload_textures(c, tex.data(), (uint32_t)(tex.size() / ((size_t)RT_TEX_SIZE * RT_TEX_SIZE * 4)));
    oracle_update_geometry(c, pos.data(), nrm.data(), uv.data(), (uint32_t)(pos.size() / 4));
    oracle_update_bvh(c, tlas.data(), (uint32_t)(tlas.size() / 8), blas.data(), (uint32_t)(blas.size() / 8));
    oracle_update_topology(c, topo.data(), topo.size());
    oracle_update_instances(c, inst.data(), inst.size());
    oracle_update_lights(c, lights.data(), lights.size());
    oracle_update_draw_commands(c, draw.data(), draw.size());
    oracle_update_screen_size(c, width, height);
    oracle_update_scene_uniforms(c, cam.data(), 0, (uint32_t)(lights.size() / 2));
    for (uint32_t f = 1; f <= 3; f++) {
      oracle_compute(c, f);
      oracle_present(c);
    }
    const uint32_t n = (uint32_t)(rays.size() / 8);
    std::vector<float> out((size_t)n * 4);
    std::vector<uint64_t> counts((size_t)n * 5);
    radiance_model_trace(c, reinterpret_cast<const rt_ray*>(rays.data()), n, depth, 2, 5, 0, out.data(), counts.data());
    uint64_t shaded = 0;
    for (uint32_t i = 0; i < n; i++) shaded += counts[(size_t)i * 5 + 2];
    std::printf("%s %u rays, %llu shaded hits\n", argv[a], n, (unsigned long long)shaded);
    oracle_destroy(c);
  }
  std::printf("hostile records ok\n");
  return 0;
}
#endif
