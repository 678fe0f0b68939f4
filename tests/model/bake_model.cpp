// bake_model.cpp — TEST INFRASTRUCTURE: the reference of the lightmap bakes (rt_bake_points, mi355rt.h "lightmap bakes").
// This file includes the gather model (and through it the radiance model and the oracle) as its translation unit - the
// result is that library plus one entry point - and restates the texel rule of the header ONCE, for the CPU, on plain
// arrays: triangle by triangle in ascending index, first come first owned, over the texels of a bounding-box sweep that
// the rule's own box test makes exact.  bake = these points, then gather_model_gather on them (tests/bake_util.py).
// build: the flags of oracle/Makefile (tests/bake_util.py does it).  With -DBAKE_MODEL_MAIN the file is a stand-alone
// program that runs hand-worked cases on the restated rule (for a sanitizer build on the CPU); it needs no scene.
#include <cmath>
#include <cstdio>
#include <vector>

#include "gather_model.cpp"

namespace {

struct BakeScene {
  const rt_topology* topo;
  uint32_t n_tris;
  const float* pos;   // 4 f32 per vertex
  const float* nrm;   // 4 f32 per vertex
  const float* uv;    // 2 f32 per vertex: the ATLAS uvs (the caller's override or the scene's)
  const rt_instance* inst;
  const uint32_t* draw;   // 4 u32 per instance
};

struct TexelTri {
  rt2 a, b, c;
  float A;
};

bool finite_f32(float x) { return (rt_f2u(x) & 0x7fffffffu) < 0x7f800000u; }
float edge(rt2 q, rt2 r, rt2 s) { return (r.x - q.x) * (s.y - q.y) - (r.y - q.y) * (s.x - q.x); }

bool texel_triangle(const BakeScene& s, const rt_bake_desc& d, uint32_t k, TexelTri& t) {
  const rt_topology& tri = s.topo[k];
  const float fw = (float)d.width, fh = (float)d.height;
  t.a = rt2_make(s.uv[2 * (size_t)tri.v0] * fw, s.uv[2 * (size_t)tri.v0 + 1] * fh);
  t.b = rt2_make(s.uv[2 * (size_t)tri.v1] * fw, s.uv[2 * (size_t)tri.v1 + 1] * fh);
  t.c = rt2_make(s.uv[2 * (size_t)tri.v2] * fw, s.uv[2 * (size_t)tri.v2 + 1] * fh);
  t.A = edge(t.a, t.b, t.c);
  return finite_f32(t.a.x) && finite_f32(t.a.y) && finite_f32(t.b.x) && finite_f32(t.b.y) && finite_f32(t.c.x) &&
         finite_f32(t.c.y) && finite_f32(t.A) && t.A != 0.0f;
}

bool covers(const TexelTri& t, rt2 p) {
  const float min_x = rt_min(rt_min(t.a.x, t.b.x), t.c.x), max_x = rt_max(rt_max(t.a.x, t.b.x), t.c.x);
  const float min_y = rt_min(rt_min(t.a.y, t.b.y), t.c.y), max_y = rt_max(rt_max(t.a.y, t.b.y), t.c.y);
  if (!(min_x <= p.x && p.x <= max_x && min_y <= p.y && p.y <= max_y)) return false;
  const float sg = t.A > 0.0f ? 1.0f : -1.0f;
  return sg * edge(t.a, t.b, p) >= 0.0f && sg * edge(t.b, t.c, p) >= 0.0f && sg * edge(t.c, t.a, p) >= 0.0f;
}

// texels 0 .. n-1 whose centre can lie in [min_v, max_v]: a superset (the box test of `covers` decides), clamped in float
bool sweep(float min_v, float max_v, uint32_t n, uint32_t& lo, uint32_t& hi) {
  const float fn = (float)n;
  if (!(max_v >= 0.5f) || !(min_v <= fn)) return false;
  lo = (uint32_t)(rt_floor(rt_max(min_v, 1.0f)) - 1.0f);
  hi = (uint32_t)rt_floor(rt_min(max_v, fn));
  if (hi > n - 1u) hi = n - 1u;
  return lo <= hi;
}

rt3 vec3_at(const float* a, uint32_t i) { return rt3_make(a[4 * (size_t)i], a[4 * (size_t)i + 1], a[4 * (size_t)i + 2]); }

// owner: W * H.  points / texels: W * H records, or null (owner map and count only).  weights: 2 f32 per record, the bu and bv
// of each point, or null (for the accuracy checks of tests/test_bake_model.py).  Returns the number of covered texels.
uint32_t bake_points(const BakeScene& s, const rt_bake_desc& d, rt_gather_point* points, uint32_t* texels, int32_t* owner,
                     float* weights = nullptr) {
  const uint32_t W = d.width, H = d.height;
  for (size_t i = 0; i < (size_t)W * H; i++) owner[i] = -1;
  const uint32_t first = s.draw[4 * (size_t)d.inst + 2] / 3u, cnt = s.draw[4 * (size_t)d.inst] / 3u;
  for (uint32_t j = 0; j < cnt; j++) {
    const uint64_t k64 = (uint64_t)first + j;
    if (k64 >= s.n_tris) break;   // at or beyond the topology: skipped, never read
    const uint32_t k = (uint32_t)k64;
    TexelTri t;
    if (!texel_triangle(s, d, k, t)) continue;
    uint32_t x0, x1, y0, y1;
    if (!sweep(rt_min(rt_min(t.a.x, t.b.x), t.c.x), rt_max(rt_max(t.a.x, t.b.x), t.c.x), W, x0, x1)) continue;
    if (!sweep(rt_min(rt_min(t.a.y, t.b.y), t.c.y), rt_max(rt_max(t.a.y, t.b.y), t.c.y), H, y0, y1)) continue;
    for (uint32_t y = y0; y <= y1; y++)
      for (uint32_t x = x0; x <= x1; x++) {
        int32_t& o = owner[(size_t)y * W + x];
        // ascending k: the first triangle that covers a texel is the lowest
        if (o < 0 && covers(t, rt2_make((float)x + 0.5f, (float)y + 0.5f))) o = (int32_t)k;
      }
  }
  uint32_t n = 0;
  const rt_instance& inst = s.inst[d.inst];
  for (uint32_t i = 0; i < W * H; i++) {
    if (owner[i] < 0) continue;
    if (points) {
      const uint32_t k = (uint32_t)owner[i], x = i % W, y = i / W;
      TexelTri t;
      texel_triangle(s, d, k, t);
      const rt2 p = rt2_make((float)x + 0.5f, (float)y + 0.5f);
      const float bu = rt_div(edge(t.c, t.a, p), t.A);
      const float bv = rt_div(edge(t.a, t.b, p), t.A);
      const float bw = 1.0f - bu - bv;
      const rt_topology& tri = s.topo[k];
      const rt3 V0 = rt_mat_mul_point(inst.transform, vec3_at(s.pos, tri.v0));
      const rt3 V1 = rt_mat_mul_point(inst.transform, vec3_at(s.pos, tri.v1));
      const rt3 V2 = rt_mat_mul_point(inst.transform, vec3_at(s.pos, tri.v2));
      const rt3 pos = bw * V0 + bu * V1 + bv * V2;
      const rt3 ln = rt_normalize(vec3_at(s.nrm, tri.v0) * bw + vec3_at(s.nrm, tri.v1) * bu + vec3_at(s.nrm, tri.v2) * bv);
      const rt3 nw = rt_normalize(rt_vec_mul_mat_dir(ln, inst.inverse));
      rt_gather_point& q = points[n];
      q.position[0] = pos.x; q.position[1] = pos.y; q.position[2] = pos.z;
      q.t_max = d.t_max;
      q.normal[0] = nw.x; q.normal[1] = nw.y; q.normal[2] = nw.z;
      q.pad = d.pad_base + i;
      texels[n] = i;
      if (weights) {
        weights[2 * (size_t)n] = bu;
        weights[2 * (size_t)n + 1] = bv;
      }
    }
    n++;
  }
  return n;
}

}  // namespace

extern "C" {

// The points of the scene uploaded to ctx.  atlas_uv: 2 f32 per vertex of the scene, or null = the scene's uvs.  points
// (W * H x rt_gather_point) and texels (W * H x u32) may both be null; owner: W * H i32; weights: W * H x 2 f32 or null.
// Returns n; UINT32_MAX when the descriptor names no instance or the scene has no draw command for it.
uint32_t bake_model_points(oracle_ctx* ctx, const rt_bake_desc* d, const float* atlas_uv, rt_gather_point* points, uint32_t* texels,
                           int32_t* owner, float* weights) {
  const Oracle& o = ctx->o;
  if (d->inst >= o.instances.size() || o.draw_commands.size() < 4 * o.instances.size()) return 0xffffffffu;
  BakeScene s;
  s.topo = o.topology.data();
  s.n_tris = (uint32_t)o.topology.size();
  s.pos = o.pos.data();
  s.nrm = o.nrm.data();
  s.uv = atlas_uv ? atlas_uv : o.uv.data();
  s.inst = o.instances.data();
  s.draw = o.draw_commands.data();
  return bake_points(s, *d, points, texels, owner, weights);
}

}  // extern "C"

#ifdef BAKE_MODEL_MAIN
// ---- hand-worked cases on the restated rule, as a program of its own (no scene, no oracle context)
namespace {

int failures = 0;
#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
      failures++;                                                \
    }                                                            \
  } while (0)

struct Mesh {
  std::vector<rt_topology> topo;
  std::vector<float> pos, nrm, uv;
  rt_instance inst;
  uint32_t draw[4];
  Mesh() {
    inst = rt_instance();
    for (int i = 0; i < 4; i++) inst.transform[5 * i] = inst.inverse[5 * i] = 1.0f;
  }
  uint32_t vertex(float x, float y, float z, float u, float v) {
    const float p[4] = {x, y, z, 1.0f}, n[4] = {0.0f, 0.0f, 1.0f, 0.0f};
    pos.insert(pos.end(), p, p + 4);
    nrm.insert(nrm.end(), n, n + 4);
    uv.push_back(u);
    uv.push_back(v);
    return (uint32_t)(uv.size() / 2 - 1);
  }
  void triangle(uint32_t a, uint32_t b, uint32_t c) {
    rt_topology t = rt_topology();
    t.v0 = a; t.v1 = b; t.v2 = c;
    topo.push_back(t);
  }
  // the position of a vertex is its uv, so a point's position must come back as its texel centre / (W, H)
  uint32_t run(uint32_t W, uint32_t H, std::vector<rt_gather_point>& points, std::vector<uint32_t>& texels, std::vector<int32_t>& owner) {
    draw[0] = 3u * (uint32_t)topo.size(); draw[1] = 1u; draw[2] = 0u; draw[3] = 0u;
    BakeScene s = {topo.data(), (uint32_t)topo.size(), pos.data(), nrm.data(), uv.data(), &inst, draw};
    rt_bake_desc d = rt_bake_desc();
    d.width = W; d.height = H; d.pad_base = 100u; d.t_max = 7.0f;
    points.assign((size_t)W * H, rt_gather_point());
    texels.assign((size_t)W * H, 0u);
    owner.assign((size_t)W * H, 0);
    return bake_points(s, d, points.data(), texels.data(), owner.data());
  }
};

void quad(Mesh& m) {   // uvs (0,0) (1,0) (1,1) (0,1): triangles (0,1,2) and (0,2,3)
  const uint32_t a = m.vertex(0, 0, 0, 0, 0), b = m.vertex(1, 0, 0, 1, 0), c = m.vertex(1, 1, 0, 1, 1), d = m.vertex(0, 1, 0, 0, 1);
  m.triangle(a, b, c);
  m.triangle(a, c, d);
}

}  // namespace

int main() {
  std::vector<rt_gather_point> P;
  std::vector<uint32_t> T;
  std::vector<int32_t> O;
  {   // the quad: every texel once; the diagonal x == y has E == 0 for both triangles and goes to triangle 0
    Mesh m;
    quad(m);
    const uint32_t W = 8;
    CHECK(m.run(W, W, P, T, O) == W * W);
    for (uint32_t y = 0; y < W; y++)
      for (uint32_t x = 0; x < W; x++) CHECK(O[y * W + x] == (x >= y ? 0 : 1));
    for (uint32_t j = 0; j < W * W; j++) {
      CHECK(T[j] == j && P[j].pad == 100u + j && P[j].t_max == 7.0f);
      CHECK(std::fabs(P[j].position[0] - ((j % W) + 0.5f) / W) < 1e-6f && std::fabs(P[j].position[1] - ((j / W) + 0.5f) / W) < 1e-6f);
      CHECK(P[j].normal[0] == 0.0f && P[j].normal[1] == 0.0f && std::fabs(P[j].normal[2] - 1.0f) < 1e-6f);
    }
    // shapes 1 x 1, 1 x 9 and 9 x 1: all covered, in order
    CHECK(m.run(1, 1, P, T, O) == 1 && O[0] == 0);
    CHECK(m.run(1, 9, P, T, O) == 9 && T[8] == 8);
    CHECK(m.run(9, 1, P, T, O) == 9 && T[8] == 8);
  }
  {   // the other winding owns the same texels; a duplicate loses everywhere
    Mesh m;
    const uint32_t a = m.vertex(0, 0, 0, 0, 0), b = m.vertex(1, 0, 0, 1, 0), c = m.vertex(1, 1, 0, 1, 1);
    m.triangle(a, c, b);
    m.triangle(a, b, c);
    CHECK(m.run(8, 8, P, T, O) == 36);
    for (uint32_t i = 0; i < 64; i++) CHECK(O[i] == ((i % 8) >= (i / 8) ? 0 : -1));
  }
  {   // one triangle over the whole atlas; a vertex exactly on a centre covers it
    Mesh m;
    m.triangle(m.vertex(0, 0, 0, -1, -1), m.vertex(0, 0, 0, 3, -1), m.vertex(0, 0, 0, -1, 3));
    CHECK(m.run(5, 3, P, T, O) == 15);
    Mesh v;
    v.triangle(v.vertex(0, 0, 0, 0.3125f, 0.3125f), v.vertex(0, 0, 0, 0.4f, 0.33f), v.vertex(0, 0, 0, 0.33f, 0.4f));
    CHECK(v.run(8, 8, P, T, O) == 1 && T[0] == 2 * 8 + 2);   // 0.3125 * 8 = 2.5: the centre of texel (2, 2)
  }
  {   // misses every centre; zero area; NaN, inf and 3e38 uvs: nothing
    Mesh m;
    m.triangle(m.vertex(0, 0, 0, 0.13f, 0.13f), m.vertex(0, 0, 0, 0.18f, 0.13f), m.vertex(0, 0, 0, 0.13f, 0.18f));
    m.triangle(m.vertex(0, 0, 0, 0, 0), m.vertex(0, 0, 0, 0.5f, 0.5f), m.vertex(0, 0, 0, 1, 1));
    const float bad[4] = {std::nanf(""), INFINITY, -INFINITY, 3e38f};
    for (float w : bad) m.triangle(m.vertex(0, 0, 0, w, 0), m.vertex(0, 0, 0, 1, 0), m.vertex(0, 0, 0, 1, 1));
    CHECK(m.run(8, 8, P, T, O) == 0);
    for (int32_t o : O) CHECK(o == -1);
  }
  std::printf(failures ? "bake model: %d checks FAILED\n" : "bake model: hand-worked cases ok\n", failures);
  return failures ? 1 : 0;
}
#endif
