/* addon.c — N-API (v8, plain C) shim over the C ABI of include/mi355rt.h and include/mi355scene.h.
 *
 * The reference's host code is TypeScript running in a browser; its WebGPURenderer talks to WebGPU.
 * Here a Node process loads this addon and index.js rebuilds the same class surface on top of it
 * (src/renderer/WebGPURenderer.ts:7-138, src/world-bridge.ts:172-205).  Every function is a thin
 * argument-unpacking wrapper: no rendering logic lives in this file.
 * Build: gcc -shared -fPIC -I/usr/include/node addon.c -L../lib -lmi355rt -lmi355scene -lmi355tex -Wl,-rpath,'$ORIGIN/../lib'
 */
#include <node_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "mi355rt.h"
#include "mi355scene.h"
#include "mi355tex.h"

#define NAPI_OK(env, call)                                              \
  do {                                                                  \
    if ((call) != napi_ok) {                                            \
      napi_throw_error((env), NULL, "N-API call failed: " #call);       \
      return NULL;                                                      \
    }                                                                   \
  } while (0)

static napi_value make_int(napi_env env, int v) {
  napi_value r;
  napi_create_int32(env, v, &r);
  return r;
}
static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value* argv) {
  size_t argc = want;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) {
    napi_throw_type_error(env, NULL, "wrong number of arguments");
    return 0;
  }
  return 1;
}
static void* get_ptr(napi_env env, napi_value v) {
  void* p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok) napi_throw_type_error(env, NULL, "expected a native handle");
  return p;
}
static uint32_t get_u32(napi_env env, napi_value v) {
  uint32_t x = 0;
  napi_get_value_uint32(env, v, &x);
  return x;
}
/* TypedArray / ArrayBuffer view -> (pointer, byte length) */
static int get_bytes(napi_env env, napi_value v, void** data, size_t* bytes) {
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  if (is_ta) {
    napi_typedarray_type t;
    size_t len = 0, off = 0;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &t, &len, data, &ab, &off) != napi_ok) return 0;
    size_t esz = (t == napi_int8_array || t == napi_uint8_array || t == napi_uint8_clamped_array) ? 1
                 : (t == napi_int16_array || t == napi_uint16_array)                              ? 2
                 : (t == napi_float64_array)                                                      ? 8
                                                                                                   : 4;
    *bytes = len * esz;
    return 1;
  }
  napi_valuetype vt;
  napi_typeof(env, v, &vt);
  if (vt == napi_null || vt == napi_undefined) {
    *data = NULL;
    *bytes = 0;
    return 1;
  }
  napi_throw_type_error(env, NULL, "expected a TypedArray");
  return 0;
}

/* ------------------------------------------------------------------ renderer */
static napi_value rtCreate(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  rt_ctx* c = rt_create((int)get_u32(env, a[0]));
  if (!c) {
    napi_throw_error(env, NULL, rt_last_error(NULL));  /* init() throws in the reference (WebGPUContext.ts:15,19) */
    return NULL;
  }
  napi_value ext;
  NAPI_OK(env, napi_create_external(env, c, NULL, NULL, &ext));
  return ext;
}
static napi_value rtDestroy(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  rt_destroy((rt_ctx*)get_ptr(env, a[0]));
  return NULL;
}
static napi_value rtLastError(napi_env env, napi_callback_info info) {
  napi_value a[1], s;
  if (!get_args(env, info, 1, a)) return NULL;
  napi_create_string_utf8(env, rt_last_error((rt_ctx*)get_ptr(env, a[0])), NAPI_AUTO_LENGTH, &s);
  return s;
}
static napi_value rtSetPipeline(napi_env env, napi_callback_info info) {
  napi_value a[3];
  if (!get_args(env, info, 3, a)) return NULL;
  return make_int(env, rt_set_pipeline((rt_ctx*)get_ptr(env, a[0]), get_u32(env, a[1]), get_u32(env, a[2])));
}
static napi_value rtResize(napi_env env, napi_callback_info info) {
  napi_value a[3];
  if (!get_args(env, info, 3, a)) return NULL;
  return make_int(env, rt_resize((rt_ctx*)get_ptr(env, a[0]), get_u32(env, a[1]), get_u32(env, a[2])));
}
static napi_value rtResetAccum(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  return make_int(env, rt_reset_accum((rt_ctx*)get_ptr(env, a[0])));
}
static napi_value rtUploadTextures(napi_env env, napi_callback_info info) {
  napi_value a[3];
  void* p;
  size_t n;
  if (!get_args(env, info, 3, a) || !get_bytes(env, a[1], &p, &n)) return NULL;
  return make_int(env, rt_upload_textures((rt_ctx*)get_ptr(env, a[0]), (const uint8_t*)p, get_u32(env, a[2])));
}
static napi_value rtUpload(napi_env env, napi_callback_info info) {
  napi_value a[3];
  void* p;
  size_t n;
  if (!get_args(env, info, 3, a) || !get_bytes(env, a[2], &p, &n)) return NULL;
  return make_int(env, rt_upload((rt_ctx*)get_ptr(env, a[0]), (rt_kind)get_u32(env, a[1]), p, n));
}
static napi_value rtUploadGeometry(napi_env env, napi_callback_info info) {
  napi_value a[4];
  void *v, *nr, *uv;
  size_t nv, nn, nu;
  if (!get_args(env, info, 4, a) || !get_bytes(env, a[1], &v, &nv) || !get_bytes(env, a[2], &nr, &nn) ||
      !get_bytes(env, a[3], &uv, &nu))
    return NULL;
  uint32_t count = (uint32_t)(nv / 16);
  if (nn < (size_t)count * 16 || nu < (size_t)count * 8) {
    napi_throw_range_error(env, NULL, "normal / uv arrays shorter than the vertex array");
    return NULL;
  }
  return make_int(env, rt_upload_geometry((rt_ctx*)get_ptr(env, a[0]), (const float*)v, (const float*)nr,
                                          (const float*)uv, count));
}
static napi_value rtUploadBVH(napi_env env, napi_callback_info info) {
  napi_value a[3];
  void *t, *b;
  size_t nt, nb;
  if (!get_args(env, info, 3, a) || !get_bytes(env, a[1], &t, &nt) || !get_bytes(env, a[2], &b, &nb)) return NULL;
  return make_int(env, rt_upload_bvh((rt_ctx*)get_ptr(env, a[0]), (const float*)t, (uint32_t)(nt / 32),
                                     (const float*)b, (uint32_t)(nb / 32)));
}
static napi_value rtSetScene(napi_env env, napi_callback_info info) {
  napi_value a[4];
  void* cam;
  size_t n;
  if (!get_args(env, info, 4, a) || !get_bytes(env, a[1], &cam, &n)) return NULL;
  if (n < 96) {
    napi_throw_range_error(env, NULL, "cameraData must hold 24 floats");
    return NULL;
  }
  return make_int(env, rt_set_scene((rt_ctx*)get_ptr(env, a[0]), (const float*)cam, get_u32(env, a[2]), get_u32(env, a[3])));
}
static napi_value rtCompute(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  return make_int(env, rt_compute((rt_ctx*)get_ptr(env, a[0]), get_u32(env, a[1])));
}
static napi_value rtComputeBatch(napi_env env, napi_callback_info info) { /* Uint32Array of frame counts */
  napi_value a[2];
  void* p;
  size_t n;
  if (!get_args(env, info, 2, a) || !get_bytes(env, a[1], &p, &n)) return NULL;
  return make_int(env, rt_compute_batch((rt_ctx*)get_ptr(env, a[0]), (const uint32_t*)p, (uint32_t)(n / 4)));
}
static napi_value rtPresent(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  return make_int(env, rt_present((rt_ctx*)get_ptr(env, a[0])));
}
static napi_value rtSync(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  return make_int(env, rt_sync((rt_ctx*)get_ptr(env, a[0])));
}
static napi_value rtCapture(napi_env env, napi_callback_info info) {
  napi_value a[2];
  void* p;
  size_t n;
  if (!get_args(env, info, 2, a) || !get_bytes(env, a[1], &p, &n)) return NULL;
  return make_int(env, rt_capture((rt_ctx*)get_ptr(env, a[0]), (uint8_t*)p, n));
}
static napi_value rtReadAccum(napi_env env, napi_callback_info info) {
  napi_value a[2];
  void* p;
  size_t n;
  if (!get_args(env, info, 2, a) || !get_bytes(env, a[1], &p, &n)) return NULL;
  return make_int(env, rt_read_accum((rt_ctx*)get_ptr(env, a[0]), (float*)p, n));
}
static napi_value rtGetCounters(napi_env env, napi_callback_info info) {
  napi_value a[1], arr;
  if (!get_args(env, info, 1, a)) return NULL;
  rt_counters c;
  memset(&c, 0, sizeof(c));
  rt_get_counters((rt_ctx*)get_ptr(env, a[0]), &c);
  const uint64_t v[6] = {c.primary_rays, c.extension_rays, c.shadow_rays, c.nodes_visited, c.tris_tested, c.shaded_hits};
  NAPI_OK(env, napi_create_array_with_length(env, 6, &arr));
  for (uint32_t i = 0; i < 6; i++) {
    napi_value d;
    napi_create_double(env, (double)v[i], &d);
    napi_set_element(env, arr, i, d);
  }
  return arr;
}

/* --------------------------------------------------------------------- world */
/* (sceneName, objSource | null, glbData | null) — World::new, lib.rs:45-102 */
static napi_value msCreate(napi_env env, napi_callback_info info) {
  napi_value a[3];
  void* glb = NULL;
  size_t glb_size = 0;
  if (!get_args(env, info, 3, a) || !get_bytes(env, a[2], &glb, &glb_size)) return NULL;
  char name[64];
  size_t len = 0;
  napi_get_value_string_utf8(env, a[0], name, sizeof(name), &len);
  char* obj = NULL;
  napi_valuetype vt;
  napi_typeof(env, a[1], &vt);
  if (vt == napi_string) {
    size_t olen = 0;
    napi_get_value_string_utf8(env, a[1], NULL, 0, &olen);
    obj = (char*)malloc(olen + 1);
    napi_get_value_string_utf8(env, a[1], obj, olen + 1, &olen);
  }
  ms_world* w = glb ? ms_world_create_glb(name, obj, (const uint8_t*)glb, glb_size) : ms_world_create(name, obj);
  free(obj);
  if (!w) {
    napi_throw_error(env, NULL, ms_last_error());
    return NULL;
  }
  napi_value ext;
  NAPI_OK(env, napi_create_external(env, w, NULL, NULL, &ext));
  return ext;
}
static napi_value msDestroy(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  ms_world_destroy((ms_world*)get_ptr(env, a[0]));
  return NULL;
}
static napi_value msUpdate(napi_env env, napi_callback_info info) {
  napi_value a[2];
  double t = 0;
  if (!get_args(env, info, 2, a)) return NULL;
  napi_get_value_double(env, a[1], &t);
  ms_world_update((ms_world*)get_ptr(env, a[0]), (float)t);
  return NULL;
}
static napi_value msUpdateCamera(napi_env env, napi_callback_info info) {
  napi_value a[3];
  double w = 0, h = 0;
  if (!get_args(env, info, 3, a)) return NULL;
  napi_get_value_double(env, a[1], &w);
  napi_get_value_double(env, a[2], &h);
  ms_world_update_camera((ms_world*)get_ptr(env, a[0]), (float)w, (float)h);
  return NULL;
}
/* msGet(world, name) -> Float32Array | Uint32Array copy (the worker also copies out of WASM memory,
 * src/worker/wasm-worker.ts:21-91) */
static napi_value msGet(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  const ms_world* w = (const ms_world*)get_ptr(env, a[0]);
  char name[32];
  size_t len = 0, n = 0;
  napi_get_value_string_utf8(env, a[1], name, sizeof(name), &len);
  const void* src = NULL;
  int is_u32 = 0;
  if (!strcmp(name, "vertices")) src = ms_world_vertices(w, &n);
  else if (!strcmp(name, "normals")) src = ms_world_normals(w, &n);
  else if (!strcmp(name, "uvs")) src = ms_world_uvs(w, &n);
  else if (!strcmp(name, "tlas")) src = ms_world_tlas(w, &n);
  else if (!strcmp(name, "blas")) src = ms_world_blas(w, &n);
  else if (!strcmp(name, "instances")) src = ms_world_instances(w, &n);
  else if (!strcmp(name, "camera")) src = ms_world_camera(w, &n);
  else if (!strcmp(name, "mesh_topology")) { src = ms_world_mesh_topology(w, &n); is_u32 = 1; }
  else if (!strcmp(name, "lights")) { src = ms_world_lights(w, &n); is_u32 = 1; }
  else if (!strcmp(name, "draw_commands")) { src = ms_world_draw_commands(w, &n); is_u32 = 1; }
  else {
    napi_throw_error(env, NULL, "unknown world array");
    return NULL;
  }
  void* dst = NULL;
  napi_value ab, ta;
  NAPI_OK(env, napi_create_arraybuffer(env, n * 4, &dst, &ab));
  if (n) memcpy(dst, src, n * 4);
  NAPI_OK(env, napi_create_typedarray(env, is_u32 ? napi_uint32_array : napi_float32_array, n, ab, 0, &ta));
  return ta;
}
static napi_value rtAllocTextureLayers(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  return make_int(env, rt_alloc_texture_layers((rt_ctx*)get_ptr(env, a[0]), get_u32(env, a[1])));
}
/* (ctx, layer, rgba | null, width, height) */
static napi_value rtUploadTextureImage(napi_env env, napi_callback_info info) {
  napi_value a[5];
  void* p = NULL;
  size_t n = 0;
  if (!get_args(env, info, 5, a) || !get_bytes(env, a[2], &p, &n)) return NULL;
  const uint32_t w = get_u32(env, a[3]), h = get_u32(env, a[4]);
  if (p && n < (size_t)w * h * 4) {
    napi_throw_error(env, NULL, "rtUploadTextureImage: buffer smaller than width * height * 4");
    return NULL;
  }
  return make_int(env, rt_upload_texture_image((rt_ctx*)get_ptr(env, a[0]), get_u32(env, a[1]), (const uint8_t*)p, w, h));
}
/* (encoded bytes) -> {data: Uint8Array, width, height}; throws with mt_last_error() when the blob does not decode */
static napi_value mtDecode(napi_env env, napi_callback_info info) {
  napi_value a[1];
  void* p = NULL;
  size_t n = 0;
  if (!get_args(env, info, 1, a) || !get_bytes(env, a[0], &p, &n)) return NULL;
  mt_image img;
  if (mt_decode((const uint8_t*)p, n, &img) != MT_OK) {
    napi_throw_error(env, NULL, mt_last_error());
    return NULL;
  }
  const size_t bytes = (size_t)img.width * img.height * 4;
  void* dst = NULL;
  napi_value ab, ta, obj, w, h;
  if (napi_create_arraybuffer(env, bytes, &dst, &ab) != napi_ok) {
    mt_free(&img);
    napi_throw_error(env, NULL, "mtDecode: allocation failed");
    return NULL;
  }
  memcpy(dst, img.rgba, bytes);
  const uint32_t iw = img.width, ih = img.height;
  mt_free(&img);
  NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, bytes, ab, 0, &ta));
  NAPI_OK(env, napi_create_object(env, &obj));
  NAPI_OK(env, napi_create_uint32(env, iw, &w));
  NAPI_OK(env, napi_create_uint32(env, ih, &h));
  NAPI_OK(env, napi_set_named_property(env, obj, "data", ta));
  NAPI_OK(env, napi_set_named_property(env, obj, "width", w));
  NAPI_OK(env, napi_set_named_property(env, obj, "height", h));
  return obj;
}
/* animations: get_animation_count/name, set_animation, load_animation_glb (lib.rs:106-147) */
static napi_value msAnimationNames(napi_env env, napi_callback_info info) {
  napi_value a[1], arr;
  if (!get_args(env, info, 1, a)) return NULL;
  const ms_world* w = (const ms_world*)get_ptr(env, a[0]);
  const size_t n = ms_world_animation_count(w);
  NAPI_OK(env, napi_create_array_with_length(env, n, &arr));
  for (size_t i = 0; i < n; i++) {
    napi_value s;
    NAPI_OK(env, napi_create_string_utf8(env, ms_world_animation_name(w, i), NAPI_AUTO_LENGTH, &s));
    NAPI_OK(env, napi_set_element(env, arr, (uint32_t)i, s));
  }
  return arr;
}
static napi_value msSetAnimation(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  ms_world_set_animation((ms_world*)get_ptr(env, a[0]), get_u32(env, a[1]));
  return NULL;
}
static napi_value msLoadAnimation(napi_env env, napi_callback_info info) {
  napi_value a[2];
  void* p = NULL;
  size_t n = 0;
  if (!get_args(env, info, 2, a) || !get_bytes(env, a[1], &p, &n)) return NULL;
  return make_int(env, ms_world_load_animation_glb((ms_world*)get_ptr(env, a[0]), (const uint8_t*)p, n));
}
/* (world, ctx | null): World::update(t) builds its BLASes with rt_build_blas (GPU) instead of the CPU builder */
static napi_value msSetBlasBuilder(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  napi_valuetype vt;
  napi_typeof(env, a[1], &vt);
  void* ctx = vt == napi_external ? get_ptr(env, a[1]) : NULL;
  ms_world_set_blas_builder((ms_world*)get_ptr(env, a[0]), ctx ? (ms_blas_builder)rt_build_blas : NULL, ctx);
  return NULL;
}
/* (world, ctx | null): the whole per-frame half of World::update(t) runs on the GPU inside the renderer's buffers
 * (rt_world_update); the host arrays are then not refreshed and nothing needs uploading */
static napi_value msSetDeviceUpdater(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  napi_valuetype vt;
  napi_typeof(env, a[1], &vt);
  void* ctx = vt == napi_external ? get_ptr(env, a[1]) : NULL;
  ms_world_set_device_updater((ms_world*)get_ptr(env, a[0]), ctx ? (ms_device_updater)rt_world_update : NULL, ctx);
  return NULL;
}
static napi_value msDeviceResident(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  return make_int(env, ms_world_device_resident((const ms_world*)get_ptr(env, a[0])));
}
static napi_value msLastError(napi_env env, napi_callback_info info) {
  napi_value s;
  (void)info;
  NAPI_OK(env, napi_create_string_utf8(env, ms_last_error(), NAPI_AUTO_LENGTH, &s));
  return s;
}
static napi_value msEncodedTextureCount(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  return make_int(env, (int)ms_world_encoded_texture_count((const ms_world*)get_ptr(env, a[0])));
}
/* (world, index) -> Uint8Array of the encoded image, or undefined for an external / missing image */
static napi_value msEncodedTexture(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  size_t n = 0;
  const uint8_t* src = ms_world_encoded_texture((const ms_world*)get_ptr(env, a[0]), get_u32(env, a[1]), &n);
  if (!src || n == 0) return NULL;
  void* dst = NULL;
  napi_value ab, ta;
  NAPI_OK(env, napi_create_arraybuffer(env, n, &dst, &ab));
  memcpy(dst, src, n);
  NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta));
  return ta;
}
static napi_value msTextureCount(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  return make_int(env, (int)ms_world_texture_count((const ms_world*)get_ptr(env, a[0])));
}
static napi_value msTexture(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  const uint8_t* src = ms_world_texture_rgba((const ms_world*)get_ptr(env, a[0]), get_u32(env, a[1]));
  if (!src) return NULL;
  void* dst = NULL;
  napi_value ab, ta;
  const size_t n = (size_t)1024 * 1024 * 4;
  NAPI_OK(env, napi_create_arraybuffer(env, n, &dst, &ab));
  memcpy(dst, src, n);
  NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta));
  return ta;
}

/* ------------------------------------------------------- the sharded image (rt_dist_*, mi355rt.h) */
static napi_value rtDeviceCount(napi_env env, napi_callback_info info) {
  (void)info;
  return make_int(env, rt_device_count());
}
static napi_value rtSetStripes(napi_env env, napi_callback_info info) {
  napi_value a[4];
  if (!get_args(env, info, 4, a)) return NULL;
  return make_int(env, rt_set_stripes((rt_ctx*)get_ptr(env, a[0]), get_u32(env, a[1]), get_u32(env, a[2]), get_u32(env, a[3])));
}
/* () -> Uint8Array(128); throws with rt_last_error(NULL) when RCCL cannot be loaded */
static napi_value rtDistUniqueId(napi_env env, napi_callback_info info) {
  (void)info;
  void* dst = NULL;
  napi_value ab, ta;
  NAPI_OK(env, napi_create_arraybuffer(env, 128, &dst, &ab));
  if (rt_dist_unique_id((uint8_t*)dst) < 0) {
    napi_throw_error(env, NULL, rt_last_error(NULL));
    return NULL;
  }
  NAPI_OK(env, napi_create_typedarray(env, napi_uint8_array, 128, ab, 0, &ta));
  return ta;
}
/* (ctx, rank, world, stripeRows, uniqueId: Uint8Array(128) | null) */
static napi_value rtDistInit(napi_env env, napi_callback_info info) {
  napi_value a[5];
  void* id = NULL;
  size_t n = 0;
  if (!get_args(env, info, 5, a) || !get_bytes(env, a[4], &id, &n)) return NULL;
  if (id && n != 128) {
    napi_throw_range_error(env, NULL, "rtDistInit: the unique id must be 128 bytes");
    return NULL;
  }
  return make_int(env, rt_dist_init((rt_ctx*)get_ptr(env, a[0]), get_u32(env, a[1]), get_u32(env, a[2]), get_u32(env, a[3]),
                                    (const uint8_t*)id));
}
static napi_value rtDistShutdown(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  return make_int(env, rt_dist_shutdown((rt_ctx*)get_ptr(env, a[0])));
}
static napi_value rtDistBlockBytes(napi_env env, napi_callback_info info) {
  napi_value a[1], d;
  if (!get_args(env, info, 1, a)) return NULL;
  NAPI_OK(env, napi_create_double(env, (double)rt_dist_block_bytes((const rt_ctx*)get_ptr(env, a[0])), &d));
  return d;
}
static napi_value rtPackStripes(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  return make_int(env, rt_pack_stripes((rt_ctx*)get_ptr(env, a[0])));
}
static napi_value rtDistReadBlock(napi_env env, napi_callback_info info) {
  napi_value a[2];
  void* p;
  size_t n;
  if (!get_args(env, info, 2, a) || !get_bytes(env, a[1], &p, &n)) return NULL;
  return make_int(env, rt_dist_read_block((rt_ctx*)get_ptr(env, a[0]), p, n));
}
static napi_value rtDistWriteBlock(napi_env env, napi_callback_info info) {
  napi_value a[3];
  void* p;
  size_t n;
  if (!get_args(env, info, 3, a) || !get_bytes(env, a[2], &p, &n)) return NULL;
  return make_int(env, rt_dist_write_block((rt_ctx*)get_ptr(env, a[0]), get_u32(env, a[1]), p, n));
}
static napi_value rtUnpackStripes(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  return make_int(env, rt_unpack_stripes((rt_ctx*)get_ptr(env, a[0])));
}
static napi_value rtGatherStripes(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  return make_int(env, rt_gather_stripes((rt_ctx*)get_ptr(env, a[0])));
}
static napi_value rtReadDisplay(napi_env env, napi_callback_info info) {
  napi_value a[2];
  void* p;
  size_t n;
  if (!get_args(env, info, 2, a) || !get_bytes(env, a[1], &p, &n)) return NULL;
  return make_int(env, rt_read_display((rt_ctx*)get_ptr(env, a[0]), (float*)p, n));
}

/* ------------------------------------------------------- ray queries (rt_trace_rays, mi355rt.h) */
static void set_u64_as_double(napi_env env, napi_value obj, const char* name, uint64_t v) {
  napi_value d;
  napi_create_double(env, (double)v, &d);
  napi_set_named_property(env, obj, name, d);
}
static napi_value ray_stats_object(napi_env env, const rt_ray_stats* st) {
  napi_value obj, d;
  if (napi_create_object(env, &obj) != napi_ok) return NULL;
  set_u64_as_double(env, obj, "rays", st->rays);
  set_u64_as_double(env, obj, "nodes_visited", st->nodes_visited);
  set_u64_as_double(env, obj, "tris_tested", st->tris_tested);
  set_u64_as_double(env, obj, "walk", st->walk);
  set_u64_as_double(env, obj, "lds", st->lds);
  set_u64_as_double(env, obj, "rayreg", st->rayreg);
  set_u64_as_double(env, obj, "workgroups", st->workgroups);
  napi_create_double(env, st->kernel_ms, &d);
  napi_set_named_property(env, obj, "kernel_ms", d);
  return obj;
}
/* (ctx, rays: Float32Array of 8 per ray {o, t_max, d, -}, mode, tMin, hits: Uint32Array of 4 per ray, wantStats)
 * -> status, or the stats object when wantStats and the call succeeded */
static napi_value rtTraceRays(napi_env env, napi_callback_info info) {
  napi_value a[6];
  void *rays = NULL, *hits = NULL;
  size_t nr = 0, nh = 0;
  double t_min = 0;
  bool want_stats = false;
  if (!get_args(env, info, 6, a) || !get_bytes(env, a[1], &rays, &nr) || !get_bytes(env, a[4], &hits, &nh)) return NULL;
  napi_get_value_double(env, a[3], &t_min);
  napi_get_value_bool(env, a[5], &want_stats);
  const size_t n = nr / sizeof(rt_ray);
  if (nr % sizeof(rt_ray) != 0 || nh < n * sizeof(rt_ray_hit) || n > 0x7fffffffu) {
    napi_throw_range_error(env, NULL, "rtTraceRays: rays must hold 8 floats per ray and hits 4 words per ray");
    return NULL;
  }
  rt_ray_stats st;
  const int rc = rt_trace_rays((rt_ctx*)get_ptr(env, a[0]), (const rt_ray*)rays, (uint32_t)n, (int)get_u32(env, a[2]), (float)t_min,
                               (rt_ray_hit*)hits, want_stats ? &st : NULL);
  if (rc < 0 || !want_stats) return make_int(env, rc);
  return ray_stats_object(env, &st);
}
static napi_value rtRayQueryStats(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  rt_ray_stats st;
  const int rc = rt_ray_query_stats((rt_ctx*)get_ptr(env, a[0]), &st);
  if (rc < 0) return make_int(env, rc);
  return ray_stats_object(env, &st);
}

/* ------------------------------------------------------- radiance queries (rt_trace_radiance, mi355rt.h) */
static napi_value radiance_stats_object(napi_env env, const rt_radiance_stats* st) {
  napi_value obj, d;
  if (napi_create_object(env, &obj) != napi_ok) return NULL;
  set_u64_as_double(env, obj, "rays", st->rays);
  set_u64_as_double(env, obj, "samples", st->samples);
  set_u64_as_double(env, obj, "extension_rays", st->extension_rays);
  set_u64_as_double(env, obj, "shadow_rays", st->shadow_rays);
  set_u64_as_double(env, obj, "shaded_hits", st->shaded_hits);
  set_u64_as_double(env, obj, "nodes_visited", st->nodes_visited);
  set_u64_as_double(env, obj, "tris_tested", st->tris_tested);
  set_u64_as_double(env, obj, "lds", st->lds);
  set_u64_as_double(env, obj, "workgroups", st->workgroups);
  napi_create_double(env, st->kernel_ms, &d);
  napi_set_named_property(env, obj, "kernel_ms", d);
  return obj;
}
/* (ctx, rays: Float32Array of 8 per ray {o, t_max, d, pad}, maxDepth, spp, seed, out: Float32Array of 4 per ray, wantStats)
 * -> status, or the stats object when wantStats and the call succeeded */
static napi_value rtTraceRadiance(napi_env env, napi_callback_info info) {
  napi_value a[7];
  void *rays = NULL, *out = NULL;
  size_t nr = 0, no = 0;
  bool want_stats = false;
  if (!get_args(env, info, 7, a) || !get_bytes(env, a[1], &rays, &nr) || !get_bytes(env, a[5], &out, &no)) return NULL;
  napi_get_value_bool(env, a[6], &want_stats);
  const size_t n = nr / sizeof(rt_ray);
  if (nr % sizeof(rt_ray) != 0 || no < n * sizeof(rt_radiance) || n > 0x7fffffffu) {
    napi_throw_range_error(env, NULL, "rtTraceRadiance: rays must hold 8 floats per ray and out 4 floats per ray");
    return NULL;
  }
  rt_radiance_stats st;
  const int rc = rt_trace_radiance((rt_ctx*)get_ptr(env, a[0]), (const rt_ray*)rays, (uint32_t)n, get_u32(env, a[2]),
                                   get_u32(env, a[3]), get_u32(env, a[4]), (rt_radiance*)out, want_stats ? &st : NULL);
  if (rc < 0 || !want_stats) return make_int(env, rc);
  return radiance_stats_object(env, &st);
}

/* ------------------------------------------------------- irradiance gathers (rt_gather_irradiance, mi355rt.h) */
/* (ctx, points: Float32Array of 8 per point {position, t_max, normal, pad}, maxDepth, spp, seed, out: Float32Array of 4 per
 * point, wantStats) -> status, or the stats object when wantStats and the call succeeded */
static napi_value rtGatherIrradiance(napi_env env, napi_callback_info info) {
  napi_value a[7];
  void *points = NULL, *out = NULL;
  size_t np = 0, no = 0;
  bool want_stats = false;
  if (!get_args(env, info, 7, a) || !get_bytes(env, a[1], &points, &np) || !get_bytes(env, a[5], &out, &no)) return NULL;
  napi_get_value_bool(env, a[6], &want_stats);
  const size_t n = np / sizeof(rt_gather_point);
  if (np % sizeof(rt_gather_point) != 0 || no < n * sizeof(rt_irradiance) || n > 0x7fffffffu) {
    napi_throw_range_error(env, NULL, "rtGatherIrradiance: points must hold 8 floats per point and out 4 floats per point");
    return NULL;
  }
  rt_radiance_stats st;
  const int rc = rt_gather_irradiance((rt_ctx*)get_ptr(env, a[0]), (const rt_gather_point*)points, (uint32_t)n, get_u32(env, a[2]),
                                      get_u32(env, a[3]), get_u32(env, a[4]), (rt_irradiance*)out, want_stats ? &st : NULL);
  if (rc < 0 || !want_stats) return make_int(env, rc);
  return radiance_stats_object(env, &st);
}

/* ------------------------------------------------------- probe gathers (rt_gather_probes, mi355rt.h) */
/* (ctx, probes: Float32Array of 8 per probe {position, t_max, 3 unused, pad}, maxDepth, spp, seed, out: Float32Array of 28 per
 * probe {sh[9][3], hit_fraction}, wantStats) -> status, or the stats object when wantStats and the call succeeded */
static napi_value rtGatherProbes(napi_env env, napi_callback_info info) {
  napi_value a[7];
  void *probes = NULL, *out = NULL;
  size_t np = 0, no = 0;
  bool want_stats = false;
  if (!get_args(env, info, 7, a) || !get_bytes(env, a[1], &probes, &np) || !get_bytes(env, a[5], &out, &no)) return NULL;
  napi_get_value_bool(env, a[6], &want_stats);
  const size_t n = np / sizeof(rt_probe);
  if (np % sizeof(rt_probe) != 0 || no < n * sizeof(rt_probe_sh9) || n > 0x7fffffffu) {
    napi_throw_range_error(env, NULL, "rtGatherProbes: probes must hold 8 floats per probe and out 28 floats per probe");
    return NULL;
  }
  rt_radiance_stats st;
  const int rc = rt_gather_probes((rt_ctx*)get_ptr(env, a[0]), (const rt_probe*)probes, (uint32_t)n, get_u32(env, a[2]),
                                  get_u32(env, a[3]), get_u32(env, a[4]), (rt_probe_sh9*)out, want_stats ? &st : NULL);
  if (rc < 0 || !want_stats) return make_int(env, rc);
  return radiance_stats_object(env, &st);
}

/* ------------------------------------------------------- irradiance volumes (rt_bake_volume, rt_sample_volume, mi355rt.h) */
/* the 64 bytes of an rt_volume_desc in a typed array, and its probe count (0: a dimension is 0 or the product overflows) */
static const rt_volume_desc* get_volume_desc(napi_env env, napi_value v, size_t* n) {
  void* d = NULL;
  size_t nd = 0;
  if (!get_bytes(env, v, &d, &nd)) return NULL;
  if (nd != sizeof(rt_volume_desc)) {
    napi_throw_range_error(env, NULL, "a volume descriptor is 64 bytes");
    return NULL;
  }
  const rt_volume_desc* desc = (const rt_volume_desc*)d;
  const uint64_t probes = (uint64_t)desc->nx * desc->ny * desc->nz;
  *n = (desc->nx > 1024 || desc->ny > 1024 || desc->nz > 1024 || probes > (1u << 24)) ? 0 : (size_t)probes;
  return desc;
}
/* (ctx, desc: 64 bytes, maxDepth, spp, seed, out: Float32Array of 28 per probe, wantStats) -> status, or the stats object */
static napi_value rtBakeVolume(napi_env env, napi_callback_info info) {
  napi_value a[7];
  void* out = NULL;
  size_t n = 0, no = 0;
  bool want_stats = false;
  if (!get_args(env, info, 7, a) || !get_bytes(env, a[5], &out, &no)) return NULL;
  const rt_volume_desc* desc = get_volume_desc(env, a[1], &n);
  if (!desc) return NULL;
  napi_get_value_bool(env, a[6], &want_stats);
  if (no < n * sizeof(rt_probe_sh9)) {
    napi_throw_range_error(env, NULL, "rtBakeVolume: out must hold 28 floats per probe");
    return NULL;
  }
  rt_radiance_stats st;
  const int rc = rt_bake_volume((rt_ctx*)get_ptr(env, a[0]), desc, get_u32(env, a[2]), get_u32(env, a[3]), get_u32(env, a[4]),
                                (rt_probe_sh9*)out, want_stats ? &st : NULL);
  if (rc < 0 || !want_stats) return make_int(env, rc);
  return radiance_stats_object(env, &st);
}
/* (ctx, desc: 64 bytes, volume: Float32Array of 28 per probe, points: Float32Array of 8 per point, out: Float32Array of 4 per
 * point) -> status */
static napi_value rtSampleVolume(napi_env env, napi_callback_info info) {
  napi_value a[5];
  void *volume = NULL, *points = NULL, *out = NULL;
  size_t n = 0, nv = 0, np = 0, no = 0;
  if (!get_args(env, info, 5, a) || !get_bytes(env, a[2], &volume, &nv) || !get_bytes(env, a[3], &points, &np) ||
      !get_bytes(env, a[4], &out, &no))
    return NULL;
  const rt_volume_desc* desc = get_volume_desc(env, a[1], &n);
  if (!desc) return NULL;
  const size_t m = np / sizeof(rt_gather_point);
  if (nv < n * sizeof(rt_probe_sh9) || np % sizeof(rt_gather_point) != 0 || no < m * sizeof(rt_irradiance) || m > 0x7fffffffu) {
    napi_throw_range_error(env, NULL, "rtSampleVolume: volume must hold 28 floats per probe, points 8 and out 4 floats per point");
    return NULL;
  }
  return make_int(env, rt_sample_volume((rt_ctx*)get_ptr(env, a[0]), desc, (const rt_probe_sh9*)volume,
                                        (const rt_gather_point*)points, (uint32_t)m, (rt_irradiance*)out));
}
/* (ctx, desc: 64 bytes, format, volume: Float32Array of 28 per probe, out: a typed array of seven layers) -> status */
static napi_value rtEncodeVolume(napi_env env, napi_callback_info info) {
  napi_value a[5];
  void *volume = NULL, *out = NULL;
  size_t n = 0, nv = 0, no = 0;
  if (!get_args(env, info, 5, a) || !get_bytes(env, a[3], &volume, &nv) || !get_bytes(env, a[4], &out, &no)) return NULL;
  const rt_volume_desc* desc = get_volume_desc(env, a[1], &n);
  if (!desc) return NULL;
  if (nv < n * sizeof(rt_probe_sh9)) {
    napi_throw_range_error(env, NULL, "rtEncodeVolume: volume must hold 28 floats per probe");
    return NULL;
  }
  return make_int(env, rt_encode_volume((rt_ctx*)get_ptr(env, a[0]), desc, get_u32(env, a[2]), (const rt_probe_sh9*)volume, out, no));
}

/* ------------------------------------------------------- probe visibility maps (rt_bake_volume_visibility, mi355rt.h) */
/* the 32 bytes of an rt_volume_visibility_desc in a typed array, and the texels of one map (0: the library will refuse the size) */
static const rt_volume_visibility_desc* get_visibility_desc(napi_env env, napi_value v, size_t* map) {
  void* d = NULL;
  size_t nd = 0;
  if (!get_bytes(env, v, &d, &nd)) return NULL;
  if (nd != sizeof(rt_volume_visibility_desc)) {
    napi_throw_range_error(env, NULL, "a visibility descriptor is 32 bytes");
    return NULL;
  }
  const rt_volume_visibility_desc* desc = (const rt_volume_visibility_desc*)d;
  *map = desc->size > 32 ? 0 : (size_t)desc->size * desc->size;
  return desc;
}
/* (ctx, desc: 64 bytes, vis: 32 bytes, seed, out: Float32Array of 2 per texel, wantStats) -> status, or the stats object */
static napi_value rtBakeVolumeVisibility(napi_env env, napi_callback_info info) {
  napi_value a[6];
  void* out = NULL;
  size_t n = 0, map = 0, no = 0;
  bool want_stats = false;
  if (!get_args(env, info, 6, a) || !get_bytes(env, a[4], &out, &no)) return NULL;
  const rt_volume_desc* desc = get_volume_desc(env, a[1], &n);
  if (!desc) return NULL;
  const rt_volume_visibility_desc* vis = get_visibility_desc(env, a[2], &map);
  if (!vis) return NULL;
  napi_get_value_bool(env, a[5], &want_stats);
  if (no < n * map * 8) {
    napi_throw_range_error(env, NULL, "rtBakeVolumeVisibility: out must hold 2 floats per texel of every probe's map");
    return NULL;
  }
  rt_ray_stats st;
  const int rc = rt_bake_volume_visibility((rt_ctx*)get_ptr(env, a[0]), desc, vis, get_u32(env, a[3]), (float*)out,
                                           want_stats ? &st : NULL);
  if (rc < 0 || !want_stats) return make_int(env, rc);
  return ray_stats_object(env, &st);
}
/* (ctx, desc: 64 bytes, vis: 32 bytes, volume: Float32Array of 28 per probe, visibility: Float32Array of 2 per texel, points:
 * Float32Array of 8 per point, out: Float32Array of 4 per point) -> status */
static napi_value rtSampleVolumeVisible(napi_env env, napi_callback_info info) {
  napi_value a[7];
  void *volume = NULL, *maps = NULL, *points = NULL, *out = NULL;
  size_t n = 0, map = 0, nv = 0, nm = 0, np = 0, no = 0;
  if (!get_args(env, info, 7, a) || !get_bytes(env, a[3], &volume, &nv) || !get_bytes(env, a[4], &maps, &nm) ||
      !get_bytes(env, a[5], &points, &np) || !get_bytes(env, a[6], &out, &no))
    return NULL;
  const rt_volume_desc* desc = get_volume_desc(env, a[1], &n);
  if (!desc) return NULL;
  const rt_volume_visibility_desc* vis = get_visibility_desc(env, a[2], &map);
  if (!vis) return NULL;
  const size_t m = np / sizeof(rt_gather_point);
  if (nv < n * sizeof(rt_probe_sh9) || nm < n * map * 8 || np % sizeof(rt_gather_point) != 0 || no < m * sizeof(rt_irradiance) ||
      m > 0x7fffffffu) {
    napi_throw_range_error(env, NULL, "rtSampleVolumeVisible: volume must hold 28 floats per probe, visibility 2 per texel, points 8 "
                                      "and out 4 floats per point");
    return NULL;
  }
  return make_int(env, rt_sample_volume_visible((rt_ctx*)get_ptr(env, a[0]), desc, vis, (const rt_probe_sh9*)volume,
                                                (const float*)maps, (const rt_gather_point*)points, (uint32_t)m,
                                                (rt_irradiance*)out));
}
/* (ctx, desc: 64 bytes, vis: 32 bytes, format, visibility: Float32Array of 2 per texel, out: a typed array of the tiled image)
 * -> status */
static napi_value rtEncodeVolumeVisibility(napi_env env, napi_callback_info info) {
  napi_value a[6];
  void *maps = NULL, *out = NULL;
  size_t n = 0, map = 0, nm = 0, no = 0;
  if (!get_args(env, info, 6, a) || !get_bytes(env, a[4], &maps, &nm) || !get_bytes(env, a[5], &out, &no)) return NULL;
  const rt_volume_desc* desc = get_volume_desc(env, a[1], &n);
  if (!desc) return NULL;
  const rt_volume_visibility_desc* vis = get_visibility_desc(env, a[2], &map);
  if (!vis) return NULL;
  if (nm < n * map * 8) {
    napi_throw_range_error(env, NULL, "rtEncodeVolumeVisibility: visibility must hold 2 floats per texel of every probe's map");
    return NULL;
  }
  return make_int(env, rt_encode_volume_visibility((rt_ctx*)get_ptr(env, a[0]), desc, vis, get_u32(env, a[3]), (const float*)maps,
                                                   out, no));
}

/* ------------------------------------------------------- reflection probes (rt_bake_reflection, rt_filter_reflection, mi355rt.h) */
/* the 32 bytes of an rt_reflection_desc in a typed array, and the texels of its level 0 and of a chain (0: the library will
 * refuse the descriptor) */
static const rt_reflection_desc* get_reflection_desc(napi_env env, napi_value v, size_t* map, size_t* chain) {
  void* d = NULL;
  size_t nd = 0;
  if (!get_bytes(env, v, &d, &nd)) return NULL;
  if (nd != sizeof(rt_reflection_desc)) {
    napi_throw_range_error(env, NULL, "a reflection descriptor is 32 bytes");
    return NULL;
  }
  const rt_reflection_desc* desc = (const rt_reflection_desc*)d;
  *map = *chain = 0;
  if (desc->size >= 8 && desc->size <= 512 && desc->levels >= 2 && desc->levels <= 32) {
    *map = (size_t)desc->size * desc->size;
    for (uint32_t m = 0; m < desc->levels; m++) *chain += (size_t)(desc->size >> m) * (desc->size >> m);
  }
  return desc;
}
/* (ctx, desc: 32 bytes, probes: Float32Array of 8 per probe, maxDepth, seed, out: Float32Array of a chain per probe, wantStats)
 * -> status, or the stats object when wantStats and the call succeeded */
static napi_value rtBakeReflection(napi_env env, napi_callback_info info) {
  napi_value a[7];
  void *probes = NULL, *out = NULL;
  size_t np = 0, no = 0, map = 0, chain = 0;
  bool want_stats = false;
  if (!get_args(env, info, 7, a) || !get_bytes(env, a[2], &probes, &np) || !get_bytes(env, a[5], &out, &no)) return NULL;
  const rt_reflection_desc* desc = get_reflection_desc(env, a[1], &map, &chain);
  if (!desc) return NULL;
  napi_get_value_bool(env, a[6], &want_stats);
  const size_t n = np / sizeof(rt_probe);
  if (np % sizeof(rt_probe) != 0 || n > 0x7fffffffu || no < n * chain * 16) {
    napi_throw_range_error(env, NULL, "rtBakeReflection: probes must hold 8 floats per probe and out a chain of 4 floats per texel per probe");
    return NULL;
  }
  rt_radiance_stats st;
  const int rc = rt_bake_reflection((rt_ctx*)get_ptr(env, a[0]), desc, (const rt_probe*)probes, (uint32_t)n, get_u32(env, a[3]),
                                    get_u32(env, a[4]), (float*)out, want_stats ? &st : NULL);
  if (rc < 0 || !want_stats) return make_int(env, rc);
  return radiance_stats_object(env, &st);
}
/* (ctx, desc: 32 bytes, maps: Float32Array of size * size * 4 per probe, out: Float32Array of a chain per probe) -> status */
static napi_value rtFilterReflection(napi_env env, napi_callback_info info) {
  napi_value a[4];
  void *maps = NULL, *out = NULL;
  size_t nm = 0, no = 0, map = 0, chain = 0;
  if (!get_args(env, info, 4, a) || !get_bytes(env, a[2], &maps, &nm) || !get_bytes(env, a[3], &out, &no)) return NULL;
  const rt_reflection_desc* desc = get_reflection_desc(env, a[1], &map, &chain);
  if (!desc) return NULL;
  const size_t n = map ? nm / (map * 16) : 0;
  if ((map && nm % (map * 16) != 0) || n > 0x7fffffffu || no < n * chain * 16) {
    napi_throw_range_error(env, NULL, "rtFilterReflection: maps must hold size * size texels of 4 floats per probe and out a chain per probe");
    return NULL;
  }
  return make_int(env, rt_filter_reflection((rt_ctx*)get_ptr(env, a[0]), desc, (const float*)maps, (uint32_t)n, (float*)out));
}

/* (ctx, desc: the 32 bytes of an rt_reflection_sample_desc, chains: Float32Array of whole chains, probes and boxes: Float32Array
 * of 8 per chain or null (read with the parallax flag only), queries: 8 floats per query {position, probe bits, direction,
 * roughness}, out: Float32Array of 4 per query) -> status */
static napi_value rtSampleReflection(napi_env env, napi_callback_info info) {
  napi_value a[7];
  void *d = NULL, *chains = NULL, *probes = NULL, *boxes = NULL, *queries = NULL, *out = NULL;
  size_t nd = 0, nc = 0, np = 0, nb = 0, nq = 0, no = 0, chain = 0;
  if (!get_args(env, info, 7, a) || !get_bytes(env, a[1], &d, &nd) || !get_bytes(env, a[2], &chains, &nc) ||
      !get_bytes(env, a[3], &probes, &np) || !get_bytes(env, a[4], &boxes, &nb) || !get_bytes(env, a[5], &queries, &nq) ||
      !get_bytes(env, a[6], &out, &no))
    return NULL;
  if (nd != sizeof(rt_reflection_sample_desc)) {
    napi_throw_range_error(env, NULL, "a reflection sample descriptor is 32 bytes");
    return NULL;
  }
  const rt_reflection_sample_desc* desc = (const rt_reflection_sample_desc*)d;
  if (desc->size >= 8 && desc->size <= 512 && desc->levels >= 2 && desc->levels <= 32)   /* else 0: the library will refuse it */
    for (uint32_t m = 0; m < desc->levels; m++) chain += (size_t)(desc->size >> m) * (desc->size >> m);
  const size_t n_probes = chain ? nc / (chain * 16) : 0, n = nq / sizeof(rt_reflection_query);
  const bool parallax = (desc->flags & RT_REFLECTION_SAMPLE_PARALLAX) != 0;
  if ((chain && nc % (chain * 16) != 0) || n_probes > 0x7fffffffu || nq % sizeof(rt_reflection_query) != 0 || n > 0x7fffffffu ||
      no < n * 16 || (parallax && probes && np < n_probes * sizeof(rt_probe)) ||   /* (a missing array: the library refuses it) */
      (parallax && boxes && nb < n_probes * sizeof(rt_reflection_box))) {
    napi_throw_range_error(env, NULL, "rtSampleReflection: chains must hold whole chains of 4 floats per texel, probes and boxes 8 "
                                      "floats per chain, queries 8 and out 4 floats per query");
    return NULL;
  }
  return make_int(env, rt_sample_reflection((rt_ctx*)get_ptr(env, a[0]), desc, (const float*)chains, (uint32_t)n_probes,
                                            (const rt_probe*)probes, (const rt_reflection_box*)boxes,
                                            (const rt_reflection_query*)queries, (uint32_t)n, (float*)out));
}

/* ------------------------------------------------------- directional gathers (rt_gather_directional, mi355rt.h) */
/* (ctx, points: Float32Array of 8 per point {position, t_max, normal, pad}, maxDepth, spp, seed, out: Float32Array of 16 per
 * point, four rows {sh[k].rgb, hit_fraction}, wantStats) -> status, or the stats object when wantStats and the call succeeded */
static napi_value rtGatherDirectional(napi_env env, napi_callback_info info) {
  napi_value a[7];
  void *points = NULL, *out = NULL;
  size_t np = 0, no = 0;
  bool want_stats = false;
  if (!get_args(env, info, 7, a) || !get_bytes(env, a[1], &points, &np) || !get_bytes(env, a[5], &out, &no)) return NULL;
  napi_get_value_bool(env, a[6], &want_stats);
  const size_t n = np / sizeof(rt_gather_point);
  if (np % sizeof(rt_gather_point) != 0 || no < n * sizeof(rt_directional) || n > 0x7fffffffu) {
    napi_throw_range_error(env, NULL, "rtGatherDirectional: points must hold 8 floats per point and out 16 floats per point");
    return NULL;
  }
  rt_radiance_stats st;
  const int rc = rt_gather_directional((rt_ctx*)get_ptr(env, a[0]), (const rt_gather_point*)points, (uint32_t)n,
                                       get_u32(env, a[2]), get_u32(env, a[3]), get_u32(env, a[4]), (rt_directional*)out,
                                       want_stats ? &st : NULL);
  if (rc < 0 || !want_stats) return make_int(env, rc);
  return radiance_stats_object(env, &st);
}

/* ------------------------------------------------------- lightmap bakes (rt_bake_points / rt_bake_irradiance, mi355rt.h) */
static double get_f64(napi_env env, napi_value v) {
  double x = 0.0;
  napi_get_value_double(env, v, &x);
  return x;
}
/* [inst, width, height, padBase] and tMax -> descriptor */
static rt_bake_desc bake_desc(napi_env env, const napi_value* a) {
  rt_bake_desc d;
  memset(&d, 0, sizeof(d));
  d.inst = get_u32(env, a[0]);
  d.width = get_u32(env, a[1]);
  d.height = get_u32(env, a[2]);
  d.pad_base = get_u32(env, a[3]);
  d.t_max = (float)get_f64(env, a[4]);
  return d;
}
/* (ctx, inst, width, height, padBase, tMax, atlasUv: Float32Array of 2 per scene vertex or null, points: Float32Array of 8
 * per record, texels: Uint32Array, owner: Int32Array of width * height or null) -> the number of covered texels, or a
 * negative status; min(n, records the arrays hold) records are written */
static napi_value rtBakePoints(napi_env env, napi_callback_info info) {
  napi_value a[10];
  void *uv = NULL, *points = NULL, *texels = NULL, *owner = NULL;
  size_t nuv = 0, np = 0, nt = 0, no = 0;
  if (!get_args(env, info, 10, a) || !get_bytes(env, a[6], &uv, &nuv) || !get_bytes(env, a[7], &points, &np) ||
      !get_bytes(env, a[8], &texels, &nt) || !get_bytes(env, a[9], &owner, &no))
    return NULL;
  const rt_bake_desc d = bake_desc(env, a + 1);
  size_t cap = np / sizeof(rt_gather_point);
  if (nt / 4 < cap) cap = nt / 4;
  if (cap > 0xffffffffu || nuv % 8 != 0 || nuv / 8 > 0xffffffffu || (owner && no / 4 < (size_t)d.width * d.height)) {
    napi_throw_range_error(env, NULL, "rtBakePoints: atlasUv must hold 2 floats per vertex and owner width * height words");
    return NULL;
  }
  uint32_t n = 0;
  const int rc = rt_bake_points((rt_ctx*)get_ptr(env, a[0]), &d, (const float*)uv, (uint32_t)(nuv / 8), (rt_gather_point*)points,
                                (uint32_t*)texels, (uint32_t)cap, &n, (int32_t*)owner);
  if (rc < 0) return make_int(env, rc);
  napi_value r;
  napi_create_uint32(env, n, &r);
  return r;
}
/* (ctx, inst, width, height, padBase, tMax, atlasUv or null, maxDepth, spp, seed, atlas: Float32Array of 4 per texel,
 * wantStats) -> {covered, stats?}, or a negative status */
static napi_value rtBakeIrradiance(napi_env env, napi_callback_info info) {
  napi_value a[12];
  void *uv = NULL, *atlas = NULL;
  size_t nuv = 0, na = 0;
  bool want_stats = false;
  if (!get_args(env, info, 12, a) || !get_bytes(env, a[6], &uv, &nuv) || !get_bytes(env, a[10], &atlas, &na)) return NULL;
  napi_get_value_bool(env, a[11], &want_stats);
  const rt_bake_desc d = bake_desc(env, a + 1);
  if (nuv % 8 != 0 || nuv / 8 > 0xffffffffu || na / sizeof(rt_irradiance) < (size_t)d.width * d.height) {
    napi_throw_range_error(env, NULL, "rtBakeIrradiance: atlasUv must hold 2 floats per vertex and atlas 4 floats per texel");
    return NULL;
  }
  rt_radiance_stats st;
  uint32_t n = 0;
  const int rc = rt_bake_irradiance((rt_ctx*)get_ptr(env, a[0]), &d, (const float*)uv, (uint32_t)(nuv / 8), get_u32(env, a[7]),
                                    get_u32(env, a[8]), get_u32(env, a[9]), (rt_irradiance*)atlas, &n, want_stats ? &st : NULL);
  if (rc < 0) return make_int(env, rc);
  napi_value obj, v;
  if (napi_create_object(env, &obj) != napi_ok) return NULL;
  napi_create_uint32(env, n, &v);
  napi_set_named_property(env, obj, "covered", v);
  if (want_stats) napi_set_named_property(env, obj, "stats", radiance_stats_object(env, &st));
  return obj;
}

/* ------------------------------------------------------- atlas bakes (rt_bake_atlas_points / rt_bake_atlas_irradiance) */
/* [width, height, padBase, tMax] and the entries (Uint32Array of 8 words per rt_bake_rect) -> descriptor; false: thrown */
static bool bake_atlas_desc(napi_env env, const napi_value* a, size_t entry_bytes, rt_bake_atlas_desc* d) {
  memset(d, 0, sizeof(*d));
  d->width = get_u32(env, a[0]);
  d->height = get_u32(env, a[1]);
  d->pad_base = get_u32(env, a[2]);
  d->t_max = (float)get_f64(env, a[3]);
  if (entry_bytes % sizeof(rt_bake_rect) != 0 || entry_bytes / sizeof(rt_bake_rect) > 0xffffffffu) {
    napi_throw_range_error(env, NULL, "atlas bake: entries must hold 8 words per entry");
    return false;
  }
  d->n_entries = (uint32_t)(entry_bytes / sizeof(rt_bake_rect));
  return true;
}
/* (ctx, width, height, padBase, tMax, entries: Uint32Array of 8 per entry {inst, x, y, w, h, 0, 0, 0}, atlasUv or null, points,
 * texels, owner: Int32Array of 2 * width * height or null) -> the number of covered texels, or a negative status */
static napi_value rtBakeAtlasPoints(napi_env env, napi_callback_info info) {
  napi_value a[10];
  void *entries = NULL, *uv = NULL, *points = NULL, *texels = NULL, *owner = NULL;
  size_t ne = 0, nuv = 0, np = 0, nt = 0, no = 0;
  if (!get_args(env, info, 10, a) || !get_bytes(env, a[5], &entries, &ne) || !get_bytes(env, a[6], &uv, &nuv) ||
      !get_bytes(env, a[7], &points, &np) || !get_bytes(env, a[8], &texels, &nt) || !get_bytes(env, a[9], &owner, &no))
    return NULL;
  rt_bake_atlas_desc d;
  if (!bake_atlas_desc(env, a + 1, ne, &d)) return NULL;
  size_t cap = np / sizeof(rt_gather_point);
  if (nt / 4 < cap) cap = nt / 4;
  if (cap > 0xffffffffu || nuv % 8 != 0 || nuv / 8 > 0xffffffffu || (owner && no / 8 < (size_t)d.width * d.height)) {
    napi_throw_range_error(env, NULL, "rtBakeAtlasPoints: atlasUv must hold 2 floats per vertex and owner 2 words per texel");
    return NULL;
  }
  uint32_t n = 0;
  const int rc = rt_bake_atlas_points((rt_ctx*)get_ptr(env, a[0]), &d, (const rt_bake_rect*)entries, (const float*)uv,
                                      (uint32_t)(nuv / 8), (rt_gather_point*)points, (uint32_t*)texels, (uint32_t)cap, &n,
                                      (int32_t*)owner);
  if (rc < 0) return make_int(env, rc);
  napi_value r;
  napi_create_uint32(env, n, &r);
  return r;
}
/* (ctx, width, height, padBase, tMax, entries, atlasUv or null, maxDepth, spp, seed, atlas: Float32Array of 4 per texel,
 * wantStats) -> {covered, stats?}, or a negative status */
static napi_value rtBakeAtlasIrradiance(napi_env env, napi_callback_info info) {
  napi_value a[12];
  void *entries = NULL, *uv = NULL, *atlas = NULL;
  size_t ne = 0, nuv = 0, na = 0;
  bool want_stats = false;
  if (!get_args(env, info, 12, a) || !get_bytes(env, a[5], &entries, &ne) || !get_bytes(env, a[6], &uv, &nuv) ||
      !get_bytes(env, a[10], &atlas, &na))
    return NULL;
  napi_get_value_bool(env, a[11], &want_stats);
  rt_bake_atlas_desc d;
  if (!bake_atlas_desc(env, a + 1, ne, &d)) return NULL;
  if (nuv % 8 != 0 || nuv / 8 > 0xffffffffu || na / sizeof(rt_irradiance) < (size_t)d.width * d.height) {
    napi_throw_range_error(env, NULL, "rtBakeAtlasIrradiance: atlasUv must hold 2 floats per vertex and atlas 4 floats per texel");
    return NULL;
  }
  rt_radiance_stats st;
  uint32_t n = 0;
  const int rc = rt_bake_atlas_irradiance((rt_ctx*)get_ptr(env, a[0]), &d, (const rt_bake_rect*)entries, (const float*)uv,
                                          (uint32_t)(nuv / 8), get_u32(env, a[7]), get_u32(env, a[8]), get_u32(env, a[9]),
                                          (rt_irradiance*)atlas, &n, want_stats ? &st : NULL);
  if (rc < 0) return make_int(env, rc);
  napi_value obj, v;
  if (napi_create_object(env, &obj) != napi_ok) return NULL;
  napi_create_uint32(env, n, &v);
  napi_set_named_property(env, obj, "covered", v);
  if (want_stats) napi_set_named_property(env, obj, "stats", radiance_stats_object(env, &st));
  return obj;
}

/* ------------------------------------------------------- atlas dilation (rt_dilate_atlas, mi355rt.h) */
/* (ctx, width, height, radius, atlas: Float32Array of 4 per texel, dilated in place, src: Uint32Array of width * height or
 * null) -> the number of filled texels, or a negative status */
static napi_value rtDilateAtlas(napi_env env, napi_callback_info info) {
  napi_value a[6];
  void *atlas = NULL, *src = NULL;
  size_t na = 0, ns = 0;
  if (!get_args(env, info, 6, a) || !get_bytes(env, a[4], &atlas, &na) || !get_bytes(env, a[5], &src, &ns)) return NULL;
  rt_dilate_desc d;
  memset(&d, 0, sizeof(d));
  d.width = get_u32(env, a[1]);
  d.height = get_u32(env, a[2]);
  d.radius = get_u32(env, a[3]);
  const size_t texels = (size_t)d.width * d.height;
  if (na / 16 < texels || (src && ns / 4 < texels)) {
    napi_throw_range_error(env, NULL, "rtDilateAtlas: atlas must hold 4 floats per texel and src width * height words");
    return NULL;
  }
  uint32_t n = 0;
  const int rc = rt_dilate_atlas((rt_ctx*)get_ptr(env, a[0]), &d, (float*)atlas, (uint32_t*)src, &n);
  if (rc < 0) return make_int(env, rc);
  napi_value r;
  napi_create_uint32(env, n, &r);
  return r;
}

/* ------------------------------------------------------- atlas denoise (rt_denoise_atlas, mi355rt.h) */
/* (ctx, width, height, step, passes, normalCos, planeEps, maxDist, atlas: Float32Array of 4 per texel (read), points:
 * Float32Array of 8 per point or null, texels: Uint32Array or null, out: Float32Array of 4 per texel) -> 0, or a negative
 * status; the number of points is the length of texels */
static napi_value rtDenoiseAtlas(napi_env env, napi_callback_info info) {
  napi_value a[12];
  void *atlas = NULL, *points = NULL, *texels = NULL, *out = NULL;
  size_t na = 0, np = 0, nt = 0, no = 0;
  if (!get_args(env, info, 12, a) || !get_bytes(env, a[8], &atlas, &na) || !get_bytes(env, a[9], &points, &np) ||
      !get_bytes(env, a[10], &texels, &nt) || !get_bytes(env, a[11], &out, &no))
    return NULL;
  rt_denoise_desc d;
  memset(&d, 0, sizeof(d));
  d.width = get_u32(env, a[1]);
  d.height = get_u32(env, a[2]);
  d.step = get_u32(env, a[3]);
  d.passes = get_u32(env, a[4]);
  d.normal_cos = (float)get_f64(env, a[5]);
  d.plane_eps = (float)get_f64(env, a[6]);
  d.max_dist = (float)get_f64(env, a[7]);
  const size_t cells = (size_t)d.width * d.height, n = nt / 4;
  if (na / 16 < cells || no / 16 < cells || np / 32 < n || n > 0xffffffffu) {
    napi_throw_range_error(env, NULL, "rtDenoiseAtlas: atlas and out must hold 4 floats per texel, points 8 floats per texel index");
    return NULL;
  }
  return make_int(env, rt_denoise_atlas((rt_ctx*)get_ptr(env, a[0]), &d, (const float*)atlas, (const rt_gather_point*)points,
                                        (const uint32_t*)texels, (uint32_t)n, (float*)out));
}

/* ------------------------------------------------------- frame denoise (rt_denoise_frame, mi355rt.h) */
/* desc: Float64Array {passes, step, flags, normalCos, planeEps, sigmaLum} -> an rt_frame_denoise_desc */
static int frame_denoise_desc(napi_env env, napi_value v, rt_frame_denoise_desc* d) {
  void* p = NULL;
  size_t n = 0;
  if (!get_bytes(env, v, &p, &n)) return 0;
  if (!p || n != 6 * sizeof(double)) {
    napi_throw_range_error(env, NULL, "frame denoise: the descriptor is a Float64Array of 6");
    return 0;
  }
  const double* s = (const double*)p;
  memset(d, 0, sizeof(*d));
  d->passes = (uint32_t)s[0];
  d->step = (uint32_t)s[1];
  d->flags = (uint32_t)s[2];
  d->normal_cos = (float)s[3];
  d->plane_eps = (float)s[4];
  d->sigma_lum = (float)s[5];
  return 1;
}
/* (ctx, desc, out: Float32Array of width * height * 4) -> 0, or a negative status */
static napi_value rtDenoiseFrame(napi_env env, napi_callback_info info) {
  napi_value a[3];
  void* out = NULL;
  size_t no = 0;
  rt_frame_denoise_desc d;
  if (!get_args(env, info, 3, a) || !frame_denoise_desc(env, a[1], &d) || !get_bytes(env, a[2], &out, &no)) return NULL;
  return make_int(env, rt_denoise_frame((rt_ctx*)get_ptr(env, a[0]), &d, (float*)out, no));
}
/* (ctx, desc or null) -> 0, or a negative status */
static napi_value rtSetPresentDenoise(napi_env env, napi_callback_info info) {
  napi_value a[2];
  napi_valuetype t;
  rt_frame_denoise_desc d;
  if (!get_args(env, info, 2, a)) return NULL;
  if (napi_typeof(env, a[1], &t) == napi_ok && (t == napi_null || t == napi_undefined))
    return make_int(env, rt_set_present_denoise((rt_ctx*)get_ptr(env, a[0]), NULL));
  if (!frame_denoise_desc(env, a[1], &d)) return NULL;
  return make_int(env, rt_set_present_denoise((rt_ctx*)get_ptr(env, a[0]), &d));
}

/* ------------------------------------------------------- frame temporal (rt_set_frame_temporal, mi355rt.h) */
/* (ctx, desc: Float64Array {flags, maxHistory, varHistory, normalCos, planeEps} or null) -> 0, or a negative status */
static napi_value rtSetFrameTemporal(napi_env env, napi_callback_info info) {
  napi_value a[2];
  napi_valuetype t;
  rt_frame_temporal_desc d;
  void* p = NULL;
  size_t n = 0;
  if (!get_args(env, info, 2, a)) return NULL;
  if (napi_typeof(env, a[1], &t) == napi_ok && (t == napi_null || t == napi_undefined))
    return make_int(env, rt_set_frame_temporal((rt_ctx*)get_ptr(env, a[0]), NULL));
  if (!get_bytes(env, a[1], &p, &n)) return NULL;
  if (!p || n != 5 * sizeof(double)) {
    napi_throw_range_error(env, NULL, "frame temporal: the descriptor is a Float64Array of 5");
    return NULL;
  }
  const double* s = (const double*)p;
  memset(&d, 0, sizeof(d));
  d.flags = (uint32_t)s[0];
  d.max_history = (uint32_t)s[1];
  d.var_history = (uint32_t)s[2];
  d.normal_cos = (float)s[3];
  d.plane_eps = (float)s[4];
  return make_int(env, rt_set_frame_temporal((rt_ctx*)get_ptr(env, a[0]), &d));
}
/* (ctx) -> 0, or a negative status */
static napi_value rtResetFrameHistory(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  return make_int(env, rt_reset_frame_history((rt_ctx*)get_ptr(env, a[0])));
}

/* ------------------------------------------------------- frame motion (RT_FRAME_TEMPORAL_MOTION, mi355rt.h) */
/* (ctx, ids: Uint32Array of one stable id per instance) -> 0, or a negative status */
static napi_value rtSetFrameMotionIds(napi_env env, napi_callback_info info) {
  napi_value a[2];
  void* p = NULL;
  size_t n = 0;
  if (!get_args(env, info, 2, a) || !get_bytes(env, a[1], &p, &n)) return NULL;
  return make_int(env, rt_set_frame_motion_ids((rt_ctx*)get_ptr(env, a[0]), (const uint32_t*)p, (uint32_t)(n / 4)));
}
/* (ctx, out: Float32Array of width * height * 8) -> 0, or a negative status */
static napi_value rtReadFrameMotion(napi_env env, napi_callback_info info) {
  napi_value a[2];
  void* out = NULL;
  size_t no = 0;
  if (!get_args(env, info, 2, a) || !get_bytes(env, a[1], &out, &no)) return NULL;
  return make_int(env, rt_read_frame_motion((rt_ctx*)get_ptr(env, a[0]), (float*)out, no / 32));
}

/* ------------------------------------------------------- lightmaps (rt_bake_atlas_lightmap, rt_encode_atlas, mi355rt.h) */
/* (ctx, width, height, padBase, tMax, entries, atlasUv or null, maxDepth, spp, seed, stages: Float64Array {passes, step,
 * normalCos, planeEps, maxDist, dilateRadius, format}, out: a typed array of width * height texels of the format, wantStats)
 * -> {covered, filled, stats?}, or a negative status */
static napi_value bake_atlas_lightmap_call(napi_env env, napi_callback_info info, int directional) {
  napi_value a[13];
  void *entries = NULL, *uv = NULL, *stages = NULL, *out = NULL;
  size_t ne = 0, nuv = 0, ns = 0, no = 0;
  bool want_stats = false;
  if (!get_args(env, info, 13, a) || !get_bytes(env, a[5], &entries, &ne) || !get_bytes(env, a[6], &uv, &nuv) ||
      !get_bytes(env, a[10], &stages, &ns) || !get_bytes(env, a[11], &out, &no))
    return NULL;
  napi_get_value_bool(env, a[12], &want_stats);
  rt_bake_atlas_desc b;
  if (!bake_atlas_desc(env, a + 1, ne, &b)) return NULL;
  if (nuv % 8 != 0 || nuv / 8 > 0xffffffffu || !stages || ns != 7 * sizeof(double)) {
    napi_throw_range_error(env, NULL, "rtBakeAtlasLightmap: atlasUv must hold 2 floats per vertex and stages 7 doubles");
    return NULL;
  }
  const double* s = (const double*)stages;
  rt_lightmap_desc d;
  memset(&d, 0, sizeof(d));
  d.width = b.width;
  d.height = b.height;
  d.pad_base = b.pad_base;
  d.t_max = b.t_max;
  d.n_entries = b.n_entries;
  d.max_depth = get_u32(env, a[7]);
  d.spp = get_u32(env, a[8]);
  d.seed = get_u32(env, a[9]);
  d.passes = (uint32_t)s[0];
  d.step = (uint32_t)s[1];
  d.normal_cos = (float)s[2];
  d.plane_eps = (float)s[3];
  d.max_dist = (float)s[4];
  d.dilate_radius = (uint32_t)s[5];
  d.format = (uint32_t)s[6];
  rt_radiance_stats st;
  uint32_t n = 0, filled = 0;
  const int rc = (directional ? rt_bake_atlas_directional_lightmap : rt_bake_atlas_lightmap)(
      (rt_ctx*)get_ptr(env, a[0]), &d, (const rt_bake_rect*)entries, (const float*)uv, (uint32_t)(nuv / 8), out, no, &n, &filled,
      want_stats ? &st : NULL);
  if (rc < 0) return make_int(env, rc);
  napi_value obj, v;
  if (napi_create_object(env, &obj) != napi_ok) return NULL;
  napi_create_uint32(env, n, &v);
  napi_set_named_property(env, obj, "covered", v);
  napi_create_uint32(env, filled, &v);
  napi_set_named_property(env, obj, "filled", v);
  if (want_stats) napi_set_named_property(env, obj, "stats", radiance_stats_object(env, &st));
  return obj;
}
static napi_value rtBakeAtlasLightmap(napi_env env, napi_callback_info info) { return bake_atlas_lightmap_call(env, info, 0); }
/* directional lightmaps (rt_bake_atlas_directional_lightmap): the same arguments; out holds FOUR layers of width * height texels
 * of the format, layer-major; filled is the count of one layer */
static napi_value rtBakeAtlasDirectionalLightmap(napi_env env, napi_callback_info info) {
  return bake_atlas_lightmap_call(env, info, 1);
}
/* (ctx, width, height, format, atlas: Float32Array of 4 per texel (read), out: a typed array of width * height texels of the
 * format) -> 0, or a negative status */
static napi_value rtEncodeAtlas(napi_env env, napi_callback_info info) {
  napi_value a[6];
  void *atlas = NULL, *out = NULL;
  size_t na = 0, no = 0;
  if (!get_args(env, info, 6, a) || !get_bytes(env, a[4], &atlas, &na) || !get_bytes(env, a[5], &out, &no)) return NULL;
  const uint32_t width = get_u32(env, a[1]), height = get_u32(env, a[2]), format = get_u32(env, a[3]);
  if (na / 16 < (size_t)width * height) {
    napi_throw_range_error(env, NULL, "rtEncodeAtlas: atlas must hold 4 floats per texel");
    return NULL;
  }
  return make_int(env, rt_encode_atlas((rt_ctx*)get_ptr(env, a[0]), width, height, format, (const float*)atlas, out, no));
}

static napi_value Init(napi_env env, napi_value exports) {
  static const struct {
    const char* name;
    napi_callback fn;
  } table[] = {{"rtCreate", rtCreate}, {"rtDestroy", rtDestroy}, {"rtLastError", rtLastError},
               {"rtSetPipeline", rtSetPipeline}, {"rtResize", rtResize}, {"rtResetAccum", rtResetAccum},
               {"rtUploadTextures", rtUploadTextures}, {"rtAllocTextureLayers", rtAllocTextureLayers},
               {"rtUploadTextureImage", rtUploadTextureImage}, {"mtDecode", mtDecode}, {"rtUpload", rtUpload}, {"rtUploadGeometry", rtUploadGeometry},
               {"rtUploadBVH", rtUploadBVH}, {"rtSetScene", rtSetScene}, {"rtCompute", rtCompute},
               {"rtComputeBatch", rtComputeBatch},
               {"rtPresent", rtPresent}, {"rtSync", rtSync}, {"rtCapture", rtCapture}, {"rtReadAccum", rtReadAccum},
               {"rtGetCounters", rtGetCounters}, {"rtDeviceCount", rtDeviceCount}, {"rtSetStripes", rtSetStripes},
               {"rtDistUniqueId", rtDistUniqueId}, {"rtDistInit", rtDistInit}, {"rtDistShutdown", rtDistShutdown},
               {"rtDistBlockBytes", rtDistBlockBytes}, {"rtPackStripes", rtPackStripes}, {"rtDistReadBlock", rtDistReadBlock},
               {"rtDistWriteBlock", rtDistWriteBlock}, {"rtUnpackStripes", rtUnpackStripes},
               {"rtGatherStripes", rtGatherStripes}, {"rtReadDisplay", rtReadDisplay}, {"rtTraceRays", rtTraceRays},
               {"rtRayQueryStats", rtRayQueryStats}, {"rtTraceRadiance", rtTraceRadiance},
               {"rtGatherIrradiance", rtGatherIrradiance}, {"rtGatherProbes", rtGatherProbes}, {"rtBakePoints", rtBakePoints},
               {"rtBakeVolume", rtBakeVolume}, {"rtSampleVolume", rtSampleVolume}, {"rtEncodeVolume", rtEncodeVolume},
               {"rtBakeVolumeVisibility", rtBakeVolumeVisibility}, {"rtSampleVolumeVisible", rtSampleVolumeVisible},
               {"rtEncodeVolumeVisibility", rtEncodeVolumeVisibility},
               {"rtBakeReflection", rtBakeReflection}, {"rtFilterReflection", rtFilterReflection},
               {"rtSampleReflection", rtSampleReflection},
               {"rtGatherDirectional", rtGatherDirectional}, {"rtBakeAtlasDirectionalLightmap", rtBakeAtlasDirectionalLightmap},
               {"rtBakeIrradiance", rtBakeIrradiance}, {"rtBakeAtlasPoints", rtBakeAtlasPoints},
               {"rtBakeAtlasIrradiance", rtBakeAtlasIrradiance}, {"rtDilateAtlas", rtDilateAtlas},
               {"rtDenoiseAtlas", rtDenoiseAtlas}, {"rtBakeAtlasLightmap", rtBakeAtlasLightmap},
               {"rtDenoiseFrame", rtDenoiseFrame}, {"rtSetPresentDenoise", rtSetPresentDenoise},
               {"rtSetFrameTemporal", rtSetFrameTemporal}, {"rtResetFrameHistory", rtResetFrameHistory},
               {"rtSetFrameMotionIds", rtSetFrameMotionIds}, {"rtReadFrameMotion", rtReadFrameMotion},
               {"rtEncodeAtlas", rtEncodeAtlas}, {"msCreate", msCreate}, {"msDestroy", msDestroy},
               {"msUpdate", msUpdate}, {"msUpdateCamera", msUpdateCamera}, {"msGet", msGet},
               {"msTextureCount", msTextureCount}, {"msTexture", msTexture},
               {"msAnimationNames", msAnimationNames}, {"msSetAnimation", msSetAnimation},
               {"msLoadAnimation", msLoadAnimation}, {"msLastError", msLastError}, {"msSetBlasBuilder", msSetBlasBuilder}, {"msSetDeviceUpdater", msSetDeviceUpdater},
               {"msDeviceResident", msDeviceResident},
               {"msEncodedTextureCount", msEncodedTextureCount}, {"msEncodedTexture", msEncodedTexture}};
  for (size_t i = 0; i < sizeof(table) / sizeof(table[0]); i++) {
    napi_value fn;
    if (napi_create_function(env, table[i].name, NAPI_AUTO_LENGTH, table[i].fn, NULL, &fn) != napi_ok) return NULL;
    napi_set_named_property(env, exports, table[i].name, fn);
  }
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, Init)
