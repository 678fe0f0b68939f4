"""WebGPURenderer — host-side mirror of src/renderer/WebGPURenderer.ts over libmi355rt.so.

Same method names, argument meaning and return values as the reference class
(WebGPURenderer.ts:7-138).  Every call goes through the C ABI in include/mi355rt.h; there is no
CPU fallback: if the HIP library is missing or no device is present the constructor raises.
"""
import ctypes
import os

import numpy as np

from . import _build

RT_OK, RT_REALLOCATED, RT_SKIPPED = 0, 1, 2
_KINDS = {"topology": 0, "instance": 1, "lights": 2, "draw_commands": 3}
COUNTER_NAMES = ("primary_rays", "extension_rays", "shadow_rays", "nodes_visited", "tris_tested", "shaded_hits")

_lib = None


class RendererError(RuntimeError):
    pass


_hip_runtime = None
hip_runtime_note = None   # what the last load_library() decided about the HIP runtime, for diagnostics


def _elf_dynamic_strings(path, want_tags):
    """DT_NEEDED (1) / DT_SONAME (14) strings of a 64-bit little-endian ELF, read straight from the file (no tool, no dlopen)."""
    import struct
    out = {t: [] for t in want_tags}
    with open(path, "rb") as f:
        data = f.read()
    if data[:4] != b"\x7fELF" or data[4] != 2 or data[5] != 1:
        return out
    e_shoff, = struct.unpack_from("<Q", data, 0x28)
    e_shentsize, e_shnum = struct.unpack_from("<HH", data, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", data, e_shoff + i * e_shentsize) for i in range(e_shnum)]
    for sh in secs:
        if sh[1] != 6:          # SHT_DYNAMIC
            continue
        stroff = secs[sh[6]][4]  # sh_link -> .dynstr
        for off in range(sh[4], sh[4] + sh[5], 16):
            tag, val = struct.unpack_from("<qQ", data, off)
            if tag == 0:
                break
            if tag in out:
                end = data.index(b"\0", stroff + val)
                out[tag].append(data[stroff + val:end].decode())
    return out


def mapped_hip_runtimes():
    """Paths of every libamdhip64 mapped into this process (/proc/self/maps): more than one = two runtimes."""
    found = set()
    try:
        with open("/proc/self/maps") as maps:
            for line in maps:
                f = line.split()
                if len(f) >= 6 and os.path.basename(f[5]).startswith("libamdhip64.so"):
                    found.add(os.path.realpath(f[5]))
    except OSError:
        pass
    return sorted(found)


def _preload_hip_runtime(rt_lib_path):
    """ONE HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so (SONAME libamdhip64.so.7) and asks for it
    as `libamdhip64.so`; libmi355rt.so asks for `libamdhip64.so.7` (RUNPATH /opt/rocm).  The loader matches by the
    requested name, so whichever came second used to get a second copy of the runtime: `import torch` after the renderer
    then found "No HIP GPUs", and stream handles or events of one copy meant nothing to the other.  When torch is installed
    its copy is therefore loaded first, globally — our NEEDED entry matches its SONAME, torch's later request resolves to
    the same file — and the renderer, torch and RCCL share one runtime whatever the import order.

    Guarded (a user who never touches torch must not be broken by it): the candidate is used only when its SONAME is what
    libmi355rt.so NEEDs (else the preload could not satisfy our request and the two-runtime bug would come back silently:
    warned instead); a candidate that fails to load (missing comgr / hsa dependencies, CPU-only torch layout) is skipped
    with a warning and the RUNPATH runtime is used.  MI355RT_HIP_RUNTIME=<path> names the runtime explicitly,
    MI355RT_HIP_RUNTIME=system never preloads.  No GPU is touched here."""
    global _hip_runtime, hip_runtime_note
    if _hip_runtime is not None:
        return
    import warnings
    _hip_runtime = False
    path = os.environ.get("MI355RT_HIP_RUNTIME")
    if path == "system":
        hip_runtime_note = "system runtime of the RUNPATH (MI355RT_HIP_RUNTIME=system)"
        return
    already = mapped_hip_runtimes()
    if already and not path:
        hip_runtime_note = "a HIP runtime is already mapped (%s): nothing preloaded" % ", ".join(already)
        return
    explicit = bool(path)
    if not path:
        import importlib.util
        try:
            spec = importlib.util.find_spec("torch")
        except (ImportError, ValueError):
            spec = None
        if spec is not None and spec.submodule_search_locations:
            cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
            if os.path.exists(cand):
                path = cand
    if not path:
        hip_runtime_note = "system runtime of the RUNPATH (no torch-bundled libamdhip64.so found)"
        return
    try:
        needed = [n for n in _elf_dynamic_strings(rt_lib_path, (1,))[1] if n.startswith("libamdhip64.so")]
        soname = _elf_dynamic_strings(path, (14,))[14]
    except (OSError, ValueError, IndexError, KeyError) as e:
        needed, soname = [], []
        warnings.warn("mi355rt: cannot read the ELF dynamic section for the HIP runtime check (%s)" % e, RuntimeWarning)
    if needed and soname and soname[0] not in needed:
        hip_runtime_note = "%s has SONAME %s but libmi355rt.so needs %s: not preloaded" % (path, soname[0], needed[0])
        warnings.warn("mi355rt: " + hip_runtime_note + " — torch and the renderer will use DIFFERENT HIP runtimes in this "
                      "process (streams / events cannot be shared; set MI355RT_HIP_RUNTIME to a matching libamdhip64.so)",
                      RuntimeWarning)
        return
    try:
        _hip_runtime = ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        hip_runtime_note = "preloaded %s%s" % (path, "" if explicit else " (torch's bundled runtime)")
    except OSError as e:
        _hip_runtime = False
        hip_runtime_note = "could not preload %s (%s): system runtime of the RUNPATH" % (path, e)
        warnings.warn("mi355rt: " + hip_runtime_note + (" — a later `import torch` would map a second HIP runtime"
                                                         if not explicit else ""), RuntimeWarning)


def load_library(path=None):
    """dlopen libmi355rt.so and declare every symbol of include/mi355rt.h.
    Loading does not touch the GPU; rt_create does."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or _build.RT_LIB
    if not os.path.exists(path):
        raise RendererError(
            "HIP renderer library not built: %s (run `python -c 'import __graft_entry__ as g; g.build()'`)" % path)
    _preload_hip_runtime(path)
    L = ctypes.CDLL(path)
    maps = mapped_hip_runtimes()
    if len(maps) > 1:   # the two-runtime state the preload exists to prevent: say so instead of failing later in odd ways
        import warnings
        warnings.warn("mi355rt: %d HIP runtimes are mapped in this process (%s); handles of one mean nothing to the other"
                      % (len(maps), ", ".join(maps)), RuntimeWarning)
    vp, u32, i32 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_int
    sigs = {
        "rt_create": (vp, [i32]), "rt_destroy": (None, [vp]), "rt_last_error": (ctypes.c_char_p, [vp]),
        "rt_set_pipeline": (i32, [vp, u32, u32]), "rt_resize": (i32, [vp, u32, u32]),
        "rt_reset_accum": (i32, [vp]), "rt_upload_textures": (i32, [vp, vp, u32]),
        "rt_alloc_texture_layers": (i32, [vp, u32]), "rt_upload_texture_image": (i32, [vp, u32, vp, u32, u32]),
        "rt_read_texture_layer": (i32, [vp, u32, vp, ctypes.c_size_t]),
        "rt_build_blas": (i32, [vp, vp, u32, vp, u32, vp, u32, ctypes.POINTER(u32), vp]),
        "rt_upload": (i32, [vp, i32, vp, ctypes.c_size_t]),
        "rt_upload_geometry": (i32, [vp, vp, vp, vp, u32]),
        "rt_upload_bvh": (i32, [vp, vp, u32, vp, u32]),
        "rt_set_scene": (i32, [vp, vp, u32, u32]), "rt_recreate_bind_group": (i32, [vp]),
        "rt_compute": (i32, [vp, u32]), "rt_present": (i32, [vp]),
        "rt_compute_batch": (i32, [vp, vp, u32]),
        "rt_capture": (i32, [vp, vp, ctypes.c_size_t]), "rt_sync": (i32, [vp]),
        "rt_read_accum": (i32, [vp, vp, ctypes.c_size_t]), "rt_write_accum": (i32, [vp, vp, ctypes.c_size_t]),
        "rt_read_gbuffer": (i32, [vp, vp, vp, vp]), "rt_read_history": (i32, [vp, vp, ctypes.c_size_t]),
        "rt_read_uniforms": (i32, [vp, vp]), "rt_get_counters": (i32, [vp, vp]),
        "rt_get_kernel_counters": (i32, [vp, i32, vp]), "rt_bind_accum": (i32, [vp, vp]),
        "rt_reset_counters": (i32, [vp]), "rt_set_counting": (i32, [vp, i32]),
        "rt_set_stripes": (i32, [vp, u32, u32, u32]), "rt_accum_device_ptr": (vp, [vp]),
        "rt_set_stream": (i32, [vp, vp]), "rt_bind_present_source": (i32, [vp, vp]),
        "rt_debug_clock_stamps": (i32, [vp, vp, u32]), "rt_debug_trace_sections": (i32, [vp, vp, i32]), "rt_debug_pt_sections": (i32, [vp, vp, i32]),
        "rt_debug_pt_launch": (i32, [vp, vp]), "rt_debug_pt_form": (i32, [vp]), "rt_debug_lane_stats": (i32, [vp, vp, i32]),
        "rt_debug_read_traversal_nodes": (i32, [vp, vp, vp, vp, u32]),
        "rt_debug_read_pairs": (i32, [vp, vp, vp, u32]),
        "rt_debug_ieee_check": (i32, [vp, i32, ctypes.c_uint64, ctypes.c_uint64, vp]),
        "rt_kernel_times": (i32, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u32), u32]),
        "rt_kernel_time_ms": (i32, [vp, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                    ctypes.POINTER(u32)]),
        "rt_set_kernel_timing": (i32, [vp, i32]), "rt_device_count": (i32, []),
        "rt_set_kernel_variant": (i32, [vp, i32]), "rt_set_walk": (i32, [vp, i32]), "rt_set_lookahead": (i32, [vp, u32]),
        "rt_set_lookahead_limit": (i32, [vp, u32]),
        "rt_build_blas_levels": (i32, [vp]),
        "rt_world_update": (i32, [vp, vp]), "rt_world_set_static_cache": (i32, [vp, i32]), "rt_world_last_ms": (ctypes.c_double, [vp]), "rt_world_last_tlas_ms": (ctypes.c_double, [vp]),
        "rt_world_read": (i32, [vp, i32, vp, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)]),
        # the sharded image (rt_dist_*)
        "rt_dist_unique_id": (i32, [vp]), "rt_dist_init": (i32, [vp, u32, u32, u32, vp]), "rt_dist_shutdown": (i32, [vp]),
        "rt_dist_block_bytes": (ctypes.c_size_t, [vp]), "rt_pack_stripes": (i32, [vp]),
        "rt_dist_read_block": (i32, [vp, vp, ctypes.c_size_t]), "rt_dist_write_block": (i32, [vp, u32, vp, ctypes.c_size_t]),
        "rt_unpack_stripes": (i32, [vp]), "rt_gather_stripes": (i32, [vp]), "rt_read_display": (i32, [vp, vp, ctypes.c_size_t]),
        # ray queries
        "rt_trace_rays": (i32, [vp, vp, u32, i32, ctypes.c_float, vp, vp]),
        "rt_trace_rays_device": (i32, [vp, vp, u32, i32, ctypes.c_float, vp]),
        "rt_ray_query_stats": (i32, [vp, vp]),
        # radiance queries
        "rt_trace_radiance": (i32, [vp, vp, u32, u32, u32, u32, vp, vp]),
        "rt_trace_radiance_device": (i32, [vp, vp, u32, u32, u32, u32, vp]),
        "rt_radiance_query_stats": (i32, [vp, vp]),
        # irradiance gathers
        "rt_gather_irradiance": (i32, [vp, vp, u32, u32, u32, u32, vp, vp]),
        "rt_gather_irradiance_device": (i32, [vp, vp, u32, u32, u32, u32, vp]),
        "rt_irradiance_gather_stats": (i32, [vp, vp]),
        # probe gathers
        "rt_gather_probes": (i32, [vp, vp, u32, u32, u32, u32, vp, vp]),
        "rt_gather_probes_device": (i32, [vp, vp, u32, u32, u32, u32, vp]),
        "rt_probe_gather_stats": (i32, [vp, vp]),
        # irradiance volumes
        "rt_bake_volume": (i32, [vp, vp, u32, u32, u32, vp, vp]),
        "rt_bake_volume_device": (i32, [vp, vp, u32, u32, u32, vp]),
        "rt_sample_volume": (i32, [vp, vp, vp, vp, u32, vp]),
        "rt_sample_volume_device": (i32, [vp, vp, vp, vp, u32, vp]),
        "rt_encode_volume": (i32, [vp, vp, u32, vp, vp, ctypes.c_size_t]),
        "rt_encode_volume_device": (i32, [vp, vp, u32, vp, vp, ctypes.c_size_t]),
        # reflection probes
        "rt_capture_reflection": (i32, [vp, vp, vp, u32, u32, u32, vp, vp]),
        "rt_capture_reflection_device": (i32, [vp, vp, vp, u32, u32, u32, vp]),
        "rt_filter_reflection": (i32, [vp, vp, vp, u32, vp]),
        "rt_filter_reflection_device": (i32, [vp, vp, vp, u32, vp]),
        "rt_bake_reflection": (i32, [vp, vp, vp, u32, u32, u32, vp, vp]),
        "rt_bake_reflection_device": (i32, [vp, vp, vp, u32, u32, u32, vp]),
        "rt_reflection_stats": (i32, [vp, vp]),
        # the reflection sampler
        "rt_sample_reflection": (i32, [vp, vp, vp, u32, vp, vp, vp, u32, vp]),
        "rt_sample_reflection_device": (i32, [vp, vp, vp, u32, vp, vp, vp, u32, vp]),
        # probe visibility maps
        "rt_bake_volume_visibility": (i32, [vp, vp, vp, u32, vp, vp]),
        "rt_bake_volume_visibility_device": (i32, [vp, vp, vp, u32, vp]),
        "rt_volume_visibility_stats": (i32, [vp, vp]),
        "rt_sample_volume_visible": (i32, [vp, vp, vp, vp, vp, vp, u32, vp]),
        "rt_sample_volume_visible_device": (i32, [vp, vp, vp, vp, vp, vp, u32, vp]),
        "rt_encode_volume_visibility": (i32, [vp, vp, vp, u32, vp, vp, ctypes.c_size_t]),
        "rt_encode_volume_visibility_device": (i32, [vp, vp, vp, u32, vp, vp, ctypes.c_size_t]),
        # directional gathers
        "rt_gather_directional": (i32, [vp, vp, u32, u32, u32, u32, vp, vp]),
        "rt_gather_directional_device": (i32, [vp, vp, u32, u32, u32, u32, vp]),
        "rt_directional_gather_stats": (i32, [vp, vp]),
        # lightmap bakes
        "rt_bake_points": (i32, [vp, vp, vp, u32, vp, vp, u32, vp, vp]),
        "rt_bake_points_device": (i32, [vp, vp, vp, vp, vp, u32, vp, vp]),
        "rt_bake_irradiance": (i32, [vp, vp, vp, u32, u32, u32, u32, vp, vp, vp]),
        # atlas bakes
        "rt_bake_atlas_points": (i32, [vp, vp, vp, vp, u32, vp, vp, u32, vp, vp]),
        "rt_bake_atlas_points_device": (i32, [vp, vp, vp, vp, vp, vp, u32, vp, vp]),
        "rt_bake_atlas_irradiance": (i32, [vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, vp]),
        # atlas dilation
        "rt_dilate_atlas": (i32, [vp, vp, vp, vp, vp]),
        "rt_dilate_atlas_device": (i32, [vp, vp, vp, vp, vp]),
        # atlas denoise
        "rt_denoise_atlas": (i32, [vp, vp, vp, vp, vp, u32, vp]),
        "rt_denoise_atlas_device": (i32, [vp, vp, vp, vp, vp, u32, vp]),
        # frame denoise
        "rt_denoise_frame": (i32, [vp, vp, vp, ctypes.c_size_t]),
        "rt_denoise_frame_device": (i32, [vp, vp, vp]),
        "rt_set_present_denoise": (i32, [vp, vp]),
        "rt_set_frame_denoise_form": (i32, [vp, ctypes.c_int]),
        "rt_frame_denoise_stats": (i32, [vp, vp]),
        # frame temporal
        "rt_set_frame_temporal": (i32, [vp, vp]),
        "rt_reset_frame_history": (i32, [vp]),
        "rt_read_frame_history": (i32, [vp, vp, vp, ctypes.c_size_t, vp]),
        # frame motion
        "rt_set_frame_motion_ids": (i32, [vp, vp, u32]),
        "rt_read_frame_motion": (i32, [vp, vp, ctypes.c_size_t]),
        # lightmaps
        "rt_bake_atlas_lightmap": (i32, [vp, vp, vp, vp, u32, vp, ctypes.c_size_t, vp, vp, vp]),
        "rt_bake_atlas_lightmap_device": (i32, [vp, vp, vp, vp, vp, ctypes.c_size_t, vp, vp, vp]),
        "rt_encode_atlas": (i32, [vp, u32, u32, u32, vp, vp, ctypes.c_size_t]),
        "rt_encode_atlas_device": (i32, [vp, u32, u32, u32, vp, vp, ctypes.c_size_t]),
        # directional lightmaps
        "rt_bake_atlas_directional": (i32, [vp, vp, vp, vp, u32, u32, u32, u32, vp, vp, vp]),
        "rt_bake_atlas_directional_lightmap": (i32, [vp, vp, vp, vp, u32, vp, ctypes.c_size_t, vp, vp, vp]),
    }
    for name, (res, args) in sigs.items():
        fn = getattr(L, name)  # AttributeError here = header/library mismatch
        fn.restype = res
        fn.argtypes = args
    if path == _build.RT_LIB:
        _lib = L
    return L


EXPORTED_SYMBOLS = (
    "rt_create rt_destroy rt_last_error rt_set_pipeline rt_resize rt_reset_accum rt_upload_textures rt_upload "
    "rt_alloc_texture_layers rt_upload_texture_image rt_read_texture_layer rt_build_blas "
    "rt_upload_geometry rt_upload_bvh rt_set_scene rt_recreate_bind_group rt_compute rt_compute_batch rt_present rt_capture "
    "rt_sync rt_read_accum rt_write_accum rt_read_gbuffer rt_read_history rt_read_uniforms rt_get_counters "
    "rt_get_kernel_counters rt_bind_accum rt_bind_present_source rt_kernel_times rt_debug_clock_stamps rt_debug_trace_sections rt_debug_pt_sections rt_debug_pt_launch rt_debug_pt_form rt_debug_lane_stats rt_debug_read_traversal_nodes rt_debug_read_pairs rt_debug_ieee_check "
    "rt_reset_counters rt_set_counting rt_set_stripes rt_accum_device_ptr rt_set_stream rt_kernel_time_ms "
    "rt_set_kernel_timing rt_device_count rt_set_kernel_variant rt_set_walk rt_set_lookahead "
    "rt_world_update rt_world_last_ms rt_world_last_tlas_ms rt_world_read rt_build_blas_levels rt_set_lookahead_limit rt_world_set_static_cache "
    "rt_dist_unique_id rt_dist_init rt_dist_shutdown rt_dist_block_bytes rt_pack_stripes rt_dist_read_block rt_dist_write_block "
    "rt_unpack_stripes rt_gather_stripes rt_read_display "
    "rt_trace_rays rt_trace_rays_device rt_ray_query_stats "
    "rt_trace_radiance rt_trace_radiance_device rt_radiance_query_stats "
    "rt_gather_irradiance rt_gather_irradiance_device rt_irradiance_gather_stats "
    "rt_gather_probes rt_gather_probes_device rt_probe_gather_stats "
    "rt_bake_volume rt_bake_volume_device rt_sample_volume rt_sample_volume_device rt_encode_volume rt_encode_volume_device "
    "rt_capture_reflection rt_capture_reflection_device rt_filter_reflection rt_filter_reflection_device rt_bake_reflection "
    "rt_bake_reflection_device rt_reflection_stats rt_sample_reflection rt_sample_reflection_device "
    "rt_bake_volume_visibility rt_bake_volume_visibility_device rt_volume_visibility_stats rt_sample_volume_visible "
    "rt_sample_volume_visible_device rt_encode_volume_visibility rt_encode_volume_visibility_device "
    "rt_gather_directional rt_gather_directional_device rt_directional_gather_stats "
    "rt_bake_points rt_bake_points_device rt_bake_irradiance "
    "rt_bake_atlas_points rt_bake_atlas_points_device rt_bake_atlas_irradiance "
    "rt_dilate_atlas rt_dilate_atlas_device "
    "rt_denoise_atlas rt_denoise_atlas_device "
    "rt_denoise_frame rt_denoise_frame_device rt_set_present_denoise rt_set_frame_denoise_form rt_frame_denoise_stats "
    "rt_set_frame_temporal rt_reset_frame_history rt_read_frame_history rt_set_frame_motion_ids rt_read_frame_motion "
    "rt_bake_atlas_lightmap rt_bake_atlas_lightmap_device rt_encode_atlas rt_encode_atlas_device "
    "rt_bake_atlas_directional rt_bake_atlas_directional_lightmap").split()


# ---- ray queries: mirrors of rt_ray / rt_ray_hit / rt_ray_stats (include/mi355rt_layout.h)
RT_RAYS_CLOSEST, RT_RAYS_ANY = 0, 1


class RtRay(ctypes.Structure):
    _fields_ = [("origin", ctypes.c_float * 3), ("t_max", ctypes.c_float), ("dir", ctypes.c_float * 3), ("pad", ctypes.c_uint32)]


class RtRayHit(ctypes.Structure):
    _fields_ = [("t", ctypes.c_float), ("tri", ctypes.c_int32), ("inst", ctypes.c_int32), ("hit", ctypes.c_uint32)]


class RtRayStats(ctypes.Structure):
    _fields_ = [("rays", ctypes.c_uint64), ("nodes_visited", ctypes.c_uint64), ("tris_tested", ctypes.c_uint64),
                ("walk", ctypes.c_uint32), ("lds", ctypes.c_uint32), ("rayreg", ctypes.c_uint32), ("workgroups", ctypes.c_uint32),
                ("kernel_ms", ctypes.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


RAY_HIT_DTYPE = np.dtype([("t", np.float32), ("tri", np.int32), ("inst", np.int32), ("hit", np.uint32)])


# ---- radiance queries: mirrors of rt_radiance / rt_radiance_stats (include/mi355rt_layout.h)
class RtRadianceStats(ctypes.Structure):
    _fields_ = [("rays", ctypes.c_uint64), ("samples", ctypes.c_uint64), ("extension_rays", ctypes.c_uint64),
                ("shadow_rays", ctypes.c_uint64), ("shaded_hits", ctypes.c_uint64), ("nodes_visited", ctypes.c_uint64),
                ("tris_tested", ctypes.c_uint64), ("lds", ctypes.c_uint32), ("workgroups", ctypes.c_uint32),
                ("kernel_ms", ctypes.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


RADIANCE_DTYPE = np.dtype([("rgb", np.float32, (3,)), ("t", np.float32)])
# irradiance gathers: mirror of rt_irradiance; their stats are an RtRadianceStats (rays = points)
IRRADIANCE_DTYPE = np.dtype([("rgb", np.float32, (3,)), ("hit_fraction", np.float32)])
# probe gathers: mirrors of rt_probe / rt_probe_sh9; their stats are an RtRadianceStats (rays = probes)
PROBE_DTYPE = np.dtype([("position", np.float32, (3,)), ("t_max", np.float32), ("unused", np.float32, (3,)), ("pad", np.uint32)])
PROBE_SH9_DTYPE = np.dtype([("sh", np.float32, (9, 3)), ("hit_fraction", np.float32)])
# cosine-lobe convolution of SH bands 0, 1, 2 (Ramamoorthi & Hanrahan 2001): pi, 2 pi / 3, pi / 4
_SH9_BAND = np.array([np.pi] + [2.0 * np.pi / 3.0] * 3 + [np.pi / 4.0] * 5)


def sh9_basis(dirs):
    """The nine real spherical harmonics of bands 0 .. 2 at unit directions (..., 3) -> (..., 9) float64, in the order and
    with the constants of the probe rule (mi355rt.h)."""
    d = np.asarray(dirs, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    return np.stack([np.full_like(x, 0.282094792), 0.488602512 * y, 0.488602512 * z, 0.488602512 * x,
                     1.092548431 * (x * y), 1.092548431 * (y * z), 0.315391565 * (3.0 * (z * z) - 1.0),
                     1.092548431 * (x * z), 0.546274215 * (x * x - y * y)], axis=-1)


def sh9_irradiance(sh, normals):
    """Irradiance from SH9 radiance coefficients: sh (..., 9, 3) as gatherProbes returns them (the "sh" field), normals
    (m, 3) unit vectors -> (..., m, 3) float64, E(n) = sum_k A_band(k) sh[k] Y_k(n) with the cosine-lobe band factors pi,
    2 pi / 3, pi / 4.  Pure numpy; no ringing filter."""
    c = np.asarray(sh, np.float64) * _SH9_BAND[:, None]
    return np.einsum("mk,...kc->...mc", sh9_basis(normals), c)


# irradiance volumes: mirror of rt_volume_desc; a volume is a PROBE_SH9_DTYPE array (nz, ny, nx), a sample an IRRADIANCE_DTYPE
VOLUME_DESC_DTYPE = np.dtype([("origin", np.float32, (3,)), ("nx", np.uint32), ("step", np.float32, (3,)), ("ny", np.uint32),
                              ("window", np.float32, (3,)), ("nz", np.uint32), ("t_max", np.float32), ("pad_first", np.uint32),
                              ("max_hit_fraction", np.float32), ("reserved", np.uint32)])


def volume_desc(origin, step, dims, window=(1.0, 1.0, 1.0), t_max=1e30, pad_first=0, max_hit_fraction=1.0):
    """A VOLUME_DESC_DTYPE record (shape ()): probe (x, y, z) of the dims = (nx, ny, nz) grid sits at origin + (x, y, z) * step
    and is record (z * ny + y) * nx + x of the volume.  window: the per-band scale of the finish (sh_hanning_window, or (1, 1,
    1) for none); max_hit_fraction: the sampler takes a probe as valid iff its hit_fraction is at most this."""
    d = np.zeros((), VOLUME_DESC_DTYPE)
    d["origin"], d["step"], d["window"] = origin, step, window
    d["nx"], d["ny"], d["nz"] = dims
    d["t_max"], d["pad_first"], d["max_hit_fraction"] = t_max, pad_first, max_hit_fraction
    return d


def sh_hanning_window(width):
    """The Hanning window against SH ringing (Sloan 2008) for bands l = 0, 1, 2: (1 + cos(pi l / width)) / 2 as three float32,
    for the window field of a volume descriptor.  Pure numpy."""
    return ((1.0 + np.cos(np.pi * np.arange(3) / float(width))) / 2.0).astype(np.float32)


def _volume_desc(desc):
    d = np.ascontiguousarray(desc)
    if d.dtype != VOLUME_DESC_DTYPE or d.size != 1:
        raise ValueError("a volume descriptor is one VOLUME_DESC_DTYPE record (volume_desc builds it)")
    return d.reshape(())


# probe visibility maps: mirror of rt_volume_visibility_desc; a visibility volume is (nz, ny, nx, size, size, 2) float32 {mean
# distance, mean squared distance}, a map in octahedral layout, texel (i, j) at [j, i]
RT_VOLUME_VIS_BACKFACE = 1
VOLUME_VISIBILITY_DESC_DTYPE = np.dtype([("size", np.uint32), ("spt", np.uint32), ("max_distance", np.float32),
                                         ("normal_bias", np.float32), ("min_visibility", np.float32),
                                         ("crush_threshold", np.float32), ("flags", np.uint32), ("reserved", np.uint32)])


def volume_visibility_desc(size, max_distance, spt=64, normal_bias=0.0, min_visibility=0.0, crush_threshold=0.0, backface=False):
    """A VOLUME_VISIBILITY_DESC_DTYPE record (shape ()): maps of size x size texels (a power of two in 4 .. 32) baked at spt
    samples per texel; max_distance is the t_max of every visibility ray and the clamp of every distance - the diagonal of a
    cell, or a little more, is the usual choice.  The sampler moves a point normal_bias along its normal before it looks at a
    probe, never lets the Chebyshev weight fall below min_visibility, cubes weights below crush_threshold (0 = none), and with
    backface weights a probe down that lies behind the surface."""
    d = np.zeros((), VOLUME_VISIBILITY_DESC_DTYPE)
    d["size"], d["spt"], d["max_distance"], d["normal_bias"] = size, spt, max_distance, normal_bias
    d["min_visibility"], d["crush_threshold"] = min_visibility, crush_threshold
    d["flags"] = RT_VOLUME_VIS_BACKFACE if backface else 0
    return d


def _volume_visibility_desc(desc):
    d = np.ascontiguousarray(desc)
    if d.dtype != VOLUME_VISIBILITY_DESC_DTYPE or d.size != 1:
        raise ValueError("a visibility descriptor is one VOLUME_VISIBILITY_DESC_DTYPE record (volume_visibility_desc builds it)")
    return d.reshape(())


def _visibility_maps(d, v, visibility, who):
    m = np.ascontiguousarray(visibility, dtype=np.float32)
    if m.size != 2 * int(d["nx"]) * int(d["ny"]) * int(d["nz"]) * int(v["size"]) ** 2:
        raise ValueError("%s: the visibility volume does not hold nx * ny * nz maps of size * size texels" % who)
    return m


# reflection probes: mirror of rt_reflection_desc; a map is (size, size, 4) float32 {r, g, b, hit_fraction} in octahedral layout,
# a chain (chain_texels, 4) float32 with level m at reflection_level_offsets(size, levels)[m]
REFLECTION_DESC_DTYPE = np.dtype([("size", np.uint32), ("levels", np.uint32), ("spt", np.uint32), ("filter_samples", np.uint32),
                                  ("reserved", np.uint32, (4,))])


def reflection_desc(size, levels, spt=1, filter_samples=256):
    """A REFLECTION_DESC_DTYPE record (shape ()): level 0 of size x size texels, `levels` levels with level m of side size >> m
    at the roughness m / (levels - 1); spt samples per texel of a capture; filter_samples lobe samples per texel of a filter."""
    d = np.zeros((), REFLECTION_DESC_DTYPE)
    d["size"], d["levels"], d["spt"], d["filter_samples"] = size, levels, spt, filter_samples
    return d


def reflection_level_offsets(size, levels):
    """levels + 1 texel offsets: level m of a chain is the texels [offsets[m], offsets[m + 1]) - (size >> m)^2 of them, texel
    (i, j) at j * (size >> m) + i - and offsets[levels] is the length of a chain."""
    sides = np.array([int(size) >> m for m in range(int(levels))], np.int64)
    return np.concatenate([[0], np.cumsum(sides * sides)])


def octa_directions(size):
    """The unit directions of the texel centres of a size x size octahedral map: (size, size, 3) float64, [j, i] for texel
    (i, j) - the mapping of the reflection rule, in double precision.  Pure numpy."""
    c = (np.arange(int(size)) + 0.5) / int(size) * 2.0 - 1.0
    px, py = np.meshgrid(c, c, indexing="xy")
    nz = 1.0 - np.abs(px) - np.abs(py)
    t = np.clip(-nz, 0.0, 1.0)
    nx = px + np.where(px >= 0.0, -t, t)
    ny = py + np.where(py >= 0.0, -t, t)
    n = np.stack([nx, ny, nz], axis=-1)
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def _reflection_desc(desc):
    d = np.ascontiguousarray(desc)
    if d.dtype != REFLECTION_DESC_DTYPE or d.size != 1:
        raise ValueError("a reflection descriptor is one REFLECTION_DESC_DTYPE record (reflection_desc builds it)")
    return d.reshape(())


def _reflection_chain_texels(d):
    """texels of a chain; 0 for a descriptor the library will refuse"""
    size, levels = int(d["size"]), int(d["levels"])
    if not (8 <= size <= 512) or not (2 <= levels <= 32):
        return 0
    return int(reflection_level_offsets(size, levels)[-1])


# the reflection sampler: mirrors of rt_reflection_sample_desc / rt_reflection_query / rt_reflection_box; a result is one texel
# {r, g, b, hit_fraction}
RT_REFLECTION_SAMPLE_PARALLAX = 1
REFLECTION_SAMPLE_DESC_DTYPE = np.dtype([("size", np.uint32), ("levels", np.uint32), ("flags", np.uint32),
                                         ("reserved", np.uint32, (5,))])
REFLECTION_QUERY_DTYPE = np.dtype([("position", np.float32, (3,)), ("probe", np.uint32), ("direction", np.float32, (3,)),
                                   ("roughness", np.float32)])
REFLECTION_BOX_DTYPE = np.dtype([("lo", np.float32, (3,)), ("unused0", np.float32), ("hi", np.float32, (3,)),
                                 ("unused1", np.float32)])


def reflection_sample_desc(size, levels, parallax=False):
    """A REFLECTION_SAMPLE_DESC_DTYPE record (shape ()): the size and levels of the chains to sample, as their bake's
    reflection_desc had them; parallax: bend every direction to where it leaves the probe's box (sampleReflection then wants
    probes and boxes)."""
    d = np.zeros((), REFLECTION_SAMPLE_DESC_DTYPE)
    d["size"], d["levels"] = size, levels
    d["flags"] = RT_REFLECTION_SAMPLE_PARALLAX if parallax else 0
    return d


def reflection_queries(positions, probes, directions, roughness):
    """A REFLECTION_QUERY_DTYPE array (n,): positions (n, 3) of the shaded points (read with parallax only), the index of each
    point's probe, the reflected directions (n, 3), which need not be unit, and the roughness of each, 0 .. 1 (scalars
    broadcast)."""
    dirs = np.asarray(directions, np.float32).reshape(-1, 3)
    q = np.zeros(dirs.shape[0], REFLECTION_QUERY_DTYPE)
    q["direction"] = dirs
    q["position"] = np.broadcast_to(np.asarray(positions, np.float32), (dirs.shape[0], 3))
    q["probe"] = np.broadcast_to(np.asarray(probes, np.uint32), dirs.shape[:1])
    q["roughness"] = np.broadcast_to(np.asarray(roughness, np.float32), dirs.shape[:1])
    return q


def _reflection_sample_desc(desc):
    d = np.ascontiguousarray(desc)
    if d.dtype != REFLECTION_SAMPLE_DESC_DTYPE or d.size != 1:
        raise ValueError("a reflection sample descriptor is one REFLECTION_SAMPLE_DESC_DTYPE record (reflection_sample_desc builds it)")
    return d.reshape(())


def _records(a, dtype, what):
    """a: an array of `dtype` or of float32 words, eight per record -> (n, 8) float32, C-contiguous"""
    r = np.ascontiguousarray(a)
    if r.dtype == dtype:
        r = r.reshape(-1).view(np.float32).reshape(-1, 8)
    r = np.ascontiguousarray(r, dtype=np.float32)
    if r.ndim != 2 or r.shape[1] != 8:
        raise ValueError("%s expects an (n, 8) float32 array" % what)
    return r


def _probe_array(probes, what):
    return _records(probes, PROBE_DTYPE, what)


# directional gathers: mirror of rt_directional; points are rt_gather_point, stats an RtRadianceStats (rays = points)
DIRECTIONAL_DTYPE = np.dtype([("layer", np.float32, (4, 4))])


def sh4_irradiance(layers_or_coeffs, normals):
    """Irradiance from the band 0 .. 1 radiance coefficients of a directional gather or bake at unit normals, by the cosine-lobe
    convolution sh9_irradiance uses: E(n) = pi * Y0 * c0 + (2 pi / 3) * 0.488602512 * (c1 n.y + c2 n.z + c3 n.x).
    layers_or_coeffs: (4, ..., 3 or 4) - four atlas layers as bakeAtlasDirectional returns them (an IRRADIANCE_DTYPE array, or
    floats whose fourth word, the hit fraction, is ignored) - or a DIRECTIONAL_DTYPE array (...,) as gatherDirectional returns
    it.  normals: (..., 3), one per texel / point (or broadcastable to that).  Returns (..., 3) float64.  Pure numpy."""
    a = np.asarray(layers_or_coeffs)
    if a.dtype == DIRECTIONAL_DTYPE:
        c = np.moveaxis(a["layer"].astype(np.float64), -2, 0)[..., :3]
    elif a.dtype == IRRADIANCE_DTYPE:
        c = a["rgb"].astype(np.float64)
    else:
        c = a.astype(np.float64)[..., :3]
    if c.shape[0] != 4:
        raise ValueError("sh4_irradiance expects four layers or coefficients first")
    n = np.asarray(normals, np.float64)
    band1 = c[1] * n[..., 1:2] + c[2] * n[..., 2:3] + c[3] * n[..., 0:1]
    return np.pi * 0.282094792 * c[0] + (2.0 * np.pi / 3.0) * 0.488602512 * band1


# lightmap bakes: mirror of rt_bake_desc
class RtBakeDesc(ctypes.Structure):
    _fields_ = [("inst", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("pad_base", ctypes.c_uint32),
                ("t_max", ctypes.c_float), ("reserved", ctypes.c_uint32 * 3)]


# atlas bakes: mirrors of rt_bake_atlas_desc / rt_bake_rect
class RtBakeAtlasDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("pad_base", ctypes.c_uint32), ("t_max", ctypes.c_float),
                ("n_entries", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


class RtBakeRect(ctypes.Structure):
    _fields_ = [("inst", ctypes.c_uint32), ("x", ctypes.c_uint32), ("y", ctypes.c_uint32), ("width", ctypes.c_uint32),
                ("height", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 3)]


# atlas dilation: mirror of rt_dilate_desc
class RtDilateDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("radius", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32 * 5)]


# atlas denoise: mirror of rt_denoise_desc
class RtDenoiseDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("step", ctypes.c_uint32), ("passes", ctypes.c_uint32),
                ("normal_cos", ctypes.c_float), ("plane_eps", ctypes.c_float), ("max_dist", ctypes.c_float),
                ("reserved", ctypes.c_uint32 * 1)]


# frame denoise: mirrors of rt_frame_denoise_desc and rt_frame_denoise_report, and the descriptor as a numpy record
RT_FRAME_DENOISE_MAX_STEP = 16
RT_FRAME_DENOISE_DEMODULATE, RT_FRAME_DENOISE_SAME_INSTANCE = 1, 2
FRAME_DENOISE_FORMS = {"auto": 0, "lds": 1, "direct": 2}


class RtFrameDenoiseDesc(ctypes.Structure):
    _fields_ = [("passes", ctypes.c_uint32), ("step", ctypes.c_uint32), ("flags", ctypes.c_uint32),
                ("normal_cos", ctypes.c_float), ("plane_eps", ctypes.c_float), ("sigma_lum", ctypes.c_float),
                ("reserved", ctypes.c_uint32 * 2)]


class RtFrameDenoiseReport(ctypes.Structure):
    _fields_ = [("prepare_ms", ctypes.c_float), ("pass_ms", ctypes.c_float * 5), ("finish_ms", ctypes.c_float),
                ("passes", ctypes.c_uint32), ("form", ctypes.c_uint8 * 5), ("cache_hit", ctypes.c_uint8),
                ("temporal", ctypes.c_uint8), ("motion", ctypes.c_uint8), ("temporal_ms", ctypes.c_float),
                ("motion_ms", ctypes.c_float)]


FRAME_DENOISE_DESC_DTYPE = np.dtype([("passes", "<u4"), ("step", "<u4"), ("flags", "<u4"), ("normal_cos", "<f4"),
                                     ("plane_eps", "<f4"), ("sigma_lum", "<f4"), ("reserved", "<u4", (2,))])


def frame_denoise_desc(passes=4, step=1, *, plane_eps, normal_cos=0.9, sigma_lum=4.0, demodulate=True, same_instance=False):
    """An rt_frame_denoise_desc as a one-element FRAME_DENOISE_DESC_DTYPE record: `passes` passes (1 .. 5) of the 5 x 5
    a-trous kernel at tap spacings step, 2 * step, ... (at most 16); a tap is accepted where its normal has a dot product >=
    normal_cos with the centre's and its world position lies within plane_eps (world units) of the centre's tangent plane;
    sigma_lum > 0 adds the luminance stop in standard deviations of the 3 x 3 neighbourhood; demodulate filters radiance /
    albedo and multiplies the albedo back; same_instance keeps taps on the centre's instance."""
    d = np.zeros(1, FRAME_DENOISE_DESC_DTYPE)
    d["passes"], d["step"] = int(passes), int(step)
    d["flags"] = (RT_FRAME_DENOISE_DEMODULATE if demodulate else 0) | (RT_FRAME_DENOISE_SAME_INSTANCE if same_instance else 0)
    d["normal_cos"], d["plane_eps"], d["sigma_lum"] = normal_cos, plane_eps, sigma_lum
    return d


# frame temporal: mirror of rt_frame_temporal_desc, and the descriptor as a numpy record
RT_FRAME_TEMPORAL_MAX_HISTORY = 256
RT_FRAME_TEMPORAL_SAME_INSTANCE = 1
RT_FRAME_TEMPORAL_MOTION = 2
# the status word of a carry texel (readFrameMotion) and the id of a pixel that has none
RT_FRAME_MOTION_BACKGROUND, RT_FRAME_MOTION_UNTRACKED, RT_FRAME_MOTION_UNMOVED, RT_FRAME_MOTION_MOVED = 0, 1, 2, 3
RT_FRAME_MOTION_NO_ID = 0xffffffff


class RtFrameTemporalDesc(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_uint32), ("max_history", ctypes.c_uint32), ("var_history", ctypes.c_uint32),
                ("normal_cos", ctypes.c_float), ("plane_eps", ctypes.c_float), ("reserved", ctypes.c_uint32 * 3)]


FRAME_TEMPORAL_DESC_DTYPE = np.dtype([("flags", "<u4"), ("max_history", "<u4"), ("var_history", "<u4"), ("normal_cos", "<f4"),
                                      ("plane_eps", "<f4"), ("reserved", "<u4", (3,))])


def frame_temporal_desc(max_history=32, var_history=4, *, plane_eps, normal_cos=0.9, same_instance=False, motion=False):
    """An rt_frame_temporal_desc as a one-element FRAME_TEMPORAL_DESC_DTYPE record: the history of a pixel grows to
    max_history frames (1 .. 256; 1 keeps none), after which the blend factor stays 1 / max_history; from var_history frames on
    the variance the passes see is the temporal one; a history tap is accepted where its normal has a dot product >= normal_cos
    with the pixel's and its world position lies within plane_eps (world units) of the pixel's tangent plane; same_instance
    keeps taps on the pixel's instance; motion carries every pixel back along its own triangle's motion first (moving instances,
    skinned surfaces), and same_instance then compares stable ids (setFrameMotionIds)."""
    d = np.zeros(1, FRAME_TEMPORAL_DESC_DTYPE)
    d["flags"] = (RT_FRAME_TEMPORAL_SAME_INSTANCE if same_instance else 0) | (RT_FRAME_TEMPORAL_MOTION if motion else 0)
    d["max_history"], d["var_history"] = int(max_history), int(var_history)
    d["normal_cos"], d["plane_eps"] = normal_cos, plane_eps
    return d


def frame_motion_pixels(carry, prev_uniforms):
    """Screen-space motion from the carry plane of readFrameMotion and the 256-byte uniform block of the PREVIOUS frame: ->
    (H, W, 2) float64, for every pixel the position (x, y) in the previous frame's image, pixel centres at whole numbers, of
    the surface point it shows now; NaN where the pixel is background or untracked, or the point lay behind that camera.
    Subtract the pixel's own coordinates for a motion vector.  Float64, a convenience: not part of the rule."""
    c = np.asarray(carry, np.float32)
    u32 = np.ascontiguousarray(prev_uniforms).view(np.uint8).reshape(-1)[:256]
    u = u32.view(np.float32).astype(np.float64)
    eye, ll, hor, ver = u[0:3], u[4:7], u[8:11], u[12:15]
    Wd, Hd = (float(v) for v in u32.view(np.uint32)[53:55])
    jx, jy = u[56], u[57]
    status = np.ascontiguousarray(c[..., 3]).view(np.uint32)
    P = c[..., 0:3].astype(np.float64)
    nrm = np.cross(hor, ver)
    with np.errstate(all="ignore"):
        s = np.dot(ll - eye, nrm) / ((P - eye) @ nrm)
        r = (P - eye) * s[..., None] - (ll - eye)
        uu, vv = (r @ hor) / np.dot(hor, hor), (r @ ver) / np.dot(ver, ver)
    out = np.stack([uu * Wd - 0.5 - jx * Wd, (1.0 - vv) * Hd - 0.5 - jy * Hd], axis=-1)
    out[(status < RT_FRAME_MOTION_UNMOVED) | ~(s > 0)] = np.nan
    return out


def _frame_temporal_record(desc):
    """a frame_temporal_desc record, or a dict of its keyword arguments -> a contiguous one-element record"""
    if isinstance(desc, dict):
        desc = frame_temporal_desc(**desc)
    d = np.ascontiguousarray(desc, dtype=FRAME_TEMPORAL_DESC_DTYPE).reshape(-1)
    if d.size != 1:
        raise ValueError("one rt_frame_temporal_desc record expected")
    return d


def _frame_denoise_record(desc):
    """a frame_denoise_desc record, or a dict of its keyword arguments -> a contiguous one-element record"""
    if isinstance(desc, dict):
        desc = frame_denoise_desc(**desc)
    d = np.ascontiguousarray(desc, dtype=FRAME_DENOISE_DESC_DTYPE).reshape(-1)
    if d.size != 1:
        raise ValueError("one rt_frame_denoise_desc record expected")
    return d


# lightmaps: mirror of rt_lightmap_desc, the RT_LIGHTMAP_* formats by name, and what a texel of each is on the host
class RtLightmapDesc(ctypes.Structure):
    _fields_ = [("width", ctypes.c_uint32), ("height", ctypes.c_uint32), ("pad_base", ctypes.c_uint32), ("t_max", ctypes.c_float),
                ("n_entries", ctypes.c_uint32), ("max_depth", ctypes.c_uint32), ("spp", ctypes.c_uint32), ("seed", ctypes.c_uint32),
                ("passes", ctypes.c_uint32), ("step", ctypes.c_uint32), ("normal_cos", ctypes.c_float),
                ("plane_eps", ctypes.c_float), ("max_dist", ctypes.c_float), ("dilate_radius", ctypes.c_uint32),
                ("format", ctypes.c_uint32), ("reserved", ctypes.c_uint32 * 1)]


RT_LIGHTMAP_F32, RT_LIGHTMAP_F16, RT_LIGHTMAP_RGBE8 = 0, 1, 2
LIGHTMAP_FORMATS = {"f32": RT_LIGHTMAP_F32, "f16": RT_LIGHTMAP_F16, "rgbe": RT_LIGHTMAP_RGBE8, "rgbe8": RT_LIGHTMAP_RGBE8}
LIGHTMAP_TEXEL_BYTES = {RT_LIGHTMAP_F32: 16, RT_LIGHTMAP_F16: 8, RT_LIGHTMAP_RGBE8: 4}


def _lightmap_format(format):
    if isinstance(format, str):
        if format.lower() not in LIGHTMAP_FORMATS:
            raise ValueError("lightmap format must be one of %s" % ", ".join(sorted(LIGHTMAP_FORMATS)))
        return LIGHTMAP_FORMATS[format.lower()]
    return int(format)


def _lightmap_array(height, width, fmt):
    """the host array of an encoded atlas: (H, W) IRRADIANCE_DTYPE, (H, W, 4) float16 or (H, W) uint32"""
    if fmt == RT_LIGHTMAP_F16:
        return np.empty((height, width, 4), np.float16)
    if fmt == RT_LIGHTMAP_RGBE8:
        return np.empty((height, width), np.uint32)
    return np.empty((height, width), dtype=IRRADIANCE_DTYPE)   # an unknown format is the library's to refuse


def decode_rgbe(words):
    """RGBE8 words (any shape, uint32; R | G << 8 | B << 16 | E << 24) -> (..., 3) float64 colours, (byte + 0.5) * 2^(E - 136)
    as a Radiance reader decodes them; the word 0 (and any word with E == 0) is black."""
    w = np.asarray(words, np.uint32)
    e = (w >> 24).astype(np.int64)
    rgb = np.stack([((w >> s) & 0xff).astype(np.float64) for s in (0, 8, 16)], axis=-1)
    return np.where((e > 0)[..., None], np.ldexp(rgb + 0.5, (e - 136)[..., None]), 0.0)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class WebGPURenderer:
    """`new WebGPURenderer(canvas)` + `await init()` (WebGPURenderer.ts:17-32).  The canvas
    argument of the reference becomes a device ordinal; width/height come from updateScreenSize."""

    def __init__(self, device=0):
        self.L = load_library()
        self.ctx = self.L.rt_create(int(device))
        if not self.ctx:
            msg = self.L.rt_last_error(None)
            raise RendererError("rt_create(%d) failed: %s" % (device, msg.decode() if msg else "unknown"))
        self.width = self.height = 0
        self._capture_buf = None  # reused between captures like readbackResultBuffer (WebGPUContext.ts:82-89)

    def __del__(self):
        self.destroy()

    def destroy(self):
        if getattr(self, "ctx", None):
            self.L.rt_destroy(self.ctx)
            self.ctx = None

    def _check(self, rc, what):
        if rc < 0:
            msg = self.L.rt_last_error(self.ctx)
            raise RendererError("%s failed (%d): %s" % (what, rc, msg.decode() if msg else ""))
        return rc

    # ---- reference surface ----
    def init(self):
        return None

    def buildPipeline(self, depth, spp):
        self._check(self.L.rt_set_pipeline(self.ctx, int(depth), int(spp)), "buildPipeline")

    def updateScreenSize(self, width, height):
        self.width, self.height = int(width), int(height)
        self._check(self.L.rt_resize(self.ctx, self.width, self.height), "updateScreenSize")

    def resetAccumulation(self):
        self._check(self.L.rt_reset_accum(self.ctx), "resetAccumulation")

    def loadTexturesFromWorld(self, bridge):
        """ResourceManager.ts:153-198: no textures -> default white texture; otherwise one 1024x1024 layer per
        encoded image of the bridge — decoded on the host (mi355tex), resized on the GPU — and the white fallback
        bitmap for an image that is missing or does not decode (the reference warns and carries on, :169-175)."""
        n = bridge.textureCount
        if n == 0:
            self._check(self.L.rt_upload_textures(self.ctx, None, 0), "loadTexturesFromWorld")
            return
        from . import textures
        self._check(self.L.rt_alloc_texture_layers(self.ctx, n), "loadTexturesFromWorld")
        self.texture_warnings = []
        for i in range(n):
            data = bridge.getTexture(i)
            img = None
            if data is not None:
                try:
                    img = textures.decode_image(data)
                except textures.ImageDecodeError as e:
                    self.texture_warnings.append("Failed tex %d: %s" % (i, e))
            self.uploadTextureImage(i, img)

    def uploadTextureImage(self, layer, rgba):
        """One layer from an (h, w, 4) uint8 image of any size (GPU bilinear resize); None = white fallback."""
        if rgba is None:
            self._check(self.L.rt_upload_texture_image(self.ctx, layer, None, 0, 0), "uploadTextureImage")
            return
        a = np.ascontiguousarray(rgba, dtype=np.uint8)
        if a.ndim != 3 or a.shape[2] != 4:
            raise RendererError("uploadTextureImage expects an (h, w, 4) uint8 array")
        self._check(self.L.rt_upload_texture_image(self.ctx, layer, _ptr(a), a.shape[1], a.shape[0]), "uploadTextureImage")

    def loadTextureLayers(self, layers):
        """Already decoded and resized (n, 1024, 1024, 4) uint8 layers (rt_upload_textures)."""
        a = np.ascontiguousarray(layers, dtype=np.uint8)
        self._check(self.L.rt_upload_textures(self.ctx, _ptr(a), a.shape[0]), "loadTextureLayers")

    def buildBlas(self, verts4, indices):
        """GPU binned-SAH BLAS build (rt_build_blas): returns (nodes (n, 8) float32, order (n_tris,) uint32)."""
        v = np.ascontiguousarray(verts4, dtype=np.float32).reshape(-1, 4)
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        n_tris = idx.size // 3
        nodes = np.empty((max(1, 2 * n_tris), 8), dtype=np.float32)
        order = np.empty(max(1, n_tris), dtype=np.uint32)
        n_nodes = ctypes.c_uint32()
        self._check(self.L.rt_build_blas(self.ctx, _ptr(v), v.shape[0], _ptr(idx), n_tris, _ptr(nodes), nodes.shape[0],
                                         ctypes.byref(n_nodes), _ptr(order)), "buildBlas")
        return nodes[:n_nodes.value].copy(), order[:n_tris].copy()

    # the bridge arrays of the device-resident world (rt_world_read): name -> (rt_world_array, dtype, row width)
    _WORLD_ARRAYS = {"vertices": (0, np.float32, 4), "normals": (1, np.float32, 4), "uvs": (2, np.float32, 2),
                     "mesh_topology": (3, np.uint32, 20), "tlas": (4, np.float32, 8), "blas": (5, np.float32, 8),
                     "instances": (6, np.float32, 36), "lights": (7, np.uint32, 2), "draw_commands": (8, np.uint32, 4),
                     "instance_order": (9, np.uint32, 1)}

    def worldRead(self, name):
        """One bridge array as the last device-resident update(t) left it in HBM (flat, the bridge getter's dtype)."""
        which, dtype, _ = self._WORLD_ARRAYS[name]
        n = ctypes.c_size_t()
        self._check(self.L.rt_world_read(self.ctx, which, None, 0, ctypes.byref(n)), "worldRead(%s)" % name)
        out = np.empty(n.value // 4, dtype=dtype)
        if n.value:
            self._check(self.L.rt_world_read(self.ctx, which, _ptr(out), out.nbytes, ctypes.byref(n)), "worldRead(%s)" % name)
        return out

    def setWorldStaticCache(self, enabled):
        """device-resident update(t): keep the BLAS / rows of geometries without a skin between frames (default on)"""
        self._check(self.L.rt_world_set_static_cache(self.ctx, 1 if enabled else 0), "setWorldStaticCache")

    def worldLastMs(self):
        """GPU stream time of the last device-resident update(t) (ms)."""
        return float(self.L.rt_world_last_ms(self.ctx))

    def worldLastTlasMs(self):
        """... of its TLAS kernel alone (ms)."""
        return float(self.L.rt_world_last_tlas_ms(self.ctx))

    def readTextureLayer(self, layer):
        out = np.empty((1024, 1024, 4), dtype=np.uint8)
        self._check(self.L.rt_read_texture_layer(self.ctx, layer, _ptr(out), out.nbytes), "readTextureLayer")
        return out

    def updateBuffer(self, kind, data):
        a = np.ascontiguousarray(data)
        rc = self._check(self.L.rt_upload(self.ctx, _KINDS[kind], _ptr(a), a.nbytes), "updateBuffer(%s)" % kind)
        return rc == RT_REALLOCATED

    def updateCombinedGeometry(self, v, n, uv):
        v, n, uv = (np.ascontiguousarray(x, dtype=np.float32) for x in (v, n, uv))
        rc = self._check(self.L.rt_upload_geometry(self.ctx, _ptr(v), _ptr(n), _ptr(uv), v.size // 4),
                         "updateCombinedGeometry")
        return rc == RT_REALLOCATED

    def updateCombinedBVH(self, tlas, blas):
        tlas, blas = (np.ascontiguousarray(x, dtype=np.float32) for x in (tlas, blas))
        rc = self._check(self.L.rt_upload_bvh(self.ctx, _ptr(tlas), tlas.size // 8, _ptr(blas), blas.size // 8),
                         "updateCombinedBVH")
        return rc == RT_REALLOCATED

    def updateSceneUniforms(self, cameraData, frameCount, lightCount):
        cam = np.ascontiguousarray(cameraData, dtype=np.float32)
        if cam.size != 24:
            raise ValueError("cameraData must hold 24 floats")
        self._check(self.L.rt_set_scene(self.ctx, _ptr(cam), int(frameCount), int(lightCount)), "updateSceneUniforms")

    def recreateBindGroup(self):
        self.L.rt_recreate_bind_group(self.ctx)

    def compute(self, frameCount):
        return self._check(self.L.rt_compute(self.ctx, int(frameCount)), "compute")

    def computeBatch(self, frameCounts):
        """`for k in batch: compute(samplesDone + k)` (VideoRecorder.ts:278-280) as one dispatch per kernel."""
        fc = np.ascontiguousarray(list(frameCounts), dtype=np.uint32)
        return self._check(self.L.rt_compute_batch(self.ctx, _ptr(fc), fc.size), "computeBatch")

    def present(self):
        return self._check(self.L.rt_present(self.ctx), "present")

    def captureFrame(self):
        if not self.width:
            raise RendererError("No render target")  # WebGPUContext.ts:43
        n = self.width * self.height * 4
        if self._capture_buf is None or self._capture_buf.size != n:
            self._capture_buf = np.empty(n, dtype=np.uint8)
        self._check(self.L.rt_capture(self.ctx, _ptr(self._capture_buf), n), "captureFrame")
        return {"data": self._capture_buf.reshape(self.height, self.width, 4),
                "width": self.width, "height": self.height}

    def sync(self):
        """`await renderer.device.queue.onSubmittedWorkDone()`"""
        self._check(self.L.rt_sync(self.ctx), "sync")

    # ---- additions (parity, checkpoint/resume, sharding, measurement) ----
    def readAccum(self):
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self.L.rt_read_accum(self.ctx, _ptr(out), out.nbytes), "readAccum")
        return out

    def writeAccum(self, a):
        a = np.ascontiguousarray(a, dtype=np.float32)
        self._check(self.L.rt_write_accum(self.ctx, _ptr(a), a.nbytes), "writeAccum")

    def readGBuffer(self):
        alb = np.empty((self.height, self.width, 4), dtype=np.uint8)
        nid = np.empty((self.height, self.width, 4), dtype=np.float32)
        dep = np.empty((self.height, self.width), dtype=np.float32)
        self._check(self.L.rt_read_gbuffer(self.ctx, _ptr(alb), _ptr(nid), _ptr(dep)), "readGBuffer")
        return alb, nid, dep

    def readHistory(self):
        out = np.empty((self.height, self.width, 4), dtype=np.uint16)
        self._check(self.L.rt_read_history(self.ctx, _ptr(out), out.nbytes), "readHistory")
        return out

    def readUniforms(self):
        out = np.empty(256, dtype=np.uint8)
        self._check(self.L.rt_read_uniforms(self.ctx, _ptr(out)), "readUniforms")
        return out

    def getCounters(self):
        out = np.zeros(6, dtype=np.uint64)
        self._check(self.L.rt_get_counters(self.ctx, _ptr(out)), "getCounters")
        return dict(zip(COUNTER_NAMES, (int(x) for x in out)))

    def debugPtLaunch(self):
        """Shape of the last persistent path-trace launch: {threads, workgroups, dyn_lds, per_cu} (all 0 before one)."""
        out = np.zeros(4, dtype=np.uint32)
        self._check(self.L.rt_debug_pt_launch(self.ctx, _ptr(out)), "debugPtLaunch")
        return dict(zip(("threads", "workgroups", "dyn_lds", "per_cu"), (int(x) for x in out)))

    def debugPtForm(self):
        """Materials the path-trace kernel of the last compute() dispatch carried code for: "plain" (the wide one-leaf form
        of a scene the host knows to hold untextured Lambertian triangles and lights only), "generic" (every other launch
        of the persistent kernel) or "none" (no dispatch yet, or one that ran another kernel).  The answer is the same
        whichever walk the kernel ran (debugPtWalk)."""
        form = int(self.L.rt_debug_pt_form(self.ctx))
        self._check(min(form, 0), "debugPtForm")
        return ("none", "generic", "plain", "generic", "plain")[form]

    def debugPtWalk(self):
        """How the path-trace kernel of the last compute() dispatch walked the BLAS: "sweep" (RT_PT_FORM_GENERIC_SWEEP,
        RT_PT_FORM_PLAIN_SWEEP: the leaves alone, in wave lock-step), "nodes" (every other launch of the persistent kernel)
        or "none" (no dispatch yet, or one that ran another kernel)."""
        form = int(self.L.rt_debug_pt_form(self.ctx))
        self._check(min(form, 0), "debugPtWalk")
        return ("none", "nodes", "nodes", "sweep", "sweep")[form]

    def getKernelCounters(self, kernel):
        """kernel: 0 = primary visibility, 1 = path trace"""
        out = np.zeros(6, dtype=np.uint64)
        self._check(self.L.rt_get_kernel_counters(self.ctx, int(kernel), _ptr(out)), "getKernelCounters")
        return dict(zip(COUNTER_NAMES, (int(x) for x in out)))

    def bindAccum(self, device_ptr):
        self._check(self.L.rt_bind_accum(self.ctx, ctypes.c_void_p(device_ptr or 0)), "bindAccum")

    def bindPresentSource(self, device_ptr):
        """present() reads this float4 device buffer instead of the accumulation buffer (0 / None = default)."""
        self._check(self.L.rt_bind_present_source(self.ctx, ctypes.c_void_p(device_ptr or 0)), "bindPresentSource")

    def resetCounters(self):
        self._check(self.L.rt_reset_counters(self.ctx), "resetCounters")

    def setCounting(self, detailed):
        self._check(self.L.rt_set_counting(self.ctx, 1 if detailed else 0), "setCounting")

    def setStripes(self, stripe_rows, rank, count):
        self._check(self.L.rt_set_stripes(self.ctx, int(stripe_rows), int(rank), int(count)), "setStripes")

    def accumDevicePtr(self):
        return self.L.rt_accum_device_ptr(self.ctx)

    def setStream(self, hip_stream_handle):
        self._check(self.L.rt_set_stream(self.ctx, ctypes.c_void_p(hip_stream_handle)), "setStream")

    # ---- ray queries against the uploaded scene (rt_trace_rays) ----
    def traceRays(self, rays, any_hit=False, t_min=0.001, stats=False):
        """rays: (n, 8) float32 in the rt_ray layout {origin, t_max, direction, -}.  Returns a structured array (n,) with
        the fields t, tri, inst, hit (RAY_HIT_DTYPE) - closest hit: a miss is (the ray's t_max, -1, -1, 0); any_hit:
        (0, -1, -1, occluded) - and with stats=True the pair (hits, stats dict of rt_ray_stats: the counting kernel runs)."""
        r = np.ascontiguousarray(rays, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] != 8:
            raise ValueError("traceRays expects an (n, 8) float32 array")
        n = r.shape[0]
        out = np.empty(n, dtype=RAY_HIT_DTYPE)
        st = RtRayStats()
        self._check(self.L.rt_trace_rays(self.ctx, _ptr(r), n, RT_RAYS_ANY if any_hit else RT_RAYS_CLOSEST, float(t_min),
                                         _ptr(out), ctypes.addressof(st) if stats else None), "traceRays")
        return (out, st.as_dict()) if stats else out

    def traceRaysDevice(self, rays_ptr, n, out_ptr, any_hit=False, t_min=0.001):
        """Enqueue a query on device arrays (n rt_ray at rays_ptr, n rt_ray_hit to out_ptr; e.g. tensor.data_ptr()) on the
        context's stream; no host synchronisation."""
        self._check(self.L.rt_trace_rays_device(self.ctx, ctypes.c_void_p(rays_ptr), int(n),
                                                RT_RAYS_ANY if any_hit else RT_RAYS_CLOSEST, float(t_min),
                                                ctypes.c_void_p(out_ptr)), "traceRaysDevice")

    def rayQueryStats(self):
        """rt_ray_stats of the last query as a dict (blocking)."""
        st = RtRayStats()
        self._check(self.L.rt_ray_query_stats(self.ctx, ctypes.addressof(st)), "rayQueryStats")
        return st.as_dict()

    # ---- radiance queries against the uploaded scene (rt_trace_radiance) ----
    def traceRadiance(self, rays, max_depth, spp, seed=0, stats=False):
        """rays: (n, 8) float32 in the rt_ray layout {origin, t_max, direction, pad}; pad holds the bits of a uint32, the
        ray's RNG stream id.  Returns a structured array (n,) with the fields rgb (3 floats) and t (RADIANCE_DTYPE): the
        path tracer's radiance along each ray, averaged over spp samples, and the first hit's distance (a miss: +0 and the
        ray's t_max) - and with stats=True the pair (results, stats dict of rt_radiance_stats: the counting kernel runs)."""
        r = np.ascontiguousarray(rays, dtype=np.float32)
        if r.ndim != 2 or r.shape[1] != 8:
            raise ValueError("traceRadiance expects an (n, 8) float32 array")
        n = r.shape[0]
        out = np.empty(n, dtype=RADIANCE_DTYPE)
        st = RtRadianceStats()
        self._check(self.L.rt_trace_radiance(self.ctx, _ptr(r), n, int(max_depth), int(spp), int(seed) & 0xffffffff, _ptr(out),
                                             ctypes.addressof(st) if stats else None), "traceRadiance")
        return (out, st.as_dict()) if stats else out

    def traceRadianceDevice(self, rays_ptr, n, out_ptr, max_depth, spp, seed=0):
        """Enqueue a radiance query on device arrays (n rt_ray at rays_ptr, n rt_radiance to out_ptr; e.g.
        tensor.data_ptr()) on the context's stream; no host synchronisation."""
        self._check(self.L.rt_trace_radiance_device(self.ctx, ctypes.c_void_p(rays_ptr), int(n), int(max_depth), int(spp),
                                                    int(seed) & 0xffffffff, ctypes.c_void_p(out_ptr)), "traceRadianceDevice")

    def radianceQueryStats(self):
        """rt_radiance_stats of the last radiance query as a dict (blocking)."""
        st = RtRadianceStats()
        self._check(self.L.rt_radiance_query_stats(self.ctx, ctypes.addressof(st)), "radianceQueryStats")
        return st.as_dict()

    # ---- irradiance gathers at surface points of the uploaded scene (rt_gather_irradiance) ----
    def gatherIrradiance(self, points, max_depth, spp, seed=0, stats=False):
        """points: (n, 8) float32 in the rt_gather_point layout {position, t_max, normal, pad}; pad holds the bits of a
        uint32 below 2^31, the point's RNG stream id.  Returns a structured array (n,) with the fields rgb (3 floats) and
        hit_fraction (IRRADIANCE_DTYPE): the cosine-weighted mean radiance arriving at each point over spp hemisphere
        directions drawn on the device (E / pi: multiply by pi for irradiance) and the fraction of them that hit something
        within t_max - and with stats=True the pair (results, stats dict of rt_radiance_stats with rays = points: the
        counting kernel runs)."""
        p = np.ascontiguousarray(points, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != 8:
            raise ValueError("gatherIrradiance expects an (n, 8) float32 array")
        n = p.shape[0]
        out = np.empty(n, dtype=IRRADIANCE_DTYPE)
        st = RtRadianceStats()
        self._check(self.L.rt_gather_irradiance(self.ctx, _ptr(p), n, int(max_depth), int(spp), int(seed) & 0xffffffff, _ptr(out),
                                                ctypes.addressof(st) if stats else None), "gatherIrradiance")
        return (out, st.as_dict()) if stats else out

    def gatherIrradianceDevice(self, points_ptr, n, out_ptr, max_depth, spp, seed=0):
        """Enqueue an irradiance gather on device arrays (n rt_gather_point at points_ptr, n rt_irradiance to out_ptr; e.g.
        tensor.data_ptr()) on the context's stream; no host synchronisation."""
        self._check(self.L.rt_gather_irradiance_device(self.ctx, ctypes.c_void_p(points_ptr), int(n), int(max_depth), int(spp),
                                                       int(seed) & 0xffffffff, ctypes.c_void_p(out_ptr)), "gatherIrradianceDevice")

    def irradianceGatherStats(self):
        """rt_radiance_stats of the last irradiance gather as a dict (blocking)."""
        st = RtRadianceStats()
        self._check(self.L.rt_irradiance_gather_stats(self.ctx, ctypes.addressof(st)), "irradianceGatherStats")
        return st.as_dict()

    # ---- probe gathers: SH9 radiance at points in space (rt_gather_probes) ----
    def gatherProbes(self, probes, max_depth, spp, seed=0, stats=False):
        """probes: (n, 8) float32 in the rt_probe layout {position, t_max, 3 unused words, pad} (or a PROBE_DTYPE array);
        pad holds the bits of a uint32 below 2^31, the probe's RNG stream id.  Returns a structured array (n,) with the
        fields sh (9 x 3 floats: coefficient-major, rgb inside) and hit_fraction (PROBE_SH9_DTYPE): the projection of the
        radiance arriving at each probe, over spp directions drawn uniformly on the sphere on the device, onto the real
        spherical harmonics of bands 0 .. 2 (sh9_irradiance turns them into irradiance at a normal) - and with stats=True
        the pair (results, stats dict of rt_radiance_stats with rays = probes: the counting kernel runs)."""
        p = np.ascontiguousarray(probes)
        if p.dtype == PROBE_DTYPE:
            p = p.reshape(-1).view(np.float32).reshape(-1, 8)
        p = np.ascontiguousarray(p, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != 8:
            raise ValueError("gatherProbes expects an (n, 8) float32 array")
        n = p.shape[0]
        out = np.empty(n, dtype=PROBE_SH9_DTYPE)
        st = RtRadianceStats()
        self._check(self.L.rt_gather_probes(self.ctx, _ptr(p), n, int(max_depth), int(spp), int(seed) & 0xffffffff, _ptr(out),
                                            ctypes.addressof(st) if stats else None), "gatherProbes")
        return (out, st.as_dict()) if stats else out

    def gatherProbesDevice(self, probes_ptr, n, out_ptr, max_depth, spp, seed=0):
        """Enqueue a probe gather on device arrays (n rt_probe at probes_ptr, n rt_probe_sh9 of 112 bytes to out_ptr; e.g.
        tensor.data_ptr()) on the context's stream; no host synchronisation."""
        self._check(self.L.rt_gather_probes_device(self.ctx, ctypes.c_void_p(probes_ptr), int(n), int(max_depth), int(spp),
                                                   int(seed) & 0xffffffff, ctypes.c_void_p(out_ptr)), "gatherProbesDevice")

    def probeGatherStats(self):
        """rt_radiance_stats of the last probe gather as a dict (blocking)."""
        st = RtRadianceStats()
        self._check(self.L.rt_probe_gather_stats(self.ctx, ctypes.addressof(st)), "probeGatherStats")
        return st.as_dict()

    # ---- irradiance volumes: a probe grid baked, sampled and exported on the device (rt_bake_volume, rt_sample_volume) ----
    def bakeVolume(self, desc, max_depth, spp, seed=0, stats=False):
        """desc: a VOLUME_DESC_DTYPE record (volume_desc).  Returns the volume, a PROBE_SH9_DTYPE array (nz, ny, nx) of
        IRRADIANCE coefficients (the probe gather of the grid's probes, times the cosine-lobe band factors and desc's window;
        hit_fraction untouched) - and with stats=True the pair (volume, stats dict of the probe gather: the counting kernel
        runs).  probeGatherStats reports a bake like a gather."""
        d = _volume_desc(desc)
        out = np.empty((int(d["nz"]), int(d["ny"]), int(d["nx"])), dtype=PROBE_SH9_DTYPE)
        st = RtRadianceStats()
        self._check(self.L.rt_bake_volume(self.ctx, _ptr(d), int(max_depth), int(spp), int(seed) & 0xffffffff,
                                          _ptr(out) if out.size else None, ctypes.addressof(st) if stats else None), "bakeVolume")
        return (out, st.as_dict()) if stats else out

    def bakeVolumeDevice(self, desc, out_ptr, max_depth, spp, seed=0):
        """Enqueue a bake into the nx * ny * nz rt_probe_sh9 records (112 bytes each) at the device pointer out_ptr on the
        context's stream; no host synchronisation."""
        d = _volume_desc(desc)
        self._check(self.L.rt_bake_volume_device(self.ctx, _ptr(d), int(max_depth), int(spp), int(seed) & 0xffffffff,
                                                 ctypes.c_void_p(out_ptr or 0)), "bakeVolumeDevice")

    def sampleVolume(self, desc, volume, points):
        """volume: the PROBE_SH9_DTYPE array of a bake (or (n, 28) float32); points: (n, 8) float32 in the rt_gather_point
        layout {position, -, normal, -}.  Returns an IRRADIANCE_DTYPE array (n,): rgb the irradiance E(normal) interpolated
        from the eight surrounding valid probes, clamped at 0, hit_fraction the valid share of the interpolation weight.  Needs
        no scene.  Uploads the volume on every call: a caller sampling every frame keeps it on the device and uses
        sampleVolumeDevice."""
        d = _volume_desc(desc)
        v = np.ascontiguousarray(volume)
        if v.dtype != PROBE_SH9_DTYPE:
            v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 28)
        if v.size * v.dtype.itemsize != 112 * int(d["nx"]) * int(d["ny"]) * int(d["nz"]):
            raise ValueError("sampleVolume: the volume does not hold nx * ny * nz records")
        p = np.ascontiguousarray(points, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != 8:
            raise ValueError("sampleVolume expects an (n, 8) float32 array of points")
        out = np.empty(p.shape[0], dtype=IRRADIANCE_DTYPE)
        self._check(self.L.rt_sample_volume(self.ctx, _ptr(d), _ptr(v), _ptr(p) if p.size else None, p.shape[0],
                                            _ptr(out) if out.size else None), "sampleVolume")
        return out

    def sampleVolumeDevice(self, desc, volume_ptr, points_ptr, n, out_ptr):
        """Enqueue the sampling of n rt_gather_point at points_ptr from the volume at volume_ptr into n rt_irradiance at
        out_ptr (device pointers, 16-byte aligned) on the context's stream; no host synchronisation."""
        d = _volume_desc(desc)
        self._check(self.L.rt_sample_volume_device(self.ctx, _ptr(d), ctypes.c_void_p(volume_ptr or 0),
                                                   ctypes.c_void_p(points_ptr or 0), int(n), ctypes.c_void_p(out_ptr or 0)),
                    "sampleVolumeDevice")

    def encodeVolume(self, desc, volume, format):
        """The volume as seven texel layers for a 3D-texture upload: (7, nz, ny, nx, 4) float32 ("f32") or float16 ("f16"),
        layer j holding the floats 4 j .. 4 j + 3 of every record.  "rgbe" is refused: coefficients are signed."""
        d = _volume_desc(desc)
        v = np.ascontiguousarray(volume)
        if v.dtype != PROBE_SH9_DTYPE:
            v = np.ascontiguousarray(v, dtype=np.float32).reshape(-1, 28)
        if v.size * v.dtype.itemsize != 112 * int(d["nx"]) * int(d["ny"]) * int(d["nz"]):
            raise ValueError("encodeVolume: the volume does not hold nx * ny * nz records")
        fmt = _lightmap_format(format)
        out = np.empty((7, int(d["nz"]), int(d["ny"]), int(d["nx"]), 4), np.float16 if fmt == RT_LIGHTMAP_F16 else np.float32)
        self._check(self.L.rt_encode_volume(self.ctx, _ptr(d), fmt, _ptr(v), _ptr(out), out.nbytes), "encodeVolume")
        return out

    # ---- reflection probes: octahedral radiance maps and their GGX-filtered chains (rt_capture_reflection, rt_filter_reflection,
    # rt_bake_reflection) ----
    def captureReflection(self, desc, probes, max_depth, seed=0, stats=False):
        """desc: a REFLECTION_DESC_DTYPE record (reflection_desc); probes: (n, 8) float32 in the rt_probe layout (or a
        PROBE_DTYPE array), pad + size * size <= 2^31.  Returns the maps, (n, size, size, 4) float32 {r, g, b, hit_fraction},
        [p, j, i] for texel (i, j) of probe p: the radiance arriving at the probe through each octahedral texel, the mean of
        desc.spt jittered samples - and with stats=True the pair (maps, stats dict of rt_radiance_stats with rays = texels: the
        counting kernel runs)."""
        d = _reflection_desc(desc)
        p = _probe_array(probes, "captureReflection")
        n, size = p.shape[0], int(d["size"])
        out = np.empty((n, size, size, 4), np.float32)
        st = RtRadianceStats()
        self._check(self.L.rt_capture_reflection(self.ctx, _ptr(d), _ptr(p) if n else None, n, int(max_depth),
                                                 int(seed) & 0xffffffff, _ptr(out) if out.size else None,
                                                 ctypes.addressof(st) if stats else None), "captureReflection")
        return (out, st.as_dict()) if stats else out

    def captureReflectionDevice(self, desc, probes_ptr, n, out_ptr, max_depth, seed=0):
        """Enqueue a capture on device arrays (n rt_probe at probes_ptr, n maps of size * size 16-byte texels to out_ptr) on the
        context's stream; no host synchronisation."""
        d = _reflection_desc(desc)
        self._check(self.L.rt_capture_reflection_device(self.ctx, _ptr(d), ctypes.c_void_p(probes_ptr or 0), int(n), int(max_depth),
                                                        int(seed) & 0xffffffff, ctypes.c_void_p(out_ptr or 0)),
                    "captureReflectionDevice")

    def filterReflection(self, desc, maps):
        """maps: (n, size, size, 4) float32 (or one (size, size, 4) map).  Returns the chains, (n, chain_texels, 4) float32:
        level 0 the map word for word, level m >= 1 its GGX-filtered form at the roughness m / (levels - 1), at the texel
        offsets of reflection_level_offsets.  Needs no scene."""
        d = _reflection_desc(desc)
        size = int(d["size"])
        m = np.ascontiguousarray(maps, dtype=np.float32)
        if m.ndim == 3:
            m = m[None]
        if m.ndim != 4 or m.shape[1:] != (size, size, 4):
            raise ValueError("filterReflection expects (n, size, size, 4) float32 maps")
        n = m.shape[0]
        out = np.empty((n, _reflection_chain_texels(d), 4), np.float32)
        self._check(self.L.rt_filter_reflection(self.ctx, _ptr(d), _ptr(m) if n else None, n, _ptr(out) if out.size else None),
                    "filterReflection")
        return out

    def filterReflectionDevice(self, desc, maps_ptr, n, chains_ptr):
        """Enqueue a filter on device arrays: n packed maps at maps_ptr into n chains at chains_ptr - or, with maps_ptr ==
        chains_ptr, in place on chains whose level 0 is there already (the layout of a bake).  No host synchronisation."""
        d = _reflection_desc(desc)
        self._check(self.L.rt_filter_reflection_device(self.ctx, _ptr(d), ctypes.c_void_p(maps_ptr or 0), int(n),
                                                       ctypes.c_void_p(chains_ptr or 0)), "filterReflectionDevice")

    def bakeReflection(self, desc, probes, max_depth, seed=0, stats=False):
        """captureReflection straight into level 0 of each chain, then filterReflection in place, without leaving the device:
        (n, chain_texels, 4) float32 - and with stats=True the pair (chains, stats dict of the capture)."""
        d = _reflection_desc(desc)
        p = _probe_array(probes, "bakeReflection")
        n = p.shape[0]
        out = np.empty((n, _reflection_chain_texels(d), 4), np.float32)
        st = RtRadianceStats()
        self._check(self.L.rt_bake_reflection(self.ctx, _ptr(d), _ptr(p) if n else None, n, int(max_depth), int(seed) & 0xffffffff,
                                              _ptr(out) if out.size else None, ctypes.addressof(st) if stats else None),
                    "bakeReflection")
        return (out, st.as_dict()) if stats else out

    def bakeReflectionDevice(self, desc, probes_ptr, n, chains_ptr, max_depth, seed=0):
        """Enqueue a bake on device arrays (n rt_probe at probes_ptr, n chains to chains_ptr) on the context's stream; no host
        synchronisation."""
        d = _reflection_desc(desc)
        self._check(self.L.rt_bake_reflection_device(self.ctx, _ptr(d), ctypes.c_void_p(probes_ptr or 0), int(n), int(max_depth),
                                                     int(seed) & 0xffffffff, ctypes.c_void_p(chains_ptr or 0)),
                    "bakeReflectionDevice")

    def reflectionStats(self):
        """rt_radiance_stats of the last reflection capture or bake as a dict (blocking)."""
        st = RtRadianceStats()
        self._check(self.L.rt_reflection_stats(self.ctx, ctypes.addressof(st)), "reflectionStats")
        return st.as_dict()

    def encodeReflection(self, desc, chain, format):
        """chain: one chain, (chain_texels, 4) float32.  Returns the list of its levels, each encodeAtlas of the level's (S, S, 4)
        texels in the format "f32", "f16" or "rgbe" (radiance is not signed, so all three apply)."""
        d = _reflection_desc(desc)
        off = reflection_level_offsets(int(d["size"]), int(d["levels"]))
        c = np.ascontiguousarray(chain, dtype=np.float32)
        if c.shape != (int(off[-1]), 4):
            raise ValueError("encodeReflection expects one chain, (chain_texels, 4) float32")
        out = []
        for m in range(int(d["levels"])):
            side = int(d["size"]) >> m
            out.append(self.encodeAtlas(c[off[m]:off[m + 1]].reshape(side, side, 4), format))
        return out

    # ---- the reflection sampler: baked chains read at a direction and a roughness (rt_sample_reflection) ----
    def sampleReflection(self, desc, chains, queries, probes=None, boxes=None):
        """desc: a REFLECTION_SAMPLE_DESC_DTYPE record (reflection_sample_desc); chains: (n_probes, chain_texels, 4) float32 as
        bakeReflection returns them; queries: a REFLECTION_QUERY_DTYPE array (reflection_queries) or (n, 8) float32.  With
        parallax also probes, the (n_probes, 8) rt_probe records the chains were baked at, and boxes, a REFLECTION_BOX_DTYPE
        array (n_probes,) or (n_probes, 8) float32.  Returns (n, 4) float32 {r, g, b, hit_fraction}: the seam-aware bilinear
        fetch at each direction from the two levels around roughness * (levels - 1), mixed (THE REFLECTION SAMPLE RULE).
        Needs no scene.  Uploads the chains on every call: a caller sampling every frame keeps them on the device and uses
        sampleReflectionDevice."""
        d = _reflection_sample_desc(desc)
        texels = _reflection_chain_texels(d)
        c = np.ascontiguousarray(chains, dtype=np.float32)
        if texels and c.size % (4 * texels) != 0:
            raise ValueError("sampleReflection: the chains do not hold whole chains of the descriptor's size and levels")
        n_probes = c.size // (4 * texels) if texels else 0   # (0: the library refuses the descriptor)
        q = _records(queries, REFLECTION_QUERY_DTYPE, "sampleReflection")
        p = b = None
        if int(d["flags"]) & RT_REFLECTION_SAMPLE_PARALLAX:
            if probes is None or boxes is None:
                raise ValueError("sampleReflection: parallax needs the probes and their boxes")
            p = _probe_array(probes, "sampleReflection")
            b = _records(boxes, REFLECTION_BOX_DTYPE, "sampleReflection")
            if p.shape[0] != n_probes or b.shape[0] != n_probes:
                raise ValueError("sampleReflection: one probe and one box per chain")
        out = np.empty((q.shape[0], 4), np.float32)
        self._check(self.L.rt_sample_reflection(self.ctx, _ptr(d), _ptr(c) if c.size else None, n_probes,
                                                _ptr(p) if p is not None and p.size else None,
                                                _ptr(b) if b is not None and b.size else None, _ptr(q) if q.size else None,
                                                q.shape[0], _ptr(out) if out.size else None), "sampleReflection")
        return out

    def sampleReflectionDevice(self, desc, chains_ptr, n_probes, queries_ptr, n, out_ptr, probes_ptr=0, boxes_ptr=0):
        """Enqueue the sampling of n rt_reflection_query at queries_ptr from the n_probes chains at chains_ptr into n texels at
        out_ptr (device pointers, 16-byte aligned; with parallax also the rt_probe and rt_reflection_box arrays) on the
        context's stream; no host synchronisation."""
        d = _reflection_sample_desc(desc)
        self._check(self.L.rt_sample_reflection_device(self.ctx, _ptr(d), ctypes.c_void_p(chains_ptr or 0), int(n_probes),
                                                       ctypes.c_void_p(probes_ptr or 0), ctypes.c_void_p(boxes_ptr or 0),
                                                       ctypes.c_void_p(queries_ptr or 0), int(n), ctypes.c_void_p(out_ptr or 0)),
                    "sampleReflectionDevice")

    # ---- probe visibility maps: distance moments per probe of a volume, and the sampler they keep from leaking light ----
    def bakeVolumeVisibility(self, desc, vis, seed=0, stats=False):
        """desc: the VOLUME_DESC_DTYPE record of the volume; vis: a VOLUME_VISIBILITY_DESC_DTYPE record
        (volume_visibility_desc).  Returns the visibility volume, (nz, ny, nx, size, size, 2) float32 {mean distance, mean
        squared distance} - and with stats=True the pair (maps, rt_ray_stats dict summed over the batches: the counting kernel
        runs).  rayQueryStats keeps reporting the last traceRays."""
        d, v = _volume_desc(desc), _volume_visibility_desc(vis)
        size = int(v["size"])
        out = np.empty((int(d["nz"]), int(d["ny"]), int(d["nx"]), size, size, 2), np.float32)
        st = RtRayStats()
        self._check(self.L.rt_bake_volume_visibility(self.ctx, _ptr(d), _ptr(v), int(seed) & 0xffffffff,
                                                     _ptr(out) if out.size else None, ctypes.addressof(st) if stats else None),
                    "bakeVolumeVisibility")
        return (out, st.as_dict()) if stats else out

    def bakeVolumeVisibilityDevice(self, desc, vis, out_ptr, seed=0):
        """Enqueue a bake into the nx * ny * nz * size * size texels (8 bytes each) at the device pointer out_ptr on the
        context's stream; no host synchronisation."""
        d, v = _volume_desc(desc), _volume_visibility_desc(vis)
        self._check(self.L.rt_bake_volume_visibility_device(self.ctx, _ptr(d), _ptr(v), int(seed) & 0xffffffff,
                                                            ctypes.c_void_p(out_ptr or 0)), "bakeVolumeVisibilityDevice")

    def volumeVisibilityStats(self):
        """rt_ray_stats of the last visibility bake as a dict (blocking)."""
        st = RtRayStats()
        self._check(self.L.rt_volume_visibility_stats(self.ctx, ctypes.addressof(st)), "volumeVisibilityStats")
        return st.as_dict()

    def sampleVolumeVisible(self, desc, vis, volume, visibility, points):
        """sampleVolume with every corner probe's trilinear weight multiplied by its visibility of the point (THE VISIBILITY
        RULE): volume as for sampleVolume, visibility the array of bakeVolumeVisibility, points (n, 8) float32.  Returns an
        IRRADIANCE_DTYPE array (n,).  Needs no scene.  Uploads the volume and the maps on every call: a caller sampling every
        frame keeps them on the device and uses sampleVolumeVisibleDevice."""
        d, v = _volume_desc(desc), _volume_visibility_desc(vis)
        vol = np.ascontiguousarray(volume)
        if vol.dtype != PROBE_SH9_DTYPE:
            vol = np.ascontiguousarray(vol, dtype=np.float32).reshape(-1, 28)
        if vol.size * vol.dtype.itemsize != 112 * int(d["nx"]) * int(d["ny"]) * int(d["nz"]):
            raise ValueError("sampleVolumeVisible: the volume does not hold nx * ny * nz records")
        m = _visibility_maps(d, v, visibility, "sampleVolumeVisible")
        p = np.ascontiguousarray(points, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != 8:
            raise ValueError("sampleVolumeVisible expects an (n, 8) float32 array of points")
        out = np.empty(p.shape[0], dtype=IRRADIANCE_DTYPE)
        self._check(self.L.rt_sample_volume_visible(self.ctx, _ptr(d), _ptr(v), _ptr(vol), _ptr(m), _ptr(p) if p.size else None,
                                                    p.shape[0], _ptr(out) if out.size else None), "sampleVolumeVisible")
        return out

    def sampleVolumeVisibleDevice(self, desc, vis, volume_ptr, visibility_ptr, points_ptr, n, out_ptr):
        """Enqueue the sampling of n rt_gather_point at points_ptr from the volume at volume_ptr and the maps at visibility_ptr
        into n rt_irradiance at out_ptr (device pointers, 16-byte aligned) on the context's stream; no host synchronisation."""
        d, v = _volume_desc(desc), _volume_visibility_desc(vis)
        self._check(self.L.rt_sample_volume_visible_device(self.ctx, _ptr(d), _ptr(v), ctypes.c_void_p(volume_ptr or 0),
                                                           ctypes.c_void_p(visibility_ptr or 0), ctypes.c_void_p(points_ptr or 0),
                                                           int(n), ctypes.c_void_p(out_ptr or 0)), "sampleVolumeVisibleDevice")

    def encodeVolumeVisibility(self, desc, vis, visibility, format):
        """The maps as one image of bordered tiles for a 2D-texture upload: (ny * nz * (size + 2), nx * (size + 2), 2) float32
        ("f32") or float16 ("f16"), probe (x, y, z) at tile (x, z * ny + y), a tile's border the wrapped neighbour texel.
        "rgbe" is refused."""
        d, v = _volume_desc(desc), _volume_visibility_desc(vis)
        m = _visibility_maps(d, v, visibility, "encodeVolumeVisibility")
        fmt = _lightmap_format(format)
        tile = int(v["size"]) + 2
        out = np.empty((int(d["ny"]) * int(d["nz"]) * tile, int(d["nx"]) * tile, 2),
                       np.float16 if fmt == RT_LIGHTMAP_F16 else np.float32)
        self._check(self.L.rt_encode_volume_visibility(self.ctx, _ptr(d), _ptr(v), fmt, _ptr(m), _ptr(out), out.nbytes),
                    "encodeVolumeVisibility")
        return out

    # ---- directional gathers: SH radiance of bands 0 .. 1 over the hemisphere of surface points (rt_gather_directional) ----
    def gatherDirectional(self, points, max_depth, spp, seed=0, stats=False):
        """points: (n, 8) float32 in the rt_gather_point layout {position, t_max, normal, pad}, as for gatherIrradiance.
        Returns a structured array (n,) with the field layer (4 x 4 floats, DIRECTIONAL_DTYPE): layer[k] = {sh[k].r, sh[k].g,
        sh[k].b, hit_fraction}, the projection of the radiance arriving at each point, over spp directions drawn uniformly on
        the hemisphere of its normal on the device, onto the real spherical harmonics Y0, Y1 (y), Y2 (z), Y3 (x) in world
        space (sh4_irradiance turns them into irradiance at a normal) - and with stats=True the pair (results, stats dict of
        rt_radiance_stats with rays = points: the counting kernel runs)."""
        p = np.ascontiguousarray(points, dtype=np.float32)
        if p.ndim != 2 or p.shape[1] != 8:
            raise ValueError("gatherDirectional expects an (n, 8) float32 array")
        n = p.shape[0]
        out = np.empty(n, dtype=DIRECTIONAL_DTYPE)
        st = RtRadianceStats()
        self._check(self.L.rt_gather_directional(self.ctx, _ptr(p), n, int(max_depth), int(spp), int(seed) & 0xffffffff,
                                                 _ptr(out), ctypes.addressof(st) if stats else None), "gatherDirectional")
        return (out, st.as_dict()) if stats else out

    def gatherDirectionalDevice(self, points_ptr, n, out_ptr, max_depth, spp, seed=0):
        """Enqueue a directional gather on device arrays (n rt_gather_point at points_ptr, n rt_directional of 64 bytes to
        out_ptr; e.g. tensor.data_ptr()) on the context's stream; no host synchronisation."""
        self._check(self.L.rt_gather_directional_device(self.ctx, ctypes.c_void_p(points_ptr), int(n), int(max_depth), int(spp),
                                                        int(seed) & 0xffffffff, ctypes.c_void_p(out_ptr)),
                    "gatherDirectionalDevice")

    def directionalGatherStats(self):
        """rt_radiance_stats of the last directional gather as a dict (blocking)."""
        st = RtRadianceStats()
        self._check(self.L.rt_directional_gather_stats(self.ctx, ctypes.addressof(st)), "directionalGatherStats")
        return st.as_dict()

    # ---- lightmap bakes: the texels of an instance's UV atlas as gather points (rt_bake_points) ----
    @staticmethod
    def _bake_desc(inst, width, height, t_max, pad_base):
        d = RtBakeDesc()
        d.inst, d.width, d.height, d.pad_base, d.t_max = int(inst), int(width), int(height), int(pad_base), float(t_max)
        return d

    @staticmethod
    def _atlas_uv(atlas_uv):
        if atlas_uv is None:
            return None, None, 0
        uv = np.ascontiguousarray(atlas_uv, dtype=np.float32).reshape(-1, 2)
        return uv, _ptr(uv), uv.shape[0]

    def bakePoints(self, inst, width, height, t_max=1e30, pad_base=0, atlas_uv=None, owner=False, cap=None):
        """The gather points of the covered texels of TLAS-order instance `inst`'s width x height atlas, by the texel rule
        of include/mi355rt.h: (points (n, 8) float32 in the rt_gather_point layout, pad = pad_base + texel index; texels
        (n,) uint32, ascending) - and with owner=True a third item, the (height, width) int32 owner map (global triangle
        index, -1 = uncovered).  atlas_uv: (vertex_count, 2) float32 override UVs of the whole scene, None = the scene's.
        cap: at most that many records are written (the first ones); the count n is then returned as a last extra item."""
        d = self._bake_desc(inst, width, height, t_max, pad_base)
        uv, uv_ptr, n_uv = self._atlas_uv(atlas_uv)
        room = int(width) * int(height) if cap is None else int(cap)
        points = np.empty((room, 8), np.float32)
        texels = np.empty(room, np.uint32)
        own = np.empty((int(height), int(width)), np.int32) if owner else None
        n = ctypes.c_uint32(0)
        self._check(self.L.rt_bake_points(self.ctx, ctypes.addressof(d), uv_ptr, n_uv, _ptr(points) if room else None,
                                          _ptr(texels) if room else None, room, ctypes.addressof(n),
                                          _ptr(own) if owner else None), "bakePoints")
        got = min(n.value, room)
        out = (points[:got], texels[:got]) + ((own,) if owner else ())
        return out + (n.value,) if cap is not None else out

    def bakePointsDevice(self, inst, width, height, points_ptr, texels_ptr, cap, count_ptr, t_max=1e30, pad_base=0,
                         atlas_uv_ptr=None, owner_ptr=None):
        """Enqueue the point pass on device arrays (cap rt_gather_point at points_ptr, cap u32 at texels_ptr, one u32 at
        count_ptr, optionally width * height u32 at owner_ptr and 2 f32 per scene vertex at atlas_uv_ptr; e.g.
        tensor.data_ptr()) on the context's stream; no host synchronisation.  EVERY pointer, the single count word included,
        must be 16-byte aligned (a fresh tensor is; a slice of one may not be) and lie on the context's device, else
        RT_ERR_INVALID."""
        d = self._bake_desc(inst, width, height, t_max, pad_base)
        self._check(self.L.rt_bake_points_device(self.ctx, ctypes.addressof(d), ctypes.c_void_p(atlas_uv_ptr or 0),
                                                 ctypes.c_void_p(points_ptr or 0), ctypes.c_void_p(texels_ptr or 0), int(cap),
                                                 ctypes.c_void_p(count_ptr or 0), ctypes.c_void_p(owner_ptr or 0)),
                    "bakePointsDevice")

    def bakeIrradiance(self, inst, width, height, max_depth, spp, seed=0, t_max=1e30, pad_base=0, atlas_uv=None, stats=False,
                       dilate=0, denoise=None):
        """The whole bake: points, the irradiance gather on them, scatter.  Returns the (height, width) IRRADIANCE_DTYPE
        atlas - texel texels[j] holds what gatherIrradiance returns for points[j] (E / pi: multiply by pi * albedo for a
        Lambert texel's outgoing radiance), uncovered texels are {0, 0, 0, -1} - and with stats=True the triple (atlas,
        number of covered texels, stats dict of the gather).  dilate > 0: dilateAtlas with that radius on the returned atlas
        (filled texels carry hit_fraction -2); it costs one more round trip of the atlas to the device and back.
        denoise: None, or a dict of denoiseAtlas's keyword arguments (plane_eps and max_dist at least): the bake then runs
        bakePoints ONCE MORE with the same arguments - an extra point pass - for the guides and denoises the atlas with them,
        before any dilation."""
        d = self._bake_desc(inst, width, height, t_max, pad_base)
        uv, uv_ptr, n_uv = self._atlas_uv(atlas_uv)
        out = np.empty((int(height), int(width)), dtype=IRRADIANCE_DTYPE)
        n = ctypes.c_uint32(0)
        st = RtRadianceStats()
        self._check(self.L.rt_bake_irradiance(self.ctx, ctypes.addressof(d), uv_ptr, n_uv, int(max_depth), int(spp),
                                              int(seed) & 0xffffffff, _ptr(out), ctypes.addressof(n),
                                              ctypes.addressof(st) if stats else None), "bakeIrradiance")
        if denoise is not None:
            points, texels = self.bakePoints(inst, width, height, t_max, pad_base, atlas_uv)
            out = self.denoiseAtlas(out, points, texels, **denoise)
        if dilate > 0:
            out = self.dilateAtlas(out, dilate)
        return (out, n.value, st.as_dict()) if stats else out

    # ---- atlas bakes: a list of (instance, rectangle) entries into one atlas (rt_bake_atlas_points) ----
    @staticmethod
    def _atlas_args(entries, width, height, t_max, pad_base):
        """-> (rt_bake_atlas_desc, the entries as an (n, 8) uint32 array in the rt_bake_rect layout)"""
        e = np.asarray(entries, dtype=np.int64).reshape(-1, 5)
        if e.size and (e.min() < 0 or e.max() > 0xffffffff):
            raise ValueError("bake atlas: entries are (inst, x, y, w, h) in uint32")
        rects = np.zeros((e.shape[0], 8), np.uint32)
        rects[:, 0:5] = e
        d = RtBakeAtlasDesc()
        d.width, d.height, d.pad_base, d.t_max, d.n_entries = int(width), int(height), int(pad_base), float(t_max), e.shape[0]
        return d, rects

    def bakeAtlasPoints(self, entries, width, height, t_max=1e30, pad_base=0, atlas_uv=None, owner=False, cap=None):
        """The gather points of the covered texels of a width x height atlas into which every entry (inst, x, y, w, h) - an
        (n, 5) array or a list of such tuples - bakes TLAS-order instance `inst` at w x h texels, placed at (x, y); by the
        atlas rule of include/mi355rt.h, the lowest entry owning a texel several cover.  Returns (points (n, 8) float32, pad =
        pad_base + atlas texel index; texels (n,) uint32, ascending) - and with owner=True a third item, the (height, width,
        2) int32 owner map {entry, global triangle index}, {-1, -1} = uncovered.  atlas_uv and cap as in bakePoints."""
        d, rects = self._atlas_args(entries, width, height, t_max, pad_base)
        uv, uv_ptr, n_uv = self._atlas_uv(atlas_uv)
        room = int(width) * int(height) if cap is None else int(cap)
        points = np.empty((room, 8), np.float32)
        texels = np.empty(room, np.uint32)
        own = np.empty((int(height), int(width), 2), np.int32) if owner else None
        n = ctypes.c_uint32(0)
        self._check(self.L.rt_bake_atlas_points(self.ctx, ctypes.addressof(d), _ptr(rects), uv_ptr, n_uv,
                                                _ptr(points) if room else None, _ptr(texels) if room else None, room,
                                                ctypes.addressof(n), _ptr(own) if owner else None), "bakeAtlasPoints")
        got = min(n.value, room)
        out = (points[:got], texels[:got]) + ((own,) if owner else ())
        return out + (n.value,) if cap is not None else out

    def bakeAtlasPointsDevice(self, entries, width, height, points_ptr, texels_ptr, cap, count_ptr, t_max=1e30, pad_base=0,
                              atlas_uv_ptr=None, owner_ptr=None):
        """Enqueue the atlas point pass on device arrays, as bakePointsDevice; the entries are a host array, copied before the
        call returns.  owner_ptr: width * height uint64, (entry << 32) | triangle, all ones = uncovered."""
        d, rects = self._atlas_args(entries, width, height, t_max, pad_base)
        self._check(self.L.rt_bake_atlas_points_device(self.ctx, ctypes.addressof(d), _ptr(rects), ctypes.c_void_p(atlas_uv_ptr or 0),
                                                       ctypes.c_void_p(points_ptr or 0), ctypes.c_void_p(texels_ptr or 0), int(cap),
                                                       ctypes.c_void_p(count_ptr or 0), ctypes.c_void_p(owner_ptr or 0)),
                    "bakeAtlasPointsDevice")

    def bakeAtlasIrradiance(self, entries, width, height, max_depth, spp, seed=0, t_max=1e30, pad_base=0, atlas_uv=None,
                            stats=False, dilate=0, denoise=None):
        """The whole atlas bake: the points of all entries, ONE irradiance gather on them, scatter.  Returns the (height,
        width) IRRADIANCE_DTYPE atlas as bakeIrradiance does - and with stats=True the triple (atlas, number of covered
        texels, stats dict of the gather).  dilate > 0: dilateAtlas with that radius on the returned atlas, at the price of
        one more round trip of the atlas to the device and back.  denoise: None, or a dict of denoiseAtlas's keyword
        arguments: the bake then runs bakeAtlasPoints ONCE MORE with the same arguments - an extra point pass - for the
        guides and denoises the atlas with them, before any dilation."""
        d, rects = self._atlas_args(entries, width, height, t_max, pad_base)
        uv, uv_ptr, n_uv = self._atlas_uv(atlas_uv)
        out = np.empty((int(height), int(width)), dtype=IRRADIANCE_DTYPE)
        n = ctypes.c_uint32(0)
        st = RtRadianceStats()
        self._check(self.L.rt_bake_atlas_irradiance(self.ctx, ctypes.addressof(d), _ptr(rects), uv_ptr, n_uv, int(max_depth),
                                                    int(spp), int(seed) & 0xffffffff, _ptr(out), ctypes.addressof(n),
                                                    ctypes.addressof(st) if stats else None), "bakeAtlasIrradiance")
        if denoise is not None:
            points, texels = self.bakeAtlasPoints(entries, width, height, t_max, pad_base, atlas_uv)
            out = self.denoiseAtlas(out, points, texels, **denoise)
        if dilate > 0:
            out = self.dilateAtlas(out, dilate)
        return (out, n.value, st.as_dict()) if stats else out

    # ---- atlas dilation: the nearest covered texel into the uncovered ones around it (rt_dilate_atlas) ----
    @staticmethod
    def _dilate_desc(width, height, radius):
        d = RtDilateDesc()
        d.width, d.height, d.radius = int(width), int(height), int(radius)
        return d

    def dilateAtlas(self, atlas, radius, src=False, filled=False):
        """atlas: an (H, W, 4) float32 array (or an (H, W) IRRADIANCE_DTYPE one, as the bakes return it), covered where its
        fourth component is >= 0.  Returns a NEW array of the same shape in which every uncovered texel within `radius` (0
        .. 24) texels of a covered one holds the first three words of the nearest covered texel - the lowest texel index
        among equally near ones - and -2 as its fourth; by the dilation rule of include/mi355rt.h.  src=True adds the (H,
        W) uint32 source map (own index in covered texels, the source's in filled ones, 0xffffffff elsewhere), filled=True
        the number of filled texels: (atlas[, src][, filled])."""
        a = np.ascontiguousarray(atlas)
        if a.dtype == IRRADIANCE_DTYPE and a.ndim == 2:
            out = a.copy()
            height, width = a.shape
        else:
            out = np.array(a, dtype=np.float32, order="C")
            if out.ndim != 3 or out.shape[2] != 4:
                raise ValueError("dilateAtlas expects an (H, W, 4) float32 array")
            height, width = out.shape[:2]
        d = self._dilate_desc(width, height, radius)
        smap = np.empty((height, width), np.uint32) if src else None
        n = ctypes.c_uint32(0)
        self._check(self.L.rt_dilate_atlas(self.ctx, ctypes.addressof(d), _ptr(out) if out.size else None,
                                           _ptr(smap) if src else None, ctypes.addressof(n) if filled else None),
                    "dilateAtlas")
        res = (out,) + ((smap,) if src else ()) + ((n.value,) if filled else ())
        return res if len(res) > 1 else out

    def dilateAtlasDevice(self, atlas_ptr, width, height, radius, src_ptr=0, filled_ptr=0):
        """Enqueue a dilation, in place, of the width x height atlas of 16-byte texels at atlas_ptr (e.g. tensor.data_ptr())
        on the context's stream; no host synchronisation.  src_ptr: width * height uint32 for the source map, filled_ptr:
        one uint32 for the count, 0 = not wanted.  Every pointer must be 16-byte aligned and lie on the context's device."""
        d = self._dilate_desc(width, height, radius)
        self._check(self.L.rt_dilate_atlas_device(self.ctx, ctypes.addressof(d), ctypes.c_void_p(atlas_ptr or 0),
                                                  ctypes.c_void_p(src_ptr or 0), ctypes.c_void_p(filled_ptr or 0)),
                    "dilateAtlasDevice")

    # ---- atlas denoise: the edge-stopped a-trous filter guided by the bake's points (rt_denoise_atlas) ----
    @staticmethod
    def _denoise_desc(width, height, plane_eps, max_dist, normal_cos, passes, step):
        d = RtDenoiseDesc()
        d.width, d.height, d.step, d.passes = int(width), int(height), int(step), int(passes)
        d.normal_cos, d.plane_eps, d.max_dist = float(normal_cos), float(plane_eps), float(max_dist)
        return d

    def denoiseAtlas(self, atlas, points, texels, *, plane_eps, max_dist, normal_cos=0.9, passes=3, step=1):
        """atlas: an (H, W, 4) float32 array (or an (H, W) IRRADIANCE_DTYPE one, as the bakes return it); points (n, 8)
        float32 in the rt_gather_point layout and texels (n,) uint32, as bakePoints / bakeAtlasPoints return them for the
        same atlas.  Returns a NEW array of the same shape: `passes` passes of the 5 x 5 a-trous kernel at tap spacings step,
        2 * step, ... (at most 4), each tap accepted only where its guide's normal has a dot product >= normal_cos with the
        texel's, and its guide's position lies within plane_eps of the texel's tangent plane and within max_dist of its
        position (world units); by the denoise rule of include/mi355rt.h.  Texels without a guide are copied."""
        a = np.ascontiguousarray(atlas)
        if a.dtype == IRRADIANCE_DTYPE and a.ndim == 2:
            height, width = a.shape
        else:
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 3 or a.shape[2] != 4:
                raise ValueError("denoiseAtlas expects an (H, W, 4) float32 array")
            height, width = a.shape[:2]
        out = np.empty_like(a)
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 8)
        tex = np.ascontiguousarray(texels, dtype=np.uint32).reshape(-1)
        if len(pts) != len(tex):
            raise ValueError("denoiseAtlas expects one texel index per point")
        d = self._denoise_desc(width, height, plane_eps, max_dist, normal_cos, passes, step)
        self._check(self.L.rt_denoise_atlas(self.ctx, ctypes.addressof(d), _ptr(a) if a.size else None,
                                            _ptr(pts) if len(pts) else None, _ptr(tex) if len(tex) else None, len(tex),
                                            _ptr(out) if out.size else None), "denoiseAtlas")
        return out

    def denoiseAtlasDevice(self, in_ptr, points_ptr, texels_ptr, n, out_ptr, width, height, *, plane_eps, max_dist,
                           normal_cos=0.9, passes=3, step=1):
        """Enqueue a denoise of the width x height atlas of 16-byte texels at in_ptr into the one at out_ptr (another
        array; e.g. tensor.data_ptr()), guided by n rt_gather_point at points_ptr and n uint32 at texels_ptr as
        bakePointsDevice wrote them, on the context's stream; no host synchronisation.  Every pointer must be 16-byte aligned
        and lie on the context's device.  The input atlas is only read."""
        d = self._denoise_desc(width, height, plane_eps, max_dist, normal_cos, passes, step)
        self._check(self.L.rt_denoise_atlas_device(self.ctx, ctypes.addressof(d), ctypes.c_void_p(in_ptr or 0),
                                                   ctypes.c_void_p(points_ptr or 0), ctypes.c_void_p(texels_ptr or 0), int(n),
                                                   ctypes.c_void_p(out_ptr or 0)), "denoiseAtlasDevice")

    # ---- frame denoise: the G-buffer-guided a-trous filter of the frame of the last compute() (rt_denoise_frame) ----
    def denoiseFrame(self, desc):
        """The filtered frame as an (H, W, 4) float32 array in the accumulator's format (rgb = radiance, a = 1 where the
        accumulation weight was > 0): by the frame denoise rule of include/mi355rt.h, from the accumulation buffer and the
        G-buffer of the last compute().  desc: a frame_denoise_desc record or a dict of its keyword arguments.  Blocking."""
        d = _frame_denoise_record(desc)
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self.L.rt_denoise_frame(self.ctx, _ptr(d), _ptr(out), out.nbytes), "denoiseFrame")
        return out

    def denoiseFrameDevice(self, tensor, desc):
        """Enqueue the same filter into `tensor` - a contiguous float32 tensor of H * W * 4 elements on the context's device,
        or a device pointer - on the context's stream; no host synchronisation.  The tensor may afterwards be given to
        bindPresentSource."""
        d = _frame_denoise_record(desc)
        ptr = tensor
        if hasattr(tensor, "data_ptr"):
            if tensor.numel() * tensor.element_size() != self.width * self.height * 16 or not tensor.is_contiguous():
                raise ValueError("denoiseFrameDevice expects a contiguous tensor of H * W * 16 bytes")
            ptr = tensor.data_ptr()
        self._check(self.L.rt_denoise_frame_device(self.ctx, _ptr(d), ctypes.c_void_p(ptr or 0)), "denoiseFrameDevice")

    def setPresentDenoise(self, desc):
        """desc (a frame_denoise_desc record or a dict): from now on present() filters the frame into a buffer the context
        owns and the post pass reads that; None restores the plain path exactly."""
        if desc is None:
            self._check(self.L.rt_set_present_denoise(self.ctx, None), "setPresentDenoise")
            return
        d = _frame_denoise_record(desc)
        self._check(self.L.rt_set_present_denoise(self.ctx, _ptr(d)), "setPresentDenoise")

    def setFrameDenoiseForm(self, form):
        """"auto" / 0 (per spacing, what was measured faster), "lds" / 1 (the staged form: spacings 1 .. 4 only) or
        "direct" / 2 (taps through L1 / L2).  Same words either way."""
        f = FRAME_DENOISE_FORMS[form.lower()] if isinstance(form, str) else int(form)
        self._check(self.L.rt_set_frame_denoise_form(self.ctx, f), "setFrameDenoiseForm")

    def frameDenoiseStats(self):
        """Stream times of the last denoiseFrame* call or filtered present(): {prepare_ms, pass_ms [per pass], finish_ms,
        forms [per pass: "lds" / "direct"], cache_hit}.  Blocking."""
        r = RtFrameDenoiseReport()
        self._check(self.L.rt_frame_denoise_stats(self.ctx, ctypes.addressof(r)), "frameDenoiseStats")
        n = int(r.passes)
        return {"prepare_ms": float(r.prepare_ms), "pass_ms": [float(r.pass_ms[p]) for p in range(n)],
                "finish_ms": float(r.finish_ms), "forms": [("none", "lds", "direct")[r.form[p]] for p in range(n)],
                "cache_hit": bool(r.cache_hit), "temporal_ms": float(r.temporal_ms),
                "temporal": ("off", "ran", "reused")[r.temporal], "motion": bool(r.motion), "motion_ms": float(r.motion_ms)}

    def setFrameTemporal(self, desc):
        """desc (a frame_temporal_desc record or a dict): from now on denoiseFrame, denoiseFrameDevice and a filtered present()
        reproject and blend last frame's history ahead of the first pass; None restores the plain path.  Any call drops the
        history."""
        if desc is None:
            self._check(self.L.rt_set_frame_temporal(self.ctx, None), "setFrameTemporal")
            return
        d = _frame_temporal_record(desc)
        self._check(self.L.rt_set_frame_temporal(self.ctx, _ptr(d)), "setFrameTemporal")

    def setFrameMotionIds(self, ids):
        """Frame motion on the upload path: ids[p] is the stable id of the instance at position p of the instance array now
        uploaded - a permutation of 0 .. n - 1 (WorldBridge.instanceOrder).  Every upload of instances resets it to the
        identity; a device-resident world update supplies its own."""
        a = np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1)
        self._check(self.L.rt_set_frame_motion_ids(self.ctx, _ptr(a), a.size), "setFrameMotionIds")

    def readFrameMotion(self):
        """-> (H, W, 8) f32, the carry plane of the last run of the motion stage: {P'.xyz, bits(status)} {N'.xyz, bits(stable
        id)}, P' where the pixel's surface point was in the previous frame (frame_motion_pixels).  Blocking."""
        out = np.empty((self.height, self.width, 8), np.float32)
        self._check(self.L.rt_read_frame_motion(self.ctx, _ptr(out), self.width * self.height), "readFrameMotion")
        return out

    def resetFrameHistory(self):
        """Drop the temporal stage's history: the next frame is a first frame.  For a caller who swaps the whole scene."""
        self._check(self.L.rt_reset_frame_history(self.ctx), "resetFrameHistory")

    def readFrameHistory(self, frames_only=False):
        """-> (colour (H, W, 4) f32 {q.rgb, n}, moments (H, W, 2) f32, frames integrated since the last drop); with
        frames_only, that count alone.  Blocking; for tests and tools."""
        n = ctypes.c_uint32(0)
        if frames_only:
            self._check(self.L.rt_read_frame_history(self.ctx, None, None, 0, ctypes.addressof(n)), "readFrameHistory")
            return int(n.value)
        col = np.empty((self.height, self.width, 4), np.float32)
        mom = np.empty((self.height, self.width, 2), np.float32)
        self._check(self.L.rt_read_frame_history(self.ctx, _ptr(col), _ptr(mom), self.width * self.height,
                                                 ctypes.addressof(n)), "readFrameHistory")
        return col, mom, int(n.value)

    # ---- lightmaps: bake, filter, gutter fill and encode in one call, without leaving the device (rt_bake_atlas_lightmap) ----
    @staticmethod
    def _lightmap_desc(d, max_depth, spp, seed, denoise, dilate, fmt):
        """rt_lightmap_desc from an rt_bake_atlas_desc and the rest; denoise: None or denoiseAtlas's keyword arguments"""
        m = RtLightmapDesc()
        m.width, m.height, m.pad_base, m.t_max, m.n_entries = d.width, d.height, d.pad_base, d.t_max, d.n_entries
        m.max_depth, m.spp, m.seed = int(max_depth), int(spp), int(seed) & 0xffffffff
        if denoise is not None:
            kw = dict(normal_cos=0.9, passes=3, step=1)
            kw.update(denoise)
            unknown = set(kw) - {"plane_eps", "max_dist", "normal_cos", "passes", "step"}
            if unknown or "plane_eps" not in kw or "max_dist" not in kw:
                raise TypeError("denoise takes denoiseAtlas's keyword arguments, plane_eps and max_dist at least")
            m.passes, m.step = int(kw["passes"]), int(kw["step"])
            m.normal_cos, m.plane_eps, m.max_dist = float(kw["normal_cos"]), float(kw["plane_eps"]), float(kw["max_dist"])
        m.dilate_radius, m.format = int(dilate), fmt
        return m

    def bakeAtlasLightmap(self, entries, width, height, max_depth, spp, seed=0, t_max=1e30, pad_base=0, atlas_uv=None,
                          denoise=None, dilate=0, format="f32", stats=False):
        """The finished lightmap in one call: the atlas bake of bakeAtlasIrradiance, then - denoise: None or a dict of
        denoiseAtlas's keyword arguments - the filter on the guides the bake already holds on the device, then - dilate > 0
        - the gutter fill of that radius, then the encode, all on the device; one read of the point count and one copy back.
        With format "f32" the result is word for word bakeAtlasIrradiance(..., denoise=..., dilate=...), the (height, width)
        IRRADIANCE_DTYPE atlas; "f16" gives (height, width, 4) float16 {r, g, b, w}; "rgbe" (or "rgbe8") (height, width)
        uint32 Radiance pixels R | G << 8 | B << 16 | E << 24 (decode_rgbe, write_hdr), 0 where no surface is and nothing was
        filled.  stats=True: the tuple (atlas, covered texels, filled texels, stats dict of the gather)."""
        d, rects = self._atlas_args(entries, width, height, t_max, pad_base)
        fmt = _lightmap_format(format)
        m = self._lightmap_desc(d, max_depth, spp, seed, denoise, dilate, fmt)
        uv, uv_ptr, n_uv = self._atlas_uv(atlas_uv)
        out = _lightmap_array(int(height), int(width), fmt)
        n, filled = ctypes.c_uint32(0), ctypes.c_uint32(0)
        st = RtRadianceStats()
        self._check(self.L.rt_bake_atlas_lightmap(self.ctx, ctypes.addressof(m), _ptr(rects), uv_ptr, n_uv,
                                                  _ptr(out) if out.size else None, out.nbytes, ctypes.addressof(n),
                                                  ctypes.addressof(filled), ctypes.addressof(st) if stats else None),
                    "bakeAtlasLightmap")
        return (out, n.value, filled.value, st.as_dict()) if stats else out

    # ---- directional lightmaps: four SH layers per atlas (rt_bake_atlas_directional, rt_bake_atlas_directional_lightmap) ----
    def bakeAtlasDirectional(self, entries, width, height, max_depth, spp, seed=0, t_max=1e30, pad_base=0, atlas_uv=None,
                             stats=False):
        """The directional atlas bake: the points of all entries, ONE directional gather on them, scatter.  Returns (layers, n):
        layers is (4, height, width) IRRADIANCE_DTYPE - layer k of texel texels[j] holds gatherDirectional(points[j]).layer[k],
        {sh[k].rgb, hit_fraction}; uncovered texels are {0, 0, 0, -1} in all four - and n the number of covered texels; with
        stats=True the triple (layers, n, stats dict of the gather)."""
        d, rects = self._atlas_args(entries, width, height, t_max, pad_base)
        uv, uv_ptr, n_uv = self._atlas_uv(atlas_uv)
        out = np.empty((4, int(height), int(width)), dtype=IRRADIANCE_DTYPE)
        n = ctypes.c_uint32(0)
        st = RtRadianceStats()
        self._check(self.L.rt_bake_atlas_directional(self.ctx, ctypes.addressof(d), _ptr(rects), uv_ptr, n_uv, int(max_depth),
                                                     int(spp), int(seed) & 0xffffffff, _ptr(out), ctypes.addressof(n),
                                                     ctypes.addressof(st) if stats else None), "bakeAtlasDirectional")
        return (out, n.value, st.as_dict()) if stats else (out, n.value)

    def bakeAtlasDirectionalLightmap(self, entries, width, height, max_depth, spp, seed=0, t_max=1e30, pad_base=0, atlas_uv=None,
                                     denoise=None, dilate=0, format="f32", stats=False):
        """The finished directional lightmap in one call: bakeAtlasDirectional, then per layer - denoise: None or a dict of
        denoiseAtlas's keyword arguments - the filter on the guides the bake holds on the device, then - dilate > 0 - the
        gutter fill, then the encode; one read of the point count and one copy back.  format "f32" gives (4, height, width)
        IRRADIANCE_DTYPE, "f16" (4, height, width, 4) float16; "rgbe" is refused (band-1 coefficients are signed).  Returns
        (layers, covered texels, filled texels of a layer), with stats=True a fourth item, the stats dict of the gather."""
        d, rects = self._atlas_args(entries, width, height, t_max, pad_base)
        fmt = _lightmap_format(format)
        m = self._lightmap_desc(d, max_depth, spp, seed, denoise, dilate, fmt)
        uv, uv_ptr, n_uv = self._atlas_uv(atlas_uv)
        out = _lightmap_array(4 * int(height), int(width), fmt)
        out = out.reshape((4, int(height)) + out.shape[1:])
        n, filled = ctypes.c_uint32(0), ctypes.c_uint32(0)
        st = RtRadianceStats()
        self._check(self.L.rt_bake_atlas_directional_lightmap(self.ctx, ctypes.addressof(m), _ptr(rects), uv_ptr, n_uv,
                                                              _ptr(out) if out.size else None, out.nbytes, ctypes.addressof(n),
                                                              ctypes.addressof(filled), ctypes.addressof(st) if stats else None),
                    "bakeAtlasDirectionalLightmap")
        return (out, n.value, filled.value, st.as_dict()) if stats else (out, n.value, filled.value)

    def bakeLightmap(self, inst, width, height, max_depth, spp, seed=0, t_max=1e30, pad_base=0, atlas_uv=None, denoise=None,
                     dilate=0, format="f32", stats=False):
        """bakeAtlasLightmap for one instance over the whole atlas: the entry (inst, 0, 0, width, height), which by identity
        (A) of the atlas rule is the single-instance bake."""
        return self.bakeAtlasLightmap([(inst, 0, 0, width, height)], width, height, max_depth, spp, seed, t_max, pad_base,
                                      atlas_uv, denoise, dilate, format, stats)

    def bakeAtlasLightmapDevice(self, entries, width, height, out_ptr, out_bytes, max_depth, spp, seed=0, t_max=1e30,
                                pad_base=0, atlas_uv_ptr=None, denoise=None, dilate=0, format="f32", stats=False):
        """bakeAtlasLightmap into a device array of out_bytes bytes at out_ptr (e.g. tensor.data_ptr(); 16-byte aligned, on
        the context's device, at least width * height * {16, 8, 4} bytes), with the override UVs at atlas_uv_ptr or None.
        NOT enqueue-only: the call reads the point count once.  Returns (covered texels, filled texels), with stats=True
        (covered, filled, stats dict); both cost a fence at the end, which the C entry spares a caller who passes NULL."""
        d, rects = self._atlas_args(entries, width, height, t_max, pad_base)
        m = self._lightmap_desc(d, max_depth, spp, seed, denoise, dilate, _lightmap_format(format))
        n, filled = ctypes.c_uint32(0), ctypes.c_uint32(0)
        st = RtRadianceStats()
        self._check(self.L.rt_bake_atlas_lightmap_device(self.ctx, ctypes.addressof(m), _ptr(rects),
                                                         ctypes.c_void_p(atlas_uv_ptr or 0), ctypes.c_void_p(out_ptr or 0),
                                                         int(out_bytes), ctypes.addressof(n), ctypes.addressof(filled),
                                                         ctypes.addressof(st) if stats else None), "bakeAtlasLightmapDevice")
        return (n.value, filled.value, st.as_dict()) if stats else (n.value, filled.value)

    def encodeAtlas(self, atlas, format):
        """atlas: an (H, W, 4) float32 array (or an (H, W) IRRADIANCE_DTYPE one) -> a NEW array in the texel format "f32",
        "f16" or "rgbe", shaped as bakeAtlasLightmap returns it; by the encoding rule of include/mi355rt.h.  No scene is
        needed."""
        a = np.ascontiguousarray(atlas)
        if a.dtype == IRRADIANCE_DTYPE and a.ndim == 2:
            height, width = a.shape
        else:
            a = np.ascontiguousarray(a, dtype=np.float32)
            if a.ndim != 3 or a.shape[2] != 4:
                raise ValueError("encodeAtlas expects an (H, W, 4) float32 array")
            height, width = a.shape[:2]
        fmt = _lightmap_format(format)
        out = _lightmap_array(height, width, fmt)
        self._check(self.L.rt_encode_atlas(self.ctx, width, height, fmt, _ptr(a) if a.size else None,
                                           _ptr(out) if out.size else None, out.nbytes), "encodeAtlas")
        return out

    def encodeAtlasDevice(self, in_ptr, width, height, format, out_ptr, out_bytes):
        """Enqueue the encode of the width x height atlas of 16-byte texels at in_ptr into the out_bytes bytes at out_ptr
        (another array) on the context's stream; no host synchronisation.  Both pointers must be 16-byte aligned and lie on
        the context's device."""
        self._check(self.L.rt_encode_atlas_device(self.ctx, int(width), int(height), _lightmap_format(format),
                                                  ctypes.c_void_p(in_ptr or 0), ctypes.c_void_p(out_ptr or 0), int(out_bytes)),
                    "encodeAtlasDevice")

    # ---- the sharded image (rt_dist_*): this context as one rank of `world` ----
    def distInit(self, rank, world, stripe_rows=8, unique_id=None):
        """Become rank `rank` of `world`.  unique_id: the 128 bytes of dist_unique_id() (RCCL gather, gatherStripes());
        None: no communicator, the host moves the blocks (readBlock / writeBlock)."""
        if unique_id is not None:
            unique_id = bytes(unique_id)
            if len(unique_id) != 128:
                raise RendererError("distInit: the unique id must be 128 bytes")
        self._check(self.L.rt_dist_init(self.ctx, int(rank), int(world), int(stripe_rows), unique_id), "distInit")

    def distShutdown(self):
        self._check(self.L.rt_dist_shutdown(self.ctx), "distShutdown")

    def distBlockBytes(self):
        return int(self.L.rt_dist_block_bytes(self.ctx))

    def packStripes(self):
        self._check(self.L.rt_pack_stripes(self.ctx), "packStripes")

    def readBlock(self):
        """This rank's compact block as (max_rows, width, 4) float32 (blocking)."""
        out = np.empty((self.distBlockBytes() // (self.width * 16) if self.width else 0, self.width, 4), dtype=np.float32)
        self._check(self.L.rt_dist_read_block(self.ctx, _ptr(out), out.nbytes), "readBlock")
        return out

    def writeBlock(self, from_rank, block):
        """Rank 0: the block of rank `from_rank` (any array or bytes-like of distBlockBytes() bytes) into its receive slot."""
        a = np.ascontiguousarray(np.frombuffer(block, dtype=np.uint8) if isinstance(block, (bytes, bytearray, memoryview)) else block)
        self._check(self.L.rt_dist_write_block(self.ctx, int(from_rank), _ptr(a), a.nbytes), "writeBlock")

    def unpackStripes(self):
        self._check(self.L.rt_unpack_stripes(self.ctx), "unpackStripes")

    def gatherStripes(self):
        """pack -> RCCL gather to rank 0 -> unpack, enqueued on the context's stream (collective: every rank calls it)."""
        self._check(self.L.rt_gather_stripes(self.ctx), "gatherStripes")

    def readDisplay(self):
        """Rank 0: the assembled float4 image as (height, width, 4) float32 (blocking)."""
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self.L.rt_read_display(self.ctx, _ptr(out), out.nbytes), "readDisplay")
        return out

    def setKernelVariant(self, variant):
        """3 = auto (default: persistent kernel for LDS-resident scenes, wavefront form for larger ones), 2 = wavefront,
        1 = persistent waves + path regeneration, 0 = one pixel per lane megakernel; all bit-identical"""
        self._check(self.L.rt_set_kernel_variant(self.ctx, int(variant)), "setKernelVariant")

    def setLookaheadLimit(self, frames_left):
        """the run of consecutive frames ends in `frames_left` frames (this one included): trace no further ahead; 0 = unknown"""
        self._check(self.L.rt_set_lookahead_limit(self.ctx, int(frames_left)), "setLookaheadLimit")

    def setLookahead(self, max_frames):
        """speculative lookahead of the live loop (rt_set_lookahead): consecutive compute(f) calls are traced ahead as batches"""
        self._check(self.L.rt_set_lookahead(self.ctx, int(max_frames)), "setLookahead")

    def setWalk(self, walk):
        """traversal of the wavefront trace kernels: 1 = child-pair records (default), 0 = single nodes; bit-identical"""
        self._check(self.L.rt_set_walk(self.ctx, int(walk)), "setWalk")

    def setKernelTiming(self, enabled):
        self._check(self.L.rt_set_kernel_timing(self.ctx, 1 if enabled else 0), "setKernelTiming")

    def kernelTimeMs(self):
        pt, pv, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_uint32()
        self._check(self.L.rt_kernel_time_ms(self.ctx, ctypes.byref(pt), ctypes.byref(pv), ctypes.byref(n)),
                    "kernelTimeMs")
        return {"pathtrace_ms": pt.value, "primary_ms": pv.value, "launches": n.value}


def dist_unique_id():
    """ncclGetUniqueId through the library (rt_dist_unique_id): 128 bytes that rank 0 hands to every other rank."""
    L = load_library()
    out = ctypes.create_string_buffer(128)
    rc = L.rt_dist_unique_id(out)
    if rc < 0:
        msg = L.rt_last_error(None)
        raise RendererError("rt_dist_unique_id failed (%d): %s" % (rc, msg.decode() if msg else ""))
    return out.raw


TIMER_NAMES = ("primary", "pathtrace", "wf_shade", "wf_trace_shadow", "wf_trace_ext", "post")


def _kernel_times(self):
    """{timer: {"ms": sum of durations, "launches": n}} since the last read (rt_kernel_times)."""
    n = len(TIMER_NAMES)
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_uint32 * n)()
    self._check(self.L.rt_kernel_times(self.ctx, ms, cnt, n), "kernelTimes")
    return {TIMER_NAMES[k]: {"ms": ms[k], "launches": int(cnt[k])} for k in range(n)}


WebGPURenderer.kernelTimes = _kernel_times


def _declare_motion_ids(renderer, bridge):
    """after an upload of the bridge's instances: their stable ids, the TLAS builder's order, for frame motion - where both
    sides have them (the oracle binding and hand-made bridges do not)"""
    order = getattr(bridge, "instanceOrder", None)
    if order is not None and len(order) and hasattr(renderer, "setFrameMotionIds"):
        renderer.setFrameMotionIds(order)


def upload_scene(renderer, bridge, width, height):
    """The reference's scene-load sequence (src/main.ts:51-67,99-116): textures, geometry, BVH,
    topology, instances, lights, draw commands, uniforms, then resolution + reset.
    Works for any object with the WebGPURenderer method surface (the oracle binding too)."""
    renderer.loadTexturesFromWorld(bridge)
    renderer.updateCombinedGeometry(bridge.vertices, bridge.normals, bridge.uvs)
    renderer.updateCombinedBVH(bridge.tlas, bridge.blas)
    renderer.updateBuffer("topology", bridge.mesh_topology)
    renderer.updateBuffer("instance", bridge.instances)
    _declare_motion_ids(renderer, bridge)
    renderer.updateBuffer("lights", bridge.lights)
    renderer.updateBuffer("draw_commands", bridge.draw_commands)
    renderer.updateScreenSize(width, height)
    bridge.updateCamera(width, height)
    renderer.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount)
    renderer.recreateBindGroup()
    renderer.resetAccumulation()


def sync_world(renderer, bridge, width, height):
    """The per-frame scene sync of the live loop (src/main.ts:133-163): when the bridge has new data, re-upload BVH,
    instances, draw commands and — if the geometry changed — vertices, topology and lights; then camera uniforms,
    rebind if a buffer grew, reset the accumulation.  Returns True when something was uploaded."""
    if not bridge.hasNewData:
        return False
    rebind = False
    if getattr(bridge, "deviceResident", False):
        # update(t) ran inside the renderer (WorldBridge.setDeviceUpdater -> rt_world_update): every array is already
        # where the kernels read it; only the camera uniforms and the accumulation restart remain of main.ts:133-163
        bridge.hasNewGeometry = False
        bridge.updateCamera(width, height)
        renderer.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount)
        renderer.resetAccumulation()
        bridge.hasNewData = False
        return True
    rebind |= bool(renderer.updateCombinedBVH(bridge.tlas, bridge.blas))
    rebind |= bool(renderer.updateBuffer("instance", bridge.instances))
    _declare_motion_ids(renderer, bridge)
    rebind |= bool(renderer.updateBuffer("draw_commands", bridge.draw_commands))
    if bridge.hasNewGeometry:
        rebind |= bool(renderer.updateCombinedGeometry(bridge.vertices, bridge.normals, bridge.uvs))
        rebind |= bool(renderer.updateBuffer("topology", bridge.mesh_topology))
        rebind |= bool(renderer.updateBuffer("lights", bridge.lights))
        bridge.hasNewGeometry = False
    bridge.updateCamera(width, height)
    renderer.updateSceneUniforms(bridge.cameraData, 0, bridge.lightCount)
    if rebind:
        renderer.recreateBindGroup()
    renderer.resetAccumulation()
    bridge.hasNewData = False
    return True


class LiveLoop:
    """`renderFrame` of src/main.ts:119-181 without the browser: every `update_interval` frames the world advances to
    t = totalFrameCount / update_interval / 60 (animation + rebuild), the scene is re-synced, accumulation restarts;
    every call traces one frame and presents."""

    def __init__(self, renderer, bridge, width, height, update_interval=0, lookahead=32):
        self.renderer, self.bridge = renderer, bridge
        if lookahead > 1 and hasattr(renderer, "setLookahead"):
            renderer.setLookahead(lookahead)    # a still scene accumulates frame after frame: trace them ahead in batches
        self.width, self.height = width, height
        self.update_interval = int(update_interval)      # <= 0: the world is never advanced (main.ts:127)
        self.frameCount = 0
        self.totalFrameCount = 0

    def render_frame(self):
        if self.update_interval > 0 and self.frameCount >= self.update_interval:
            self.bridge.update(self.totalFrameCount / (self.update_interval or 1) / 60)
        if sync_world(self.renderer, self.bridge, self.width, self.height):
            self.frameCount = 0
        self.frameCount += 1
        self.totalFrameCount += 1
        if self.update_interval > 0 and hasattr(self.renderer, "setLookaheadLimit"):
            # the world moves again in update_interval - frameCount + 1 frames: nothing is traced ahead past that
            self.renderer.setLookaheadLimit(max(1, self.update_interval - self.frameCount + 1))
        self.renderer.compute(self.frameCount)
        self.renderer.present()
