"""The resource budget of every kernel of the library, as data: what the compiler's resource report for gfx950
(tests/kernel_report.py) may say about each.  tests/test_kernel_budgets.py holds the report to it and
tools/kernel_resources.py prints it beside the measured figures.  A new kernel gets a row in GROUPS or a pattern in
UNBUDGETED (or REFERENCES); the completeness test fails until it has one.

A name is the readable kernel name or an fnmatch pattern of a template family.  The limit kinds (KINDS, nothing else):
  vgprs_max, vgprs_eq, sgprs_max (TotalSGPRs)           registers
  vgpr_spill_max, sgpr_spill_max, scratch_max           spilled registers, scratch bytes per lane; 0 means none
  waves_min, waves_eq                                   waves per SIMD
  lds_eq, lds_max, lds_min_blocks_per_cu                static LDS bytes per workgroup; lds > 0 and 160 KiB // lds >= n
  no_dynamic_stack                                      nothing is called, everything is inlined
A row without limits of its own (the path queries) is held by TWINS alone; REFERENCES are the kernels TWINS measures
against, which have no budget.  Where a bound was tightened by several
changes in turn, the row carries the last, tightest one; `git log` and DESIGN.md have the others."""
import fnmatch

NO_SPILL = dict(vgpr_spill_max=0, scratch_max=0)
CLEAN = dict(NO_SPILL, sgpr_spill_max=0)
PRIMARY = dict(NO_SPILL, vgprs_max=64, waves_eq=8, no_dynamic_stack=True)
ONE_LEAF = "<false, true, true>"    # product build, records in LDS, one-leaf TLAS

# (why, limits, kernel names or patterns)
GROUPS = [
    # ------------------------------------------------------------------------------------------- the persistent path tracer
    ("DESIGN.md 4.1, profiles/r06_one_leaf_five_waves.txt, r11_tile_refill.txt: the headline kernel runs at RT_PT_ONE_INST_WAVES"
     " = 5 waves per SIMD, which leaves it 96 VGPRs; a spill there costs more than the fifth wave gains.  90 VGPRs is what the"
     " tile prepass left it at.",
     dict(NO_SPILL, vgprs_max=90, waves_min=5), ["rtk::k_pathtrace_persistent" + ONE_LEAF]),
    ("DESIGN.md 4.1, profiles/r11_tile_refill.txt: the counting build of the headline kernel keeps the 5 waves the compiler"
     " reports for it and stays out of scratch.",
     dict(scratch_max=0, vgprs_max=95, waves_min=5), ["rtk::k_pathtrace_persistent<true, true, true>"]),
    ("DESIGN.md 4.1, profiles/r07_one_leaf_six_waves.txt, r10_trip_surface_pass.txt: 512-thread workgroups at RT_PT_WIDE_WAVES = 6"
     " leave 80 VGPRs.  The generic form does not fit them: it spills 13 VGPRs for its materials and measures faster than"
     " the 5-wave form all the same.  28 B/lane is what one surface pass per trip left (the frame no longer lives across the"
     " walks); a change that brings spills back shows here.  No static LDS: the host launches wide and plain alike.",
     dict(vgprs_max=80, scratch_max=28, waves_min=6, lds_eq=0), ["rtk::k_pathtrace_persistent_wide" + ONE_LEAF]),
    ("DESIGN.md 4.1, profiles/r12_plain_materials.txt: without the GGX, dielectric, texture and emissive-length code that"
     " untextured Lambertian scenes never run, the wide form holds 80 VGPRs with no spill.  Shares the wide form's launch.",
     dict(NO_SPILL, vgprs_max=80, waves_min=6, lds_eq=0), ["rtk::k_pathtrace_persistent_plain" + ONE_LEAF]),
    ("DESIGN.md 4.1, profiles/r13_leaf_sweep.txt, r14_sweep_cold.txt: the leaf sweep with the node sweep as its cold path and no"
     " node walk inlined is exactly what the sweep alone was measured at.",
     dict(NO_SPILL, vgprs_eq=80, waves_eq=6, lds_eq=0, no_dynamic_stack=True), ["rtk::k_pathtrace_sweep_plain" + ONE_LEAF]),
    ("DESIGN.md 4.1, profiles/r14_sweep_cold.txt: spills for its materials as its node-walk twin does (13, 28 B); 19 VGPRs and"
     " 44 B/lane is its one-loop form (traverse_leaves<.., ONE_LOOP>), and a loop per record array spills 20, which is why it"
     " has one loop.",
     dict(vgprs_max=80, vgpr_spill_max=19, scratch_max=44, waves_min=6, lds_eq=0, no_dynamic_stack=True),
     ["rtk::k_pathtrace_sweep_wide" + ONE_LEAF]),
    # ---------------------------------------------------------------------------------------------------- primary visibility
    ("DESIGN.md 4.2, profiles/r15_primary_tiles.txt: bound by instruction issue at low throughput per SIMD, so it wants all eight"
     " waves: 64 VGPRs, and at most 96 SGPRs, more would cost the eighth wave whatever the VGPRs.  The tile loop keeps what"
     " it reads once per wave in scalar registers.",
     dict(PRIMARY, sgprs_max=96), ["rtk::k_primary_visibility_tiles<false>", "rtk::k_primary_visibility<false, true>"]),
    ("DESIGN.md 4.2: the global-memory form and the counting builds keep eight waves too.",
     PRIMARY, ["rtk::k_primary_visibility<false, false>", "rtk::k_primary_visibility<true, false>",
               "rtk::k_primary_visibility<true, true>", "rtk::k_primary_visibility_tiles<true>"]),
    # ------------------------------------------------------------------------------------------------------- queries, gathers
    ("DESIGN.md 4.1d, profiles/ray_query_rate.txt: no instantiation spills; TWINS holds each to the waves of the wavefront trace"
     " kernel of its form.",
     CLEAN, ["rtk::k_ray_query<*>"]),
    ("DESIGN.md 4.1e, 4.1f, profiles/radiance_query_rate.txt, irradiance_gather_rate.txt: one path-query loop under the launch"
     " bounds of k_pathtrace_persistent<D, L, false>; TWINS holds each to no more scratch, no more spills and no fewer waves"
     " than that kernel.  (The LDS forms sit at 122 - 128 of 128 VGPRs.)",
     {}, ["rtk::k_radiance_query<*>", "rtk::k_irradiance_gather<*>"]),
    # ------------------------------------------------------------------------------------------------------ lightmap pipeline
    ("DESIGN.md 4.1g, 4.1h, profiles/bake_rate.txt, atlas_bake_rate.txt: the point passes of the lightmap and atlas bakes.",
     NO_SPILL, ["rtk::k_bake_owner", "rtk::k_bake_count", "rtk::k_bake_emit", "rtk::k_bake_scatter", "rtk::k_atlas_items",
                "rtk::k_atlas_scan", "rtk::k_atlas_owner", "rtk::k_atlas_count", "rtk::k_atlas_emit", "rtk::k_atlas_scatter"]),
    ("DESIGN.md 4.7, profiles/build_scan_ab.txt: callers of the force-inlined block primitives of csrc/k_block_scan.hip.h; bloat"
     " would show here.  (k_scan_counts also runs between the count and emit passes of the bakes.)",
     NO_SPILL, ["rtk::k_treelet_count", "rtk::k_treelet_number", "rtk::k_treelet_pick<0>", "rtk::k_treelet_pick<1>",
                "rtk::k_pair_count", "rtk::k_pair_number", "rtk::k_scan_counts", "bvhb::k_scan_blocks", "bvhb::k_scan_top",
                "bvhb::k_scan_apply", "bvhb::k_big_plan", "wu::k_emissive_apply"]),
    ("DESIGN.md 4.1i, profiles/probe_gather_rate.txt; 4.1m, profiles/directional_gather_rate.txt: ray making and projection around"
     " k_radiance_query, which does the trace.",
     dict(NO_SPILL, lds_eq=0), ["rtk::k_probe_rays", "rtk::k_probe_project", "rtk::k_dir_rays", "rtk::k_dir_project",
                                "rtk::k_dir_scatter"]),
    ("DESIGN.md 4.1j, profiles/dilate_rate.txt.", dict(NO_SPILL, lds_eq=0), ["rtk::k_dilate_mask", "rtk::k_dilate_apply"]),
    ("DESIGN.md 4.1j: keeps its 64-row window and four wave counts in LDS.", NO_SPILL, ["rtk::k_dilate_source"]),
    ("DESIGN.md 4.1k, profiles/denoise_rate.txt.", dict(CLEAN, lds_eq=0), ["rtk::k_denoise_index"]),
    ("DESIGN.md 4.1k, profiles/denoise_rate.txt: eleven window planes in LDS, at most the figure of the section's resource table"
     " (DESIGN_FIGURES), three workgroups per CU.",
     dict(CLEAN, lds_min_blocks_per_cu=3), ["rtk::k_denoise_pass"]),
    ("DESIGN.md 4.1l, profiles/lightmap_rate.txt: a streaming kernel, one load and one store per texel.",
     dict(CLEAN, lds_eq=0, waves_min=8), ["rtk::k_encode_atlas"]),
    # ------------------------------------------------------------------------------------------------------- volumes, probes
    ("DESIGN.md 4.1n, profiles/volume_rate.txt; 4.1p, profiles/volume_visibility_rate.txt: the path work of a bake is the probe"
     " gather's, the ray work the ray query's.  The VGPR count of k_volume_sample_visible (eight lanes per point, the hot one)"
     " is recorded in 4.1p, not gated: IMPLIED_WAVES holds it to the waves that count implies.",
     dict(NO_SPILL, lds_eq=0), ["rtk::k_volume_probes", "rtk::k_volume_finish", "rtk::k_volume_sample", "rtk::k_volume_layers",
                                "rtk::k_visibility_rays", "rtk::k_visibility_texels", "rtk::k_visibility_tiles",
                                "rtk::k_volume_sample_visible"]),
    ("DESIGN.md 4.1o, profiles/reflection_rate.txt: the path work of a capture is the radiance query's.",
     dict(CLEAN, lds_eq=0), ["rtk::k_reflection_rays", "rtk::k_reflection_texels", "rtk::k_reflection_copy"]),
    ("DESIGN.md 4.1o: 4, 16 and 64 samples per lane; each build keeps the waves its register arrays were sized for.",
     dict(CLEAN, lds_eq=0, waves_min=8), ["rtk::k_reflection_filter<4>"]),
    ("DESIGN.md 4.1o: as k_reflection_filter<4>.", dict(CLEAN, lds_eq=0, waves_min=4), ["rtk::k_reflection_filter<16>"]),
    ("DESIGN.md 4.1o: as k_reflection_filter<4>.", dict(CLEAN, lds_eq=0, waves_min=2), ["rtk::k_reflection_filter<64>"]),
    # -------------------------------------------------------------------------------------------------------- frame denoiser
    ("DESIGN.md 4.3b, profiles/frame_denoise_rate.txt.",
     dict(CLEAN, lds_eq=0), ["rtk::k_frame_prepare", "rtk::k_frame_pass_direct", "rtk::k_frame_finish"]),
    ("DESIGN.md 4.3b: the staged pass; its LDS is the window of ITS spacing (DESIGN_FIGURES), two workgroups per CU at the"
     " largest.",
     dict(CLEAN, lds_min_blocks_per_cu=2), ["rtk::k_frame_pass_lds<*>"]),
    ("DESIGN.md 4.3c, profiles/frame_temporal_rate.txt: 79 VGPRs, measured before the body became a template and unchanged by"
     " the motion flag; at least four waves per SIMD.",
     dict(CLEAN, lds_eq=0, vgprs_eq=79), ["rtk::k_frame_temporal"]),
    ("DESIGN.md 4.3d, profiles/frame_motion_rate.txt: the register counts are those of the section's resource table"
     " (DESIGN_FIGURES); 128 VGPRs is four waves per SIMD.",
     dict(CLEAN, lds_eq=0, vgprs_max=128), ["rtk::k_frame_motion", "rtk::k_frame_motion_scatter", "rtk::k_frame_temporal_motion"]),
]

# pattern -> why: kernels without a budget of their own that TWINS measures others against
REFERENCES = {
    "rtk::k_pathtrace_persistent<*, false>": "the persistent kernel without the one-leaf form; the path queries share its launch bounds",
    "rtk::k_wf_trace<*, 256, *>": "the wavefront trace kernel in 256-thread workgroups, the form of the ray queries",
    "rtk::k_wf_trace_pairs<*, 256>": "the wavefront pair-walk trace kernel in 256-thread workgroups, the form of the ray queries",
}

# (why there is no budget, kernel names or patterns).  No kernel that a row or a relation names may match one of these.
_UNBUDGETED = [
    ("variant 0, one thread per pixel: the reference form, not the product path", ["rtk::k_pathtrace<*>"]),
    ("wavefront shade; the time of the wavefront form is in its trace kernels (DESIGN.md 4.1b)", ["rtk::k_wf_shade<*>"]),
    ("the 256-thread trace kernels, which TWINS reads, at the other workgroup sizes of launch_plan.h trace_shape",
     ["rtk::k_wf_trace<*, 512, *>", "rtk::k_wf_trace<*, 1024, *>", "rtk::k_wf_trace_pairs<*, 512>", "rtk::k_wf_trace_pairs<*, 1024>"]),
    ("diagnostic: runs in tests/test_gpu_ieee.py only", ["rtk::k_ieee_check<*>"]),
    ("tests/test_native_gather_abi.py holds them on a compile of csrc/k_stripes.hip.h alone",
     ["rtk::k_pack_stripes", "rtk::k_unpack_stripes"]),
    ("once per frame, streaming; k_postprocess is sized by its 14.5 KB of LDS (DESIGN.md 4.3)",
     ["rtk::k_postprocess", "rtk::k_accumulate_frames"]),
    ("upload time, once per scene or texture (DESIGN.md 3, 4.5)",
     ["rtk::k_prepare_*", "rtk::k_validate_scene", "rtk::k_resize_texture"]),
    ("pair-layout and treelet-order builds at upload time (DESIGN.md 4.1c); the callers of the block primitives among them"
     " have rows",
     ["rtk::k_pair_emit", "rtk::k_pair_parent", "rtk::k_pair_roots", "rtk::k_treelet_hist<*>", "rtk::k_treelet_inst_roots",
      "rtk::k_treelet_iota", "rtk::k_treelet_remap", "rtk::k_treelet_weight"]),
    ("BLAS builder, timed as a whole by tools/blas_build_time.py (DESIGN.md 4.7); its callers of the block primitives have rows",
     ["bvhb::k_level<*>", "bvhb::k_emit", "bvhb::k_tri_boxes", "bvhb::k_big_bin", "bvhb::k_big_bounds", "bvhb::k_big_copy",
      "bvhb::k_big_count", "bvhb::k_big_scan", "bvhb::k_big_scatter", "bvhb::k_big_setup", "bvhb::k_big_split", "bvhb::k_big_swap"]),
    ("device world update, timed as a whole by tools/animate_bench.py (DESIGN.md 4.7b)",
     ["wu::k_build_stats", "wu::k_lights", "wu::k_skin", "wu::k_static_nodes", "wu::k_tlas", "wu::k_tlas_small", "wu::k_topology"]),
]
UNBUDGETED = {name: why for why, names in _UNBUDGETED for name in names}

_BOOLS = ("false", "true")
_PAIRS = [(a, b) for a in _BOOLS for b in _BOOLS]
# family pattern -> exactly these instantiations exist
FAMILIES = {
    "rtk::k_ray_query<*>": ["rtk::k_ray_query<%s, %s, %d>" % (a, d, f) for a, d in _PAIRS for f in range(5)],
    "rtk::k_irradiance_gather<*>": ["rtk::k_irradiance_gather<%s, %s>" % p for p in _PAIRS],
    "rtk::k_radiance_query<*>": ["rtk::k_radiance_query<%s, %s>" % p for p in _PAIRS],
    "rtk::k_primary_visibility<*>": ["rtk::k_primary_visibility<%s, %s>" % p for p in _PAIRS],
    "rtk::k_primary_visibility_tiles<*>": ["rtk::k_primary_visibility_tiles<%s>" % d for d in _BOOLS],
    "rtk::k_reflection_filter<*>": ["rtk::k_reflection_filter<%d>" % n for n in (4, 16, 64)],
    "rtk::k_frame_pass_lds<*>": ["rtk::k_frame_pass_lds<%d>" % s for s in (1, 2, 3, 4)],
    "rtk::k_pathtrace_persistent_wide<*>": ["rtk::k_pathtrace_persistent_wide" + ONE_LEAF],
    "rtk::k_pathtrace_persistent_plain<*>": ["rtk::k_pathtrace_persistent_plain" + ONE_LEAF],
    "rtk::k_pathtrace_sweep_wide<*>": ["rtk::k_pathtrace_sweep_wide" + ONE_LEAF],
    "rtk::k_pathtrace_sweep_plain<*>": ["rtk::k_pathtrace_sweep_plain" + ONE_LEAF],
}

# k_ray_query's FORM -> the wavefront kernel of the same form: (pairs, LDS, RAYREG)
_RQ_FORMS = {0: (False, True, False), 1: (False, False, False), 2: (False, False, True), 3: (True, True, False), 4: (True, False, False)}


def _wf_twin(a, d, form):
    pairs, lds, rayreg = _RQ_FORMS[form]
    if pairs:
        return "rtk::k_wf_trace_pairs<%s, %s, %s, 256>" % (a, d, _BOOLS[lds])
    return "rtk::k_wf_trace<%s, %s, %s, 256, %s>" % (a, d, _BOOLS[lds], _BOOLS[rayreg])


# (kernel, its twin in the same report, kinds compared): the kernel is no worse than the twin in each
TWINS = ([("rtk::%s<%s, %s>" % (k, d, l), "rtk::k_pathtrace_persistent<%s, %s, false>" % (d, l), ("scratch", "vgpr_spill", "waves"))
          for k in ("k_irradiance_gather", "k_radiance_query") for d, l in _PAIRS] +
         [("rtk::k_ray_query<%s, %s, %d>" % (a, d, f), _wf_twin(a, d, f), ("waves",)) for a, d in _PAIRS for f in sorted(_RQ_FORMS)])

# (kernel, report field, relation to the figure, regex of the figure's row in DESIGN.md, the section the row is looked for in)
DESIGN_FIGURES = (
    [("rtk::k_frame_pass_lds<%d>" % s, "lds", "eq", r"^\| `k_frame_pass_lds<%d>` \|.*?\| (\d+) B \|" % s, None) for s in (1, 2, 3, 4)] +
    [("rtk::k_denoise_pass", "lds", "max", r"^\| `k_denoise_pass` \|.*?\| (\d+) B \|", None),
     ("rtk::k_frame_temporal", "vgprs", "eq", r"^\| `k_frame_temporal` \| (\d+) \|", None)] +
    [("rtk::" + k, "vgprs", "eq", r"^\| `%s` \| (\d+) \|" % k, "4.3d")
     for k in ("k_frame_motion", "k_frame_motion_scatter", "k_frame_temporal_motion")])

# kernels whose waves per SIMD equal what their registers imply (512 per lane and SIMD, allocated in steps of 8, at most 8
# waves): nothing else, an LDS allocation or a launch bound, holds them lower
IMPLIED_WAVES = ["rtk::k_volume_sample_visible"]

FIELDS = {"vgprs": "VGPRs", "sgprs": "TotalSGPRs", "vgpr_spill": "VGPRs Spill", "sgpr_spill": "SGPRs Spill",
          "scratch": "ScratchSize [bytes/lane]", "waves": "Occupancy [waves/SIMD]", "lds": "LDS Size [bytes/block]"}
KINDS = ("vgprs_max", "vgprs_eq", "sgprs_max", "vgpr_spill_max", "sgpr_spill_max", "scratch_max", "waves_min", "waves_eq",
         "lds_eq", "lds_max", "lds_min_blocks_per_cu", "no_dynamic_stack")
LDS_PER_CU = 160 * 1024

ROWS = {name: dict(limits, why=why) for why, limits, names in GROUPS for name in names}
assert len(ROWS) == sum(len(names) for _, _, names in GROUPS), "a kernel has two rows"


def matching(name, patterns):
    return [p for p in patterns if fnmatch.fnmatchcase(name, p)]


def violations(limits, entry):
    """What of `limits` (kind -> bound) the report entry breaks, as strings; an unknown kind is an error."""
    out = []
    for kind, bound in limits.items():
        if kind == "why":
            continue
        if kind not in KINDS:
            raise KeyError("unknown limit kind %r" % kind)
        if kind == "no_dynamic_stack":
            got, ok = entry["Dynamic Stack"], entry["Dynamic Stack"] == "False"
        elif kind == "lds_min_blocks_per_cu":
            got = entry[FIELDS["lds"]]
            ok = got > 0 and LDS_PER_CU // got >= bound
        else:
            field, op = kind.rsplit("_", 1)
            got = entry[FIELDS[field]]
            ok = got <= bound if op == "max" else got >= bound if op == "min" else got == bound
        if not ok:
            out.append("%s %s: measured %s" % (kind, bound, got))
    return out
