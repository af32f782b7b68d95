"""ctypes binding of librestir_hip.so (include/restir_hip.h) plus thin Python mirrors of the
reference's host objects (Scene / GBuffer / ReSTIR module state / LeveledEAWFilter).

This is plumbing for tests and bench.py; the product is the shared library.  There is NO fallback:
if the library is missing or no MI355X is visible, calls raise.
"""
import ctypes as C
import os

import numpy as np

from .ctypes_structs import Camera, Material, Reservoir, MATERIAL_DTYPE, RESERVOIR_DTYPE, INDIRECT_RESERVOIR_DTYPE, LIGHT_SAMPLE_DTYPE, copy_camera
from .ctypes_structs import DIRTY_BOXES_KEPT, DIRTY_BOX_DTYPE  # noqa: F401
from .ctypes_structs import GeometryEditLights, GeometryEditPlan, GeometryEditView
from .ctypes_structs import STREAM_CHOICES_KEPT, StreamChoice, StreamChoiceInputs, StreamChoicePlan, StreamChoices

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RESTIR_HIP_LIB") or os.path.join(_HERE, "librestir_hip.so")   # env override: A/B builds


class RestirHipError(RuntimeError):
    pass


RS_ERR_INVALID_ARGUMENT, RS_ERR_UNSUPPORTED = 10001, 10002
RS_GI_SPATIAL_MAX_TAPS, RS_GI_SPATIAL_DIM, RS_GI_SPATIAL_JACOBIAN_MAX = 16, 150, 10.0      # rs_restir_set_indirect_spatial

# rs_transport (include/restir_hip.h): the exchange of the strip driver as callbacks
TRANSPORT_GROUP = C.CFUNCTYPE(C.c_int, C.c_void_p)
TRANSPORT_SEND = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)
TRANSPORT_RECV = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p)


class Transport(C.Structure):
    _fields_ = [("ctx", C.c_void_p), ("group_begin", TRANSPORT_GROUP), ("send", TRANSPORT_SEND), ("recv", TRANSPORT_RECV),
                ("group_end", TRANSPORT_GROUP), ("stream_ordered", C.c_int)]


class SceneDesc(C.Structure):
    _fields_ = [
        ("numPrims", C.c_int),
        ("vertices", C.c_void_p),
        ("normals", C.c_void_p),
        ("texcoords", C.c_void_p),
        ("materialIds", C.c_void_p),
        ("numMaterials", C.c_int),
        ("materials", C.c_void_p),
        ("bvhSize", C.c_int),
        ("boundingBoxes", C.c_void_p),
        ("bvhNodes", C.c_void_p * 6),
        ("numLights", C.c_int),
        ("lightPrimIds", C.c_void_p),
        ("lightUnitRadiance", C.c_void_p),
        ("lightProb", C.c_void_p),
        ("lightFailId", C.c_void_p),
        ("sumLightPower", C.c_float),
        ("numTextures", C.c_int),
        ("textures", C.c_void_p),
        ("envMapTexId", C.c_int),
        ("envMapProb", C.c_void_p),
        ("envMapFailId", C.c_void_p),
    ]


class Texture(C.Structure):
    _fields_ = [("width", C.c_int), ("height", C.c_int), ("data", C.c_void_p)]


class SceneFileView(C.Structure):
    _fields_ = [
        ("numPrims", C.c_int),
        ("vertices", C.c_void_p),
        ("normals", C.c_void_p),
        ("texcoords", C.c_void_p),
        ("materialIds", C.c_void_p),
        ("numMaterials", C.c_int),
        ("materials", C.c_void_p),
        ("numTextures", C.c_int),
        ("textures", C.c_void_p),
        ("envMapTexId", C.c_int),
        ("camera", Camera),
        ("iterations", C.c_int),
        ("traceDepth", C.c_int),
        ("imageName", C.c_char_p),
        ("numSkippedObjects", C.c_int),
    ]


class SVGFView(C.Structure):
    _fields_ = [
        ("devAccumColor", C.c_void_p * 2),
        ("devAccumMoment", C.c_void_p * 2),
        ("devVariance", C.c_void_p),
        ("frameIdx", C.c_int),
        ("width", C.c_int),
        ("height", C.c_int),
    ]


class GBufferView(C.Structure):
    _fields_ = [
        ("devAlbedo", C.c_void_p),
        ("devMotion", C.c_void_p),
        ("devNormal", C.c_void_p * 2),
        ("devPrimId", C.c_void_p * 2),
        ("devDepth", C.c_void_p * 2),
        ("frameIdx", C.c_int),
        ("width", C.c_int),
        ("height", C.c_int),
    ]


class PhaseAInputs(C.Structure):
    """rs_phase_a_inputs (include/restir_hip.h): what a phase-A call of ReSTIRDirect decides from."""
    _fields_ = [(n, C.c_int) for n in (
        "async_", "chainStreams", "smallChains", "shadowOnMain", "fuseMode", "denoiseStream", "chainsInFlight", "reusedThree", "phaseACalls",
        "width", "y0", "y1", "deferredValid", "deferredMatches", "deferredY0", "deferredY1", "reusedFrame", "tuneChoice", "tuneFrame",
        "chain", "smallChain", "idle", "numLights", "envMap", "risGlobalBelow", "cutState")]


class PhaseAPlan(C.Structure):
    """rs_phase_a_plan (include/restir_hip.h): what it decides."""
    _fields_ = [(n, C.c_int) for n in (
        "fuse", "tuneCounted", "tuneRestart", "stream", "lastChains", "splitSlot", "splitCall", "splitMode", "shadowOnLibrary", "risForm",
        "tilesX", "tilesY", "fusedTilesY", "cut")]


RIS_GLOBAL, RIS_LDS, RIS_ALIAS_LDS = 0, 1, 2


class PrimaryCutKey(C.Structure):
    """rs_primary_cut_key (include/restir_hip.h): what a slot's cuts and leaf lists were built from."""
    _fields_ = [("sceneId", C.c_ulonglong), ("geomEdits", C.c_ulonglong), ("cam", Camera), ("y0", C.c_int), ("y1", C.c_int),
                ("cap", C.c_uint), ("listCap", C.c_uint)]


class PrimaryCutSlot(C.Structure):
    """rs_primary_cut_slot: the stored key and what became of the two arenas under it (CUT_ARENA_*)."""
    _fields_ = [("keyValid", C.c_int), ("cuts", C.c_int), ("lists", C.c_int), ("key", PrimaryCutKey)]


class PrimaryCutSizes(C.Structure):
    """rs_primary_cut_sizes: the arenas of one launch geometry."""
    _fields_ = [("numCells", C.c_int), ("capacity", C.c_uint), ("numTiles", C.c_int), ("listCapacity", C.c_uint)]


CUT_ARENA_NOTHING, CUT_ARENA_NO_MEMORY, CUT_ARENA_BUILT = 0, 1, 2
STREAMS_HELD_NONE, STREAMS_HELD_MEASURED, STREAMS_HELD_PLAIN = 0, 1, 2
STREAMS_PENDING_NONE, STREAMS_PENDING_AGAIN, STREAMS_PENDING_AGAIN_FORGET = 0, 1, 2


# every symbol include/restir_hip.h declares; tests check that the library exports all of them
EXPORTS = [
    "rs_last_error", "rs_context_create", "rs_context_destroy", "rs_context_set_current", "rs_init", "rs_set_stream", "rs_set_sync", "rs_set_side_stream", "rs_set_ris_table_pixels", "rs_set_internal_stream_priority", "rs_internal_streams_info", "rs_choose_internal_streams_again", "rs_prepare_streams", "rs_set_stream_plan", "rs_set_denoise_stream", "rs_join_denoise_stream", "rs_set_tile_split", "rs_debug_split_tiles", "rs_synchronize",
    "rs_build_bvh", "rs_build_light_table", "rs_build_alias_table", "rs_build_envmap_pdf", "rs_scene_build", "rs_scene_build_textured", "rs_scene_create",
    "rs_scene_host_desc", "rs_scene_set_sample_sequence", "rs_scene_set_emission", "rs_scene_set_materials", "rs_scene_set_texture", "rs_scene_set_triangles", "rs_scene_set_geometry", "rs_scene_set_motion_tracking", "rs_scene_advance_motion", "rs_scene_download_prev_vertices", "rs_refit_boxes", "rs_debug_scene_table", "rs_debug_scene_grid", "rs_debug_scene_emissive_grid", "rs_debug_grid_box", "rs_scene_destroy", "rs_camera_update", "rs_trace_closest", "rs_trace_closest_wave", "rs_scene_set_ordered_tree", "rs_ordered_bvh_host_check", "rs_trace_occlusion",
    "rs_gbuffer_create", "rs_gbuffer_destroy", "rs_gbuffer_render", "rs_gbuffer_render_rows", "rs_gbuffer_update",
    "rs_gbuffer_get_view", "rs_gbuffer_set_reuse", "rs_gbuffer_reuse_stats", "rs_gbuffer_invalidate", "rs_gbuffer_rows_bytes", "rs_gbuffer_rows_pack", "rs_gbuffer_rows_unpack", "rs_restir_init", "rs_restir_free", "rs_restir_reset", "rs_restir_direct",
    "rs_restir_phase_a", "rs_restir_phase_b", "rs_restir_end_frame", "rs_restir_launch_choice", "rs_restir_halo_bytes", "rs_restir_halo_pack",
    "rs_restir_halo_unpack", "rs_restir_rows_bytes", "rs_restir_rows_pack", "rs_restir_rows_unpack", "rs_restir_download", "rs_restir_upload", "rs_restir_set_light_tracking", "rs_restir_download_light_ids", "rs_restir_set_light_retargeting", "rs_restir_get_light_retargeting", "rs_restir_download_light_samples", "rs_debug_restir_retarget", "rs_debug_restir_retarget_launched", "rs_debug_restir_surface_wo", "rs_scene_light_moves", "rs_restir_set_shadow_revalidation", "rs_restir_get_shadow_revalidation", "rs_scene_geometry_edits", "rs_scene_dirty_boxes", "rs_debug_restir_revalidate", "rs_debug_restir_revalidate_launched", "rs_debug_plan_dirty_box", "rs_debug_plan_revalidation", "rs_debug_segment_in_boxes", "rs_restir_set_indirect_revalidation", "rs_restir_get_indirect_revalidation", "rs_debug_restir_indirect_revalidate", "rs_debug_restir_indirect_revalidate_launched", "rs_debug_indirect_candidate_classes", "rs_restir_light_rows_bytes", "rs_restir_light_rows_pack", "rs_restir_light_rows_unpack", "rs_restir_ray_count", "rs_restir_ray_total", "rs_restir_pass_times",
    "rs_restir_enable_timing", "rs_restir_spatial_times", "rs_restir_set_probe", "rs_restir_last_launch", "rs_debug_phase_a_plan", "rs_restir_set_primary_cuts", "rs_debug_set_primary_cut_cap", "rs_debug_primary_cut_info", "rs_debug_primary_cut_missing", "rs_restir_set_primary_leaf_lists", "rs_debug_set_primary_leaf_list_cap", "rs_debug_primary_leaf_list_info", "rs_debug_primary_leaf_list_missing", "rs_debug_plan_primary_leaf_list", "rs_debug_plan_primary_cut", "rs_debug_plan_primary_cut_slot", "rs_restir_set_shadow_regroup", "rs_debug_plan_shadow_regroup", "rs_debug_shadow_pass", "rs_debug_plan_stream_choice", "rs_debug_plan_stream_switch", "rs_debug_restir_surface", "rs_pbo_register", "rs_pbo_map", "rs_pbo_unmap", "rs_pbo_unregister", "rs_save_image", "rs_save_image_jpg", "rs_write_png", "rs_write_jpg", "rs_debug_tap_estimate_error", "rs_debug_sqrt_of_uniform_mismatches", "rs_debug_sqrt_of_unit_floats_mismatches", "rs_debug_exact_ops_mismatches", "rs_debug_rng_step_mismatches", "rs_debug_rng_step_host_mismatches", "rs_debug_surface_ops", "rs_debug_div_sigma_mismatches", "rs_path_trace_init", "rs_path_trace_free", "rs_path_trace_direct",
    "rs_path_trace", "rs_path_trace_indirect", "rs_restir_indirect", "rs_restir_download_indirect",
    "rs_restir_set_indirect_spatial", "rs_restir_get_indirect_spatial", "rs_restir_download_indirect_spatial", "rs_debug_restir_indirect_spatial", "rs_debug_restir_indirect_spatial_launched", "rs_debug_restir_indirect_primary", "rs_debug_seeded_uniforms",
    "rs_svgf_create", "rs_svgf_destroy", "rs_svgf_filter", "rs_svgf_next_frame", "rs_svgf_get_view",
    "rs_copy_image_to_pbo", "rs_copy_image2_to_pbo", "rs_copy_imagef_to_pbo", "rs_copy_imagei_to_pbo", "rs_eaw_create", "rs_eaw_destroy", "rs_eaw_set_params", "rs_eaw_get_params", "rs_eaw_set_tiled", "rs_eaw_set_fused", "rs_svgf_set_params", "rs_svgf_get_params", "rs_svgf_set_tiled", "rs_svgf_set_fused", "rs_eaw_filter", "rs_eaw_positions_rows", "rs_eaw_level_rows", "rs_modulate_albedo",
    "rs_add_image", "rs_add_image3", "rs_comm_create_rccl", "rs_comm_create_rccl_lib", "rs_comm_create", "rs_comm_destroy", "rs_comm_self_exchange", "rs_strips_create", "rs_strips_destroy", "rs_strips_rows", "rs_strips_set_comm_stream", "rs_strips_set_gbuffer_halo", "rs_strips_set_light_tracking", "rs_strips_frame", "rs_strips_eaw_filter", "rs_strips_svgf_filter", "rs_strips_exchange_svgf_history", "rs_strips_exchange_history", "rs_strips_gather", "rs_strips_gather_begin", "rs_strips_gather_end", "rs_strips_enable_timing", "rs_strips_halo_wait_ms",
    "rs_scene_file_load", "rs_scene_file_get", "rs_scene_file_free", "rs_build_transformation_matrix", "rs_bake_instance",
    "rs_bake_matrix", "rs_scene_file_objects", "rs_scene_define_parts", "rs_scene_set_part_transforms", "rs_scene_parts_info", "rs_scene_download_part_rest", "rs_debug_scene_staged_bytes", "rs_debug_plan_geometry_edit",
    "rs_scene_set_partial_refit", "rs_scene_get_partial_refit", "rs_scene_refit_counts", "rs_debug_scene_refit_dirty", "rs_debug_plan_refit",
    "rs_skin_corners", "rs_scene_define_skin", "rs_scene_set_bone_transforms", "rs_scene_skin_info", "rs_scene_download_skin",
    "rs_morph_corners", "rs_scene_define_morph", "rs_scene_define_skin_morph", "rs_scene_set_morph_weights", "rs_scene_set_skin_pose", "rs_scene_morph_info", "rs_scene_download_morph",
]

_lib = None


def lib():
    """Load librestir_hip.so.  Raises if it has not been built (python __graft_entry__.py build)."""
    global _lib
    if _lib is not None:
        return _lib
    try:
        # PyTorch bundles its own HIP/HSA runtime; it has to be the first one loaded in the process,
        # otherwise two runtimes race for the device and hipGetDeviceCount reports none.
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise RestirHipError(
            f"{LIB_PATH} is missing: build it with `make -C restir_amd/csrc` (or __graft_entry__.build()). "
            "There is no CPU fallback for the MI355X path.")
    L = C.CDLL(LIB_PATH)
    vp, ci, cf = C.c_void_p, C.c_int, C.c_float
    L.rs_last_error.restype = C.c_char_p
    L.rs_init.argtypes = [ci]
    L.rs_context_create.argtypes = [ci, C.POINTER(vp)]
    L.rs_context_destroy.argtypes = [vp]
    L.rs_context_set_current.argtypes = [vp]
    L.rs_set_stream.argtypes = [vp]
    L.rs_set_sync.argtypes = [ci]
    L.rs_debug_split_tiles.argtypes = [vp, vp, C.POINTER(C.c_uint), C.POINTER(C.c_uint)]
    L.rs_set_side_stream.argtypes = [ci]
    L.rs_set_ris_table_pixels.argtypes = [ci]
    L.rs_build_bvh.argtypes = [ci, vp, vp, C.POINTER(vp * 6), C.POINTER(ci)]
    L.rs_build_light_table.argtypes = [ci, vp, vp, ci, vp, C.POINTER(ci), vp, vp, vp]
    L.rs_build_alias_table.argtypes = [ci, vp, vp, vp, C.POINTER(cf)]
    L.rs_scene_build.argtypes = [ci, vp, vp, vp, vp, ci, vp, C.POINTER(vp)]
    L.rs_scene_build_textured.argtypes = [ci, vp, vp, vp, vp, ci, vp, ci, vp, ci, C.POINTER(vp)]
    L.rs_build_envmap_pdf.argtypes = [ci, ci, vp, vp]
    L.rs_scene_create.argtypes = [C.POINTER(SceneDesc), C.POINTER(vp)]
    L.rs_scene_file_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.rs_scene_file_get.argtypes = [vp, C.POINTER(SceneFileView)]
    L.rs_scene_file_free.argtypes = [vp]
    L.rs_build_transformation_matrix.argtypes = [vp, vp, vp, vp]
    L.rs_bake_instance.argtypes = [vp, vp, vp, ci, vp, vp, vp, vp]
    L.rs_bake_matrix.argtypes = [vp, ci, vp, vp, vp, vp]
    L.rs_scene_file_objects.argtypes = [vp, C.POINTER(ci), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.rs_scene_define_parts.argtypes = [vp, ci, vp, vp, vp, vp]
    L.rs_scene_set_part_transforms.argtypes = [vp, ci, vp, vp]
    L.rs_scene_parts_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    L.rs_scene_download_part_rest.argtypes = [vp, vp, vp, vp]
    L.rs_debug_scene_staged_bytes.argtypes = [vp, C.POINTER(C.c_size_t)]
    if hasattr(L, "rs_skin_corners"):                     # (an A/B build from before skinned meshes, RESTIR_HIP_LIB)
        L.rs_skin_corners.argtypes = [ci, vp, C.c_size_t, vp, vp, vp, vp, vp, vp]
        L.rs_scene_define_skin.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp]
        L.rs_scene_set_bone_transforms.argtypes = [vp, ci, vp, vp]
        L.rs_scene_skin_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
        L.rs_scene_download_skin.argtypes = [vp, vp, vp, vp, vp, vp]
    if hasattr(L, "rs_morph_corners"):                    # (an A/B build from before morph targets, RESTIR_HIP_LIB)
        L.rs_morph_corners.argtypes = [ci, vp, vp, vp, vp, vp, C.c_size_t, vp, vp, vp, vp]
        L.rs_scene_define_morph.argtypes = [vp, ci, ci, vp, vp, vp, vp, vp, vp, vp]
        L.rs_scene_define_skin_morph.argtypes = [vp, ci, vp, vp, vp, vp]
        L.rs_scene_set_morph_weights.argtypes = [vp, ci, vp, vp]
        L.rs_scene_set_skin_pose.argtypes = [vp, ci, vp, vp, ci, vp, vp]
        L.rs_scene_morph_info.argtypes = [vp, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci)]
        L.rs_scene_download_morph.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.rs_scene_host_desc.argtypes = [vp, C.POINTER(SceneDesc)]
    L.rs_scene_destroy.argtypes = [vp]
    L.rs_scene_set_emission.argtypes = [vp, ci, vp, vp]
    L.rs_scene_set_materials.argtypes = [vp, ci, vp, vp]
    L.rs_scene_set_texture.argtypes = [vp, ci, ci, ci, vp]
    L.rs_scene_set_triangles.argtypes = [vp, ci, vp, vp, vp]
    L.rs_scene_set_geometry.argtypes = [vp, ci, vp, vp, vp]
    L.rs_scene_set_motion_tracking.argtypes = [vp, ci]
    L.rs_scene_advance_motion.argtypes = [vp]
    L.rs_scene_download_prev_vertices.argtypes = [vp, vp]
    L.rs_debug_scene_emissive_grid.argtypes = [vp, vp, vp, C.POINTER(C.c_double), C.POINTER(ci), C.POINTER(ci)]
    L.rs_refit_boxes.argtypes = [ci, vp, ci, vp, vp]
    L.rs_debug_scene_table.argtypes = [vp, ci, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.rs_debug_scene_grid.argtypes = [vp, vp, vp, C.POINTER(C.c_double), vp, vp, C.POINTER(ci), C.POINTER(ci)]
    L.rs_debug_grid_box.argtypes = [vp, vp, vp, vp, C.c_double, vp, C.POINTER(ci)]
    L.rs_restir_set_light_tracking.argtypes = [vp, ci]
    L.rs_restir_download_light_ids.argtypes = [vp, ci, vp]
    if hasattr(L, "rs_restir_set_light_retargeting"):     # (an A/B build from before retargeting, RESTIR_HIP_LIB: tools/bench_light_retarget.py)
        L.rs_restir_set_light_retargeting.argtypes = [vp, ci]
        L.rs_restir_get_light_retargeting.argtypes = [vp, C.POINTER(ci)]
        L.rs_restir_download_light_samples.argtypes = [vp, ci, vp]
        L.rs_debug_restir_retarget.argtypes = [vp, C.POINTER(C.c_ulonglong * 3)]
        L.rs_debug_restir_retarget_launched.argtypes = [vp, C.POINTER(ci)]
        L.rs_debug_restir_surface_wo.argtypes = [vp, vp]
        L.rs_scene_light_moves.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    if hasattr(L, "rs_restir_set_shadow_revalidation"):   # (an A/B build from before shadow revalidation, RESTIR_HIP_LIB: tools/bench_shadow_revalidate.py)
        ull = C.c_ulonglong
        L.rs_restir_set_shadow_revalidation.argtypes = [vp, ci]
        L.rs_restir_get_shadow_revalidation.argtypes = [vp, C.POINTER(ci)]
        L.rs_scene_geometry_edits.argtypes = [vp, C.POINTER(ull)]
        L.rs_scene_dirty_boxes.argtypes = [vp, ull, ci, vp, C.POINTER(ci), C.POINTER(ci)]
        L.rs_debug_restir_revalidate.argtypes = [vp, C.POINTER(ull * 3)]
        L.rs_debug_restir_revalidate_launched.argtypes = [vp, C.POINTER(ci)]
        L.rs_debug_plan_dirty_box.argtypes = [ci, vp, ci, vp, vp, vp, vp]
        L.rs_debug_plan_revalidation.argtypes = [ci, ull, vp, ull, ull, ci, C.POINTER(ci), C.POINTER(ci), C.POINTER(ci), vp]
        L.rs_debug_segment_in_boxes.argtypes = [ci, vp, ci, vp, ci, vp]
    if hasattr(L, "rs_restir_set_indirect_revalidation"):   # (an A/B build from before indirect revalidation, RESTIR_HIP_LIB: tools/bench_indirect_revalidate.py)
        L.rs_restir_set_indirect_revalidation.argtypes = [vp, ci]
        L.rs_restir_get_indirect_revalidation.argtypes = [vp, C.POINTER(ci)]
        L.rs_debug_restir_indirect_revalidate.argtypes = [vp, C.POINTER(C.c_ulonglong * 4)]
        L.rs_debug_restir_indirect_revalidate_launched.argtypes = [vp, C.POINTER(ci)]
        L.rs_debug_indirect_candidate_classes.argtypes = [ci, vp, ci, vp, ci, vp]
    if hasattr(L, "rs_restir_set_indirect_spatial"):        # (an A/B build from before GI's spatial pass, RESTIR_HIP_LIB: tools/bench_indirect_spatial.py)
        L.rs_restir_set_indirect_spatial.argtypes = [vp, ci, ci, C.c_float]
        L.rs_restir_get_indirect_spatial.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_float)]
        L.rs_restir_download_indirect_spatial.argtypes = [vp, vp]
        L.rs_debug_restir_indirect_spatial.argtypes = [vp, C.POINTER(C.c_ulonglong * 8)]
        L.rs_debug_restir_indirect_spatial_launched.argtypes = [vp, C.POINTER(ci)]
        L.rs_debug_restir_indirect_primary.argtypes = [vp, vp, vp, vp, vp]
        L.rs_debug_seeded_uniforms.argtypes = [vp, ci, ci, ci, ci, vp]
    L.rs_restir_light_rows_bytes.argtypes = [vp, ci]
    L.rs_restir_light_rows_bytes.restype = C.c_size_t
    L.rs_restir_light_rows_pack.argtypes = [vp, ci, ci, ci, vp]
    L.rs_restir_light_rows_unpack.argtypes = [vp, ci, ci, ci, vp]
    L.rs_camera_update.argtypes = [C.POINTER(Camera)]
    L.rs_trace_closest.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.rs_trace_occlusion.argtypes = [vp, ci, vp, vp]
    L.rs_trace_closest_wave.argtypes = [vp, ci, vp, vp, vp, vp, vp]
    L.rs_scene_set_ordered_tree.argtypes = [vp, ci, vp]
    L.rs_gbuffer_create.argtypes = [ci, ci, C.POINTER(vp)]
    L.rs_gbuffer_destroy.argtypes = [vp]
    L.rs_gbuffer_render.argtypes = [vp, vp, C.POINTER(Camera)]
    L.rs_gbuffer_render_rows.argtypes = [vp, vp, C.POINTER(Camera), ci, ci]
    L.rs_gbuffer_update.argtypes = [vp, C.POINTER(Camera)]
    L.rs_gbuffer_get_view.argtypes = [vp, C.POINTER(GBufferView)]
    L.rs_gbuffer_set_reuse.argtypes = [vp, ci]
    L.rs_gbuffer_reuse_stats.argtypes = [vp, C.POINTER(C.c_ulonglong), C.POINTER(C.c_ulonglong)]
    L.rs_gbuffer_invalidate.argtypes = [vp]
    L.rs_restir_init.argtypes = [ci, ci, C.POINTER(vp)]
    L.rs_restir_free.argtypes = [vp]
    L.rs_restir_reset.argtypes = [vp]
    L.rs_restir_direct.argtypes = [vp, vp, C.POINTER(Camera), vp, vp, ci, ci, ci]
    L.rs_restir_phase_a.argtypes = [vp, vp, C.POINTER(Camera), vp, ci, ci, ci, ci]
    L.rs_restir_phase_b.argtypes = [vp, vp, C.POINTER(Camera), vp, vp, ci, ci, ci, ci]
    L.rs_restir_end_frame.argtypes = [vp]
    L.rs_restir_launch_choice.argtypes = [vp, C.POINTER(ci)]
    L.rs_restir_halo_bytes.argtypes = [vp, ci]
    L.rs_restir_halo_bytes.restype = C.c_size_t
    L.rs_restir_halo_pack.argtypes = [vp, ci, ci, vp]
    L.rs_restir_halo_unpack.argtypes = [vp, ci, ci, vp]
    L.rs_restir_rows_bytes.argtypes = [vp, ci, ci]
    L.rs_restir_rows_bytes.restype = C.c_size_t
    L.rs_debug_tap_estimate_error.argtypes = [ci, C.POINTER(cf)]
    L.rs_restir_last_launch.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    L.rs_debug_phase_a_plan.argtypes = [C.POINTER(PhaseAInputs), C.POINTER(PhaseAPlan)]
    L.rs_debug_plan_geometry_edit.argtypes = [C.POINTER(GeometryEditView), C.c_char_p, ci, ci, vp, vp, vp, ci, C.POINTER(GeometryEditPlan), vp,
                                              C.POINTER(GeometryEditLights), vp, vp, vp]
    if hasattr(L, "rs_scene_set_partial_refit"):          # (an A/B build from before the partial refit, RESTIR_HIP_LIB: tools/bench_partial_refit.py)
        ull = C.c_ulonglong
        L.rs_scene_set_partial_refit.argtypes = [vp, ci, ci]
        L.rs_scene_get_partial_refit.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
        L.rs_scene_refit_counts.argtypes = [vp, C.POINTER(ull), C.POINTER(ull)]
        L.rs_debug_scene_refit_dirty.argtypes = [vp, C.POINTER(ull)]
        L.rs_debug_plan_refit.argtypes = [ci, ci, ci, ci, ci, vp, ull, ull, C.POINTER(ci), C.POINTER(ull)]
    L.rs_restir_set_primary_cuts.argtypes = [vp, ci]
    L.rs_debug_set_primary_cut_cap.argtypes = [vp, ci]
    L.rs_debug_primary_cut_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_ulonglong), C.POINTER(ci), C.POINTER(C.c_ulonglong)]
    L.rs_debug_primary_cut_missing.argtypes = [vp, vp, ci, ci, vp, C.POINTER(C.c_ulonglong * 4)]
    L.rs_restir_set_primary_leaf_lists.argtypes = [vp, ci]
    L.rs_debug_set_primary_leaf_list_cap.argtypes = [vp, ci]
    L.rs_debug_primary_leaf_list_info.argtypes = [vp, C.POINTER(ci), C.POINTER(ci), C.POINTER(C.c_ulonglong), C.POINTER(ci), C.POINTER(C.c_ulonglong)]
    L.rs_debug_primary_leaf_list_missing.argtypes = [vp, vp, ci, vp, C.POINTER(C.c_ulonglong * 4)]
    L.rs_debug_plan_primary_leaf_list.argtypes = [vp, ci, ci, ci, vp, C.POINTER(vp * 6), ci, C.POINTER(ci), C.POINTER(ci), vp]
    L.rs_debug_plan_primary_cut.argtypes = [vp, ci, ci, ci, ci, ci, vp, C.POINTER(vp * 6), ci, C.POINTER(ci), C.POINTER(ci), vp, vp]
    L.rs_debug_plan_primary_cut_slot.argtypes = [ci, ci, C.POINTER(PrimaryCutSlot), C.POINTER(PrimaryCutKey), ci, ci, C.POINTER(ci), C.POINTER(PrimaryCutSizes)]
    if hasattr(L, "rs_restir_set_shadow_regroup"):        # (an A/B build from before the regrouped shadow rays, RESTIR_HIP_LIB: tools/ab.sh)
        L.rs_restir_set_shadow_regroup.argtypes = [vp, ci]
        L.rs_debug_plan_shadow_regroup.argtypes = [ci, vp, vp, C.c_float, vp, vp, vp, vp, C.POINTER(ci), C.POINTER(C.c_float)]
        L.rs_debug_shadow_pass.argtypes = [vp, vp, ci, ci, vp, vp, vp, vp, C.POINTER(C.c_float)]
    L.rs_debug_plan_stream_choice.argtypes = [C.POINTER(StreamChoiceInputs), C.POINTER(StreamChoicePlan)]
    L.rs_debug_plan_stream_switch.argtypes = [C.POINTER(StreamChoices), ci, vp, ci, C.POINTER(StreamChoice), C.POINTER(ci)]
    L.rs_debug_restir_surface.argtypes = [vp, vp, vp, vp]
    L.rs_pbo_register.argtypes = [C.c_uint, C.POINTER(vp)]
    L.rs_pbo_map.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_size_t)]
    L.rs_pbo_unmap.argtypes = [vp]
    L.rs_pbo_unregister.argtypes = [vp]
    L.rs_save_image.argtypes = [C.c_char_p, vp, ci, ci, ci]
    L.rs_write_png.argtypes = [C.c_char_p, vp, ci, ci]
    L.rs_write_jpg.argtypes = [C.c_char_p, vp, ci, ci]
    L.rs_svgf_set_tiled.argtypes = [vp, ci]
    L.rs_svgf_set_fused.argtypes = [vp, ci]
    L.rs_save_image_jpg.argtypes = [C.c_char_p, vp, ci, ci, ci]
    L.rs_debug_sqrt_of_uniform_mismatches.argtypes = [C.POINTER(C.c_ulonglong)]
    L.rs_debug_sqrt_of_unit_floats_mismatches.argtypes = [C.POINTER(C.c_ulonglong)]
    L.rs_debug_exact_ops_mismatches.argtypes = [ci, C.c_uint, C.c_uint, ci, ci, C.POINTER(C.c_ulonglong)]
    L.rs_debug_div_sigma_mismatches.argtypes = [C.c_float, C.POINTER(C.c_ulonglong)]
    L.rs_debug_rng_step_mismatches.argtypes = [C.POINTER(C.c_ulonglong * 2)]
    L.rs_debug_rng_step_host_mismatches.argtypes = [C.c_uint, C.c_uint, C.POINTER(C.c_ulonglong * 2)]
    L.rs_debug_surface_ops.argtypes = [ci, ci, vp, vp, ci, ci, vp]
    L.rs_scene_set_sample_sequence.argtypes = [vp, vp, ci, ci]
    L.rs_set_stream_plan.argtypes = [ci, ci, ci]
    L.rs_set_denoise_stream.argtypes = [ci]
    L.rs_join_denoise_stream.argtypes = []
    L.rs_restir_rows_pack.argtypes = [vp, ci, ci, ci, vp]
    L.rs_restir_rows_unpack.argtypes = [vp, ci, ci, ci, vp]
    L.rs_gbuffer_rows_bytes.argtypes = [vp, ci]
    L.rs_gbuffer_rows_bytes.restype = C.c_size_t
    L.rs_gbuffer_rows_pack.argtypes = [vp, ci, ci, ci, vp]
    L.rs_gbuffer_rows_unpack.argtypes = [vp, ci, ci, ci, vp]
    L.rs_restir_download.argtypes = [vp, ci, vp]
    L.rs_restir_upload.argtypes = [vp, ci, vp]
    L.rs_restir_ray_count.argtypes = [vp, C.POINTER(C.c_ulonglong)]
    L.rs_restir_ray_total.argtypes = [vp, ci, C.POINTER(C.c_ulonglong)]
    L.rs_restir_pass_times.argtypes = [vp, C.POINTER(cf * 4)]
    L.rs_restir_enable_timing.argtypes = [vp, ci]
    L.rs_restir_spatial_times.argtypes = [vp, C.POINTER(cf), ci, C.POINTER(ci)]
    L.rs_restir_set_probe.argtypes = [vp, ci]
    L.rs_path_trace_direct.argtypes = [vp, C.POINTER(Camera), vp, ci, ci, C.POINTER(C.c_ulonglong)]
    L.rs_path_trace.argtypes = [vp, C.POINTER(Camera), vp, vp, ci, ci, ci, C.POINTER(C.c_ulonglong)]
    L.rs_path_trace_indirect.argtypes = [vp, C.POINTER(Camera), vp, ci, ci, ci, C.POINTER(C.c_ulonglong)]
    L.rs_restir_indirect.argtypes = [vp, vp, C.POINTER(Camera), vp, vp, ci, ci, ci, ci, C.POINTER(C.c_ulonglong)]
    L.rs_restir_download_indirect.argtypes = [vp, ci, vp]
    L.rs_svgf_create.argtypes = [ci, ci, ci, C.POINTER(vp)]
    L.rs_svgf_destroy.argtypes = [vp]
    L.rs_svgf_filter.argtypes = [vp, C.POINTER(vp), vp, vp, C.POINTER(Camera)]
    L.rs_svgf_next_frame.argtypes = [vp]
    L.rs_svgf_get_view.argtypes = [vp, C.POINTER(SVGFView)]
    L.rs_copy_image_to_pbo.argtypes = [vp, vp, ci, ci, ci, cf]
    for name in ("rs_copy_image2_to_pbo", "rs_copy_imagef_to_pbo", "rs_copy_imagei_to_pbo"):
        getattr(L, name).argtypes = [vp, vp, ci, ci]
    L.rs_comm_create_rccl.argtypes = [vp, ci, ci, C.POINTER(vp)]
    L.rs_comm_create.argtypes = [C.POINTER(Transport), ci, ci, C.POINTER(vp)]
    L.rs_comm_destroy.argtypes = [vp]
    L.rs_strips_create.argtypes = [vp, ci, ci, C.POINTER(ci), C.POINTER(vp)]
    L.rs_strips_destroy.argtypes = [vp]
    L.rs_strips_rows.argtypes = [vp, C.POINTER(ci), C.POINTER(ci)]
    L.rs_strips_set_comm_stream.argtypes = [vp, ci]
    L.rs_strips_set_gbuffer_halo.argtypes = [vp, ci]
    L.rs_strips_set_light_tracking.argtypes = [vp, ci]
    L.rs_strips_frame.argtypes = [vp, vp, vp, C.POINTER(Camera), vp, vp, ci, ci, ci]
    L.rs_strips_eaw_filter.argtypes = [vp, vp, vp, C.POINTER(Camera), vp, C.POINTER(vp)]
    L.rs_strips_exchange_history.argtypes = [vp, vp, vp]
    L.rs_strips_svgf_filter.argtypes = [vp, vp, vp, C.POINTER(Camera), vp, C.POINTER(vp)]
    L.rs_strips_exchange_svgf_history.argtypes = [vp, vp]
    L.rs_strips_gather.argtypes = [vp, vp, C.c_size_t, ci]
    L.rs_strips_gather_begin.argtypes = [vp, vp, C.c_size_t, ci, ci]
    L.rs_strips_gather_end.argtypes = [vp, ci]
    L.rs_strips_enable_timing.argtypes = [vp, ci]
    L.rs_strips_halo_wait_ms.argtypes = [vp, C.POINTER(C.c_float)]
    L.rs_comm_create_rccl_lib.argtypes = [vp, ci, ci, C.c_char_p, C.POINTER(vp)]
    L.rs_eaw_create.argtypes = [ci, ci, ci, C.POINTER(vp)]
    for name in ("rs_eaw_set_params", "rs_svgf_set_params"):
        getattr(L, name).argtypes = [vp, C.c_float, C.c_float, C.c_float, ci]
    for name in ("rs_eaw_get_params", "rs_svgf_get_params"):
        getattr(L, name).argtypes = [vp, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(ci)]
    L.rs_eaw_set_tiled.argtypes = [vp, ci]
    L.rs_eaw_set_fused.argtypes = [vp, ci]
    L.rs_eaw_destroy.argtypes = [vp]
    L.rs_eaw_filter.argtypes = [vp, C.POINTER(vp), vp, vp, C.POINTER(Camera)]
    L.rs_eaw_positions_rows.argtypes = [vp, vp, C.POINTER(Camera), ci, ci]
    L.rs_eaw_level_rows.argtypes = [vp, vp, vp, vp, ci, ci, ci]
    L.rs_modulate_albedo.argtypes = [vp, vp]
    L.rs_add_image.argtypes = [vp, vp, ci, ci]
    L.rs_add_image3.argtypes = [vp, vp, vp, ci, ci]
    _lib = L
    return L


def check(code):
    if code != 0:
        raise RestirHipError(f"librestir_hip error {code}: {lib().rs_last_error().decode()}")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def init(device=0):
    check(lib().rs_init(device))


class Context:
    """rs_context: device, stream, launch mode and internal streams of the objects created while it is current (per thread)."""

    def __init__(self, device=0):
        self.handle = C.c_void_p()
        check(lib().rs_context_create(device, C.byref(self.handle)))

    def make_current(self):
        check(lib().rs_context_set_current(self.handle))

    @staticmethod
    def use_default():
        check(lib().rs_context_set_current(None))

    def destroy(self):
        if self.handle:
            lib().rs_context_destroy(self.handle)
            self.handle = C.c_void_p()


def set_sync(sync):
    check(lib().rs_set_sync(1 if sync else 0))


def set_stream(hip_stream):
    """The stream the library enqueues on (rs_set_stream); 0 / None = the legacy default stream."""
    check(lib().rs_set_stream(C.c_void_p(int(hip_stream or 0))))


def set_side_stream(enable):
    """Overlapped frames when launches are asynchronous (include/restir_hip.h): 0 off, 1 on with GBuffer::render as its own launch,
    2 / 3 on with the render deferred into ReSTIRDirect's primary-ray launch (3: at any size), 4 on with that choice measured."""
    check(lib().rs_set_side_stream(int(enable)))


def set_internal_stream_priority(level):
    """-1 high / 0 normal / 1 low / 2 automatic: the level of the library's own streams (before the first frame)."""
    check(lib().rs_set_internal_stream_priority(int(level)))


def internal_streams_info():
    """(level, calibration us of the chosen streams, fastest candidate us) of the library's own streams; (level, 0, 0): plain streams."""
    p, a, b = C.c_int(0), C.c_double(0), C.c_double(0)
    check(lib().rs_internal_streams_info(C.byref(p), C.byref(a), C.byref(b)))
    return p.value, a.value, b.value


def choose_internal_streams_again():
    check(lib().rs_choose_internal_streams_again())


def set_ris_table_pixels(pixels):
    """Launches of fewer pixels read the RIS light table from global memory instead of LDS (rs_set_ris_table_pixels); 0 = always LDS."""
    check(lib().rs_set_ris_table_pixels(int(pixels)))


def phase_a_plan(**inputs):
    """The plan of a phase-A call for these inputs (rs_debug_phase_a_plan; fields of PhaseAInputs, the rest 0): needs no device."""
    i, o = PhaseAInputs(**inputs), PhaseAPlan()
    check(lib().rs_debug_phase_a_plan(C.byref(i), C.byref(o)))
    return o


def geometry_edit_view(material_ids, materials, vertices, grid=None, light_prim_ids=(), light_radiance=(), light_area=(), env_power=None,
                       emi_leaf_prims=None):
    """rs_geometry_edit_view of plain arrays: grid = (lo, hi) of a bounded scene or None; env_power: the environment map's sampler entry
    or None for a scene without one; emi_leaf_prims: the emissive tree's primitives by slot, or None for a scene without that tree."""
    keep = dict(materialIds=np.ascontiguousarray(material_ids, np.int32), materials=np.ascontiguousarray(materials, MATERIAL_DTYPE),
                vertices=np.ascontiguousarray(vertices, np.float32).reshape(-1), lightPrimIds=np.ascontiguousarray(light_prim_ids, np.int32),
                lightRadiance=np.ascontiguousarray(light_radiance, np.float32).reshape(-1), lightArea=np.ascontiguousarray(light_area, np.float32),
                emiLeafPrims=np.ascontiguousarray(() if emi_leaf_prims is None else emi_leaf_prims, np.int32))
    v = GeometryEditView(**{k: a.ctypes.data for k, a in keep.items()})
    v.keep = keep                                    # (the view points into these arrays)
    v.numPrims = len(keep["materialIds"])
    v.bounded = int(grid is not None)
    if grid is not None:
        v.gridLo[:], v.gridHi[:] = [float(x) for x in grid[0]], [float(x) for x in grid[1]]
    v.numLightPrims = len(keep["lightPrimIds"])
    v.numLights = v.numLightPrims + int(env_power is not None)
    v.envPower = 0.0 if env_power is None else float(env_power)
    v.emissiveTree, v.numEmissive = int(emi_leaf_prims is not None), len(keep["emiLeafPrims"])
    return v


def plan_geometry_edit(view, name, emitters, prim_ids, vertices, normals=None, num_part_recs=0, count=None):
    """The plans of a geometry edit made through the entry point `name` (rs_debug_plan_geometry_edit): needs no device.  Returns
    (GeometryEditPlan, slots, lights): slots [count] the place of every record among the m staged; lights None unless the edit names an
    emitter, else a dict of the fields of GeometryEditLights and area, prob, fail.  A refusal raises as the entry point's would."""
    ids = np.ascontiguousarray(prim_ids, np.int32)
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1)
    n = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1)
    count = len(ids) if count is None else count
    plan, lights, slots = GeometryEditPlan(), GeometryEditLights(), np.full(max(count, 0), -1, np.int32)
    area, prob, fail = np.zeros(view.numLightPrims, np.float32), np.zeros(view.numLights, np.float32), np.zeros(view.numLights, np.int32)
    check(lib().rs_debug_plan_geometry_edit(C.byref(view), name.encode(), int(emitters), count, _p(ids), _p(v), None if n is None else _p(n),
                                            num_part_recs, C.byref(plan), _p(slots), C.byref(lights), _p(area), _p(prob), _p(fail)))
    if not plan.lamps:
        return plan, slots, None
    out = dict(sumAll=np.float32(lights.sumAll), emiGrid=lights.emiGrid, emiMargin=lights.emiMargin, area=area, prob=prob, fail=fail)
    for k in ("emiLo", "emiHi", "emiBase", "emiScale"):
        out[k] = np.array(getattr(lights, k)[:], np.float32)
    return plan, slots, out


def plan_refit(on, max_triangles, keys_valid, m, tree_depths, num_nodes=0, capacity=0xfffffffe):
    """rs_debug_plan_refit: whether an edit of m distinct triangles is partial, and its bound on dirty nodes; needs no device.
    tree_depths: the deepest leaf of every tree (the root at 0).  Returns (partial, bound)."""
    d = np.ascontiguousarray(tree_depths, np.int32).reshape(-1)
    partial, bound = C.c_int(-1), C.c_ulonglong(0)
    check(lib().rs_debug_plan_refit(int(on), int(max_triangles), int(keys_valid), int(m), int(d.size), _p(d), int(num_nodes), int(capacity),
                                    C.byref(partial), C.byref(bound)))
    return bool(partial.value), int(bound.value)


def prepare_streams():
    """Choose the library's own streams now rather than inside the first overlapped frame (rs_prepare_streams)."""
    check(lib().rs_prepare_streams())


def set_stream_plan(chain_streams=-1, small_chains=-1, shadow_on_main=-1):
    """How the overlapped mode spreads a frame's kernels over the internal streams (rs_set_stream_plan); -1 keeps a value."""
    check(lib().rs_set_stream_plan(int(chain_streams), int(small_chains), int(shadow_on_main)))


def set_denoise_stream(enable):
    """LeveledEAWFilter and the tone map of its result on a stream of the library, next to the next frame's passes (rs_set_denoise_stream);
    their outputs are then ordered by events: join_denoise_stream() or synchronize() before reading them outside the library."""
    check(lib().rs_set_denoise_stream(int(enable)))


def join_denoise_stream():
    """The library stream waits (on the device) for everything enqueued on the denoise stream so far (rs_join_denoise_stream)."""
    check(lib().rs_join_denoise_stream())


def set_tile_split(threshold):
    """Closest-hit kernels: tiles whose last walk visited at least `threshold` nodes are traced by four waves (rs_set_tile_split); 0 = off."""
    check(lib().rs_set_tile_split(int(threshold)))


def split_tiles(gbuf=None, restir=None):
    """rs_debug_split_tiles (test hook): (render, primary) -- tiles that helper blocks took over in the most recent split launch of the
    G-buffer's own render and of the ReSTIR object's primary-ray launches; 0 = the four-wave form did not run there."""
    a, b = C.c_uint(0), C.c_uint(0)
    check(lib().rs_debug_split_tiles(gbuf.handle if gbuf else None, restir.handle if restir else None, C.byref(a), C.byref(b)))
    return a.value, b.value


def write_jpg(path, rgb):
    """Image::saveJPG's file (stbi_write_jpg, quality 90) from an (H, W, 3) uint8 array."""
    a = np.ascontiguousarray(rgb, np.uint8)
    check(lib().rs_write_jpg(os.fsencode(path), _p(a), a.shape[1], a.shape[0]))


def save_image_jpg(path, dev_image_ptr, width, height, tone_mapping):
    """saveImage(true) (src/main.cpp:105-144): tone map + gamma, mirrored in x, JPEG at quality 90."""
    check(lib().rs_save_image_jpg(os.fsencode(path), dev_image_ptr, width, height, tone_mapping))


def save_image(path, dev_image_ptr, width, height, tone_mapping):
    """saveImage(false) (src/main.cpp:105-144): tone map + gamma, mirrored in x, 8-bit RGB PNG."""
    check(lib().rs_save_image(str(path).encode(), dev_image_ptr, width, height, tone_mapping))


def write_png(path, rgb):
    """rgb: uint8 numpy array (height, width, 3)."""
    import numpy as np
    a = np.ascontiguousarray(rgb, dtype=np.uint8)
    check(lib().rs_write_png(str(path).encode(), a.ctypes.data_as(C.c_void_p), a.shape[1], a.shape[0]))


def synchronize():
    check(lib().rs_synchronize())


def camera_update(cam):
    check(lib().rs_camera_update(C.byref(cam)))
    return cam


def plan_primary_leaf_list(cam, x0, y0, boxes, nodes, cap):
    """rs_debug_plan_primary_leaf_list (host only): the leaf list of the 8x8 tile at pixel (x0, y0) over build_bvh's outputs.  Returns
    (order, count, positions): order -1 when the tile takes no list; count = cap + 1 when it has more than cap leaves; positions = the
    record indices of the first min(count, cap) leaves in nodes[order]."""
    boxes = np.ascontiguousarray(boxes, np.float32); nodes = np.ascontiguousarray(nodes, np.int32)
    arr = (C.c_void_p * 6)(*[nodes[i].ctypes.data for i in range(6)])
    order, count = C.c_int(), C.c_int()
    pos = np.zeros(max(int(cap), 1), np.int32)
    check(lib().rs_debug_plan_primary_leaf_list(C.byref(cam), int(x0), int(y0), nodes.shape[1], _p(boxes), C.byref(arr), int(cap), C.byref(order), C.byref(count), _p(pos)))
    return order.value, count.value, pos[:min(count.value, int(cap))].copy()


def plan_primary_cut(cam, x0, y0, w, h, boxes, nodes, cap):
    """rs_debug_plan_primary_cut (host only): the node cut of the w x h pixels at (x0, y0) over build_bvh's outputs.  Returns (order,
    count, positions, links): order -1 when the cell takes no cut; count = cap + 1 when it has more than cap records; positions = the
    record indices of the first min(count, cap) kept records in nodes[order]; links = their miss links within the cut (empty past the cap)."""
    boxes = np.ascontiguousarray(boxes, np.float32); nodes = np.ascontiguousarray(nodes, np.int32)
    arr = (C.c_void_p * 6)(*[nodes[i].ctypes.data for i in range(6)])
    order, count = C.c_int(), C.c_int()
    pos, links = np.zeros(max(int(cap), 1), np.int32), np.zeros(max(int(cap), 1), np.int32)
    check(lib().rs_debug_plan_primary_cut(C.byref(cam), int(x0), int(y0), int(w), int(h), nodes.shape[1], _p(boxes), C.byref(arr), int(cap),
                                          C.byref(order), C.byref(count), _p(pos), _p(links)))
    kept = min(count.value, int(cap))
    return order.value, count.value, pos[:kept].copy(), links[:kept if count.value <= int(cap) else 0].copy()


def plan_primary_cut_slot(slot, key, on=True, capturing=False, tiles=(1, 1)):
    """rs_debug_plan_primary_cut_slot (host only): a phase-A call with PrimaryCutKey `key` meets PrimaryCutSlot `slot`, which is updated
    as the call leaves it.  Returns (cutState, PrimaryCutSizes of a launch of tiles[0] x tiles[1] blocks under the key's caps)."""
    state, sizes = C.c_int(), PrimaryCutSizes()
    check(lib().rs_debug_plan_primary_cut_slot(int(on), int(capturing), C.byref(slot), C.byref(key), int(tiles[0]), int(tiles[1]), C.byref(state), C.byref(sizes)))
    return state.value, sizes


def plan_shadow_regroup(lengths, bins_over_extent=None, root=None, active=None, plan=False):
    """rs_debug_plan_shadow_regroup (host only): the length bins of the segments `lengths` under bins_over_extent, or under the value the
    launch computes from the root box root = (lo, hi).  Returns (bins, bins_over_extent), and with plan=True (at most 256 segments: the
    lanes of one block; active[i] false: no segment) (bins, bins_over_extent, first[64], count)."""
    lengths = np.ascontiguousarray(lengths, np.float32).reshape(-1)
    n = len(lengths)
    bins, first, count, used = np.zeros(max(n, 1), np.int32), np.zeros(64, np.int32), C.c_int(), C.c_float()
    act = None if active is None else np.ascontiguousarray(np.asarray(active) != 0, np.uint8)
    lo, hi = (None, None) if root is None else (np.ascontiguousarray(root[0], np.float32), np.ascontiguousarray(root[1], np.float32))
    check(lib().rs_debug_plan_shadow_regroup(n, _p(lengths), None if act is None else _p(act), float(bins_over_extent or 0.0), None if lo is None else _p(lo),
                                             None if hi is None else _p(hi), _p(bins), _p(first) if plan else None, C.byref(count) if plan else None, C.byref(used)))
    return (bins[:n], used.value, first, count.value) if plan else (bins[:n], used.value)


def plan_dirty_box(old_vertices, prim_ids, new_vertices):
    """rs_debug_plan_dirty_box (host only): (lo, hi) of the edit that gives the primitives prim_ids of the table old_vertices (n, 3, 3) the
    corners new_vertices (len(prim_ids), 3, 3); an id named twice takes its last record."""
    old = np.ascontiguousarray(old_vertices, np.float32).reshape(-1, 9)
    ids = np.ascontiguousarray(prim_ids, np.int32).reshape(-1)
    new = np.ascontiguousarray(new_vertices, np.float32).reshape(-1, 9)
    if len(new) != len(ids):
        raise ValueError("plan_dirty_box: three new vertices per id")
    lo, hi = np.zeros(3, np.float32), np.zeros(3, np.float32)
    check(lib().rs_debug_plan_dirty_box(len(old), _p(old), len(ids), _p(ids), _p(new), _p(lo), _p(hi)))
    return lo, hi


def plan_revalidation(boxes, seen, now, same_scene=True, first_edit=1):
    """rs_debug_plan_revalidation (host only): the edits first_edit, first_edit + 1, ... with the boxes `boxes` (k, 6: lo, hi) go through
    the scene's ring; a frame whose previous frame saw `seen` edits then chooses at `now`.  Returns (launch, everything, boxes (n, 6))."""
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    launch, everything, n = C.c_int(), C.c_int(), C.c_int()
    out = np.zeros((DIRTY_BOXES_KEPT, 6), np.float32)
    check(lib().rs_debug_plan_revalidation(len(b), int(first_edit), _p(b) if len(b) else None, int(seen), int(now), 1 if same_scene else 0,
                                           C.byref(launch), C.byref(everything), C.byref(n), _p(out)))
    return bool(launch.value), bool(everything.value), out[:n.value].copy()


def segment_in_boxes(segments, boxes, everything=False):
    """rs_debug_segment_in_boxes (host only): which of the segments (n, 6: a, b) are walked against the boxes (m <= 8, 6: lo, hi)."""
    seg = np.ascontiguousarray(segments, np.float32).reshape(-1, 6)
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    flags = np.zeros(max(len(seg), 1), np.uint8)
    check(lib().rs_debug_segment_in_boxes(len(seg), _p(seg) if len(seg) else None, len(b), _p(b) if len(b) else None, 1 if everything else 0, _p(flags)))
    return flags[:len(seg)] != 0


def indirect_candidate_classes(reservoirs, boxes, everything=False):
    """rs_debug_indirect_candidate_classes (host only): the class of every reservoir (INDIRECT_RESERVOIR_DTYPE) against the boxes (m <= 8,
    6: lo, hi) -- 0 not examined, 1 stale, 2 walk, 3 examined and kept."""
    resv = np.ascontiguousarray(reservoirs, INDIRECT_RESERVOIR_DTYPE).reshape(-1)
    b = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    classes = np.zeros(max(len(resv), 1), np.uint8)
    check(lib().rs_debug_indirect_candidate_classes(len(resv), _p(resv) if len(resv) else None, len(b), _p(b) if len(b) else None, 1 if everything else 0,
                                                    _p(classes)))
    return classes[:len(resv)].copy()


def seeded_uniforms(scene, iter_, index, dim, n):
    """rs_debug_seeded_uniforms (host only): n draws of the library's sampler seeded(table, iter, index, dim) -- `scene`'s Sobol table, or
    the default engine when `scene` is None or has no table."""
    out = np.zeros(max(n, 1), np.float32)
    check(lib().rs_debug_seeded_uniforms(scene.handle if scene is not None else None, int(iter_), int(index), int(dim), int(n), _p(out)))
    return out[:n]


def plan_stream_choice(priority_range, asked=2, caller_priority=None, times_us=None):
    """rs_debug_plan_stream_choice (host only): priority_range = (least, greatest) of the device, asked -1 / 0 / 1 / 2 = automatic,
    caller_priority None for the default stream, times_us[3][4] the measured triples (None: all 1.0).  Returns StreamChoicePlan."""
    i, o = StreamChoiceInputs(), StreamChoicePlan()
    i.least, i.greatest, i.asked = int(priority_range[0]), int(priority_range[1]), int(asked)
    i.callerHasStream, i.callerPriority = int(caller_priority is not None), int(caller_priority or 0)
    for lvl in range(3):
        for k in range(4):
            i.timesUs[lvl][k] = 1.0 if times_us is None else float(times_us[lvl][k])
    check(lib().rs_debug_plan_stream_choice(C.byref(i), C.byref(o)))
    return o


def plan_stream_switch(state, caller, level_key=2, forget=False):
    """rs_debug_plan_stream_switch (host only): the first use after a change under caller stream `caller` (an opaque integer) and
    `level_key` meets StreamChoices `state`, which is updated in place.  Returns the list of StreamChoice released."""
    released, n = (StreamChoice * (STREAM_CHOICES_KEPT + 1))(), C.c_int()
    check(lib().rs_debug_plan_stream_switch(C.byref(state), int(forget), C.c_void_p(caller), int(level_key), released, C.byref(n)))
    return [released[k] for k in range(n.value)]


# ---- host builders (no GPU needed) ----------------------------------------------------------------
def build_bvh(vertices):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1)
    n = v.size // 9
    size = 2 * n - 1
    boxes = np.zeros((size, 6), np.float32)
    nodes = np.zeros((6, size, 3), np.int32)
    arr = (C.c_void_p * 6)(*[nodes[i].ctypes.data for i in range(6)])
    got = C.c_int(0)
    check(lib().rs_build_bvh(n, _p(v), _p(boxes), C.byref(arr), C.byref(got)))
    assert got.value == size
    return boxes, nodes


def refit_boxes(vertices, order0):
    """rs_refit_boxes: the reference tree's boxes refitted to `vertices` ((n, 3, 3) float32); order0 = bvhNodes[0] ((2n - 1, 3) int32).
    Host only.  Returns (2n - 1, 6) float32 by boundingBoxId."""
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1)
    o = np.ascontiguousarray(order0, np.int32).reshape(-1, 3)
    boxes = np.zeros((len(o), 6), np.float32)
    check(lib().rs_refit_boxes(v.size // 9, _p(v), len(o), _p(o), _p(boxes)))
    return boxes


def grid_box(lo, hi, base, scale, margin):
    """rs_debug_grid_box (test hook, host only): the three box dwords of the exact box [lo, hi] on the grid (base, scale, margin), or
    None when the box does not fit the grid's 16 bits.  Also returns the output array, which a box that does not fit leaves untouched."""
    a = [np.ascontiguousarray(x, np.float32).reshape(3) for x in (lo, hi, base, scale)]
    out = np.full(3, 0xdeadbeef, np.uint32)
    fits = C.c_int(-1)
    check(lib().rs_debug_grid_box(_p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]), float(margin), _p(out), C.byref(fits)))
    return (out if fits.value else None), out


SURFACE_OPS = {"linear_sample": (0, 2, 3), "procedural_texture": (1, 2, 3), "to_sphere": (2, 2, 3), "to_plane": (3, 3, 2), "local_to_world": (4, 6, 3)}


def surface_op(name, rows, texture=None):
    """rs_debug_surface_ops (test hook): the device's rs_surface.h function `name` on every row of `rows` ((n, 2): (u, v); to_plane
    (n, 3): a direction; local_to_world (n, 6): normal, vector); texture: the (H, W, 3) float32 map linear_sample reads."""
    op, win, wout = SURFACE_OPS[name]
    a = np.ascontiguousarray(rows, np.float32).reshape(-1, win)
    out = np.zeros((len(a), wout), np.float32)
    if texture is None:
        check(lib().rs_debug_surface_ops(op, len(a), _p(a), _p(out), 0, 0, None))
    else:
        t = np.ascontiguousarray(texture, np.float32)
        assert t.ndim == 3 and t.shape[2] == 3, "textures are (H, W, 3) float32"
        check(lib().rs_debug_surface_ops(op, len(a), _p(a), _p(out), t.shape[1], t.shape[0], _p(t)))
    return out


# rs_debug_scene_table: name -> (RS_TABLE_*, record dtype)
TRI_DTYPE = np.dtype([("v0", np.float32, 3), ("pad0", np.uint32), ("e1", np.float32, 3), ("pad1", np.uint32), ("e2", np.float32, 3), ("pad2", np.uint32)])
NODE_DTYPE = np.dtype([("min", np.float32, 3), ("maxz", np.float32), ("maxx", np.float32), ("maxy", np.float32), ("primId", np.int32), ("next", np.int32)])
GRID_DTYPE = np.dtype([("box", np.uint32, 3), ("w", np.int32)])
SCENE_TABLES = {
    "vertices": (0, np.dtype((np.float32, (3, 3)))), "normals": (1, np.dtype((np.float32, (3, 3)))), "tris": (2, TRI_DTYPE),
    "nodesAll": (3, NODE_DTYPE), "occNodes": (4, GRID_DTYPE), "occChain": (5, NODE_DTYPE), "occTris": (6, TRI_DTYPE),
    "ordNodes": (7, GRID_DTYPE), "ordTris": (8, TRI_DTYPE), "emiNodes": (9, GRID_DTYPE), "emiTris": (10, TRI_DTYPE),
}
# ... and the tables that record the scene's history of edits, which a scene built afresh from the edited arrays does not share
HISTORY_TABLES = {"lightMoved": (32, np.dtype(np.uint32))}


def ordered_bvh_host_check(boxes, nodes):
    """rs_ordered_bvh_host_check on rs_build_bvh's outputs; returns (error code, node counts per axis, depth per axis)."""
    boxes = np.ascontiguousarray(boxes, np.float32); nodes = [np.ascontiguousarray(nodes[k], np.int32) for k in range(6)]
    size = boxes.shape[0]
    arr = (C.c_void_p * 6)(*[nodes[i].ctypes.data for i in range(6)])
    counts = (C.c_int * 3)(); depth = (C.c_int * 3)()
    fn = lib().rs_ordered_bvh_host_check
    fn.argtypes = [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_void_p * 6), C.POINTER(C.c_int * 3), C.POINTER(C.c_int * 3)]
    e = fn((size + 1) // 2, size, _p(boxes), C.byref(arr), C.byref(counts), C.byref(depth))
    return e, list(counts), list(depth)


def build_alias_table(values):
    values = np.ascontiguousarray(values, np.float32)
    n = values.size
    prob = np.zeros(n, np.float32); fail = np.zeros(n, np.int32); s = C.c_float(0)
    check(lib().rs_build_alias_table(n, _p(values), _p(prob), _p(fail), C.byref(s)))
    return prob, fail, np.float32(s.value)


def build_light_table(vertices, material_ids, materials):
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1)
    n = v.size // 9
    mats = np.ascontiguousarray(materials, MATERIAL_DTYPE)
    ids = np.zeros(n, np.int32); rad = np.zeros((n, 3), np.float32); power = np.zeros(n, np.float32)
    k = C.c_int(0)
    check(lib().rs_build_light_table(n, _p(v), _p(np.ascontiguousarray(material_ids, np.int32)), len(mats), _p(mats),
                                     C.byref(k), _p(ids), _p(rad), _p(power)))
    return ids[:k.value].copy(), rad[:k.value].copy(), power[:k.value].copy()


def build_envmap_pdf(env):
    """Scene::createLightSampler's environment-map pdf (src/scene.cpp:139-146) for an (H, W, 3) float32 map."""
    env = np.ascontiguousarray(env, np.float32)
    pdf = np.zeros(env.shape[0] * env.shape[1], np.float32)
    check(lib().rs_build_envmap_pdf(env.shape[1], env.shape[0], _p(env), _p(pdf)))
    return pdf


def build_transformation_matrix(translation, rotation, scale):
    """Math::buildTransformationMatrix (src/mathUtil.cpp:13-20): (4, 4) float32, [column][row]."""
    t, r, sc = (np.ascontiguousarray(a, np.float32) for a in (translation, rotation, scale))
    out = np.zeros((4, 4), np.float32)
    check(lib().rs_build_transformation_matrix(_p(t), _p(r), _p(sc), _p(out)))
    return out


def bake_instance(translation, rotation, scale, vertices, normals):
    """Instance baking of Scene::buildDevData (src/scene.cpp:167-168) for (n, 3) vertices / normals."""
    t, r, sc = (np.ascontiguousarray(a, np.float32) for a in (translation, rotation, scale))
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    vo, no = np.zeros_like(v), np.zeros_like(n)
    check(lib().rs_bake_instance(_p(t), _p(r), _p(sc), len(v), _p(v), _p(n), _p(vo), _p(no)))
    return vo, no


def bake_matrix(matrix, vertices, normals):
    """rs_bake_matrix: bake_instance for a caller-supplied (4, 4) float32 matrix, [column][row]."""
    m = np.ascontiguousarray(matrix, np.float32).reshape(16)
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    vo, no = np.zeros_like(v), np.zeros_like(n)
    check(lib().rs_bake_matrix(_p(m), len(v), _p(v), _p(n), _p(vo), _p(no)))
    return vo, no


def skin_corners(matrices, vertices, normals, bone_ids, weights):
    """rs_skin_corners (host only): (k, 3) corners blended by 4 bone ids and 4 weights each over a palette of (4, 4) float32 matrices,
    [column][row]; the weights are used as given."""
    m = np.ascontiguousarray(matrices, np.float32).reshape(-1, 16)
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    b = np.ascontiguousarray(bone_ids, np.int32).reshape(-1, 4)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1, 4)
    if not (len(v) == len(n) == len(b) == len(w)):
        raise ValueError("skin_corners: one normal, four bone ids and four weights per corner")
    vo, no = np.zeros_like(v), np.zeros_like(n)
    check(lib().rs_skin_corners(len(m), _p(m), len(v), _p(v), _p(n), _p(b), _p(w), _p(vo), _p(no)))
    return vo, no


# rs::MorphEntry, the 32-byte record of a morph's by-corner table (rs_scene_download_morph)
MORPH_ENTRY = np.dtype([("target", np.int32), ("dp", np.float32, 3), ("dn", np.float32, 3), ("pad", np.int32)])


def _morph_table(target_first, entry_corner, delta_positions, delta_normals):
    """The by-target table as contiguous arrays: (numTargets, offsets, corners, position deltas, normal deltas or None)."""
    first = np.ascontiguousarray(target_first, np.int32).reshape(-1)
    ec = np.ascontiguousarray(entry_corner, np.int32).reshape(-1)
    dp = np.ascontiguousarray(delta_positions, np.float32).reshape(-1, 3)
    dn = None if delta_normals is None else np.ascontiguousarray(delta_normals, np.float32).reshape(-1, 3)
    if first.size < 1 or len(dp) != ec.size or (dn is not None and len(dn) != ec.size):
        raise ValueError("a morph table: numTargets + 1 offsets, and one corner, position delta and normal delta per entry")
    return first.size - 1, first, ec, dp, dn


def morph_corners(target_first, entry_corner, delta_positions, delta_normals, weights, vertices, normals):
    """rs_morph_corners (host only): (k, 3) corners with the weighted deltas of a by-target table over those k corners added, in ascending
    target order; delta_normals may be None (zeros); weights are used as given and a weight of 0 skips its entries."""
    t, first, ec, dp, dn = _morph_table(target_first, entry_corner, delta_positions, delta_normals)
    w = np.ascontiguousarray(weights, np.float32).reshape(-1)
    v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    if len(v) != len(n) or w.size != t:
        raise ValueError("morph_corners: one normal per corner and one weight per target")
    vo, no = np.zeros_like(v), np.zeros_like(n)
    check(lib().rs_morph_corners(t, _p(first), _p(ec), _p(dp), None if dn is None else _p(dn), _p(w), len(v), _p(v), _p(n), _p(vo), _p(no)))
    return vo, no


class SceneFile:
    """Scene::Scene(filename) (src/scene.cpp:96-131): the parsed scene as flat host arrays (copies)."""

    def __init__(self, path):
        h = C.c_void_p()
        check(lib().rs_scene_file_load(os.fsencode(path), C.byref(h)))
        try:
            v = SceneFileView()
            check(lib().rs_scene_file_get(h, C.byref(v)))
            n = v.numPrims

            def arr(ptr, count, dtype):
                return np.frombuffer(C.string_at(ptr, count * np.dtype(dtype).itemsize), dtype=dtype).copy() if count else np.zeros(0, dtype)
            self.vertices = arr(v.vertices, n * 9, np.float32).reshape(n, 3, 3)
            self.normals = arr(v.normals, n * 9, np.float32).reshape(n, 3, 3)
            self.texcoords = arr(v.texcoords, n * 6, np.float32).reshape(n, 3, 2)
            self.material_ids = arr(v.materialIds, n, np.int32)
            self.materials = arr(v.materials, v.numMaterials, MATERIAL_DTYPE)
            tex = C.cast(v.textures, C.POINTER(Texture))
            self.textures = [arr(tex[i].data, tex[i].width * tex[i].height * 3, np.float32).reshape(tex[i].height, tex[i].width, 3)
                             for i in range(v.numTextures)]
            self.env_map_tex = v.envMapTexId
            self.camera = copy_camera(v.camera)
            self.iterations, self.trace_depth = v.iterations, v.traceDepth
            self.image_name = (v.imageName or b"").decode()
            self.num_skipped_objects = v.numSkippedObjects
            # rs_scene_file_objects: per "Object" block dict(first, count, transform (4, 4), vertices, normals (count, 3, 3) in object space,
            # mesh = (address of the shared mesh's vertices, of its normals))
            count, first, tr, mv, mn = C.c_int(0), C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
            check(lib().rs_scene_file_objects(h, C.byref(count), C.byref(first), C.byref(tr), C.byref(mv), C.byref(mn)))
            firsts = arr(first.value, count.value + 1, np.int32)
            trs = arr(tr.value, count.value * 16, np.float32).reshape(-1, 4, 4)
            mvp, mnp = C.cast(mv, C.POINTER(C.c_void_p)), C.cast(mn, C.POINTER(C.c_void_p))
            self.object_first = firsts
            self.objects = []
            for i in range(count.value):
                k = int(firsts[i + 1] - firsts[i])
                self.objects.append(dict(first=int(firsts[i]), count=k, transform=trs[i], mesh=(mvp[i], mnp[i]),
                                         vertices=arr(mvp[i], k * 9, np.float32).reshape(k, 3, 3),
                                         normals=arr(mnp[i], k * 9, np.float32).reshape(k, 3, 3)))
        finally:
            lib().rs_scene_file_free(h)

    def build(self):
        """Scene::buildDevData + DevScene::create of the parsed scene."""
        return Scene(self.vertices, self.normals, self.texcoords, self.material_ids, self.materials,
                     textures=self.textures, env_map_tex=self.env_map_tex)


def _texture_table(textures):
    keep = [np.ascontiguousarray(t, np.float32) for t in textures]
    arr = (Texture * max(1, len(keep)))()
    for i, t in enumerate(keep):
        assert t.ndim == 3 and t.shape[2] == 3, "textures are (H, W, 3) float32"
        arr[i].height, arr[i].width, arr[i].data = t.shape[0], t.shape[1], t.ctypes.data
    return keep, arr


# ---- device objects ---------------------------------------------------------------------------------
class Scene:
    """Scene::buildDevData + DevScene (src/scene.cpp:159-215): builds light table, alias table and the
    MTBVH on the host (C++ in the library) and uploads the CDNA4 layout."""

    def __init__(self, vertices, normals, texcoords, material_ids, materials, textures=(), env_map_tex=-1):
        """textures: (H, W, 3) float32 linear-RGB arrays (what Image holds, src/image.h); env_map_tex: index or -1."""
        self._keep = (np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(normals, np.float32),
                      np.ascontiguousarray(texcoords, np.float32), np.ascontiguousarray(material_ids, np.int32),
                      np.ascontiguousarray(materials, MATERIAL_DTYPE))
        v, n, t, m, mats = self._keep
        self.num_prims = v.size // 9
        self.handle = C.c_void_p()
        self._tex, tex = _texture_table(textures)
        check(lib().rs_scene_build_textured(self.num_prims, _p(v), _p(n), _p(t), _p(m), len(mats), _p(mats),
                                            len(self._tex), C.cast(tex, C.c_void_p), int(env_map_tex), C.byref(self.handle)))

    @classmethod
    def from_tables(cls, vertices, normals, texcoords, material_ids, materials, tables, textures=(), env_map_tex=-1, env_sampler=None):
        """DevScene::create from caller-built tables (rs_scene_create): `tables` as returned by host_desc();
        env_sampler = (prob, failId) of the environment map's alias table when env_map_tex >= 0; texcoords None = a scene created
        without texture coordinates (rs_scene_desc::texcoords == NULL: it takes no texture map, at creation or by set_materials)."""
        self = cls.__new__(cls)
        t = tables
        self._tex, tex = _texture_table(textures)
        self._keep = (np.ascontiguousarray(vertices, np.float32), np.ascontiguousarray(normals, np.float32),
                      None if texcoords is None else np.ascontiguousarray(texcoords, np.float32), np.ascontiguousarray(material_ids, np.int32),
                      np.ascontiguousarray(materials, MATERIAL_DTYPE),
                      np.ascontiguousarray(t["boxes"], np.float32), [np.ascontiguousarray(t["nodes"][k], np.int32) for k in range(6)],
                      np.ascontiguousarray(t["light_prim_ids"], np.int32), np.ascontiguousarray(t["light_radiance"], np.float32),
                      np.ascontiguousarray(t["light_prob"], np.float32), np.ascontiguousarray(t["light_fail"], np.int32))
        v, n, tc, m, mats, boxes, nodes, lp, lr, lpr, lf = self._keep
        self.num_prims = v.size // 9
        d = SceneDesc()
        d.numPrims = self.num_prims
        d.vertices, d.normals, d.texcoords, d.materialIds = _p(v), _p(n), (None if tc is None else _p(tc)), _p(m)
        d.numMaterials, d.materials = len(mats), _p(mats)
        d.bvhSize, d.boundingBoxes = len(boxes), _p(boxes)
        for k in range(6):
            d.bvhNodes[k] = _p(nodes[k])
        d.numLights = len(lpr)                      # sampler length (light primitives + 1 with an environment map)
        d.lightPrimIds, d.lightUnitRadiance, d.lightProb, d.lightFailId = _p(lp), _p(lr), _p(lpr), _p(lf)
        d.sumLightPower = float(t["sum_power"])
        d.numTextures = len(self._tex); d.textures = C.cast(tex, C.c_void_p); d.envMapTexId = int(env_map_tex)
        if env_sampler is not None:
            self._env = (np.ascontiguousarray(env_sampler[0], np.float32), np.ascontiguousarray(env_sampler[1], np.int32))
            d.envMapProb, d.envMapFailId = _p(self._env[0]), _p(self._env[1])
        self.handle = C.c_void_p()
        check(lib().rs_scene_create(C.byref(d), C.byref(self.handle)))
        return self

    def set_sample_sequence(self, table):
        """DevScene::sampleSequence: uint32 [numSamples, 200] selects the Sobol sampler (src/sampler.h:9-36), None the default engine."""
        if table is None:
            check(lib().rs_scene_set_sample_sequence(self.handle, None, 0, 0))
            return
        t = np.ascontiguousarray(table, np.uint32)
        check(lib().rs_scene_set_sample_sequence(self.handle, _p(t), t.shape[0], t.shape[1]))

    def set_emission(self, material_ids, radiance):
        """rs_scene_set_emission: baseColor of the Light materials `material_ids` := rows of `radiance` ((n, 3) float32), ordered on
        the library stream after the frames enqueued so far (no synchronisation)."""
        ids = np.ascontiguousarray(material_ids, np.int32).reshape(-1)
        rad = np.ascontiguousarray(radiance, np.float32).reshape(-1, 3)
        if rad.shape[0] != ids.size:
            raise ValueError("set_emission: one radiance row per material id")
        check(lib().rs_scene_set_emission(self.handle, int(ids.size), _p(ids), _p(rad)))

    def set_materials(self, material_ids, records):
        """rs_scene_set_materials: the records (MATERIAL_DTYPE) of the materials `material_ids`, none of them a Light before or after,
        ordered on the library stream like set_emission (no synchronisation)."""
        ids = np.ascontiguousarray(material_ids, np.int32).reshape(-1)
        rec = np.ascontiguousarray(records, MATERIAL_DTYPE).reshape(-1)
        if rec.size != ids.size:
            raise ValueError("set_materials: one record per material id")
        check(lib().rs_scene_set_materials(self.handle, int(ids.size), _p(ids), _p(rec)))

    def set_texture(self, tex_id, image):
        """rs_scene_set_texture: the texels of texture `tex_id` := `image` ((H, W, 3) float32 of the texture's own size), ordered like
        set_emission; for the environment map its sampler and the light sampler are rebuilt as well."""
        img = np.ascontiguousarray(image, np.float32)
        if img.ndim != 3 or img.shape[2] != 3:
            raise ValueError("set_texture: textures are (H, W, 3) float32")
        check(lib().rs_scene_set_texture(self.handle, int(tex_id), img.shape[1], img.shape[0], _p(img)))

    def _set_vertices(self, call, what, prim_ids, vertices, normals):
        ids = np.ascontiguousarray(prim_ids, np.int32).reshape(-1)
        v = np.ascontiguousarray(vertices, np.float32).reshape(-1, 9)
        n = None if normals is None else np.ascontiguousarray(normals, np.float32).reshape(-1, 9)
        if v.shape[0] != ids.size or (n is not None and n.shape[0] != ids.size):
            raise ValueError(what + ": three vertices (and three normals) per primitive id")
        check(call(self.handle, int(ids.size), _p(ids), _p(v), None if n is None else _p(n)))

    def set_triangles(self, prim_ids, vertices, normals=None):
        """rs_scene_set_triangles: the vertices ((n, 3, 3) float32) and, unless None, the vertex normals of the primitives `prim_ids`,
        none of them emissive; every tree is refitted on the device, ordered on the library stream like set_emission (no synchronisation)."""
        self._set_vertices(lib().rs_scene_set_triangles, "set_triangles", prim_ids, vertices, normals)

    def set_geometry(self, prim_ids, vertices, normals=None):
        """rs_scene_set_geometry: set_triangles that also takes emissive triangles; an edit that names one rebuilds the light sampler and the
        light records and refits the emissive tree at the same point of the library stream."""
        self._set_vertices(lib().rs_scene_set_geometry, "set_geometry", prim_ids, vertices, normals)

    def define_parts(self, parts, rest_vertices=None, rest_normals=None):
        """rs_scene_define_parts: `parts` is a list of primitive-id lists (an empty list drops the definition); the rest pose is
        (listed, 3, 3) float32 vertices and normals in the order of the concatenated ids, or None: the scene's current pose."""
        first = np.zeros(len(parts) + 1, np.int32)
        first[1:] = np.cumsum([len(p) for p in parts])
        ids = np.ascontiguousarray(np.concatenate([np.asarray(p, np.int32).reshape(-1) for p in parts]) if parts else np.zeros(0, np.int32), np.int32)
        v = None if rest_vertices is None else np.ascontiguousarray(rest_vertices, np.float32).reshape(-1, 9)
        n = None if rest_normals is None else np.ascontiguousarray(rest_normals, np.float32).reshape(-1, 9)
        for a in (v, n):
            if a is not None and a.shape[0] != ids.size:
                raise ValueError("define_parts: three rest vertices and three rest normals per listed primitive")
        check(lib().rs_scene_define_parts(self.handle, len(parts), _p(first), _p(ids), None if v is None else _p(v), None if n is None else _p(n)))

    def light_moves(self):
        """rs_scene_light_moves: accepted geometry edits that named an emitter so far (host only)."""
        n = C.c_ulonglong(0)
        check(lib().rs_scene_light_moves(self.handle, C.byref(n)))
        return int(n.value)

    def geometry_edits(self):
        """rs_scene_geometry_edits: accepted geometry edits so far (host only)."""
        n = C.c_ulonglong(0)
        check(lib().rs_scene_geometry_edits(self.handle, C.byref(n)))
        return int(n.value)

    def dirty_boxes(self, since_edit):
        """rs_scene_dirty_boxes: (boxes (n, 6: lo, hi), everything) a frame whose previous frame saw since_edit edits would take now."""
        out = np.zeros((DIRTY_BOXES_KEPT, 6), np.float32)
        n, everything = C.c_int(), C.c_int()
        check(lib().rs_scene_dirty_boxes(self.handle, int(since_edit), DIRTY_BOXES_KEPT, _p(out), C.byref(n), C.byref(everything)))
        return out[:n.value].copy(), bool(everything.value)

    def set_part_transforms(self, part_ids, matrices):
        """rs_scene_set_part_transforms: one (4, 4) float32 matrix, [column][row], per entry of `part_ids`; does what set_geometry does
        with the parts' rest pose baked by those matrices, the baking done on the device (one small record per part crosses the bus)."""
        ids = np.ascontiguousarray(part_ids, np.int32).reshape(-1)
        m = np.ascontiguousarray(matrices, np.float32).reshape(-1, 16)
        if m.shape[0] != ids.size:
            raise ValueError("set_part_transforms: one matrix per part id")
        check(lib().rs_scene_set_part_transforms(self.handle, int(ids.size), _p(ids), _p(m)))

    def parts_info(self):
        """rs_scene_parts_info: (number of parts, number of primitives listed in them); (0, 0) when none are defined."""
        a, b = C.c_int(0), C.c_int(0)
        check(lib().rs_scene_parts_info(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def part_rest(self):
        """rs_scene_download_part_rest (test hook): the device copies of (primitive ids, rest vertices, rest normals)."""
        n = self.parts_info()[1]
        ids, v, nn = np.zeros(n, np.int32), np.zeros((n, 3, 3), np.float32), np.zeros((n, 3, 3), np.float32)
        check(lib().rs_scene_download_part_rest(self.handle, _p(ids), _p(v), _p(nn)))
        return ids, v, nn

    def define_skin(self, num_bones, prim_ids, bone_ids, weights, rest_vertices=None, rest_normals=None):
        """rs_scene_define_skin: the listed primitives follow a blend of `num_bones` bone matrices; bone_ids / weights are (listed, 3, 4),
        4 per corner; the rest pose is (listed, 3, 3) float32 vertices and normals, or None: the scene's current pose.  num_bones == 0 with
        no primitive drops the definition."""
        ids = np.ascontiguousarray(prim_ids, np.int32).reshape(-1)
        b = np.ascontiguousarray(bone_ids, np.int32).reshape(-1, 12)
        w = np.ascontiguousarray(weights, np.float32).reshape(-1, 12)
        v = None if rest_vertices is None else np.ascontiguousarray(rest_vertices, np.float32).reshape(-1, 9)
        n = None if rest_normals is None else np.ascontiguousarray(rest_normals, np.float32).reshape(-1, 9)
        for a in (b, w, v, n):
            if a is not None and a.shape[0] != ids.size:
                raise ValueError("define_skin: per listed primitive three rest vertices and normals, and four bone ids and weights per corner")
        check(lib().rs_scene_define_skin(self.handle, int(num_bones), int(ids.size), _p(ids), None if v is None else _p(v), None if n is None else _p(n),
                                         _p(b), _p(w)))

    def set_bone_transforms(self, bone_ids, matrices):
        """rs_scene_set_bone_transforms: one (4, 4) float32 matrix, [column][row], per entry of `bone_ids`; does what set_geometry does with
        the skin's rest pose blended by the whole palette, the skinning done on the device (one small record per bone crosses the bus)."""
        ids = np.ascontiguousarray(bone_ids, np.int32).reshape(-1)
        m = np.ascontiguousarray(matrices, np.float32).reshape(-1, 16)
        if m.shape[0] != ids.size:
            raise ValueError("set_bone_transforms: one matrix per bone id")
        check(lib().rs_scene_set_bone_transforms(self.handle, int(ids.size), _p(ids), _p(m)))

    def skin_info(self):
        """rs_scene_skin_info: (number of bones, number of primitives the skin lists); (0, 0) when none is defined."""
        a, b = C.c_int(0), C.c_int(0)
        check(lib().rs_scene_skin_info(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def download_skin(self):
        """rs_scene_download_skin (test hook): the device copies of (primitive ids, rest vertices, rest normals, bone ids, weights)."""
        n = self.skin_info()[1]
        ids, v, nn = np.zeros(n, np.int32), np.zeros((n, 3, 3), np.float32), np.zeros((n, 3, 3), np.float32)
        b, w = np.zeros((n, 3, 4), np.int32), np.zeros((n, 3, 4), np.float32)
        check(lib().rs_scene_download_skin(self.handle, _p(ids), _p(v), _p(nn), _p(b), _p(w)))
        return ids, v, nn, b, w

    def define_morph(self, prim_ids, target_first, entry_corner, delta_positions, delta_normals=None, rest_vertices=None, rest_normals=None):
        """rs_scene_define_morph: morph targets over the corners of the listed primitives (entry_corner: listed index * 3 + corner), as a
        by-target table; the rest pose is (listed, 3, 3) vertices and normals, or None: the scene's current pose.  No target and no
        primitive drops the definition."""
        ids = np.ascontiguousarray(prim_ids, np.int32).reshape(-1)
        t, first, ec, dp, dn = _morph_table(target_first, entry_corner, delta_positions, delta_normals)
        v = None if rest_vertices is None else np.ascontiguousarray(rest_vertices, np.float32).reshape(-1, 9)
        n = None if rest_normals is None else np.ascontiguousarray(rest_normals, np.float32).reshape(-1, 9)
        for a in (v, n):
            if a is not None and a.shape[0] != ids.size:
                raise ValueError("define_morph: three rest vertices and three rest normals per listed primitive")
        check(lib().rs_scene_define_morph(self.handle, t, int(ids.size), _p(ids), None if v is None else _p(v), None if n is None else _p(n),
                                          _p(first), _p(ec), _p(dp), None if dn is None else _p(dn)))

    def define_skin_morph(self, target_first, entry_corner, delta_positions, delta_normals=None):
        """rs_scene_define_skin_morph: morph targets over the corners the skin lists, evaluated before its bones; no target drops it."""
        t, first, ec, dp, dn = _morph_table(target_first, entry_corner, delta_positions, delta_normals)
        check(lib().rs_scene_define_skin_morph(self.handle, t, _p(first), _p(ec), _p(dp), None if dn is None else _p(dn)))

    def set_morph_weights(self, target_ids, weights):
        """rs_scene_set_morph_weights: one weight per entry of `target_ids`; does what set_geometry does with the morph's rest pose and
        all its weighted deltas, the sum taken on the device (only the weights cross the bus)."""
        ids = np.ascontiguousarray(target_ids, np.int32).reshape(-1)
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        if w.size != ids.size:
            raise ValueError("set_morph_weights: one weight per target id")
        check(lib().rs_scene_set_morph_weights(self.handle, int(ids.size), _p(ids), _p(w)))

    def set_skin_pose(self, bone_ids, matrices, target_ids, weights):
        """rs_scene_set_skin_pose: bones and morph targets of the skin in one edit -- the targets first, then the bones, in one kernel."""
        b = np.ascontiguousarray(bone_ids, np.int32).reshape(-1)
        m = np.ascontiguousarray(matrices, np.float32).reshape(-1, 16)
        t = np.ascontiguousarray(target_ids, np.int32).reshape(-1)
        w = np.ascontiguousarray(weights, np.float32).reshape(-1)
        if m.shape[0] != b.size or w.size != t.size:
            raise ValueError("set_skin_pose: one matrix per bone id and one weight per target id")
        check(lib().rs_scene_set_skin_pose(self.handle, int(b.size), _p(b), _p(m), int(t.size), _p(t), _p(w)))

    def morph_info(self, which=0):
        """rs_scene_morph_info: (targets, listed primitives, entries) of the scene's morph (which = 0) or the skin's (1); zeros: none."""
        a, b, c = C.c_int(0), C.c_int(0), C.c_int(0)
        check(lib().rs_scene_morph_info(self.handle, int(which), C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def download_morph(self, which=0):
        """rs_scene_download_morph (test hook): the device copies of (cornerFirst, entries as MORPH_ENTRY records) and, for the scene's
        own morph, (primitive ids, rest vertices, rest normals) after them."""
        _, listed, entries = self.morph_info(which)
        first, recs = np.zeros(listed * 3 + 1, np.int32), np.zeros(entries, MORPH_ENTRY)
        if which:
            check(lib().rs_scene_download_morph(self.handle, 1, None, None, None, _p(first), _p(recs)))
            return first, recs
        ids, v, nn = np.zeros(listed, np.int32), np.zeros((listed, 3, 3), np.float32), np.zeros((listed, 3, 3), np.float32)
        check(lib().rs_scene_download_morph(self.handle, 0, _p(ids), _p(v), _p(nn), _p(first), _p(recs)))
        return first, recs, ids, v, nn

    def set_partial_refit(self, on=True, max_triangles=-1):
        """rs_scene_set_partial_refit: an edit of at most max_triangles triangles (< 0: the library's default) recomputes only the boxes
        above those triangles' leaves; host only."""
        check(lib().rs_scene_set_partial_refit(self.handle, 1 if on else 0, int(max_triangles)))

    def partial_refit(self):
        """rs_scene_get_partial_refit: (on, the threshold in force)."""
        on, m = C.c_int(-1), C.c_int(0)
        check(lib().rs_scene_get_partial_refit(self.handle, C.byref(on), C.byref(m)))
        return bool(on.value), m.value

    def refit_counts(self):
        """rs_scene_refit_counts: (whole, partial) refits of the accepted edits so far (host only)."""
        w, p = C.c_ulonglong(0), C.c_ulonglong(0)
        check(lib().rs_scene_refit_counts(self.handle, C.byref(w), C.byref(p)))
        return int(w.value), int(p.value)

    def refit_dirty(self):
        """rs_debug_scene_refit_dirty (test hook): distinct nodes the most recent edit recomputed on the partial path (0: it was whole)."""
        n = C.c_ulonglong(0)
        check(lib().rs_debug_scene_refit_dirty(self.handle, C.byref(n)))
        return int(n.value)

    def staged_bytes(self):
        """rs_debug_scene_staged_bytes (test hook): bytes the last accepted geometry edit copied from the host to the device."""
        b = C.c_size_t(0)
        check(lib().rs_debug_scene_staged_bytes(self.handle, C.byref(b)))
        return b.value

    def set_motion_tracking(self, on=True):
        """rs_scene_set_motion_tracking: the scene keeps its pose at the last advance_motion() on the device, and the G-buffer's motion
        plane follows moved triangles to where they were; off: camera-only again."""
        check(lib().rs_scene_set_motion_tracking(self.handle, 1 if on else 0))

    def advance_motion(self):
        """rs_scene_advance_motion: the geometry as it stands becomes the previous pose for every launch enqueued from here on; once per
        frame, next to GBuffer.update.  Nothing on an untracked scene or when no geometry edit was accepted since the last call."""
        check(lib().rs_scene_advance_motion(self.handle))

    def prev_vertices(self):
        """rs_scene_download_prev_vertices (test hook): the previous pose, (n, 3, 3) float32, after everything enqueued so far."""
        d = SceneDesc()
        check(lib().rs_scene_host_desc(self.handle, C.byref(d)))
        out = np.zeros((d.numPrims, 3, 3), np.float32)
        check(lib().rs_scene_download_prev_vertices(self.handle, _p(out)))
        return out

    def emissive_grid(self):
        """rs_debug_scene_emissive_grid (test hook): dict(base, scale, margin, state, count) of the emissive tree's grid."""
        base, scale = np.zeros(3, np.float32), np.zeros(3, np.float32)
        margin, state, count = C.c_double(0), C.c_int(0), C.c_int(0)
        check(lib().rs_debug_scene_emissive_grid(self.handle, _p(base), _p(scale), C.byref(margin), C.byref(state), C.byref(count)))
        return dict(base=base, scale=scale, margin=margin.value, state=state.value, count=count.value)

    def debug_table(self, name):
        """rs_debug_scene_table (test hook): a copy of one device array of the scene, after everything enqueued so far, as a NumPy array of
        its records (SCENE_TABLES; pads and grid-box dwords as uint32 so that they compare bit for bit); length 0 when the scene has none."""
        which, dtype = SCENE_TABLES[name] if name in SCENE_TABLES else HISTORY_TABLES[name]
        size = C.c_size_t(0)
        check(lib().rs_debug_scene_table(self.handle, which, None, 0, C.byref(size)))
        raw = np.zeros(size.value, np.uint8)
        if size.value:
            check(lib().rs_debug_scene_table(self.handle, which, _p(raw), raw.size, C.byref(size)))
        base = dtype.base if dtype.subdtype else dtype
        out = raw.view(base)
        return out.reshape((-1,) + dtype.shape) if dtype.subdtype else out

    def debug_grid(self):
        """rs_debug_scene_grid (test hook): dict(base, scale, margin, lo, hi, occ_count, ord_stride) of the grid of the grid-box trees;
        the counts are 0 when the tree is absent."""
        base, scale, lo, hi = (np.zeros(3, np.float32) for _ in range(4))
        margin, occ, stride = C.c_double(0), C.c_int(0), C.c_int(0)
        check(lib().rs_debug_scene_grid(self.handle, _p(base), _p(scale), C.byref(margin), _p(lo), _p(hi), C.byref(occ), C.byref(stride)))
        return dict(base=base, scale=scale, margin=margin.value, lo=lo, hi=hi, occ_count=occ.value, ord_stride=stride.value)

    def geometry(self):
        """The scene's vertices and vertex normals as rs_scene_host_desc returns them: two (n, 3, 3) float32 copies."""
        d = SceneDesc()
        check(lib().rs_scene_host_desc(self.handle, C.byref(d)))
        n = d.numPrims
        f = C.POINTER(C.c_float)
        return (np.ctypeslib.as_array(C.cast(d.vertices, f), (n * 9,)).reshape(n, 3, 3).copy(),
                np.ctypeslib.as_array(C.cast(d.normals, f), (n * 9,)).reshape(n, 3, 3).copy())

    def host_desc(self):
        """numpy views of the arrays the scene was built from (for parity checks of the host build)."""
        d = SceneDesc()
        check(lib().rs_scene_host_desc(self.handle, C.byref(d)))
        n, s, l = d.numPrims, d.bvhSize, d.numLights
        lp = l - (1 if d.envMapTexId >= 0 else 0)       # light primitives; the environment map is the last sampler entry
        ne = 0
        if d.envMapTexId >= 0:
            t = C.cast(d.textures, C.POINTER(Texture))[d.envMapTexId]
            ne = t.width * t.height

        def arr(ptr, ctype, count, shape):
            if count == 0:
                return np.zeros(shape, ctype)
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(np.ctypeslib.as_ctypes_type(ctype))), (count,)).reshape(shape).copy()

        return dict(
            boxes=arr(d.boundingBoxes, np.float32, s * 6, (s, 6)),
            nodes=np.stack([arr(d.bvhNodes[k], np.int32, s * 3, (s, 3)) for k in range(6)]),
            light_prim_ids=arr(d.lightPrimIds, np.int32, lp, (lp,)),
            light_radiance=arr(d.lightUnitRadiance, np.float32, lp * 3, (lp, 3)),
            light_prob=arr(d.lightProb, np.float32, l, (l,)),
            light_fail=arr(d.lightFailId, np.int32, l, (l,)),
            sum_power=np.float32(d.sumLightPower), num_lights=l, bvh_size=s, num_prims=n,
            env_map_tex=d.envMapTexId,
            env_prob=arr(d.envMapProb, np.float32, ne, (ne,)), env_fail=arr(d.envMapFailId, np.int32, ne, (ne,)),
            materials=np.frombuffer(C.string_at(d.materials, d.numMaterials * MATERIAL_DTYPE.itemsize), MATERIAL_DTYPE).copy(),
            textures=[arr(t.data, np.float32, t.width * t.height * 3, (t.height, t.width, 3))
                      for t in C.cast(d.textures, C.POINTER(Texture))[:d.numTextures]],
        )

    def destroy(self):
        if self.handle:
            lib().rs_scene_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class GBuffer:
    def __init__(self, width, height):
        self.width, self.height = width, height
        self.handle = C.c_void_p()
        check(lib().rs_gbuffer_create(width, height, C.byref(self.handle)))

    def render(self, scene, cam, y0=None, y1=None):
        if y0 is None:
            check(lib().rs_gbuffer_render(self.handle, scene.handle, C.byref(cam)))
        else:
            check(lib().rs_gbuffer_render_rows(self.handle, scene.handle, C.byref(cam), y0, y1))

    def update(self, cam):
        check(lib().rs_gbuffer_update(self.handle, C.byref(cam)))

    def rows_bytes(self, rows):
        return int(lib().rs_gbuffer_rows_bytes(self.handle, rows))

    def rows_pack(self, sel, y0, rows, dev_ptr):
        check(lib().rs_gbuffer_rows_pack(self.handle, sel, y0, rows, dev_ptr))

    def rows_unpack(self, sel, y0, rows, dev_ptr):
        check(lib().rs_gbuffer_rows_unpack(self.handle, sel, y0, rows, dev_ptr))

    def view(self):
        v = GBufferView()
        check(lib().rs_gbuffer_get_view(self.handle, C.byref(v)))
        return v

    def set_reuse(self, on):
        """Render requests whose inputs equal the two previous frames' are answered from the retained planes (rs_gbuffer_set_reuse; default on)."""
        check(lib().rs_gbuffer_set_reuse(self.handle, 1 if on else 0))

    def reuse_stats(self):
        """(rendered, reused): render requests that launched the walk / that were answered from retained planes (rs_gbuffer_reuse_stats)."""
        a, b = C.c_ulonglong(0), C.c_ulonglong(0)
        check(lib().rs_gbuffer_reuse_stats(self.handle, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def invalidate(self):
        """After writing planes through the view's pointers: the next render requests walk again (rs_gbuffer_invalidate)."""
        check(lib().rs_gbuffer_invalidate(self.handle))

    def download(self):
        """Copies every plane to host numpy arrays (torch is only used for the D2H copy)."""
        import torch
        v = self.view()
        n = self.width * self.height

        def grab(ptr, count, dtype):
            t = torch.empty(count, dtype=dtype, device="cuda")
            hip_memcpy_d2d(t.data_ptr(), ptr, count * t.element_size())
            return t.cpu().numpy()

        return dict(
            albedo=grab(v.devAlbedo, n * 3, torch.float32).reshape(n, 3),
            motion=grab(v.devMotion, n, torch.int32),
            normal=[grab(v.devNormal[i], n * 3, torch.float32).reshape(n, 3) for i in range(2)],
            prim_id=[grab(v.devPrimId[i], n, torch.int32) for i in range(2)],
            depth=[grab(v.devDepth[i], n, torch.float32) for i in range(2)],
            frame_idx=v.frameIdx,
        )

    def destroy(self):
        if self.handle:
            lib().rs_gbuffer_destroy(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


_hip = None


def _hiprt():
    global _hip
    if _hip is None:
        _hip = C.CDLL("libamdhip64.so")
        _hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        _hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        _hip.hipStreamSynchronize.argtypes = [C.c_void_p]
        _hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        _hip.hipFree.argtypes = [C.c_void_p]
    return _hip


def hip_malloc(nbytes):
    p = C.c_void_p()
    e = _hiprt().hipMalloc(C.byref(p), nbytes)
    if e != 0:
        raise RestirHipError(f"hipMalloc failed: {e}")
    return p.value


def hip_free(ptr):
    _hiprt().hipFree(ptr)


def hip_memcpy_d2d(dst, src, nbytes):
    """Device-to-device copy that has finished when the call returns, ordered after everything the library has enqueued.  (hipMemcpy of
    device memory goes through the null stream and need not block the host; a caller whose own work runs on a NON-BLOCKING stream -- torch's
    torch.cuda.Stream() -- is not ordered with the null stream either, so the copy is waited for here.  bench.py's strips-against-full-frame
    check found the missing wait: the gloo rehearsal transport read a staging buffer before this copy had written it.)"""
    _hiprt()
    synchronize()
    e = _hip.hipMemcpy(dst, src, nbytes, 3)   # hipMemcpyDeviceToDevice
    if e == 0:
        e = _hip.hipStreamSynchronize(None)
    if e != 0:
        raise RestirHipError(f"hipMemcpy failed: {e}")


def hip_memcpy_d2d_async(dst, src, nbytes):
    """Device-to-device copy enqueued on the default stream (the library's stream unless rs_set_stream changed it)."""
    _hiprt()
    e = _hip.hipMemcpyAsync(C.c_void_p(dst), C.c_void_p(src), C.c_size_t(nbytes), 3, None)
    if e != 0:
        raise RestirHipError(f"hipMemcpyAsync failed: {e}")


class ReSTIR:
    """restir.cu module state + ReSTIRInit/Free/Reset/Direct."""

    def __init__(self, width, height):
        self.width, self.height = width, height
        self.handle = C.c_void_p()
        check(lib().rs_restir_init(width, height, C.byref(self.handle)))

    def reset(self):
        check(lib().rs_restir_reset(self.handle))

    def direct(self, scene, cam, gbuf, dev_direct_illum_ptr, iter_, looper, reuse):
        check(lib().rs_restir_direct(self.handle, scene.handle, C.byref(cam), gbuf.handle, dev_direct_illum_ptr, iter_, looper, reuse))

    def indirect(self, scene, cam, gbuf, dev_indirect_illum_ptr, iter_, looper, reuse, max_depth):
        """ReSTIRIndirect (src/restir.cu:448-476); returns the number of BVH walks."""
        n = C.c_ulonglong(0)
        check(lib().rs_restir_indirect(self.handle, scene.handle, C.byref(cam), gbuf.handle, dev_indirect_illum_ptr, iter_, looper, reuse, max_depth, C.byref(n)))
        return n.value

    def download_indirect(self, which):
        out = np.zeros(self.width * self.height, INDIRECT_RESERVOIR_DTYPE)
        check(lib().rs_restir_download_indirect(self.handle, which, _p(out)))
        return out

    def phase_a(self, scene, cam, gbuf, looper, reuse, y0, y1):
        check(lib().rs_restir_phase_a(self.handle, scene.handle, C.byref(cam), gbuf.handle, looper, reuse, y0, y1))

    def phase_b(self, scene, cam, gbuf, dev_direct_illum_ptr, iter_, reuse, y0, y1):
        check(lib().rs_restir_phase_b(self.handle, scene.handle, C.byref(cam), gbuf.handle, dev_direct_illum_ptr, iter_, reuse, y0, y1))

    def end_frame(self):
        check(lib().rs_restir_end_frame(self.handle))

    def last_launch(self):
        """(fused, chains) of the last phase-A launch: render in the primary rays' launch? chain streams in turn (0: synchronous)."""
        a, b = C.c_int(), C.c_int()
        check(lib().rs_restir_last_launch(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_primary_cuts(self, on=True):
        """rs_restir_set_primary_cuts: still-camera primary rays walk per-block cuts of the BVH (on by default)."""
        check(lib().rs_restir_set_primary_cuts(self.handle, 1 if on else 0))

    def set_primary_cut_cap(self, records):
        """rs_debug_set_primary_cut_cap: the most records one block's cut may have."""
        check(lib().rs_debug_set_primary_cut_cap(self.handle, records))

    def primary_cut_info(self):
        """dict(cells, without_cut, records, used, builds) of the last phase-A call's cuts (rs_debug_primary_cut_info)."""
        a, b, u = C.c_int(), C.c_int(), C.c_int()
        n, k = C.c_ulonglong(), C.c_ulonglong()
        check(lib().rs_debug_primary_cut_info(self.handle, C.byref(a), C.byref(b), C.byref(n), C.byref(u), C.byref(k)))
        return dict(cells=a.value, without_cut=b.value, records=n.value, used=bool(u.value), builds=k.value)

    def primary_cut_missing(self, scene, cell, rays):
        """rs_debug_primary_cut_missing: rays = (n, 4) float32 { pixel x, pixel y, jitter x, jitter y }; returns dict(missing, passed,
        left_out, records) for block `cell`."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 4)
        out = (C.c_ulonglong * 4)()
        check(lib().rs_debug_primary_cut_missing(self.handle, scene.handle, cell, len(rays), _p(rays), C.byref(out)))
        return dict(missing=out[0], passed=out[1], left_out=out[2], records=out[3])

    def set_primary_leaf_lists(self, on=True):
        """rs_restir_set_primary_leaf_lists: whole tiles of such a launch walk the leaf lists of their own 8x8 pixels (on by default)."""
        check(lib().rs_restir_set_primary_leaf_lists(self.handle, 1 if on else 0))

    def set_shadow_regroup(self, on=True):
        """rs_restir_set_shadow_regroup: the shadow-ray kernel hands a block's segments out to its waves by length (on by default)."""
        check(lib().rs_restir_set_shadow_regroup(self.handle, 1 if on else 0))

    def shadow_pass(self, scene, pos_tag, cand_li, cand_wi, rows=None):
        """rs_debug_shadow_pass: the shadow-ray pass alone, in the form the switch chooses, over (n, 4) f32 planes { position, tag bits },
        { Li, dist }, { wi, weight }.  Returns (cand_wi after the pass, slots (n,) i32: -1 without a segment or under the plain form, shadow_bin's scale
        for the scene: 0 without the shadow tree)."""
        n = self.width * self.height
        y0, y1 = rows or (0, self.height)
        a, b = np.ascontiguousarray(pos_tag, np.float32).reshape(n, 4), np.ascontiguousarray(cand_li, np.float32).reshape(n, 4)
        w, slots, k = np.array(cand_wi, np.float32).reshape(n, 4).copy(), np.zeros(n, np.int32), C.c_float()
        check(lib().rs_debug_shadow_pass(self.handle, scene.handle, y0, y1, _p(a), _p(b), _p(w), _p(slots), C.byref(k)))
        return w, slots, k.value

    def set_primary_leaf_list_cap(self, records):
        """rs_debug_set_primary_leaf_list_cap: the most records one tile's leaf list may have (0: no tile takes a list)."""
        check(lib().rs_debug_set_primary_leaf_list_cap(self.handle, records))

    def primary_leaf_list_info(self):
        """dict(tiles, without_list, records, used, builds) of the last phase-A call's leaf lists (rs_debug_primary_leaf_list_info)."""
        a, b, u = C.c_int(), C.c_int(), C.c_int()
        n, k = C.c_ulonglong(), C.c_ulonglong()
        check(lib().rs_debug_primary_leaf_list_info(self.handle, C.byref(a), C.byref(b), C.byref(n), C.byref(u), C.byref(k)))
        return dict(tiles=a.value, without_list=b.value, records=n.value, used=bool(u.value), builds=k.value)

    def primary_leaf_list_missing(self, scene, rays):
        """rs_debug_primary_leaf_list_missing: rays = (n, 4) float32 { pixel x, pixel y, jitter x, jitter y }, each looked up in its own
        tile's list; returns dict(missing, passed, left_out)."""
        rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 4)
        out = (C.c_ulonglong * 4)()
        check(lib().rs_debug_primary_leaf_list_missing(self.handle, scene.handle, len(rays), _p(rays), C.byref(out)))
        return dict(missing=out[0], passed=out[1], left_out=out[2])

    def surface(self):
        """rs_debug_restir_surface: (pos_tag (n, 4) f32, normal (n, 4) f32, rng_tag (n, 2) u32) of the last ended frame."""
        n = self.width * self.height
        a, b, c = np.zeros((n, 4), np.float32), np.zeros((n, 4), np.float32), np.zeros((n, 2), np.uint32)
        check(lib().rs_debug_restir_surface(self.handle, _p(a), _p(b), _p(c)))
        return a, b, c

    def surface_wo(self):
        """rs_debug_restir_surface_wo: the (n, 4) f32 plane { wo, roughness } beside surface()'s; only MetallicWorkflow pixels wrote it."""
        out = np.zeros((self.width * self.height, 4), np.float32)
        check(lib().rs_debug_restir_surface_wo(self.handle, _p(out)))
        return out

    def launch_choice(self):
        """0 two launches, 1 GBuffer::render walked together with the primary rays, -1 still measuring, -2 nothing to choose."""
        c = C.c_int(-1)
        check(lib().rs_restir_launch_choice(self.handle, C.byref(c)))
        return c.value

    def halo_bytes(self, rows):
        return int(lib().rs_restir_halo_bytes(self.handle, rows))

    def halo_pack(self, y0, rows, dev_ptr):
        check(lib().rs_restir_halo_pack(self.handle, y0, rows, dev_ptr))

    def halo_unpack(self, y0, rows, dev_ptr):
        check(lib().rs_restir_halo_unpack(self.handle, y0, rows, dev_ptr))

    def rows_bytes(self, which, rows):
        return int(lib().rs_restir_rows_bytes(self.handle, which, rows))

    def rows_pack(self, which, y0, rows, dev_ptr):
        check(lib().rs_restir_rows_pack(self.handle, which, y0, rows, dev_ptr))

    def rows_unpack(self, which, y0, rows, dev_ptr):
        check(lib().rs_restir_rows_unpack(self.handle, which, y0, rows, dev_ptr))

    def download(self, which):
        out = np.zeros(self.width * self.height, RESERVOIR_DTYPE)
        check(lib().rs_restir_download(self.handle, which, _p(out)))
        return out

    def upload(self, which, arr):
        arr = np.ascontiguousarray(arr, RESERVOIR_DTYPE)
        check(lib().rs_restir_upload(self.handle, which, _p(arr)))

    def set_light_tracking(self, on=True):
        """rs_restir_set_light_tracking: re-evaluate the temporal candidate under the scene's current emission (off by default)."""
        check(lib().rs_restir_set_light_tracking(self.handle, 1 if on else 0))

    def download_light_ids(self, which):
        """Light-sampler index of every reservoir's sample (which: 0 or 1 as download); -1 = none / unknown."""
        out = np.zeros(self.width * self.height, np.int32)
        check(lib().rs_restir_download_light_ids(self.handle, which, _p(out)))
        return out

    def set_light_retargeting(self, on=True):
        """rs_restir_set_light_retargeting: temporal candidates of lamps moved since the previous frame are evaluated again (switches
        tracking on too; set_light_tracking(False) switches both off)."""
        check(lib().rs_restir_set_light_retargeting(self.handle, 1 if on else 0))

    def get_light_retargeting(self):
        on = C.c_int(0)
        check(lib().rs_restir_get_light_retargeting(self.handle, C.byref(on)))
        return bool(on.value)

    def download_light_samples(self, which):
        """rs_restir_download_light_samples: LIGHT_SAMPLE_DTYPE record of every reservoir's sample (which as download); light -1 = none / unknown."""
        out = np.zeros(self.width * self.height, LIGHT_SAMPLE_DTYPE)
        check(lib().rs_restir_download_light_samples(self.handle, which, _p(out)))
        return out

    def retarget_stats(self):
        """rs_debug_restir_retarget: (samples evaluated again, shadow segments walked, samples left with W = 0) of the last ended frame."""
        out = (C.c_ulonglong * 3)()
        check(lib().rs_debug_restir_retarget(self.handle, C.byref(out)))
        return tuple(int(x) for x in out)

    def retarget_launched(self):
        """rs_debug_restir_retarget_launched: did the last ended frame launch the retargeting kernel?"""
        on = C.c_int(0)
        check(lib().rs_debug_restir_retarget_launched(self.handle, C.byref(on)))
        return bool(on.value)

    def set_shadow_revalidation(self, on=True):
        """rs_restir_set_shadow_revalidation: after a geometry edit, temporal candidates whose shadow segment crosses the edit's box are
        walked again before the merge; an occluded one merges as W = 0."""
        check(lib().rs_restir_set_shadow_revalidation(self.handle, 1 if on else 0))

    def get_shadow_revalidation(self):
        on = C.c_int(0)
        check(lib().rs_restir_get_shadow_revalidation(self.handle, C.byref(on)))
        return bool(on.value)

    def revalidate_stats(self):
        """rs_debug_restir_revalidate: (candidates examined, segments walked, candidates found occluded) of the last ended frame."""
        out = (C.c_ulonglong * 3)()
        check(lib().rs_debug_restir_revalidate(self.handle, C.byref(out)))
        return tuple(int(x) for x in out)

    def revalidate_launched(self):
        """rs_debug_restir_revalidate_launched: did the last ended frame launch the revalidation kernel?"""
        on = C.c_int(0)
        check(lib().rs_debug_restir_revalidate_launched(self.handle, C.byref(on)))
        return bool(on.value)

    def set_indirect_revalidation(self, on=True):
        """rs_restir_set_indirect_revalidation: after a geometry edit, the ReSTIR-GI history slots whose sample point lies in the edit's
        box, or whose segment xv -> xs crosses it and is blocked now, are emptied before rs_restir_indirect merges them."""
        check(lib().rs_restir_set_indirect_revalidation(self.handle, 1 if on else 0))

    def get_indirect_revalidation(self):
        on = C.c_int(0)
        check(lib().rs_restir_get_indirect_revalidation(self.handle, C.byref(on)))
        return bool(on.value)

    def indirect_revalidate_stats(self):
        """rs_debug_restir_indirect_revalidate: (slots examined, found stale, segments walked, walkers found occluded) of the last
        rs_restir_indirect call."""
        out = (C.c_ulonglong * 4)()
        check(lib().rs_debug_restir_indirect_revalidate(self.handle, C.byref(out)))
        return tuple(int(x) for x in out)

    def indirect_revalidate_launched(self):
        """rs_debug_restir_indirect_revalidate_launched: did the last rs_restir_indirect call launch the revalidation kernel?"""
        on = C.c_int(0)
        check(lib().rs_debug_restir_indirect_revalidate_launched(self.handle, C.byref(on)))
        return bool(on.value)

    def set_indirect_spatial(self, on=True, taps=0, radius=0.0):
        """rs_restir_set_indirect_spatial: rs_restir_indirect calls with reuse & 2 merge up to 16 neighbours' GI reservoirs into every
        pixel's (reconnection shift with its Jacobian), test the winner's visibility and shade that; taps / radius <= 0: 5 and 5.0."""
        check(lib().rs_restir_set_indirect_spatial(self.handle, 1 if on else 0, int(taps), float(radius)))

    def get_indirect_spatial(self):
        """(enabled, taps, radius)"""
        on, taps, radius = C.c_int(0), C.c_int(0), C.c_float(0)
        check(lib().rs_restir_get_indirect_spatial(self.handle, C.byref(on), C.byref(taps), C.byref(radius)))
        return bool(on.value), int(taps.value), float(radius.value)

    def download_indirect_spatial(self):
        """devIndSpatialReservoir of the last rs_restir_indirect call that ran the pass."""
        out = np.zeros(self.width * self.height, INDIRECT_RESERVOIR_DTYPE)
        check(lib().rs_restir_download_indirect_spatial(self.handle, _p(out)))
        return out

    def indirect_spatial_stats(self):
        """rs_debug_restir_indirect_spatial: (taking part, accepted, failed the neighbour test, ns == 0, Jacobian, horizon, walked, blocked)
        of the last rs_restir_indirect call."""
        out = (C.c_ulonglong * 8)()
        check(lib().rs_debug_restir_indirect_spatial(self.handle, C.byref(out)))
        return tuple(int(x) for x in out)

    def indirect_spatial_launched(self):
        on = C.c_int(0)
        check(lib().rs_debug_restir_indirect_spatial_launched(self.handle, C.byref(on)))
        return bool(on.value)

    def record_indirect_primary(self):
        """rs_debug_restir_indirect_primary with null outputs: from now on the pass records the receiver's surface."""
        check(lib().rs_debug_restir_indirect_primary(self.handle, None, None, None, None))

    def indirect_primary(self):
        """rs_debug_restir_indirect_primary: (xv (n, 3), nv (n, 3), wo (n, 3), material id (n,), -1 where the pixel does not take part) of
        the last call that ran the pass, after record_indirect_primary()."""
        n = self.width * self.height
        xv, nv, wo = (np.zeros((n, 4), np.float32) for _ in range(3))
        mat = np.zeros(n, np.int32)
        check(lib().rs_debug_restir_indirect_primary(self.handle, _p(xv), _p(nv), _p(wo), _p(mat)))
        return xv[:, :3].copy(), nv[:, :3].copy(), wo[:, :3].copy(), mat

    def light_rows_bytes(self, rows):
        return int(lib().rs_restir_light_rows_bytes(self.handle, rows))

    def light_rows_pack(self, which, y0, rows, dev_ptr):
        """Rows of the id plane of reservoir buffer `which` (as download_light_ids), 4 B/px; refused while tracking is off."""
        check(lib().rs_restir_light_rows_pack(self.handle, which, y0, rows, dev_ptr))

    def light_rows_unpack(self, which, y0, rows, dev_ptr):
        check(lib().rs_restir_light_rows_unpack(self.handle, which, y0, rows, dev_ptr))

    def ray_count(self):
        n = C.c_ulonglong(0)
        check(lib().rs_restir_ray_count(self.handle, C.byref(n)))
        return n.value

    def ray_total(self, frames):
        n = C.c_ulonglong(0)
        check(lib().rs_restir_ray_total(self.handle, frames, C.byref(n)))
        return n.value

    def enable_timing(self, on=True):
        """True / 1: every pass bracketed, kernels on the library stream; 2: the spatial pass only, launches as in the overlapped mode."""
        check(lib().rs_restir_enable_timing(self.handle, 2 if on == 2 else (1 if on else 0)))

    def pass_times(self):
        ms = (C.c_float * 4)()
        check(lib().rs_restir_pass_times(self.handle, C.byref(ms)))
        return [float(x) for x in ms]

    def spatial_times(self, capacity=256):
        """enable_timing(2): the spatial pass's duration (ms) in each of the last frames, oldest first (rs_restir_spatial_times)."""
        ms = (C.c_float * capacity)()
        n = C.c_int(0)
        check(lib().rs_restir_spatial_times(self.handle, ms, capacity, C.byref(n)))
        return [float(ms[i]) for i in range(n.value)]

    def set_probe(self, on):
        """The spatial pass under the name k_spatial_shade_probe (a measurement's own launches; rs_restir_set_probe)."""
        check(lib().rs_restir_set_probe(self.handle, 1 if on else 0))

    def destroy(self):
        if self.handle:
            lib().rs_restir_free(self.handle)
            self.handle = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


class Comm:
    """rs_comm: the exchange of the strip driver.  Comm.rccl(nccl_comm_ptr, rank, world) wraps an ncclComm_t; Comm(callbacks...)
    takes host callbacks send(dev_ptr, nbytes, peer) / recv(dev_ptr, nbytes, peer) / group_begin() / group_end() (tests)."""

    def __init__(self, rank, world, send, recv, group_begin=None, group_end=None, stream_ordered=False):
        def guard(fn):
            def call(*a):
                try:
                    fn(*a)
                    return 0
                except Exception as e:                      # an exception must not cross the C frame
                    print("transport callback failed:", repr(e), flush=True)
                    return RS_ERR_UNSUPPORTED
            return call
        self._cbs = (TRANSPORT_GROUP(guard(lambda ctx: group_begin() if group_begin else None)),
                     TRANSPORT_SEND(guard(lambda ctx, p, n, peer, st: send(p, n, peer))),
                     TRANSPORT_RECV(guard(lambda ctx, p, n, peer, st: recv(p, n, peer))),
                     TRANSPORT_GROUP(guard(lambda ctx: group_end() if group_end else None)))
        t = Transport(None, self._cbs[0], self._cbs[1], self._cbs[2], self._cbs[3], 1 if stream_ordered else 0)
        self.handle = C.c_void_p()
        check(lib().rs_comm_create(C.byref(t), rank, world, C.byref(self.handle)))

    @classmethod
    def rccl(cls, nccl_comm_ptr, rank, world, librccl_path=None):
        """librccl_path: the copy of RCCL that created the communicator (None: the library searches, rs_comm_create_rccl)."""
        self = cls.__new__(cls)
        self._cbs = ()
        self.handle = C.c_void_p()
        check(lib().rs_comm_create_rccl_lib(C.c_void_p(nccl_comm_ptr), rank, world, os.fsencode(librccl_path) if librccl_path else None, C.byref(self.handle)))
        return self

    def destroy(self):
        if self.handle:
            lib().rs_comm_destroy(self.handle)
            self.handle = C.c_void_p()


class Strips:
    """rs_strips: the row-strip frame of one rank (include/restir_hip.h), the C form of tiling.StripRenderer."""

    def __init__(self, comm, width, height, bounds=None):
        self.comm = comm
        self.handle = C.c_void_p()
        b = (C.c_int * len(bounds))(*bounds) if bounds is not None else None
        check(lib().rs_strips_create(comm.handle, width, height, b, C.byref(self.handle)))
        y0, y1 = C.c_int(), C.c_int()
        check(lib().rs_strips_rows(self.handle, C.byref(y0), C.byref(y1)))
        self.y0, self.y1 = y0.value, y1.value

    def set_comm_stream(self, own_stream):
        """Stream-ordered transports: transfers on the library stream (False, default) or on a stream of the driver (True)."""
        check(lib().rs_strips_set_comm_stream(self.handle, 1 if own_stream else 0))

    def set_gbuffer_halo(self, rows):
        """G-buffer rows that travel with the reservoir rows of a frame: 5 (default), or 32 when a denoiser follows (rs_strips_set_gbuffer_halo)."""
        check(lib().rs_strips_set_gbuffer_halo(self.handle, int(rows)))

    def set_light_tracking(self, on=True):
        """The frames take a tracked ReSTIR and the history messages carry its light ids (rs_strips_set_light_tracking); the same on every rank."""
        check(lib().rs_strips_set_light_tracking(self.handle, 1 if on else 0))

    def frame(self, restir, scene, cam, gbuf, dev_direct_illum_ptr, iter_, looper, reuse):
        check(lib().rs_strips_frame(self.handle, restir.handle, scene.handle, C.byref(cam), gbuf.handle, dev_direct_illum_ptr, iter_, looper, reuse))

    def eaw_filter(self, eaw, gbuf, cam, dev_color_ptr):
        """LeveledEAWFilter on the strip (before GBuffer.update); returns the device pointer of the driver's result buffer."""
        p = C.c_void_p()
        check(lib().rs_strips_eaw_filter(self.handle, eaw.handle, gbuf.handle, C.byref(cam), dev_color_ptr, C.byref(p)))
        return p.value

    def svgf_filter(self, svgf, gbuf, cam, dev_color_ptr):
        """SpatioTemporalFilter on the strip (before GBuffer.update); `svgf` is a capi.SVGFFilter, whose out pointer is handed over as
        by its own filter(); returns the device pointer of the filtered image (rows of this strip valid)."""
        p = C.c_void_p(svgf.out_ptr)
        check(lib().rs_strips_svgf_filter(self.handle, svgf.handle, gbuf.handle, C.byref(cam), dev_color_ptr, C.byref(p)))
        svgf.out_ptr = p.value
        return svgf.out_ptr

    def exchange_svgf_history(self, svgf):
        """Moving camera: after svgf_filter and before svgf.next_frame(), the filter's history rows travel to every other rank."""
        check(lib().rs_strips_exchange_svgf_history(self.handle, svgf.handle))

    def exchange_history(self, restir, gbuf):
        """Moving camera: after GBuffer.update, every rank's history rows travel to every other rank."""
        check(lib().rs_strips_exchange_history(self.handle, restir.handle, gbuf.handle))

    def gather(self, dev_image_ptr, bytes_per_pixel, root=-1):
        check(lib().rs_strips_gather(self.handle, dev_image_ptr, bytes_per_pixel, root))

    def gather_begin(self, dev_image_ptr, bytes_per_pixel, root, slot):
        check(lib().rs_strips_gather_begin(self.handle, dev_image_ptr, bytes_per_pixel, root, slot))

    def gather_end(self, slot):
        check(lib().rs_strips_gather_end(self.handle, slot))

    def enable_timing(self, enable=True):
        check(lib().rs_strips_enable_timing(self.handle, 1 if enable else 0))

    def halo_wait_ms(self):
        ms = C.c_float(0)
        check(lib().rs_strips_halo_wait_ms(self.handle, C.byref(ms)))
        return ms.value

    def destroy(self):
        if self.handle:
            lib().rs_strips_destroy(self.handle)
            self.handle = C.c_void_p()


class EAWFilter:
    """LeveledEAWFilter (src/denoiser.h:33-43)."""

    def __init__(self, width, height, level=5):
        self.handle = C.c_void_p()
        check(lib().rs_eaw_create(width, height, level, C.byref(self.handle)))

    def filter(self, out_ptr, in_ptr, gbuf, cam):
        """Returns the device pointer that holds the result (the reference swaps the caller's pointer)."""
        p = C.c_void_p(out_ptr)
        check(lib().rs_eaw_filter(self.handle, C.byref(p), in_ptr, gbuf.handle, C.byref(cam)))
        return p.value

    def set_params(self, sig_lumin, sig_normal, sig_depth, level=5):
        """waveletFilter.sigLumin / sigNormal / sigDepth and level, the members the viewer edits (src/preview.cpp:262-265)."""
        check(lib().rs_eaw_set_params(self.handle, sig_lumin, sig_normal, sig_depth, level))

    def set_tiled(self, tiled):
        """Levels of step 1, 2, 4 from an LDS tile (default) or as plain gathers; same bits."""
        check(lib().rs_eaw_set_tiled(self.handle, int(bool(tiled))))

    def set_fused(self, fused):
        """Taps in fused arithmetic (1, the library's default) or every operation rounded separately in the reference's order (0)."""
        check(lib().rs_eaw_set_fused(self.handle, int(bool(fused))))

    def get_params(self):
        a, b, c, lv = C.c_float(), C.c_float(), C.c_float(), C.c_int()
        check(lib().rs_eaw_get_params(self.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(lv)))
        return a.value, b.value, c.value, lv.value

    def positions_rows(self, gbuf, cam, y0, y1):
        check(lib().rs_eaw_positions_rows(self.handle, gbuf.handle, C.byref(cam), y0, y1))

    def level_rows(self, out_ptr, in_ptr, gbuf, level, y0, y1):
        check(lib().rs_eaw_level_rows(self.handle, out_ptr, in_ptr, gbuf.handle, level, y0, y1))

    def destroy(self):
        if self.handle:
            lib().rs_eaw_destroy(self.handle)
            self.handle = C.c_void_p()


class SVGFFilter:
    """SpatioTemporalFilter (src/denoiser.h:45-70).  The caller-side `devColorOut` buffer of the reference is kept
    here: it comes from hipMalloc and is swapped with the filter's buffers by every call, as in the reference."""

    def __init__(self, width, height, level=5):
        self.n = width * height
        self.handle = C.c_void_p()
        check(lib().rs_svgf_create(width, height, level, C.byref(self.handle)))
        self.out_ptr = hip_malloc(self.n * 12)

    def filter(self, in_ptr, gbuf, cam):
        """Returns the device pointer that holds the filtered image."""
        p = C.c_void_p(self.out_ptr)
        check(lib().rs_svgf_filter(self.handle, C.byref(p), in_ptr, gbuf.handle, C.byref(cam)))
        self.out_ptr = p.value
        return self.out_ptr

    def set_params(self, sig_lumin, sig_normal, sig_depth, level=5):
        """waveletFilter.sig* and level of SpatioTemporalFilter (src/preview.cpp:278-286)."""
        check(lib().rs_svgf_set_params(self.handle, sig_lumin, sig_normal, sig_depth, level))

    def get_params(self):
        a, b, c, lv = C.c_float(), C.c_float(), C.c_float(), C.c_int()
        check(lib().rs_svgf_get_params(self.handle, C.byref(a), C.byref(b), C.byref(c), C.byref(lv)))
        return a.value, b.value, c.value, lv.value

    def set_tiled(self, tiled):
        """a-trous levels from the LDS tile (True, default) or as plain gathers (False): same bits."""
        check(lib().rs_svgf_set_tiled(self.handle, 1 if tiled else 0))

    def set_fused(self, fused):
        """Taps in fused arithmetic (True) or every operation rounded separately in the reference's order (False)."""
        check(lib().rs_svgf_set_fused(self.handle, 1 if fused else 0))

    def next_frame(self):
        check(lib().rs_svgf_next_frame(self.handle))

    def view(self):
        v = SVGFView()
        check(lib().rs_svgf_get_view(self.handle, C.byref(v)))
        return v

    def destroy(self):
        if self.handle:
            lib().rs_svgf_destroy(self.handle)
            hip_free(self.out_ptr)
            self.handle = C.c_void_p()


def path_trace(scene, cam, dev_direct_ptr, dev_indirect_ptr, iter_, looper, max_depth):
    n = C.c_ulonglong(0)
    check(lib().rs_path_trace(scene.handle, C.byref(cam), dev_direct_ptr, dev_indirect_ptr, iter_, looper, max_depth, C.byref(n)))
    return n.value


def path_trace_indirect(scene, cam, dev_indirect_ptr, iter_, looper, max_depth):
    n = C.c_ulonglong(0)
    check(lib().rs_path_trace_indirect(scene.handle, C.byref(cam), dev_indirect_ptr, iter_, looper, max_depth, C.byref(n)))
    return n.value


def path_trace_direct(scene, cam, dev_direct_illum_ptr, iter_, looper):
    n = C.c_ulonglong(0)
    check(lib().rs_path_trace_direct(scene.handle, C.byref(cam), dev_direct_illum_ptr, iter_, looper, C.byref(n)))
    return n.value


def copy_image_to_pbo(dev_pbo_ptr, dev_image_ptr, width, height, tone_mapping, scale=1.0):
    check(lib().rs_copy_image_to_pbo(dev_pbo_ptr, dev_image_ptr, width, height, tone_mapping, scale))


def copy_debug_image_to_pbo(dev_pbo_ptr, dev_image_ptr, width, height, kind):
    """The vec2 (kind 0) / float (1) / int (2) overloads of copyImageToPBO."""
    fn = (lib().rs_copy_image2_to_pbo, lib().rs_copy_imagef_to_pbo, lib().rs_copy_imagei_to_pbo)[kind]
    check(fn(dev_pbo_ptr, dev_image_ptr, width, height))


def trace_closest(scene, rays_t):
    """rays_t: torch float32 cuda tensor (n,6). Returns (primId, matId, pos, norm) torch tensors."""
    import torch
    n = rays_t.shape[0]
    prim = torch.empty(n, dtype=torch.int32, device="cuda"); mat = torch.empty(n, dtype=torch.int32, device="cuda")
    pos = torch.empty((n, 3), dtype=torch.float32, device="cuda"); nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    check(lib().rs_trace_closest(scene.handle, n, rays_t.data_ptr(), prim.data_ptr(), mat.data_ptr(), pos.data_ptr(), nrm.data_ptr()))
    return prim, mat, pos, nrm


def trace_closest_wave(scene, rays_t):
    """As trace_closest, through the wave-level service of the multi-bounce kernels (rs_trace_closest_wave)."""
    import torch
    n = rays_t.shape[0]
    prim = torch.empty(n, dtype=torch.int32, device="cuda"); mat = torch.empty(n, dtype=torch.int32, device="cuda")
    pos = torch.empty((n, 3), dtype=torch.float32, device="cuda"); nrm = torch.empty((n, 3), dtype=torch.float32, device="cuda")
    check(lib().rs_trace_closest_wave(scene.handle, n, rays_t.data_ptr(), prim.data_ptr(), mat.data_ptr(), pos.data_ptr(), nrm.data_ptr()))
    return prim, mat, pos, nrm


def set_ordered_tree(scene, on):
    """rs_scene_set_ordered_tree; returns whether the closest-hit trees were in use before the call."""
    import ctypes
    was = ctypes.c_int(0)
    check(lib().rs_scene_set_ordered_tree(scene.handle, 1 if on else 0, ctypes.byref(was)))
    return bool(was.value)


def trace_occlusion(scene, seg_t):
    import torch
    n = seg_t.shape[0]
    occ = torch.empty(n, dtype=torch.int32, device="cuda")
    check(lib().rs_trace_occlusion(scene.handle, n, seg_t.data_ptr(), occ.data_ptr()))
    return occ
