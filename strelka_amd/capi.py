"""ctypes binding of the C ABI in include/strelka_hip.h (libstrelka_hip.so, HIP / gfx950).

This is the only way Python reaches the renderer: there is NO CPU fallback.  Loading fails loudly when the library
has not been built (strelka_amd.build) and skh_create fails loudly when no GPU is visible.
"""
import ctypes as C
import os

import numpy as np

from . import scene as S
from .build import LIB

_lib = None

STATS = np.dtype([("rays_radiance", np.uint64), ("rays_shadow", np.uint64), ("nodes_visited", np.uint64, 2),
                  ("prims_tested", np.uint64, 2), ("segs_tested", np.uint64, 2), ("instances_entered", np.uint64, 2),
                  ("ms_trace_closest", np.float64), ("ms_trace_shadow", np.float64), ("ms_shade", np.float64),
                  ("ms_raygen", np.float64), ("ms_accumulate", np.float64), ("ms_build", np.float64), ("ms_sort", np.float64),
                  ("launches_trace_closest", np.uint32), ("launches_trace_shadow", np.uint32),
                  ("launches_shade", np.uint32), ("launches_other", np.uint32), ("stack_overflows", np.uint32),
                  ("speculated_discarded", np.uint32)])

SYMBOLS = ["skh_create", "skh_destroy", "skh_last_error", "skh_abi_version", "skh_set_geometry", "skh_set_curves",
           "skh_set_instances", "skh_set_lights", "skh_set_textures", "skh_set_materials", "skh_build_accel", "skh_resize", "skh_set_tiles",
           "skh_render_subframe", "skh_render_subframes", "skh_tonemap", "skh_read_accum", "skh_read_aov",
           "skh_buffer_alloc", "skh_buffer_free", "skh_buffer_download", "skh_copy_accum", "skh_copy_accum_tiles", "skh_scatter_tiles", "skh_trace", "skh_trace_device",
           "skh_set_option", "skh_get_stats", "skh_reset_stats", "skh_synchronize", "skh_get_stream", "skh_bsdf_probe", "skh_get_device_info", "skh_comm_unique_id", "skh_comm_init",
           "skh_comm_destroy", "skh_gather_tiles", "skh_host_register", "skh_host_unregister", "skh_get_baked", "skh_comm_info", "skh_probe_memory", "skh_unit_probe", "skh_copy_aov", "skh_get_build_info", "skh_refit_accel",
           "skh_update_accel", "skh_set_environment", "skh_set_environment_transform", "skh_get_environment_info",
           "skh_set_emission", "skh_get_emitter_info", "skh_emitter_probe",
           "skh_set_material_textures", "skh_material_probe", "skh_set_material_cutouts", "skh_get_cutout_info",
           "skh_set_material_blend", "skh_get_blend_info", "skh_blend_probe",
           "skh_set_light_shapes", "skh_get_light_shape_info", "skh_light_shape_probe",
           "skh_adaptive_check", "skh_set_adaptive", "skh_get_adaptive_info", "skh_read_adaptive",
           "skh_aov_check", "skh_render_aovs", "skh_get_aov_info",
           "skh_denoise_check", "skh_denoise", "skh_get_denoise_info", "skh_buffer_upload",
           "skh_temporal_check", "skh_temporal", "skh_get_temporal_info",
           "skh_moments", "skh_get_moments_info", "skh_vdenoise_check", "skh_denoise_variance", "skh_get_vdenoise_info",
           "skh_instance_motion_from_transforms", "skh_instance_motion_check", "skh_set_instance_motion", "skh_rewind_guides", "skh_get_rewind_info",
           "skh_rectify_check", "skh_rectify", "skh_get_rectify_info"]

BUILD_INFO = np.dtype([("triangles", np.uint32), ("nodes", np.uint32), ("reinsert_rounds", np.uint32), ("reinsert_moves", np.uint32),
                       ("reinsert_min_size", np.uint32), ("refit", np.uint32), ("cost_before", np.float64), ("cost_after", np.float64),
                       ("ms_reinsert", np.float64), ("ms_build", np.float64), ("ms_refit", np.float64)])
DEVICE_INFO = np.dtype([("compute_units", np.uint32), ("simds_per_cu", np.uint32), ("clock_khz", np.uint32), ("memory_clock_khz", np.uint32),
                        ("memory_bus_bits", np.uint32), ("wavefront_size", np.uint32), ("total_memory_bytes", np.uint64), ("name", "S64")])

ENVIRONMENT_INFO = np.dtype([("width", np.uint32), ("height", np.uint32), ("sum_w", np.float64), ("ms_build", np.float64), ("bytes", np.uint64)])
CUTOUT_INFO = np.dtype([("active_materials", np.uint32), ("instances", np.uint32), ("continued_closest", np.uint64), ("continued_shadow", np.uint64),
                        ("accepted_by_cap", np.uint64), ("bytes", np.uint64)])
BLEND_INFO = np.dtype([("active_materials", np.uint32), ("instances", np.uint32), ("passed_radiance", np.uint64), ("crossed_shadow", np.uint64),
                       ("accepted_by_cap", np.uint64), ("bytes", np.uint64)])
EMITTER_INFO = np.dtype([("triangles", np.uint32), ("instances", np.uint32), ("sum_w", np.float64), ("ms_build", np.float64), ("bytes", np.uint64)])
LIGHT_SHAPE_INFO = np.dtype([("sampled_discs", np.uint32), ("cones", np.uint32)])
ADAPTIVE = np.dtype([("threshold", np.float32), ("dark_level", np.float32), ("min_samples", np.uint32), ("interval", np.uint32), ("reserved", np.uint32, 4)])
ADAPTIVE_INFO = np.dtype([("enabled", np.uint32), ("tiles", np.uint32), ("active_tiles", np.uint32), ("checks", np.uint32), ("min_observations", np.uint32),
                          ("max_observations", np.uint32), ("pixel_observations", np.uint64), ("pixel_observations_saved", np.uint64)])
assert ADAPTIVE.itemsize == 32 and ADAPTIVE_INFO.itemsize == 40
AOV_INFO = np.dtype([("calls", np.uint64), ("rays", np.uint64), ("ms_last", np.float64), ("bytes_last", np.uint64)])
assert AOV_INFO.itemsize == 32
DENOISE_INFO = np.dtype([("calls", np.uint64), ("pixels", np.uint64), ("ms_last", np.float64), ("scratch_bytes", np.uint64)])
assert DENOISE_INFO.itemsize == 32
DENOISE_GUIDES = ("ids", "normal", "position", "albedo")  # the planes skh_denoise reads, in its argument order
TEMPORAL_INFO = np.dtype([("calls", np.uint64), ("pixels", np.uint64), ("ms_last", np.float64)])
assert TEMPORAL_INFO.itemsize == 24
TEMPORAL_PREV = ("history", "ids", "normal", "position")  # the previous-frame images skh_temporal reads, in its argument order
MOMENTS_INFO = np.dtype([("calls", np.uint64), ("pixels", np.uint64), ("ms_last", np.float64)])
assert MOMENTS_INFO.itemsize == 24
VDENOISE_INFO = np.dtype([("calls", np.uint64), ("pixels", np.uint64), ("ms_last", np.float64), ("scratch_bytes", np.uint64)])
assert VDENOISE_INFO.itemsize == 32
REWIND_INFO = np.dtype([("calls", np.uint64), ("pixels", np.uint64), ("ms_last", np.float64), ("entries", np.uint64)])
assert REWIND_INFO.itemsize == 32
RECTIFY_INFO = np.dtype([("calls", np.uint64), ("pixels", np.uint64), ("ms_last", np.float64)])
assert RECTIFY_INFO.itemsize == 24
# skh_light_shape_probe: kind -> (number, words in, words out) per record
LSHAPE_PROBES = {"sample": (0, 6, 13), "pdf": (1, 7, 2)}
# skh_emitter_probe: kind -> (number, words in, words out) per record
EMIT_PROBES = {"sample": (0, 6, 13), "pdf": (1, 8, 4)}


class SkhEnvironment(C.Structure):  # skh_environment
    _fields_ = [("rgb", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32), ("scale", C.c_float * 3), ("world_to_env", C.c_float * 9)]


BSDF_QUERY = np.dtype([("normal", np.float32, 3), ("geom_normal", np.float32, 3), ("tangent_u", np.float32, 3), ("k1", np.float32, 3),
                       ("k2", np.float32, 3), ("xi", np.float32, 4), ("material", np.uint32), ("inside", np.uint32)])
BSDF_RESULT = np.dtype([("k2", np.float32, 3), ("bsdf_over_pdf", np.float32, 3), ("pdf", np.float32), ("event_type", np.int32),
                        ("bsdf_diffuse", np.float32, 3), ("bsdf_glossy", np.float32, 3), ("eval_pdf", np.float32), ("reserved0", np.uint32)])
assert BSDF_QUERY.itemsize == 84 and BSDF_RESULT.itemsize == 64


class SkhError(RuntimeError):
    pass


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB):
        raise SkhError(f"{LIB} is missing: build it with `python -m strelka_amd.build` (hipcc, gfx950). "
                       "There is no CPU fallback.")
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64; when torch is used in the same process
    # (device tensors for d_image, torch.distributed/RCCL) it must be the copy that gets loaded first, otherwise
    # torch later reports "No HIP GPUs are available".  torch is plumbing here, not a dependency of the kernels.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB)
    vp, u32, i32, f32 = C.c_void_p, C.c_uint32, C.c_int, C.c_float
    lib.skh_create.argtypes = [i32, C.POINTER(vp)]
    lib.skh_destroy.argtypes = [vp]
    lib.skh_destroy.restype = None
    lib.skh_last_error.argtypes = [vp]
    lib.skh_last_error.restype = C.c_char_p
    lib.skh_abi_version.restype = u32
    lib.skh_set_geometry.argtypes = [vp, vp, u32, vp, u32, vp, u32]
    lib.skh_set_curves.argtypes = [vp, vp, u32, vp, u32, vp, u32, vp, u32]
    for n in ("skh_set_instances", "skh_set_lights", "skh_set_textures", "skh_set_materials"):
        getattr(lib, n).argtypes = [vp, vp, u32]
    lib.skh_build_accel.argtypes = [vp, u32]
    lib.skh_refit_accel.argtypes = [vp]
    lib.skh_update_accel.argtypes = [vp, vp, u32]
    lib.skh_set_environment.argtypes = [vp, C.POINTER(SkhEnvironment)]
    lib.skh_set_environment_transform.argtypes = [vp, vp, vp]
    lib.skh_get_environment_info.argtypes = [vp, vp]
    lib.skh_set_emission.argtypes = [vp, vp, u32]
    lib.skh_get_emitter_info.argtypes = [vp, vp]
    lib.skh_emitter_probe.argtypes = [vp, u32, vp, u32, vp]
    lib.skh_set_material_textures.argtypes = [vp, vp, u32]
    lib.skh_material_probe.argtypes = [vp, u32, vp, vp, vp]
    lib.skh_set_material_cutouts.argtypes = [vp, vp, u32]
    lib.skh_get_cutout_info.argtypes = [vp, vp]
    lib.skh_set_material_blend.argtypes = [vp, vp, u32]
    lib.skh_get_blend_info.argtypes = [vp, vp]
    lib.skh_blend_probe.argtypes = [vp, u32, vp, vp]
    lib.skh_set_light_shapes.argtypes = [vp, vp, u32]
    lib.skh_get_light_shape_info.argtypes = [vp, vp]
    lib.skh_light_shape_probe.argtypes = [vp, u32, vp, u32, vp]
    lib.skh_adaptive_check.argtypes = [vp]
    lib.skh_set_adaptive.argtypes = [vp, vp]
    lib.skh_get_adaptive_info.argtypes = [vp, vp]
    lib.skh_read_adaptive.argtypes = [vp, vp]
    lib.skh_aov_check.argtypes = [vp, u32, u32]
    lib.skh_render_aovs.argtypes = [vp, vp, u32, vp]
    lib.skh_get_aov_info.argtypes = [vp, vp]
    lib.skh_denoise_check.argtypes = [vp]
    lib.skh_denoise.argtypes = [vp, vp, vp, vp, vp, vp, vp, vp]
    lib.skh_get_denoise_info.argtypes = [vp, vp]
    lib.skh_temporal_check.argtypes = [vp]
    lib.skh_temporal.argtypes = [vp] * 14
    lib.skh_get_temporal_info.argtypes = [vp, vp]
    lib.skh_moments.argtypes = [vp] * 9
    lib.skh_get_moments_info.argtypes = [vp, vp]
    lib.skh_vdenoise_check.argtypes = [vp]
    lib.skh_denoise_variance.argtypes = [vp] * 10
    lib.skh_get_vdenoise_info.argtypes = [vp, vp]
    lib.skh_instance_motion_from_transforms.argtypes = [vp, vp, vp]
    lib.skh_instance_motion_check.argtypes = [vp, u32]
    lib.skh_set_instance_motion.argtypes = [vp, vp, u32]
    lib.skh_rewind_guides.argtypes = [vp, u32, u32, vp, vp, vp, vp, vp]
    lib.skh_get_rewind_info.argtypes = [vp, vp]
    lib.skh_rectify_check.argtypes = [vp]
    lib.skh_rectify.argtypes = [vp] * 10
    lib.skh_get_rectify_info.argtypes = [vp, vp]
    lib.skh_buffer_upload.argtypes = [vp, vp, vp, C.c_size_t]
    lib.skh_resize.argtypes = [vp, u32, u32]
    lib.skh_set_tiles.argtypes = [vp, u32, vp, u32]
    lib.skh_render_subframe.argtypes = [vp, vp, vp]
    lib.skh_render_subframes.argtypes = [vp, vp, u32, vp]
    lib.skh_tonemap.argtypes = [vp, vp, u32, u32, u32, vp, f32]
    lib.skh_buffer_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.skh_buffer_free.argtypes = [vp, vp]
    lib.skh_buffer_download.argtypes = [vp, vp, vp, C.c_size_t]
    lib.skh_read_accum.argtypes = [vp, vp]
    lib.skh_read_aov.argtypes = [vp, u32, vp]
    lib.skh_copy_accum.argtypes = [vp, vp]
    lib.skh_copy_aov.argtypes = [vp, u32, vp]
    lib.skh_copy_accum_tiles.argtypes = [vp, vp]
    lib.skh_scatter_tiles.argtypes = [vp, vp, vp, u32, u32, vp, u32, u32]
    lib.skh_trace.argtypes = [vp, vp, u32, u32, vp]
    lib.skh_trace_device.argtypes = [vp, vp, u32, u32, vp, u32]
    lib.skh_bsdf_probe.argtypes = [vp, vp, u32, vp]
    lib.skh_unit_probe.argtypes = [vp, u32, u32, vp, vp, u32, vp]
    lib.skh_get_device_info.argtypes = [vp, vp]
    lib.skh_get_build_info.argtypes = [vp, vp]
    lib.skh_host_register.argtypes = [vp, vp, C.c_size_t]
    lib.skh_host_unregister.argtypes = [vp, vp]
    lib.skh_comm_unique_id.argtypes = [vp]
    lib.skh_comm_init.argtypes = [vp, vp, i32, i32]
    lib.skh_comm_destroy.argtypes = [vp]
    lib.skh_comm_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.skh_probe_memory.argtypes = [vp, u32, C.c_uint64, u32, u32, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    lib.skh_gather_tiles.argtypes = [vp, u32, vp, i32]
    lib.skh_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
    lib.skh_get_baked.argtypes = [vp, vp, u32, C.POINTER(u32), C.POINTER(u32)]
    lib.skh_get_stats.argtypes = [vp, vp]
    lib.skh_reset_stats.argtypes = [vp]
    lib.skh_synchronize.argtypes = [vp]
    lib.skh_get_stream.argtypes = [vp]
    lib.skh_get_stream.restype = vp
    for n in SYMBOLS:
        if n not in ("skh_destroy", "skh_last_error", "skh_abi_version", "skh_get_stream"):
            getattr(lib, n).restype = i32
    _lib = lib
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def adaptive_record(threshold, dark_level, min_samples, interval):
    """an skh_adaptive record (one ADAPTIVE element)"""
    a = np.zeros((), ADAPTIVE)
    a["threshold"], a["dark_level"], a["min_samples"], a["interval"] = threshold, dark_level, min_samples, interval
    return a


def aov_check(params, image_w, image_h):
    """skh_aov_check: would skh_render_aovs accept these S.AOV_PARAMS for an image of image_w x image_h?  (needs no context and no GPU)"""
    p = np.ascontiguousarray(params, dtype=S.AOV_PARAMS)
    return load().skh_aov_check(_p(p), int(image_w), int(image_h)) == 0


def denoise_check(params):
    """skh_denoise_check: would skh_denoise accept these S.DENOISE_PARAMS?  (needs no context and no GPU)"""
    p = np.ascontiguousarray(params, dtype=S.DENOISE_PARAMS)
    return load().skh_denoise_check(_p(p)) == 0


def temporal_check(params):
    """skh_temporal_check: would skh_temporal accept these S.TEMPORAL_PARAMS?  (needs no context and no GPU)"""
    p = np.ascontiguousarray(params, dtype=S.TEMPORAL_PARAMS)
    return load().skh_temporal_check(_p(p)) == 0


def rectify_check(params):
    """skh_rectify_check: would skh_rectify accept these S.RECTIFY_PARAMS?  (needs no context and no GPU)"""
    p = np.ascontiguousarray(params, dtype=S.RECTIFY_PARAMS)
    return load().skh_rectify_check(_p(p)) == 0


def moments_check(params):
    """would skh_moments accept these S.TEMPORAL_PARAMS?  It takes the struct skh_temporal took, and skh_temporal_check is its check."""
    return temporal_check(params)


def instance_motion_check(table):
    """skh_instance_motion_check: would skh_set_instance_motion accept this S.INSTANCE_MOTION table?  (needs no context and no GPU)"""
    t = np.ascontiguousarray(table, dtype=S.INSTANCE_MOTION).reshape(-1)
    return load().skh_instance_motion_check(_p(t), len(t)) == 0


def vdenoise_check(params):
    """skh_vdenoise_check: would skh_denoise_variance accept these S.VDENOISE_PARAMS?  (needs no context and no GPU)"""
    p = np.ascontiguousarray(params, dtype=S.VDENOISE_PARAMS)
    return load().skh_vdenoise_check(_p(p)) == 0


def adaptive_dark_level(radiance, exposure):
    """skh_adaptive.dark_level for a scene radiance level: the LDR luminance the accumulator's tonemap gives a grey pixel of that radiance under the
    frame's exposure (frame_params' `exposure`, three factors) -- below it, a pixel's error is taken relative to this level instead of its own mean."""
    e = np.asarray(exposure, np.float32).reshape(3)
    c = np.float32(radiance) * e
    t = c / (c + np.float32(1.0))
    return float(np.float32(0.2126) * t[0] + np.float32(0.7152) * t[1] + np.float32(0.0722) * t[2])


class Context:
    """One renderer context per GPU (skh_context).  Method names follow the C ABI."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        st = self.lib.skh_create(device, C.byref(h))
        if st != 0 or not h:
            raise SkhError(f"skh_create(device={device}) failed with status {st}: no usable MI355X/HIP device. "
                           "This renderer has no CPU fallback.")
        self.h = h
        self.width = self.height = 0
        self.tile_size = 32
        self.tile_xy = None

    def close(self):
        if getattr(self, "h", None):
            self.lib.skh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, st, what):
        if st != 0:
            raise SkhError(f"{what} failed ({st}): {self.lib.skh_last_error(self.h).decode()}")

    def set_scene(self, arr, build=True, flags=0):
        L = self.lib
        self._ck(L.skh_set_geometry(self.h, _p(arr["vertices"]), len(arr["vertices"]), _p(arr["indices"]),
                                    len(arr["indices"]), _p(arr["meshes"]), len(arr["meshes"])), "skh_set_geometry")
        if len(arr.get("curves", [])):
            self._ck(L.skh_set_curves(self.h, _p(arr["curve_points"]), len(arr["curve_points"]), _p(arr["curve_radii"]),
                                      len(arr["curve_radii"]), _p(arr["curve_vertex_counts"]),
                                      len(arr["curve_vertex_counts"]), _p(arr["curves"]), len(arr["curves"])),
                     "skh_set_curves")
        self._ck(L.skh_set_instances(self.h, _p(arr["instances"]), len(arr["instances"])), "skh_set_instances")
        self._ck(L.skh_set_lights(self.h, _p(arr["lights"]), len(arr["lights"])), "skh_set_lights")
        self.set_textures(arr.get("textures") or [])
        self._ck(L.skh_set_materials(self.h, _p(arr["materials"]), len(arr["materials"])), "skh_set_materials")
        # a scene without an environment removes the one a reused context may still hold (a no-op when it holds none)
        env = arr.get("environment")
        if env is None:
            self.set_environment(None)
        else:
            self.set_environment(env["rgb"], env.get("scale", (1, 1, 1)), env.get("world_to_env"))
        self.set_emission(arr.get("emission"))  # (likewise: a scene without emissive materials removes what a reused context holds)
        self.set_material_textures(arr.get("material_textures"))  # (likewise)
        self.set_material_cutouts(arr.get("material_cutouts"))  # (likewise)
        self.set_material_blend(arr.get("material_blend"))  # (likewise)
        self.set_light_shapes(arr.get("light_shapes"))  # (likewise)
        if build:
            self.build_accel(flags)

    def set_textures(self, textures):
        """textures: list of HxWx4 uint8 images (rows top to bottom).  skh_texture = {const uint8_t* rgba8; u32 width, height}."""

        class SkhTexture(C.Structure):
            _fields_ = [("rgba8", C.c_void_p), ("width", C.c_uint32), ("height", C.c_uint32)]

        keep = [np.ascontiguousarray(t, np.uint8) for t in textures]
        for t in keep:
            if t.ndim != 3 or t.shape[2] != 4:
                raise ValueError("textures must be HxWx4 uint8")
        recs = (SkhTexture * max(1, len(keep)))()
        for k, t in enumerate(keep):
            recs[k].rgba8, recs[k].width, recs[k].height = t.ctypes.data, t.shape[1], t.shape[0]
        self._ck(self.lib.skh_set_textures(self.h, C.cast(recs, C.c_void_p), len(keep)), "skh_set_textures")

    @staticmethod
    def _env_transform(scale, world_to_env):
        sc = np.ascontiguousarray(scale, np.float32).reshape(3)
        m = np.eye(3, dtype=np.float32) if world_to_env is None else np.ascontiguousarray(world_to_env, np.float32).reshape(3, 3)
        return sc, np.ascontiguousarray(m.reshape(9))

    def set_environment(self, rgb, scale=(1, 1, 1), world_to_env=None):
        """skh_set_environment: `rgb` an (H, W, 3) float array, lat-long, row 0 = the +Y pole, column 0 at phi = 0 on +X (None removes the
        environment); `scale` = intensity * colour; `world_to_env` a 3x3 rotation (None = identity).  The sampling tables are built on the device."""
        e = SkhEnvironment()
        sc, m = self._env_transform(scale, world_to_env)
        e.scale[:], e.world_to_env[:] = sc.tolist(), m.tolist()
        keep = None
        if rgb is not None:
            keep = np.ascontiguousarray(rgb, np.float32)
            if keep.ndim != 3 or keep.shape[2] != 3:
                raise ValueError("the environment map must be an (H, W, 3) array")
            e.rgb, e.width, e.height = keep.ctypes.data, keep.shape[1], keep.shape[0]
        self._ck(self.lib.skh_set_environment(self.h, C.byref(e)), "skh_set_environment")

    def set_environment_transform(self, scale=(1, 1, 1), world_to_env=None):
        """skh_set_environment_transform: new intensity * colour and rotation for the environment in place (no table rebuild)"""
        sc, m = self._env_transform(scale, world_to_env)
        self._ck(self.lib.skh_set_environment_transform(self.h, _p(sc), _p(m)), "skh_set_environment_transform")

    def environment_info(self):
        d = np.zeros((), ENVIRONMENT_INFO)
        self._ck(self.lib.skh_get_environment_info(self.h, _p(d)), "skh_get_environment_info")
        return {k: (float(d[k]) if d[k].dtype.kind == "f" else int(d[k])) for k in ENVIRONMENT_INFO.names}

    def set_emission(self, rgb):
        """skh_set_emission: `rgb` an (n, 3) float array, the radiance Le of the first n materials (None or empty removes all emission)"""
        if rgb is None or len(rgb) == 0:
            self._ck(self.lib.skh_set_emission(self.h, None, 0), "skh_set_emission")
            return
        keep = np.ascontiguousarray(rgb, np.float32)
        if keep.ndim != 2 or keep.shape[1] != 3:
            raise ValueError("the emission must be an (n_materials, 3) array")
        self._ck(self.lib.skh_set_emission(self.h, _p(keep), keep.shape[0]), "skh_set_emission")

    def emitter_info(self):
        """skh_get_emitter_info (builds the emitter table when it is stale)"""
        d = np.zeros((), EMITTER_INFO)
        self._ck(self.lib.skh_get_emitter_info(self.h, _p(d)), "skh_get_emitter_info")
        return {k: (float(d[k]) if d[k].dtype.kind == "f" else int(d[k])) for k in EMITTER_INFO.names}

    def emitter_probe(self, kind, records):
        """skh_emitter_probe: `kind` "sample" ({u', ux, uy, P[3]} -> 13 words) or "pdf" ({instance, prim, hitPoint[3], origin[3]} -> 4 words);
        `records` an (n, words in) array of 32-bit words; returns (n, words out) uint32 (view as float32 where the header says f32)."""
        num, win, wout = EMIT_PROBES[kind]
        rec = np.ascontiguousarray(records)
        if rec.dtype.itemsize != 4 or rec.ndim != 2 or rec.shape[1] != win:
            raise ValueError(f"{kind}: records must be (n, {win}) 32-bit words")
        out = np.zeros((rec.shape[0], wout), np.uint32)
        self._ck(self.lib.skh_emitter_probe(self.h, num, _p(rec), rec.shape[0], _p(out)), "skh_emitter_probe")
        return out

    def set_material_textures(self, table):
        """skh_set_material_textures: `table` an S.MATERIAL_TEXTURES array, one entry per material (None or empty removes the table)"""
        if table is None or len(table) == 0:
            self._ck(self.lib.skh_set_material_textures(self.h, None, 0), "skh_set_material_textures")
            return
        t = np.ascontiguousarray(table, S.MATERIAL_TEXTURES).reshape(-1)
        self._ck(self.lib.skh_set_material_textures(self.h, _p(t), len(t)), "skh_set_material_textures")

    def set_material_cutouts(self, table):
        """skh_set_material_cutouts: `table` an S.MATERIAL_CUTOUT array, one entry per material (None or empty removes the table)"""
        if table is None or len(table) == 0:
            self._ck(self.lib.skh_set_material_cutouts(self.h, None, 0), "skh_set_material_cutouts")
            return
        t = np.ascontiguousarray(table, S.MATERIAL_CUTOUT).reshape(-1)
        self._ck(self.lib.skh_set_material_cutouts(self.h, _p(t), len(t)), "skh_set_material_cutouts")

    def cutout_info(self):
        """skh_get_cutout_info: materials with an active cutout, mesh instances using them, rays continued / accepted by the round limit since the last reset_stats"""
        d = np.zeros((), CUTOUT_INFO)
        self._ck(self.lib.skh_get_cutout_info(self.h, _p(d)), "skh_get_cutout_info")
        return {k: int(d[k]) for k in CUTOUT_INFO.names}

    def set_material_blend(self, table):
        """skh_set_material_blend: `table` an S.MATERIAL_BLEND array, one entry per material (None or empty removes the table)"""
        if table is None or len(table) == 0:
            self._ck(self.lib.skh_set_material_blend(self.h, None, 0), "skh_set_material_blend")
            return
        t = np.ascontiguousarray(table, S.MATERIAL_BLEND).reshape(-1)
        self._ck(self.lib.skh_set_material_blend(self.h, _p(t), len(t)), "skh_set_material_blend")

    def blend_info(self):
        """skh_get_blend_info: materials with an active blend entry, mesh instances using them, radiance rays passed / shadow crossings / hits accepted by
        the round limit since the last reset_stats"""
        d = np.zeros((), BLEND_INFO)
        self._ck(self.lib.skh_get_blend_info(self.h, _p(d)), "skh_get_blend_info")
        return {k: int(d[k]) for k in BLEND_INFO.names}

    def blend_probe(self, tuples):
        """skh_blend_probe: the draw on the device for (n, 6) uint32 {px, py, pixel sample index, spp_total, depth, round} -> (n,) float32 xi"""
        t = np.ascontiguousarray(tuples, np.uint32).reshape(-1, 6)
        out = np.zeros(len(t), np.float32)
        self._ck(self.lib.skh_blend_probe(self.h, len(t), _p(t), _p(out)), "skh_blend_probe")
        return out

    def set_light_shapes(self, table):
        """skh_set_light_shapes: `table` an S.LIGHT_SHAPE array, one entry per light (None or empty removes the table)"""
        if table is None or len(table) == 0:
            self._ck(self.lib.skh_set_light_shapes(self.h, None, 0), "skh_set_light_shapes")
            return
        t = np.ascontiguousarray(table, S.LIGHT_SHAPE).reshape(-1)
        self._ck(self.lib.skh_set_light_shapes(self.h, _p(t), len(t)), "skh_set_light_shapes")

    def light_shape_info(self):
        """skh_get_light_shape_info: entries in use inside the light list -- sampled disks, cones"""
        d = np.zeros((), LIGHT_SHAPE_INFO)
        self._ck(self.lib.skh_get_light_shape_info(self.h, _p(d)), "skh_get_light_shape_info")
        return {k: int(d[k]) for k in LIGHT_SHAPE_INFO.names}

    def light_shape_probe(self, kind, records):
        """skh_light_shape_probe: `kind` "sample" ({light, ux, uy, P[3]} -> point[3], normal[3], L[3], dist, pdf, s, area) or "pdf"
        ({light, lightHitPoint[3], surfacePoint[3]} -> pdf, s); `records` an (n, words in) array of 32-bit words; returns (n, words out) float32."""
        num, win, wout = LSHAPE_PROBES[kind]
        rec = np.ascontiguousarray(records)
        if rec.dtype.itemsize != 4 or rec.ndim != 2 or rec.shape[1] != win:
            raise ValueError(f"{kind}: records must be (n, {win}) 32-bit words")
        out = np.zeros((rec.shape[0], wout), np.float32)
        self._ck(self.lib.skh_light_shape_probe(self.h, num, _p(rec), rec.shape[0], _p(out)), "skh_light_shape_probe")
        return out

    def material_probe(self, material, uv):
        """skh_material_probe: the device function k_shade calls for a triangle hit of material[i] at uv[i] -> (n, 8) float32:
        base_color[3], roughness, metallic, Le[3]"""
        m = np.ascontiguousarray(material, np.uint32).reshape(-1)
        t = np.ascontiguousarray(uv, np.float32).reshape(-1, 2)
        if len(m) != len(t):
            raise ValueError("one uv pair per material id")
        out = np.zeros((len(m), 8), np.float32)
        self._ck(self.lib.skh_material_probe(self.h, len(m), _p(m), _p(t), _p(out)), "skh_material_probe")
        return out

    def build_accel(self, flags=0):
        self._ck(self.lib.skh_build_accel(self.h, flags), "skh_build_accel")

    def resize(self, w, h):
        self.width, self.height = w, h
        self._ck(self.lib.skh_resize(self.h, w, h), "skh_resize")

    def set_tiles(self, tile_size, tile_xy=None):
        self.tile_size = tile_size
        if tile_xy is not None:
            tile_xy = np.ascontiguousarray(tile_xy, np.uint32).reshape(-1, 2)
        self.tile_xy = tile_xy
        self._ck(self.lib.skh_set_tiles(self.h, tile_size, _p(tile_xy), 0 if tile_xy is None else len(tile_xy)),
                 "skh_set_tiles")

    def set_adaptive(self, threshold=None, dark_level=0.01, min_samples=16, interval=8):
        """skh_set_adaptive: a tile stops once the relative standard error of every pixel's LDR luminance is at most `threshold` (checked at `min_samples`
        observations and every `interval` after); None turns the feature off.  adaptive_dark_level() gives `dark_level` from a radiance."""
        if threshold is None:
            self._ck(self.lib.skh_set_adaptive(self.h, None), "skh_set_adaptive")
            return
        a = adaptive_record(threshold, dark_level, min_samples, interval)
        self._ck(self.lib.skh_set_adaptive(self.h, _p(a)), "skh_set_adaptive")

    def adaptive_info(self):
        d = np.zeros((), ADAPTIVE_INFO)
        self._ck(self.lib.skh_get_adaptive_info(self.h, _p(d)), "skh_get_adaptive_info")
        return {k: int(d[k]) for k in ADAPTIVE_INFO.names}

    def read_adaptive(self):
        """skh_read_adaptive: (H, W, 4) float32 {n, mean, M2, q at the tile's last check}; 0 where this context owns no tile"""
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._ck(self.lib.skh_read_adaptive(self.h, _p(out)), "skh_read_adaptive")
        return out

    def buffer_alloc(self, nbytes):
        """skh_buffer_alloc: a caller-owned device buffer (free it with buffer_free)"""
        d = C.c_void_p()
        self._ck(self.lib.skh_buffer_alloc(self.h, int(nbytes), C.byref(d)), "skh_buffer_alloc")
        return d

    def buffer_free(self, d_ptr):
        self._ck(self.lib.skh_buffer_free(self.h, d_ptr), "skh_buffer_free")

    def render_aovs_device(self, params, planes_mask, d_planes):
        """skh_render_aovs on caller-owned device buffers: `d_planes` a sequence of len(S.AOV_PLANES) device pointers (None where the bit is clear)"""
        p = np.ascontiguousarray(params, dtype=S.AOV_PARAMS)
        ptrs = (C.c_void_p * len(S.AOV_PLANES))(*[getattr(d, "value", d) for d in d_planes])
        self._ck(self.lib.skh_render_aovs(self.h, _p(p), int(planes_mask), C.cast(ptrs, C.c_void_p)), "skh_render_aovs")

    def render_aovs(self, params, planes=S.AOV_PLANES, region=None, sample_index=None, spp_total=64):
        """skh_render_aovs: the first-hit planes named in `planes` (S.AOV_PLANES) of `region` (x0, y0, width, height; None = the region of `params`, which
        S.aov_params leaves at the whole image) -> {name: (h, w, 4) array}, `ids` uint32, the rest float32.  `sample_index` None = the ray of `params`
        (S.aov_params: the pixel centre), else the camera ray of that sample of `spp_total`.  Device buffers come from skh_buffer_alloc and are freed here."""
        p = np.array(params, dtype=S.AOV_PARAMS)
        if region is not None:
            p["x0"], p["y0"], p["width"], p["height"] = region
        if sample_index is not None:
            p["sample_index"], p["spp_total"] = sample_index, spp_total
        w, h = (int(p["width"]), int(p["height"])) if int(p["width"]) or int(p["height"]) else (self.width, self.height)
        names = [n for n in S.AOV_PLANES if n in planes]
        if len(names) != len(set(planes)):
            raise ValueError(f"planes must be among {S.AOV_PLANES}")
        mask = sum(1 << S.AOV_PLANES.index(n) for n in names)
        bufs = {}
        try:
            for n in names:
                bufs[n] = self.buffer_alloc(16 * max(1, w * h))
            self.render_aovs_device(p, mask, [bufs.get(n) for n in S.AOV_PLANES])
            out = {}
            for n in names:
                out[n] = np.zeros((h, w, 4), np.uint32 if n == "ids" else np.float32)
                self.buffer_download(bufs[n], out[n])
            return out
        finally:
            for d in bufs.values():
                self.buffer_free(d)

    def pick(self, params, x, y):
        """what is under pixel (x, y): a 1 x 1 region call of render_aovs with every plane -> {plane name: its four words}"""
        return {n: a[0, 0] for n, a in self.render_aovs(params, region=(x, y, 1, 1)).items()}

    def aov_info(self):
        """skh_get_aov_info: calls and rays since the last reset_stats, the last call's wall time and plane bytes"""
        d = np.zeros((), AOV_INFO)
        self._ck(self.lib.skh_get_aov_info(self.h, _p(d)), "skh_get_aov_info")
        return {k: (float(d[k]) if d[k].dtype.kind == "f" else int(d[k])) for k in AOV_INFO.names}

    def buffer_upload(self, d_dst, host):
        """skh_buffer_upload: host -> device copy of the numpy array `host` into a caller-owned device buffer"""
        h = np.ascontiguousarray(host)
        self._ck(self.lib.skh_buffer_upload(self.h, d_dst, _p(h), h.nbytes), "skh_buffer_upload")

    def denoise_device(self, params, d_color, d_ids, d_normal, d_position, d_albedo, d_out):
        """skh_denoise on caller-owned device images (d_out may be d_color; d_albedo may be None when neither flag is set); params None frees the scratch"""
        p = None if params is None else np.ascontiguousarray(params, dtype=S.DENOISE_PARAMS)
        self._ck(self.lib.skh_denoise(self.h, _p(p), d_color, d_ids, d_normal, d_position, d_albedo, d_out), "skh_denoise")

    def denoise(self, image, guides, params):
        """skh_denoise, numpy in and numpy out: `image` an (h, w, 4) float32 colour image, `guides` {"ids", "normal", "position", "albedo"} -> (h, w, 4) arrays as
        render_aovs / render_guides return them ("albedo" may be missing when `params` sets neither flag), `params` S.denoise_params -> the filtered (h, w, 4) image.
        Device buffers come from skh_buffer_alloc and are freed here."""
        img = np.ascontiguousarray(image, np.float32)
        p = np.array(params, dtype=S.DENOISE_PARAMS)
        h, w = int(p["height"]), int(p["width"])
        if img.shape != (h, w, 4):
            raise ValueError(f"the image must be ({h}, {w}, 4)")
        bufs = {}
        try:
            bufs["color"] = self.buffer_alloc(img.nbytes)
            self.buffer_upload(bufs["color"], img)
            for n in DENOISE_GUIDES:
                if guides.get(n) is None:
                    continue
                g = np.ascontiguousarray(guides[n], np.uint32 if n == "ids" else np.float32)
                if g.shape != (h, w, 4):
                    raise ValueError(f"guide {n} must be ({h}, {w}, 4)")
                bufs[n] = self.buffer_alloc(g.nbytes)
                self.buffer_upload(bufs[n], g)
            self.denoise_device(p, bufs["color"], bufs.get("ids"), bufs.get("normal"), bufs.get("position"), bufs.get("albedo"), bufs["color"])
            out = np.zeros_like(img)
            self.buffer_download(bufs["color"], out)
            return out
        finally:
            for d in bufs.values():
                self.buffer_free(d)

    def render_guides(self, aov_params):
        """the four planes skh_denoise reads -- ids, normal, position, albedo -- through the pixel centres of the whole image: render_aovs with the region
        and the sample of `aov_params` set to that"""
        p = np.array(aov_params, dtype=S.AOV_PARAMS)
        p["x0"] = p["y0"] = p["width"] = p["height"] = 0
        p["sample_index"] = S.AOV_PIXEL_CENTRE
        return self.render_aovs(p, planes=DENOISE_GUIDES)

    def denoise_info(self):
        """skh_get_denoise_info: calls and pixels since the last reset_stats, the last call's wall time, the scratch bytes the context holds"""
        d = np.zeros((), DENOISE_INFO)
        self._ck(self.lib.skh_get_denoise_info(self.h, _p(d)), "skh_get_denoise_info")
        return {k: (float(d[k]) if d[k].dtype.kind == "f" else int(d[k])) for k in DENOISE_INFO.names}

    def temporal_device(self, params, d_color, d_ids, d_normal, d_position, d_albedo, d_prev_history, d_prev_ids, d_prev_normal, d_prev_position, d_out, d_history_out,
                        d_motion=None):
        """skh_temporal on caller-owned device images (d_out may be d_color; d_albedo may be None without DEMODULATE; d_prev_history None = no previous frame;
        d_motion None = no motion plane)"""
        p = np.ascontiguousarray(params, dtype=S.TEMPORAL_PARAMS)
        self._ck(self.lib.skh_temporal(self.h, _p(p), d_color, d_ids, d_normal, d_position, d_albedo, d_prev_history, d_prev_ids, d_prev_normal, d_prev_position,
                                       d_out, d_history_out, d_motion), "skh_temporal")

    def temporal(self, image, guides, prev, params):
        """skh_temporal, numpy in and numpy out: `image` an (h, w, 4) float32 colour image, `guides` {"ids", "normal", "position", "albedo"} of the current frame as
        render_guides returns them ("albedo" may be missing without DEMODULATE), `prev` None (no previous frame) or {"history", "ids", "normal", "position"} of the
        previous one, `params` S.temporal_params -> {"image", "history", "motion"}, (h, w, 4) float32 each.  Device buffers come from skh_buffer_alloc and are freed here."""
        img = np.ascontiguousarray(image, np.float32)
        p = np.array(params, dtype=S.TEMPORAL_PARAMS)
        h, w = int(p["height"]), int(p["width"])
        if img.shape != (h, w, 4):
            raise ValueError(f"the image must be ({h}, {w}, 4)")
        planes = {"color": img}
        for n in DENOISE_GUIDES:
            if guides.get(n) is not None:
                planes[n] = np.ascontiguousarray(guides[n], np.uint32 if n == "ids" else np.float32)
        if prev is not None:
            for n in TEMPORAL_PREV:
                planes["prev_" + n] = np.ascontiguousarray(prev[n], np.uint32 if n == "ids" else np.float32)
        for n, a in planes.items():
            if a.shape != (h, w, 4):
                raise ValueError(f"{n} must be ({h}, {w}, 4)")
        bufs = {}
        try:
            for n, a in planes.items():
                bufs[n] = self.buffer_alloc(a.nbytes)
                self.buffer_upload(bufs[n], a)
            for n in ("image", "history", "motion"):
                bufs[n] = self.buffer_alloc(img.nbytes)
            self.temporal_device(p, bufs["color"], bufs.get("ids"), bufs.get("normal"), bufs.get("position"), bufs.get("albedo"), bufs.get("prev_history"),
                                 bufs.get("prev_ids"), bufs.get("prev_normal"), bufs.get("prev_position"), bufs["image"], bufs["history"], bufs["motion"])
            out = {}
            for n in ("image", "history", "motion"):
                out[n] = np.zeros_like(img)
                self.buffer_download(bufs[n], out[n])
            return out
        finally:
            for d in bufs.values():
                self.buffer_free(d)

    def temporal_info(self):
        """skh_get_temporal_info: calls and pixels since the last reset_stats, the last call's wall time"""
        d = np.zeros((), TEMPORAL_INFO)
        self._ck(self.lib.skh_get_temporal_info(self.h, _p(d)), "skh_get_temporal_info")
        return {k: (float(d[k]) if d[k].dtype.kind == "f" else int(d[k])) for k in TEMPORAL_INFO.names}

    def _info(self, fn, dtype):
        d = np.zeros((), dtype)
        self._ck(getattr(self.lib, fn)(self.h, _p(d)), fn)
        return {k: (float(d[k]) if d[k].dtype.kind == "f" else int(d[k])) for k in dtype.names}

    def _with_planes(self, planes, h, w, outputs, call):
        """uploads the (h, w, 4) arrays of `planes` (None entries are left out), allocates `outputs`, runs call(bufs) and downloads the outputs as float32"""
        planes = {n: a for n, a in planes.items() if a is not None}
        for n, a in planes.items():
            if a.shape != (h, w, 4):
                raise ValueError(f"{n} must be ({h}, {w}, 4)")
        bufs = {}
        try:
            for n, a in planes.items():
                bufs[n] = self.buffer_alloc(a.nbytes)
                self.buffer_upload(bufs[n], a)
            for n in outputs:
                bufs[n] = self.buffer_alloc(16 * h * w)
            call(bufs)
            out = {}
            for n in outputs:
                out[n] = np.zeros((h, w, 4), np.float32)
                self.buffer_download(bufs[n], out[n])
            return out
        finally:
            for d in bufs.values():
                self.buffer_free(d)

    def moments_device(self, params, d_color, d_ids, d_position, d_albedo, d_motion, d_prev_moments, d_moments_out):
        """skh_moments on caller-owned device images: `params` the S.TEMPORAL_PARAMS skh_temporal took for this frame, d_color the RAW colour it took, d_motion the
        motion plane it wrote; d_motion and d_prev_moments both None = no previous frame; d_albedo may be None without DEMODULATE"""
        p = np.ascontiguousarray(params, dtype=S.TEMPORAL_PARAMS)
        self._ck(self.lib.skh_moments(self.h, _p(p), d_color, d_ids, d_position, d_albedo, d_motion, d_prev_moments, d_moments_out), "skh_moments")

    def moments(self, image, guides, motion, prev_moments, params):
        """skh_moments, numpy in and numpy out: `image` the raw (h, w, 4) colour, `guides` {"ids", "position", "albedo"} of the current frame, `motion` the motion plane
        temporal() returned and `prev_moments` the previous MOMENTS plane (both None: no previous frame), `params` S.temporal_params -> (h, w, 4) float32 MOMENTS"""
        p = np.array(params, dtype=S.TEMPORAL_PARAMS)
        h, w = int(p["height"]), int(p["width"])
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        planes = {"color": f32(image), "ids": None if guides.get("ids") is None else np.ascontiguousarray(guides["ids"], np.uint32),
                  "position": f32(guides.get("position")), "albedo": f32(guides.get("albedo")), "motion": f32(motion), "prev_moments": f32(prev_moments)}
        return self._with_planes(planes, h, w, ("moments",), lambda b: self.moments_device(
            p, b.get("color"), b.get("ids"), b.get("position"), b.get("albedo"), b.get("motion"), b.get("prev_moments"), b["moments"]))["moments"]

    def moments_info(self):
        """skh_get_moments_info: calls and pixels since the last reset_stats, the last call's wall time"""
        return self._info("skh_get_moments_info", MOMENTS_INFO)

    def denoise_variance_device(self, params, d_color, d_ids, d_normal, d_position, d_albedo, d_moments, d_out, d_moments_out=None):
        """skh_denoise_variance on caller-owned device images (d_out may be d_color, d_moments_out may be d_moments or None; d_albedo may be None when neither
        modulation flag is set); params None frees the scratch"""
        p = None if params is None else np.ascontiguousarray(params, dtype=S.VDENOISE_PARAMS)
        self._ck(self.lib.skh_denoise_variance(self.h, _p(p), d_color, d_ids, d_normal, d_position, d_albedo, d_moments, d_out, d_moments_out), "skh_denoise_variance")

    def denoise_variance(self, image, guides, moments, params, moments_out=True):
        """skh_denoise_variance, numpy in and numpy out: `image` and `guides` as denoise(), `moments` an (h, w, 4) MOMENTS plane, `params` S.vdenoise_params ->
        {"image", "moments"} ((h, w, 4) float32; without `moments_out` the call gets no d_moments_out and "moments" is missing)"""
        p = np.array(params, dtype=S.VDENOISE_PARAMS)
        h, w = int(p["height"]), int(p["width"])
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        planes = {"color": f32(image), "ids": None if guides.get("ids") is None else np.ascontiguousarray(guides["ids"], np.uint32),
                  "normal": f32(guides.get("normal")), "position": f32(guides.get("position")), "albedo": f32(guides.get("albedo")), "moments_in": f32(moments)}
        outputs = ("image", "moments") if moments_out else ("image",)
        return self._with_planes(planes, h, w, outputs, lambda b: self.denoise_variance_device(
            p, b.get("color"), b.get("ids"), b.get("normal"), b.get("position"), b.get("albedo"), b.get("moments_in"), b["image"], b.get("moments")))

    def vdenoise_info(self):
        """skh_get_vdenoise_info: calls and pixels since the last reset_stats, the last call's wall time, the scratch bytes the context holds (the denoiser's)"""
        return self._info("skh_get_vdenoise_info", VDENOISE_INFO)

    def set_instance_motion(self, table):
        """skh_set_instance_motion: the S.INSTANCE_MOTION table (scene.instance_motion builds it) that rewind_guides applies, one entry per instance; None or an
        empty table frees the context's copy"""
        t = np.zeros(0, S.INSTANCE_MOTION) if table is None else np.ascontiguousarray(table, dtype=S.INSTANCE_MOTION).reshape(-1)
        self._ck(self.lib.skh_set_instance_motion(self.h, _p(t) if len(t) else None, len(t)), "skh_set_instance_motion")

    def rewind_guides_device(self, width, height, d_ids, d_position, d_normal, d_position_out, d_normal_out):
        """skh_rewind_guides on caller-owned device planes (an out plane may be its own in plane)"""
        self._ck(self.lib.skh_rewind_guides(self.h, width, height, d_ids, d_position, d_normal, d_position_out, d_normal_out), "skh_rewind_guides")

    def rewind_guides(self, guides):
        """skh_rewind_guides, numpy in and numpy out: `guides` {"ids", "position", "normal"} of the current frame as render_guides returns them ->
        {"position", "normal"}, (h, w, 4) float32: what to hand temporal() and moments() in their place"""
        ids = np.ascontiguousarray(guides["ids"], np.uint32)
        h, w = ids.shape[:2]
        planes = {"ids": ids, "position_in": np.ascontiguousarray(guides["position"], np.float32), "normal_in": np.ascontiguousarray(guides["normal"], np.float32)}
        return self._with_planes(planes, h, w, ("position", "normal"), lambda b: self.rewind_guides_device(
            w, h, b["ids"], b["position_in"], b["normal_in"], b["position"], b["normal"]))

    def rewind_info(self):
        """skh_get_rewind_info: calls and pixels since the last reset_stats, the last call's wall time, the entries of the table in force"""
        return self._info("skh_get_rewind_info", REWIND_INFO)

    def rectify_device(self, params, d_image, d_ids, d_albedo, d_history, d_fast, d_out, d_history_out, d_info=None):
        """skh_rectify on caller-owned device planes (d_out may be d_image and d_history_out may be d_history; neither may be d_fast; d_albedo may be None without
        REMODULATE; d_info None = no info plane)"""
        p = np.ascontiguousarray(params, dtype=S.RECTIFY_PARAMS)
        self._ck(self.lib.skh_rectify(self.h, _p(p), d_image, d_ids, d_albedo, d_history, d_fast, d_out, d_history_out, d_info), "skh_rectify")

    def rectify(self, image, guides, history, fast, params, info=True):
        """skh_rectify, numpy in and numpy out: `image` and `history` as temporal() returned them, `fast` the "history" of the temporal() call with the short
        max_history, `guides` {"ids", "albedo"} of the current frame ("albedo" may be missing without REMODULATE), `params` S.rectify_params ->
        {"image", "history", "info"}, (h, w, 4) float32 each (without `info` the call gets no d_info and "info" is missing)"""
        p = np.array(params, dtype=S.RECTIFY_PARAMS)
        h, w = int(p["height"]), int(p["width"])
        f32 = lambda a: None if a is None else np.ascontiguousarray(a, np.float32)
        planes = {"image_in": f32(image), "ids": None if guides.get("ids") is None else np.ascontiguousarray(guides["ids"], np.uint32),
                  "albedo": f32(guides.get("albedo")), "history_in": f32(history), "fast": f32(fast)}
        outputs = ("image", "history", "info") if info else ("image", "history")
        return self._with_planes(planes, h, w, outputs, lambda b: self.rectify_device(
            p, b.get("image_in"), b.get("ids"), b.get("albedo"), b.get("history_in"), b.get("fast"), b["image"], b["history"], b.get("info")))

    def rectify_info(self):
        """skh_get_rectify_info: calls and pixels since the last reset_stats, the last call's wall time"""
        return self._info("skh_get_rectify_info", RECTIFY_INFO)

    def render_subframe(self, params, d_image=None):
        p = np.ascontiguousarray(params, dtype=S.FRAME_PARAMS)
        self._ck(self.lib.skh_render_subframe(self.h, _p(p), d_image), "skh_render_subframe")

    def render_subframes(self, params, n, d_image=None):
        p = np.ascontiguousarray(params, dtype=S.FRAME_PARAMS)
        self._ck(self.lib.skh_render_subframes(self.h, _p(p), n, d_image), "skh_render_subframes")

    def read_accum(self):
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._ck(self.lib.skh_read_accum(self.h, _p(out)), "skh_read_accum")
        return out

    def read_aov(self, which):
        out = np.zeros((self.height, self.width, 4), np.float32)
        self._ck(self.lib.skh_read_aov(self.h, which, _p(out)), "skh_read_aov")
        return out

    def copy_accum(self, d_dst):
        self._ck(self.lib.skh_copy_accum(self.h, d_dst), "skh_copy_accum")

    def copy_aov(self, which, d_dst):
        """the diffuse (0) / specular (1) AOV accumulator -> a device image (OptixRender.cpp:1029-1042)"""
        self._ck(self.lib.skh_copy_aov(self.h, which, d_dst), "skh_copy_aov")

    def copy_accum_tiles(self, d_dst):
        self._ck(self.lib.skh_copy_accum_tiles(self.h, d_dst), "skh_copy_accum_tiles")

    def scatter_tiles(self, d_src, tile_xy, tile_size, d_dst, width, height):
        t = np.ascontiguousarray(tile_xy, np.uint32).reshape(-1, 2)
        self._ck(self.lib.skh_scatter_tiles(self.h, d_src, _p(t), len(t), tile_size, d_dst, width, height),
                 "skh_scatter_tiles")

    def buffer_download(self, d_src, host):
        """Buffer::map(): device -> host copy of a caller-owned device buffer into the numpy array `host`."""
        self._ck(self.lib.skh_buffer_download(self.h, d_src, _p(host), host.nbytes), "skh_buffer_download")

    def host_register(self, host):
        """page-lock a numpy array that buffer_download will fill (Buffer::map's host mirror)"""
        self._ck(self.lib.skh_host_register(self.h, _p(host), host.nbytes), "skh_host_register")

    def host_unregister(self, host):
        self._ck(self.lib.skh_host_unregister(self.h, _p(host)), "skh_host_unregister")

    def tonemap(self, d_image, width, height, type_, exposure, gamma):
        e = np.ascontiguousarray(exposure, np.float32)
        self._ck(self.lib.skh_tonemap(self.h, d_image, width, height, type_, _p(e), gamma), "skh_tonemap")

    def trace(self, rays, mode=0):
        rays = np.ascontiguousarray(rays, dtype=S.RAY)
        hits = np.zeros(len(rays), S.HIT)
        self._ck(self.lib.skh_trace(self.h, _p(rays), len(rays), mode, _p(hits)), "skh_trace")
        return hits

    def trace_device(self, d_rays, n, mode, d_hits, repeat=1):
        self._ck(self.lib.skh_trace_device(self.h, d_rays, n, mode, d_hits, repeat), "skh_trace_device")

    def set_lights(self, lights):
        """skh_set_lights alone: `lights` an S.LIGHT array (which light-shape entries are in use is derived again from it)"""
        l = np.ascontiguousarray(lights, S.LIGHT).reshape(-1)
        self._ck(self.lib.skh_set_lights(self.h, _p(l), len(l)), "skh_set_lights")

    def set_materials(self, materials):
        m = np.ascontiguousarray(materials, S.MATERIAL).reshape(-1)
        self._ck(self.lib.skh_set_materials(self.h, _p(m), len(m)), "skh_set_materials")

    def bsdf_probe(self, queries):
        """mdlcode_sample + mdlcode_evaluate on the device for each BSDF_QUERY record -> BSDF_RESULT records"""
        q = np.ascontiguousarray(queries, BSDF_QUERY)
        out = np.zeros(len(q), BSDF_RESULT)
        self._ck(self.lib.skh_bsdf_probe(self.h, _p(q), len(q), _p(out)), "skh_bsdf_probe")
        return out

    # skh_unit: (words in, words out) per record
    UNITS = {"sampler": (0, 5, 3), "sobol": (1, 2, 1), "light_sample": (2, 5, 12), "light_pdf": (3, 6, 1), "light_normal": (4, 3, 4),
             "mis": (5, 2, 1), "accumulate": (6, 3, 3), "tonemap": (7, 3, 6), "libm": (8, 2, 10),
             "env_sample": (9, 2, 9), "env_eval": (10, 3, 6)}

    def unit_probe(self, unit, records, param=0, consts=None):
        """skh_unit_probe: one device call of the named function per record (include/strelka_hip.h lists the record layouts);
        `records` is an (n, words_in) array of 32-bit words, the result an (n, words_out) uint32 array (view it as float32)."""
        uid, win, wout = self.UNITS[unit]
        r = np.ascontiguousarray(records).reshape(-1, win)
        assert r.dtype.itemsize == 4
        out = np.zeros((len(r), wout), np.uint32)
        cst = None if consts is None else np.ascontiguousarray(consts)
        self._ck(self.lib.skh_unit_probe(self.h, uid, int(param), None if cst is None else _p(cst), _p(r), len(r), _p(out)), "skh_unit_probe")
        return out

    @staticmethod
    def comm_unique_id():
        """rank 0: the 128 bytes every rank hands to comm_init (distribute them with whatever the host has)"""
        buf = np.zeros(128, np.uint8)
        st = load().skh_comm_unique_id(_p(buf))
        if st != 0:
            raise SkhError(f"skh_comm_unique_id failed ({st}): RCCL (librccl.so.1) is not available")
        return buf

    def comm_init(self, unique_id, world_size, rank):
        u = np.ascontiguousarray(unique_id, np.uint8)
        assert u.nbytes == 128
        self._ck(self.lib.skh_comm_init(self.h, _p(u), world_size, rank), "skh_comm_init")

    def comm_info(self):
        """(world size, rank, ranks RCCL itself reports for the communicator -- ncclCommCount; 0 = no communicator)"""
        w, r, n = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._ck(self.lib.skh_comm_info(self.h, C.byref(w), C.byref(r), C.byref(n)), "skh_comm_info")
        return w.value, r.value, n.value

    def probe_memory(self, kind, nbytes, record_bytes=64, repeat=3):
        """measured memory ceiling: kind 0 stream copy, 1 independent random record fetches, 2 dependent ones -> (GB/s, ms)"""
        g, ms = C.c_double(0), C.c_double(0)
        self._ck(self.lib.skh_probe_memory(self.h, kind, int(nbytes), record_bytes, repeat, C.byref(g), C.byref(ms)), "skh_probe_memory")
        return g.value, ms.value

    def comm_destroy(self):
        self._ck(self.lib.skh_comm_destroy(self.h), "skh_comm_destroy")

    def gather_tiles(self, max_tiles, d_recv=None, root=0):
        """one RCCL gather of this context's tile accumulators into the root's [world][max_tiles][T*T] float4 buffer"""
        self._ck(self.lib.skh_gather_tiles(self.h, max_tiles, d_recv, root), "skh_gather_tiles")

    def device_info(self):
        d = np.zeros((), DEVICE_INFO)
        self._ck(self.lib.skh_get_device_info(self.h, _p(d)), "skh_get_device_info")
        return {k: (d[k].item().decode() if k == "name" else int(d[k])) for k in DEVICE_INFO.names}

    def set_geometry(self, scene):
        """skh_set_geometry alone (a vertex edit: follow it with refit_accel)"""
        v, idx, m = scene["vertices"], scene["indices"], scene["meshes"]
        self._ck(self.lib.skh_set_geometry(self.h, _p(v), len(v), _p(idx), len(idx), _p(m), len(m)), "skh_set_geometry")

    def set_curves(self, scene):
        """skh_set_curves alone (edited control points / radii: follow it with refit_accel)"""
        self._ck(self.lib.skh_set_curves(self.h, _p(scene["curve_points"]), len(scene["curve_points"]), _p(scene["curve_radii"]), len(scene["curve_radii"]),
                                         _p(scene["curve_vertex_counts"]), len(scene["curve_vertex_counts"]), _p(scene["curves"]), len(scene["curves"])), "skh_set_curves")

    def refit_accel(self):
        """skh_refit_accel: keep the hierarchy's topology, recompute leaf records and boxes from the current vertices (falls back to a build)"""
        self._ck(self.lib.skh_refit_accel(self.h), "skh_refit_accel")

    def set_instances(self, instances):
        """skh_set_instances alone (the table update_accel(None) then takes, or the next build)"""
        inst = np.ascontiguousarray(instances, dtype=S.INSTANCE)
        self._ck(self.lib.skh_set_instances(self.h, _p(inst), len(inst)), "skh_set_instances")

    def update_accel(self, instances=None):
        """skh_update_accel: update every level of the hierarchy in place after edited instance transforms (`instances`: the structured S.INSTANCE
        array of the last build with new transforms; None = the table as it is) and / or vertex and control-point edits (set_geometry / set_curves
        first).  build_info()["refit"] says 2 when it updated in place, 0 when it fell back to a build."""
        if instances is None:
            self._ck(self.lib.skh_update_accel(self.h, None, 0), "skh_update_accel")
            return
        inst = np.ascontiguousarray(instances, dtype=S.INSTANCE)
        self._ck(self.lib.skh_update_accel(self.h, _p(inst), len(inst)), "skh_update_accel")

    def build_info(self):
        """what the last skh_build_accel did to the triangle hierarchy (reinsertion rounds / moves, cost before and after)"""
        d = np.zeros((), BUILD_INFO)
        self._ck(self.lib.skh_get_build_info(self.h, _p(d)), "skh_get_build_info")
        return {k: (float(d[k]) if d[k].dtype.kind == "f" else int(d[k])) for k in BUILD_INFO.names if k != "reserved"}

    def baked(self, n_instances):
        """(per-instance flags, baked instances, baked triangles) of option bake_world after the build"""
        flags = np.zeros(max(1, n_instances), np.uint8)
        ni, nt = C.c_uint32(0), C.c_uint32(0)
        self._ck(self.lib.skh_get_baked(self.h, _p(flags), n_instances, C.byref(ni), C.byref(nt)), "skh_get_baked")
        return flags[:n_instances], ni.value, nt.value

    def set_option(self, name, value):
        self._ck(self.lib.skh_set_option(self.h, name.encode(), int(value)), f"skh_set_option({name})")

    def stats(self):
        s = np.zeros((), STATS)
        self._ck(self.lib.skh_get_stats(self.h, _p(s)), "skh_get_stats")
        out = {}
        for k in STATS.names:
            v = s[k]
            if v.ndim:
                out[k] = [int(x) for x in v]
            else:
                out[k] = float(v) if v.dtype.kind == "f" else int(v)
        return out

    def reset_stats(self):
        self._ck(self.lib.skh_reset_stats(self.h), "skh_reset_stats")

    def synchronize(self):
        self._ck(self.lib.skh_synchronize(self.h), "skh_synchronize")

    def stream(self):
        return self.lib.skh_get_stream(self.h)
