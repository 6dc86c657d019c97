"""raytracer-public_amd -- MI355X-native drop-in for the per-pixel-sample hot path of
31415Hacker/RayTracer-public (src/shaders/renderer.wgsl) behind the reference's own
PathTracer / Scene API.

This module is the ctypes binding of the C ABI in include/mi355pt.h (libmi355pt.so, built
in-tree by raytracer-public_amd/csrc/Makefile) plus a small Python mirror of the reference's
``PathTracer`` class (src/libs/PathTracer.js) used by tests and bench.py.  The production
host is the Node side in raytracer-public_amd/js/ over the N-API addon.

There is no CPU fallback: if the shared library is missing the import fails, and creating a
context without a HIP device raises ``PtError``.
"""
import collections
import ctypes as C
import math
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi355pt.so")

PT_MODE_REFERENCE_PACKET, PT_MODE_REFERENCE, PT_MODE_PATH = 0, 1, 2
PT_FLAG_STATS = 1
PT_FLAG_SIMPLE_KERNEL = 2
PT_FLAG_BRUTE_FORCE = 4
PT_FLAG_COMPACT = 8
SCENE_DRAGON_CLASS, SCENE_SPONZA_CLASS = 0, 1
# opt-in tree quality of build_bvh (include/mi355pt.h PT_ACCEL_*): 0 = the reference's tree
PT_ACCEL_REFERENCE, PT_ACCEL_AREA_COLLAPSE, PT_ACCEL_PLOC = 0, 1, 2
# batched ray queries (include/mi355pt.h pt_trace_rays)
PT_TRACE_ANY_HIT, PT_TRACE_STATS, PT_TRACE_SIMPLE_KERNEL = 1, 2, 4
# batched closest-point queries (include/mi355pt.h pt_closest_points)
PT_CLOSEST_STATS, PT_CLOSEST_SIMPLE_KERNEL, PT_CLOSEST_BRUTE_FORCE = 1, 2, 4
# batched ambient-occlusion queries (include/mi355pt.h pt_occlusion)
PT_OCCLUSION_STATS, PT_OCCLUSION_SIMPLE_KERNEL = 1, 2
PT_COUNT_STATS, PT_COUNT_SIMPLE_KERNEL, PT_COUNT_BRUTE_FORCE = 1, 2, 4
PT_CONTAIN_STATS, PT_CONTAIN_SIMPLE_KERNEL = 1, 2
# radius queries (include/mi355pt.h pt_radius_search)
PT_RADIUS_STATS, PT_RADIUS_SIMPLE_KERNEL, PT_RADIUS_BRUTE_FORCE = 1, 2, 4
# hit lists (include/mi355pt.h pt_list_hits)
PT_HITS_STATS, PT_HITS_SIMPLE_KERNEL, PT_HITS_BRUTE_FORCE, PT_HITS_SORTED = 1, 2, 4, 8
# box-overlap queries (include/mi355pt.h pt_box_search)
PT_BOX_STATS, PT_BOX_SIMPLE_KERNEL, PT_BOX_BRUTE_FORCE = 1, 2, 4
# triangle-overlap queries (include/mi355pt.h pt_tri_search)
PT_TRI_STATS, PT_TRI_SIMPLE_KERNEL, PT_TRI_BRUTE_FORCE = 1, 2, 4
# plane-cut queries (include/mi355pt.h pt_cut_search)
PT_CUT_STATS, PT_CUT_SIMPLE_KERNEL, PT_CUT_BRUTE_FORCE = 1, 2, 4
# sphere-cast queries (include/mi355pt.h pt_sweep_spheres)
PT_SWEEP_STATS, PT_SWEEP_SIMPLE_KERNEL, PT_SWEEP_BRUTE_FORCE = 1, 2, 4
# k-nearest queries (include/mi355pt.h pt_nearest_k)
PT_NEAREST_STATS, PT_NEAREST_SIMPLE_KERNEL, PT_NEAREST_BRUTE_FORCE = 1, 2, 4
PT_NEAREST_MAX_K = 64
PRIM_NONE = 0xFFFFFFFF


class PtError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libmi355pt error %d: %s" % (code, message))
        self.code = code


class PtRenderParams(C.Structure):
    _fields_ = [
        ("width", C.c_uint32), ("height", C.c_uint32),
        ("focal", C.c_float), ("aspect", C.c_float),
        ("cam_pos", C.c_float * 3), ("num_tris", C.c_uint32),
        ("cam_quat", C.c_float * 4),
        ("frame", C.c_uint32), ("mode", C.c_uint32),
        ("spp", C.c_uint32), ("max_bounces", C.c_uint32), ("seed", C.c_uint32),
        ("accumulate", C.c_uint32),
        ("tile_rank", C.c_uint32), ("tile_count", C.c_uint32),
        ("flags", C.c_uint32),
    ]


class PtStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "rays_closest", "rays_shadow", "nodes_examined", "tris_tested", "stack_drops", "max_stack", "samples")]

    def as_dict(self):
        return {n: int(getattr(self, n)) for n, _ in self._fields_}


class PtRay(C.Structure):
    """include/mi355pt.h PtRay (32 B); arrays of it must be 16-byte aligned.  As numpy / torch data: 8 float32 per ray."""
    _fields_ = [("org", C.c_float * 3), ("t_max", C.c_float), ("dir", C.c_float * 3), ("reserved", C.c_uint32)]


class PtHit(C.Structure):
    """include/mi355pt.h PtHit (16 B): t (+inf on a miss), prim (0xFFFFFFFF on a miss), barycentrics u, v."""
    _fields_ = [("t", C.c_float), ("prim", C.c_uint32), ("u", C.c_float), ("v", C.c_float)]


class PtPoint(C.Structure):
    """include/mi355pt.h PtPoint (16 B); arrays of it must be 16-byte aligned.  As numpy / torch data: 4 float32 per point (x, y, z, r_max)."""
    _fields_ = [("p", C.c_float * 3), ("r_max", C.c_float)]


class PtClosest(C.Structure):
    """include/mi355pt.h PtClosest (16 B): dist (+inf when nothing is found), prim (0xFFFFFFFF then), u, v of the closest point."""
    _fields_ = [("dist", C.c_float), ("prim", C.c_uint32), ("u", C.c_float), ("v", C.c_float)]


class PtSweep(C.Structure):
    """include/mi355pt.h PtSweep (32 B, the shape of PtRay with the radius in the reserved word); arrays of it must be 16-byte aligned.  As
    numpy / torch data: 8 float32 per sweep (org xyz, t_max, dir xyz, radius)."""
    _fields_ = [("org", C.c_float * 3), ("t_max", C.c_float), ("dir", C.c_float * 3), ("radius", C.c_float)]


class PtBox(C.Structure):
    """include/mi355pt.h PtBox (32 B); arrays of it must be 16-byte aligned.  As numpy / torch data: 8 float32 per box (lo xyz, pad, hi xyz, pad)."""
    _fields_ = [("lo", C.c_float * 3), ("pad0", C.c_float), ("hi", C.c_float * 3), ("pad1", C.c_float)]


class PtOverlap(C.Structure):
    """include/mi355pt.h PtOverlap (16 B): prim, verts_inside (bit i: vertex i lies in the closed box; 7: the whole triangle), two zero words."""
    _fields_ = [("prim", C.c_uint32), ("verts_inside", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class PtTri(C.Structure):
    """include/mi355pt.h PtTri (48 B); arrays of it must be 16-byte aligned.  As numpy / torch data: 12 float32 per caller triangle (v0 xyz,
    pad, v1 xyz, pad, v2 xyz, pad)."""
    _fields_ = [("v0", C.c_float * 3), ("pad0", C.c_float), ("v1", C.c_float * 3), ("pad1", C.c_float), ("v2", C.c_float * 3), ("pad2", C.c_float)]


class PtCross(C.Structure):
    """include/mi355pt.h PtCross (16 B): prim, edges (bits 0-2: the caller triangle's edges that cross mesh triangle prim; bits 3-5: the mesh
    triangle's edges that cross the caller's triangle), two zero words."""
    _fields_ = [("prim", C.c_uint32), ("edges", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class PtCutPlane(C.Structure):
    """include/mi355pt.h PtCutPlane (48 B); arrays of it must be 16-byte aligned.  As numpy / torch data: 12 float32 per record (n xyz, d,
    lo xyz, pad, hi xyz, pad): the plane n.x = d and the window [lo, hi]."""
    _fields_ = [("n", C.c_float * 3), ("d", C.c_float), ("lo", C.c_float * 3), ("pad0", C.c_float), ("hi", C.c_float * 3), ("pad1", C.c_float)]


class PtCut(C.Structure):
    """include/mi355pt.h PtCut (16 B): prim, code (bits 0-2: the crossing edges v0-v1, v1-v2, v0-v2 of mesh triangle prim, exactly two;
    bits 3-5: the classes s_i >= 0 of its vertices), t0 and t1 (where the plane crosses the lowest and the highest crossing edge,
    measured from the edge's vertex below the plane)."""
    _fields_ = [("prim", C.c_uint32), ("code", C.c_uint32), ("t0", C.c_float), ("t1", C.c_float)]


class PtSurfel(C.Structure):
    """include/mi355pt.h PtSurfel (32 B, the shape of PtRay); arrays of it must be 16-byte aligned.  As numpy / torch data: 8 float32 per surfel
    (p xyz, r_max, n xyz, 0)."""
    _fields_ = [("p", C.c_float * 3), ("r_max", C.c_float), ("n", C.c_float * 3), ("reserved", C.c_uint32)]


class PtOcclusion(C.Structure):
    """include/mi355pt.h PtOcclusion (16 B): visibility = unoccluded / samples; all zero for a surfel that is not traced."""
    _fields_ = [("visibility", C.c_float), ("unoccluded", C.c_uint32), ("samples", C.c_uint32), ("reserved", C.c_uint32)]


class PtOcclusionParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("seed", C.c_uint32), ("index_base", C.c_uint32), ("bias", C.c_float), ("flags", C.c_uint32)]


class PtContainment(C.Structure):
    """include/mi355pt.h PtContainment (16 B): inside = (2 * odd > samples), odd = sample rays with an odd crossing count; all zero for a
    point that is not traced."""
    _fields_ = [("inside", C.c_uint32), ("odd", C.c_uint32), ("samples", C.c_uint32), ("reserved", C.c_uint32)]


class PtContainParams(C.Structure):
    _fields_ = [("samples", C.c_uint32), ("seed", C.c_uint32), ("index_base", C.c_uint32), ("flags", C.c_uint32)]


class PtAccumInfo(C.Structure):
    _fields_ = [("width", C.c_uint32), ("height", C.c_uint32), ("tile_rank", C.c_uint32), ("tile_count", C.c_uint32),
                ("compact", C.c_uint32), ("samples", C.c_uint32), ("floats", C.c_uint64)]


# every symbol include/mi355pt.h declares (tests/test_host_build.py::test_library_exports_every_declared_symbol checks the header against this)
EXPORTS = [
    "pt_create", "pt_destroy", "pt_last_error", "pt_version", "pt_set_stream", "pt_get_stream", "pt_synchronize",
    "pt_compute_bvh2_sizing", "pt_compute_bvh4_sizing", "pt_morton_sort", "pt_collapse_lbvh2_to_bvh4",
    "pt_collapse_bvh2_to_bvh4_accel", "pt_build_bvh2_ploc", "pt_bvh2_to_bvh4_wide", "pt_file_write_u32", "pt_file_read_u32", "pt_scene_procedural",
    "pt_set_triangles", "pt_build_bvh", "pt_build_bvh_accel", "pt_build_lbvh2", "pt_read_bvh2", "pt_set_bvh4", "pt_set_bvh2",
    "pt_read_bvh4", "pt_set_spheres", "pt_scene_info", "pt_render", "pt_last_render_ms", "pt_set_batch", "pt_flush", "pt_timing_begin", "pt_timing_collect", "pt_timing_collect_spans", "pt_set_compact_buffer", "pt_set_output_buffer", "pt_get_stats", "pt_read_radiance",
    "pt_read_rgba8", "pt_read_tonemapped", "pt_tile_layout", "pt_tile_ids", "pt_compact_radiance", "pt_deinterleave", "pt_deinterleave_batch", "pt_buffer_busy",
    "pt_accum_info", "pt_read_accum", "pt_set_accum",
    "pt_trace_rays", "pt_trace_rays_host", "pt_camera_rays",
    "pt_closest_points", "pt_closest_points_host", "pt_closest_points_bvh4",
    "pt_occlusion", "pt_occlusion_host", "pt_occlusion_rays", "pt_occlusion_rays_host", "pt_hit_surfels", "pt_hit_surfels_host",
    "pt_count_hits", "pt_count_hits_host", "pt_count_hits_bvh4", "pt_contains", "pt_contains_host", "pt_contains_bvh4",
    "pt_signed_distance", "pt_signed_distance_host",
    "pt_radius_count", "pt_radius_count_host", "pt_radius_search", "pt_radius_search_host", "pt_radius_search_bvh4",
    "pt_box_count", "pt_box_count_host", "pt_box_search", "pt_box_search_host", "pt_box_search_bvh4",
    "pt_tri_count", "pt_tri_count_host", "pt_tri_search", "pt_tri_search_host", "pt_tri_search_bvh4",
    "pt_cut_count", "pt_cut_count_host", "pt_cut_search", "pt_cut_search_host", "pt_cut_search_bvh4",
    "pt_list_hits", "pt_list_hits_host", "pt_list_hits_bvh4",
    "pt_nearest_k", "pt_nearest_k_host", "pt_nearest_k_bvh4",
    "pt_sweep_spheres", "pt_sweep_spheres_host", "pt_sweep_spheres_bvh4",
    "pt_update_triangles", "pt_update_triangles_device", "pt_bvh_cost", "pt_refit_bvh4", "pt_refit_bvh2", "pt_bvh4_cost", "pt_group_update_triangles",
    "pt_traced_tile_rect", "pt_packed_layout", "pt_packed_tile_ids", "pt_pack_shares", "pt_unpack_batch",
    "pt_group_create", "pt_group_destroy", "pt_group_last_error", "pt_group_size", "pt_group_context", "pt_group_set_triangles", "pt_group_build_bvh",
    "pt_group_build_bvh_accel",
    "pt_group_set_bvh2", "pt_group_set_bvh4", "pt_group_set_batch", "pt_group_render", "pt_group_flush", "pt_group_synchronize", "pt_group_read_radiance",
    "pt_group_read_rgba8", "pt_group_read_tonemapped",
    "pt_debug_set_tune", "pt_debug_counters", "pt_debug_wave_times", "pt_debug_launch_plan", "pt_debug_launch_plan_tuned", "pt_debug_traced_tiles", "pt_debug_exposure", "pt_exposure_flags_host", "pt_debug_exposure_tier2", "pt_exposure_flags_host_gate",     # diagnostics section of the header
]


def _load():
    # the trace phases of consecutive frames overlap on side streams; ROCm's default of 4 hardware
    # queues would serialise them (read by the HIP runtime when it initialises)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "12")
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libmi355pt.so is not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C raytracer-public_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    lib.pt_last_error.restype = C.c_char_p
    lib.pt_last_error.argtypes = [C.c_void_p]
    lib.pt_version.restype = C.c_char_p
    lib.pt_destroy.restype = None
    lib.pt_destroy.argtypes = [C.c_void_p]
    return lib


# torch ships its own copy of the HIP runtime, and one process can drive the GPU through one copy only: libmi355pt binds to torch's when
# torch was imported first (bench.py does that).  The torch route of the ray queries needs that, and checks it.
_TORCH_FIRST = "torch" in sys.modules
lib = _load()


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _aligned_zeros(shape, dtype, align=16):
    """A zeroed numpy array whose data starts on an `align`-byte boundary (what the ray-query entry points require)."""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape)) * dtype.itemsize
    raw = np.zeros(n + align, np.uint8)
    off = (-raw.ctypes.data) % align
    return raw[off: off + n].view(dtype).reshape(shape)


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _torch_route():
    if not _TORCH_FIRST:
        raise RuntimeError("the torch route of the ray queries needs `import torch` before this package is imported: both must use "
                           "the same HIP runtime (torch ships its own)")


EXPOSE_GATES = (0.0999, 0.2999)      # the two tiers' f64 gates (pt_expose.h: kGate, kGate2)


def exposure_flags_host(tris, s_max, d_max, gate=None):
    """CPU twin of the exposure mask: bool per triangle (every pair tested; no GPU).  gate: None = the first tier's, or the f64 bound on
    |n . d| / |d| of the hits covered (EXPOSE_GATES)."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    n = tris.size // 9
    words = ((n + 63) // 64) * 2
    bits = np.zeros(max(words, 1), np.uint32); cnt = C.c_uint32()
    if gate is None:
        _check(lib.pt_exposure_flags_host(_p(tris, C.c_float), C.c_uint32(n), C.c_double(s_max), C.c_double(d_max), _p(bits, C.c_uint32), C.c_uint32(words), C.byref(cnt)))
    else:
        _check(lib.pt_exposure_flags_host_gate(_p(tris, C.c_float), C.c_uint32(n), C.c_double(s_max), C.c_double(d_max), C.c_double(gate), _p(bits, C.c_uint32), C.c_uint32(words), C.byref(cnt)))
    return np.unpackbits(bits.view(np.uint8), bitorder="little").astype(bool)[:n]


def pack_rays(origins, directions, t_max=None):
    """numpy: (n, 8) float32 PtRay records (org xyz, t_max, dir xyz, 0) in a 16-byte aligned buffer; t_max None = +inf, a scalar or (n,)."""
    o = np.asarray(origins, np.float32).reshape(-1, 3)
    d = np.asarray(directions, np.float32).reshape(-1, 3)
    if o.shape != d.shape:
        raise ValueError("origins and directions differ in shape: %s vs %s" % (o.shape, d.shape))
    out = _aligned_zeros((o.shape[0], 8), np.float32)
    out[:, 0:3] = o
    out[:, 3] = np.inf if t_max is None else np.broadcast_to(np.asarray(t_max, np.float32), (o.shape[0],))
    out[:, 4:7] = d
    return out


def pack_points(points, r_max=None):
    """numpy: (n, 4) float32 PtPoint records (x, y, z, r_max) in a 16-byte aligned buffer; r_max None = +inf, a scalar or (n,)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    out = _aligned_zeros((p.shape[0], 4), np.float32)
    out[:, 0:3] = p
    out[:, 3] = np.inf if r_max is None else np.broadcast_to(np.asarray(r_max, np.float32), (p.shape[0],))
    return out


def _records(a, overrides=()):
    """The one numpy rule: aligned contiguous float32 (n, w) records for the C side.  The caller's array when it already qualifies and nothing
    is overridden, a copy otherwise.  overrides: (column, value) pairs; a value of None leaves the column as it is."""
    rec = a
    if rec.ctypes.data % 16 or not rec.flags.c_contiguous:
        rec = _aligned_zeros(a.shape, a.dtype); rec[...] = a
    for c, v in overrides:
        if v is not None:
            if rec is a:
                rec = _aligned_zeros(a.shape, a.dtype); rec[...] = a       # (the caller's records are never written)
            rec[:, c] = v
    return rec


def _torch_device(t, what):
    """the device of a torch argument of query `what`, which must be the context's GPU"""
    _torch_route()
    if t.device.type != "cuda":
        raise ValueError("%s: torch tensors must be on the context's GPU (got %s)" % (what, t.device))
    return t.device


def _torch_records(t, what, overrides=(), dtype="float32", width=None):
    """The one torch rule, the same as _records: aligned contiguous `dtype` records on the context's GPU (reshaped to `width` words each
    where one is given), the caller's tensor when it already qualifies and nothing is overridden."""
    import torch
    _torch_device(t, what)
    rec, dtype = t if width is None else t.reshape(-1, width), getattr(torch, dtype)
    if rec.dtype != dtype or not rec.is_contiguous() or rec.data_ptr() % 16:
        rec = rec.to(dtype).contiguous().clone()
    for c, v in overrides:
        if v is not None:
            rec = rec.clone() if rec.data_ptr() == t.data_ptr() else rec       # (a copy only while the records still alias the caller's tensor)
            rec[:, c] = v
    return rec


def _torch_column(value, n, dev, default):
    """(n, 1) float32 on dev: `default` where value is None, else the scalar or (n,) value"""
    import torch
    if value is None:
        return torch.full((n, 1), default, dtype=torch.float32, device=dev)
    return torch.as_tensor(value, dtype=torch.float32, device=dev).reshape(-1, 1).expand(n, 1)


def _point_records(points, r_max, what=None):
    """(n, 3) points + r_max, or (n, 4) PtPoint records (r_max None: taken from the records) -> aligned (n, 4) float32 records; of a torch
    tensor (`what` names the query in its errors) the same as a tensor."""
    if _is_torch(points):
        if points.dim() == 2 and points.shape[1] == 4:
            return _torch_records(points, what, ((3, r_max),))
        import torch
        dev, p = _torch_device(points, what), points.reshape(-1, 3).to(torch.float32)
        return torch.cat([p, _torch_column(r_max, p.shape[0], dev, float("inf"))], dim=1).contiguous()
    a = np.asarray(points, np.float32)
    return _records(a, ((3, r_max),)) if a.ndim == 2 and a.shape[1] == 4 else pack_points(a, r_max)


def pack_sweeps(origins, directions, radius, t_max=None):
    """numpy: (n, 8) float32 PtSweep records (org xyz, t_max, dir xyz, radius) in a 16-byte aligned buffer; radius a scalar or (n,); t_max
    None = +inf, a scalar or (n,)."""
    out = pack_rays(origins, directions, t_max)
    out[:, 7] = np.broadcast_to(np.asarray(radius, np.float32), (out.shape[0],))
    return out


def _sweep_records(origins, directions, radius, t_max, what=None):
    """(n, 3) origins + directions + radius + t_max, or (n, 8) PtSweep records (directions None; radius, t_max None: taken from the records)
    -> aligned (n, 8) float32 records; of torch tensors the same as a tensor."""
    if directions is None:
        return _ray_records(origins, None, t_max, what, radius)
    if _is_torch(origins):
        rec = _ray_records(origins, directions, t_max, what)
        rec[:, 7] = 0.0 if radius is None else radius
        return rec
    return pack_sweeps(origins, directions, 0.0 if radius is None else radius, t_max)


def pack_boxes(lo, hi):
    """numpy: (n, 8) float32 PtBox records (lo xyz, 0, hi xyz, 0) in a 16-byte aligned buffer."""
    a = np.asarray(lo, np.float32).reshape(-1, 3)
    b = np.asarray(hi, np.float32).reshape(-1, 3)
    if a.shape != b.shape:
        raise ValueError("lo and hi differ in shape: %s vs %s" % (a.shape, b.shape))
    out = _aligned_zeros((a.shape[0], 8), np.float32)
    out[:, 0:3] = a
    out[:, 4:7] = b
    return out


def _box_records(lo, hi, what=None):
    """(n, 3) lo + hi, or (n, 8) PtBox records (hi None) -> aligned (n, 8) float32 records; of torch tensors the same as a tensor."""
    if not _is_torch(lo):
        return pack_boxes(lo, hi) if hi is not None else _records8(lo, "box records")
    import torch
    dev = _torch_device(lo, what)
    if hi is None:
        if lo.dim() != 2 or lo.shape[1] != 8:
            raise ValueError("%s: expected (n, 8) PtBox records or lo and hi of shape (n, 3), got shape %s" % (what, tuple(lo.shape)))
        return _torch_records(lo, what)
    a = lo.reshape(-1, 3).to(torch.float32); b = hi.reshape(-1, 3).to(device=dev, dtype=torch.float32)
    if a.shape != b.shape:
        raise ValueError("%s: lo and hi differ in shape: %s vs %s" % (what, tuple(a.shape), tuple(b.shape)))
    z = torch.zeros((a.shape[0], 1), dtype=torch.float32, device=dev)
    return torch.cat([a, z, b, z], dim=1).contiguous()


def pack_tris(verts):
    """numpy: (n, 12) float32 PtTri records (v0 xyz, 0, v1 xyz, 0, v2 xyz, 0) in a 16-byte aligned buffer, from (n, 3, 3) or (n, 9) vertices."""
    v = np.asarray(verts, np.float32).reshape(-1, 3, 3)
    out = _aligned_zeros((v.shape[0], 12), np.float32)
    out.reshape(-1, 3, 4)[:, :, 0:3] = v
    return out


def _tri_records(tris, what=None):
    """(n, 3, 3) or (n, 9) vertices, or (n, 12) PtTri records -> aligned (n, 12) float32 records; of a torch tensor the same as a tensor."""
    if not _is_torch(tris):
        a = np.asarray(tris, np.float32)
        return _records(a) if a.ndim == 2 and a.shape[1] == 12 else pack_tris(a)
    if tris.dim() == 2 and tris.shape[1] == 12:
        return _torch_records(tris, what)
    import torch
    dev = _torch_device(tris, what)
    if tuple(tris.shape[1:]) not in ((3, 3), (9,)):
        raise ValueError("%s: expected (n, 12) PtTri records or vertices of shape (n, 3, 3) or (n, 9), got shape %s" % (what, tuple(tris.shape)))
    v = tris.reshape(-1, 3, 3).to(torch.float32)
    return torch.cat([v, torch.zeros((v.shape[0], 3, 1), dtype=torch.float32, device=dev)], dim=2).reshape(-1, 12).contiguous()


CUT_WINDOW = 32.0        # the default window of a plane-cut record: [-32, 32]^3, the largest the completeness claim covers


def pack_cuts(normal, d, lo=None, hi=None):
    """numpy: (n, 12) float32 PtCutPlane records (n xyz, d, lo xyz, 0, hi xyz, 0) in a 16-byte aligned buffer.  normal: one normal (3,) or
    (n, 3); d: a scalar or (n,); lo, hi: the window, one corner (3,) or (n, 3) each, None = -32 and +32 on every axis."""
    nv = np.asarray(normal, np.float32).reshape(-1, 3)
    dv = np.asarray(d, np.float32).reshape(-1)
    a = np.asarray(-CUT_WINDOW if lo is None else lo, np.float32)
    b = np.asarray(CUT_WINDOW if hi is None else hi, np.float32)
    n = max(nv.shape[0], dv.shape[0], a.size // 3, b.size // 3)
    out = _aligned_zeros((n, 12), np.float32)
    try:
        out[:, 0:3] = nv
        out[:, 3] = dv
        out[:, 4:7] = a if a.ndim == 0 else a.reshape(-1, 3)
        out[:, 8:11] = b if b.ndim == 0 else b.reshape(-1, 3)
    except ValueError:
        raise ValueError("normal, d, lo and hi differ in length: %s, %s, %s, %s" % (nv.shape, dv.shape, a.shape, b.shape)) from None
    return out


def _cut_records(normal, d, lo, hi, what=None):
    """normal + d (+ lo, hi), or (n, 12) PtCutPlane records (d None) -> aligned (n, 12) float32 records; of torch tensors the same as a
    tensor."""
    if not _is_torch(normal):
        if d is not None:
            return pack_cuts(normal, d, lo, hi)
        a = np.asarray(normal, np.float32)
        if a.ndim != 2 or a.shape[1] != 12:
            raise ValueError("%s: expected (n, 12) PtCutPlane records or a normal and d, got shape %s" % (what or "cut records", a.shape))
        return _records(a)
    import torch
    dev = _torch_device(normal, what)
    if d is None:
        if normal.dim() != 2 or normal.shape[1] != 12:
            raise ValueError("%s: expected (n, 12) PtCutPlane records or a normal and d, got shape %s" % (what, tuple(normal.shape)))
        return _torch_records(normal, what)
    nv = normal.reshape(-1, 3).to(torch.float32)
    dv = torch.as_tensor(d, dtype=torch.float32, device=dev).reshape(-1, 1)
    a = torch.as_tensor(-CUT_WINDOW if lo is None else lo, dtype=torch.float32, device=dev)
    b = torch.as_tensor(CUT_WINDOW if hi is None else hi, dtype=torch.float32, device=dev)
    a = a.reshape(1, 1) if a.dim() == 0 else a.reshape(-1, 3)
    b = b.reshape(1, 1) if b.dim() == 0 else b.reshape(-1, 3)
    n = max(nv.shape[0], dv.shape[0], a.shape[0], b.shape[0])
    z = torch.zeros((n, 1), dtype=torch.float32, device=dev)
    try:
        return torch.cat([nv.expand(n, 3), dv.expand(n, 1), a.expand(n, 3), z, b.expand(n, 3), z], dim=1).contiguous()
    except RuntimeError:
        raise ValueError("%s: normal, d, lo and hi differ in length: %s, %s, %s, %s" % (what, tuple(nv.shape), tuple(dv.shape), tuple(a.shape), tuple(b.shape))) from None


_CUT_EDGES = np.array([[0, 1], [1, 2], [0, 2]], np.int64)     # the vertices of edge bit 0, 1, 2


def cut_segments(tris, prim, code, t0, t1):
    """The segments of cut_search's entries: (m, 2, 3) float32, from the caller's own vertices tris ((num_tris, 3, 3) or (num_tris, 9), the
    mesh the context holds) and the entry columns (numpy).  Each end point is va + t (vb - va), evaluated in float64 and rounded once.
    segments[:, 0] lies on the lowest crossing edge of the triangle (the lowest set bit of code & 7, in the order v0-v1, v1-v2, v0-v2)
    at t0, segments[:, 1] on the highest at t1; va is that edge's vertex below the plane (its class bit in code is 0) and vb the one on or
    above it, so t runs from below the plane upwards.  t0 and t1 come from the f32 records the tree stores (v0, v1 - v0, v2 - v0), not from
    `tris`: two triangles that share an edge give the same point on it only as far as their record vertices agree and the edge has the
    same direction in both, which is to within a few float32 roundings, not bit for bit."""
    v = np.asarray(tris, np.float64).reshape(-1, 3, 3)[np.asarray(prim, np.int64)]
    code = np.asarray(code, np.int64)
    m = code.shape[0]
    lowest = np.where(code & 1, 0, 1)
    highest = np.where(code & 4, 2, 1)
    out = np.empty((m, 2, 3), np.float32)
    rows = np.arange(m)
    for end, (edge, t) in enumerate(((lowest, t0), (highest, t1))):
        i, j = _CUT_EDGES[edge, 0], _CUT_EDGES[edge, 1]
        i_above = ((code >> (3 + i)) & 1).astype(bool)
        a, b = np.where(i_above, j, i), np.where(i_above, i, j)
        va, vb = v[rows, a], v[rows, b]
        out[:, end] = va + np.asarray(t, np.float64)[:, None] * (vb - va)
    return out


def pack_surfels(points, normals, r_max=None):
    """numpy: (n, 8) float32 PtSurfel records (p xyz, r_max, n xyz, 0) in a 16-byte aligned buffer; r_max None = +inf, a scalar or (n,)."""
    return pack_rays(points, normals, r_max)


def _records8(a, what):
    """(n, 8) float32 records in a 16-byte aligned, contiguous numpy buffer (the caller's array when it already is one); of a torch tensor
    the same as a tensor."""
    if _is_torch(a):
        return _torch_records(a, what, width=8)
    a = np.asarray(a, np.float32)
    if a.ndim != 2 or a.shape[1] != 8:
        raise ValueError("%s: expected (n, 8) float32 records, got shape %s" % (what, a.shape))
    return _records(a)


# one flag word serves every query but trace_rays (whose bit 1 is PT_TRACE_ANY_HIT): the headers' constants share their values, as the C
# front end asserts for box and radius
_QUERY_STATS, _QUERY_SIMPLE_KERNEL, _QUERY_BRUTE_FORCE = 1, 2, 4
assert {PT_CLOSEST_STATS, PT_OCCLUSION_STATS, PT_COUNT_STATS, PT_CONTAIN_STATS, PT_RADIUS_STATS, PT_HITS_STATS, PT_BOX_STATS, PT_TRI_STATS, PT_CUT_STATS,
        PT_SWEEP_STATS, PT_NEAREST_STATS} == {_QUERY_STATS}
assert {PT_CLOSEST_SIMPLE_KERNEL, PT_OCCLUSION_SIMPLE_KERNEL, PT_COUNT_SIMPLE_KERNEL, PT_CONTAIN_SIMPLE_KERNEL, PT_RADIUS_SIMPLE_KERNEL,
        PT_HITS_SIMPLE_KERNEL, PT_BOX_SIMPLE_KERNEL, PT_TRI_SIMPLE_KERNEL, PT_CUT_SIMPLE_KERNEL, PT_SWEEP_SIMPLE_KERNEL, PT_NEAREST_SIMPLE_KERNEL} == {_QUERY_SIMPLE_KERNEL}
assert {PT_CLOSEST_BRUTE_FORCE, PT_COUNT_BRUTE_FORCE, PT_RADIUS_BRUTE_FORCE, PT_HITS_BRUTE_FORCE, PT_BOX_BRUTE_FORCE, PT_TRI_BRUTE_FORCE, PT_CUT_BRUTE_FORCE, PT_SWEEP_BRUTE_FORCE,
        PT_NEAREST_BRUTE_FORCE} == {_QUERY_BRUTE_FORCE}


def _flags(stats, simple, brute_force=False, sort=False):
    """the flag word of a query: PT_*_STATS | PT_*_SIMPLE_KERNEL | PT_*_BRUTE_FORCE | PT_HITS_SORTED"""
    return (_QUERY_STATS if stats else 0) | (_QUERY_SIMPLE_KERNEL if simple else 0) | (_QUERY_BRUTE_FORCE if brute_force else 0) | (PT_HITS_SORTED if sort else 0)


def _occlusion_params(samples, seed, bias, index_base, stats=False, simple=False):
    p = PtOcclusionParams()
    p.samples, p.seed, p.index_base, p.bias = int(samples), int(seed) & 0xFFFFFFFF, int(index_base) & 0xFFFFFFFF, float(bias)
    p.flags = _flags(stats, simple)
    return p


def occlusion_rays_host(surfels, samples, seed=0, bias=1e-4, index_base=0):
    """Host twin of Context.occlusion_rays (no GPU): the n * samples sample rays of (n, 8) PtSurfel records as (n * samples, 8) float32 PtRay
    records, sample s of surfel i at i * samples + s, with the bits the device produces."""
    sf = _records8(surfels, "occlusion_rays_host")
    n = sf.shape[0]
    p = _occlusion_params(samples, seed, bias, index_base)
    rays = _aligned_zeros((n * max(int(samples), 0) if 0 < int(samples) <= 65536 else 0, 8), np.float32)
    _check(lib.pt_occlusion_rays_host(sf.ctypes.data_as(C.POINTER(PtSurfel)), C.c_uint64(n), C.byref(p), rays.ctypes.data_as(C.POINTER(PtRay))))
    return rays


def _contain_params(samples, seed, index_base, stats=False, simple=False):
    p = PtContainParams()
    p.samples, p.seed, p.index_base = int(samples) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFF, int(index_base) & 0xFFFFFFFF
    p.flags = _flags(stats, simple)
    return p


def _ray_records(origins, directions, t_max, what=None, radius=None):
    """(n, 3) origins + directions + t_max, or (n, 8) PtRay records (t_max None: taken from the records) -> aligned (n, 8) float32 records
    (radius: a sweep's, over the eighth float of packed records); of torch tensors the same as a tensor."""
    if _is_torch(origins):
        if directions is None:
            return _torch_records(origins, what, ((3, t_max), (7, radius)), width=8)
        import torch
        dev, o = _torch_device(origins, what), origins.reshape(-1, 3).to(torch.float32)
        d, n = directions.reshape(-1, 3).to(device=dev, dtype=torch.float32), o.shape[0]
        return torch.cat([o, _torch_column(t_max, n, dev, float("inf")), d, _torch_column(None, n, dev, 0.0)], dim=1).contiguous()
    if directions is not None:
        return pack_rays(origins, directions, t_max)
    return _records(np.asarray(origins, np.float32).reshape(-1, 8), ((3, t_max), (7, radius)))   # (numpy's own error for a wrong size)


def _check(rc, ctx=None):
    if rc != 0:
        msg = lib.pt_last_error(ctx)
        raise PtError(rc, msg.decode() if msg else "")


def focal_aspect(width, height):
    """PathTracer.js:761-769: fov 70 degrees; doubles on the host, f32 in the UBO."""
    fov = (70.0 * math.pi) / 180
    return float(np.float32(1.0 / math.tan(0.5 * fov))), float(np.float32(width / height))


# ---- host-side functions (no GPU) ---------------------------------------------------------

def compute_bvh2_sizing(num_tris):
    nn, by = C.c_uint32(), C.c_uint64()
    _check(lib.pt_compute_bvh2_sizing(C.c_uint32(num_tris), C.byref(nn), C.byref(by)))
    return {"numNodes2": nn.value, "bytes": by.value}


def compute_bvh4_sizing(num_nodes4):
    by = C.c_uint64()
    _check(lib.pt_compute_bvh4_sizing(C.c_uint32(num_nodes4), C.byref(by)))
    return {"bytes": by.value}


def morton_sort(tris):
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    n = tris.size // 9
    m = np.zeros(n, np.uint32); t = np.zeros(n, np.uint32)
    _check(lib.pt_morton_sort(_p(tris, C.c_float), C.c_uint32(n), _p(m, C.c_uint32), _p(t, C.c_uint32)))
    return m, t


def collapse_lbvh2_to_bvh4(bvh2, num_tris):
    bvh2 = np.ascontiguousarray(bvh2, np.uint32)
    cap = 1 + 8 * max(2 * num_tris - 1, 0)
    out = np.zeros(cap, np.uint32)
    n4 = C.c_uint32()
    _check(lib.pt_collapse_lbvh2_to_bvh4(_p(bvh2, C.c_uint32), C.c_uint32(num_tris), _p(out, C.c_uint32), C.c_uint64(cap), C.byref(n4)))
    return out[: 1 + 8 * n4.value].copy(), n4.value


def collapse_bvh2_to_bvh4_accel(bvh2, num_tris, accel):
    """The collapse of build level `accel` on the host (1, 2: area-guided, needs a complete BVH2); returns (bvh4, numNodes4)."""
    bvh2 = np.ascontiguousarray(bvh2, np.uint32)
    cap = 1 + 8 * max(2 * num_tris - 1, 0)
    out = np.zeros(cap, np.uint32)
    n4 = C.c_uint32()
    _check(lib.pt_collapse_bvh2_to_bvh4_accel(_p(bvh2, C.c_uint32), C.c_uint32(num_tris), C.c_uint32(accel), _p(out, C.c_uint32),
                                              C.c_uint64(cap), C.byref(n4)))
    return out[: 1 + 8 * n4.value].copy(), n4.value


def build_bvh2_ploc(tris):
    """The PLOC BVH2 of PT_ACCEL_PLOC on the host, refit bounds included (what Context.read_bvh2 returns after build_bvh(accel=2))."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    n = tris.size // 9
    out = np.zeros(1 + 6 * max(2 * n - 1, 0), np.uint32)
    _check(lib.pt_build_bvh2_ploc(_p(tris, C.c_float), C.c_uint32(n), _p(out, C.c_uint32), C.c_uint64(out.size)))
    return out


def bvh2_to_bvh4_wide(bvh2):
    bvh2 = np.ascontiguousarray(bvh2, np.uint32)
    out = np.zeros(1 + 8 * int(bvh2[0]), np.uint32)
    _check(lib.pt_bvh2_to_bvh4_wide(_p(bvh2, C.c_uint32), C.c_uint64(bvh2.size), _p(out, C.c_uint32), C.c_uint64(out.size)))
    return out


def refit_bvh4(tris, bvh4):
    """Host twin of Context.update_triangles: the BVH4 words for the same topology and the triangles `tris` (a new array)."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    out = np.array(bvh4, np.uint32).reshape(-1)
    _check(lib.pt_refit_bvh4(_p(tris, C.c_float), C.c_uint32(tris.size // 9), _p(out, C.c_uint32), C.c_uint64(out.size)))
    return out


def _bvh4_arg(bvh4):
    if bvh4 is None:
        return None, None, 0
    bvh4 = np.ascontiguousarray(bvh4, np.uint32).reshape(-1)
    return bvh4, _p(bvh4, C.c_uint32), bvh4.size


def _unpack(rec, cols):
    """(..., 4) uint32 result records -> their leading columns as copies: 'f' a float32 column, 'u' a uint32 one (PtHit and PtClosest are
    "fuff": t | dist, prim, u, v).  cols None: uint32 counts, as they are.  Of a torch int32 tensor the same, as views of it."""
    if isinstance(rec, np.ndarray):
        f = rec.view(np.float32)
        return rec if cols is None else tuple([(f if c == "f" else rec)[..., i].copy() for i, c in enumerate(cols)])
    import torch
    u = rec.view(torch.uint32)
    return u if cols is None else tuple([(rec.view(torch.float32) if c == "f" else u)[..., i] for i, c in enumerate(cols)])


# What both routes and the twin of a query read.  record: the ctypes type of an input record (its width is sizeof / 4 floats); entry: that of
# a result; cols, tail: the result kind (_unpack's columns; the shape of one record's results in words); guess: of a list query, the entries
# per record of the host route's first run; device, host, twin: the C entry points (twin None where there is none).
_Query = collections.namedtuple("_Query", "record entry cols tail guess device host twin")


def _query(name, record, entry, cols, tail=(4,), guess=0):
    return _Query(record, entry, cols, tail, guess, getattr(lib, "pt_" + name), getattr(lib, "pt_%s_host" % name), getattr(lib, "pt_%s_bvh4" % name, None))


_TRACE = _query("trace_rays", PtRay, PtHit, "fuff")
_CLOSEST = _query("closest_points", PtPoint, PtClosest, "fuff")
_SWEEP = _query("sweep_spheres", PtSweep, PtHit, "fuff")
_NEAREST = _query("nearest_k", PtPoint, PtClosest, "fuff")                  # tail: (k, 4), the caller's
_SIGNED = _query("signed_distance", PtPoint, PtClosest, "fuff")
_OCCLUSION = _query("occlusion", PtSurfel, PtOcclusion, "fuu")
_CONTAINS = _query("contains", PtPoint, PtContainment, "uuu")
_COUNT = _query("count_hits", PtRay, C.c_uint32, None, ())
_RADIUS_COUNT = _query("radius_count", PtPoint, C.c_uint32, None, ())
_BOX_COUNT = _query("box_count", PtBox, C.c_uint32, None, ())
_RADIUS = _query("radius_search", PtPoint, PtClosest, "fuff", guess=16)
_BOX = _query("box_search", PtBox, PtOverlap, "uu", guess=16)               # (two columns, not four: prim, verts_inside)
_TRI_COUNT = _query("tri_count", PtTri, C.c_uint32, None, ())
_TRI = _query("tri_search", PtTri, PtCross, "uu", guess=16)                 # (two columns: prim, edges)
_CUT_COUNT = _query("cut_count", PtCutPlane, C.c_uint32, None, ())
_CUT = _query("cut_search", PtCutPlane, PtCut, "uuff", guess=16)            # (prim, code, t0, t1)
_HITS = _query("list_hits", PtRay, PtHit, "fuff", guess=4)


def _twin(q, tris, bvh4, rec, extra, stats, tail=None, capacity=None):
    """The host twin of query q (no GPU) for the triangles `tris` under the tree `bvh4` and the numpy records `rec`; extra: the ctypes
    arguments between the record count and the results.  Returns what the query does, and the counters as a dict after it with stats."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    keep, bp, words = _bvh4_arg(bvh4)
    n, st = rec.shape[0], PtStats()

    def call(*results):
        _check(q.twin(_p(tris, C.c_float), C.c_uint32(tris.size // 9), bp, C.c_uint64(words), rec.ctypes.data_as(C.POINTER(q.record)), C.c_uint64(n),
                      *extra, *results, C.byref(st) if stats else None))
    if q.guess:                                         # a list query: capacity None runs it twice, once for the total
        offsets = np.zeros(n + 1, np.uint64)
        if capacity is None:
            call(_p(offsets, C.c_uint64), None, C.c_uint64(0))
            capacity = int(offsets[n])
        capacity = int(capacity)
        entries = _aligned_zeros((capacity, 4), np.uint32)
        call(_p(offsets, C.c_uint64), entries.ctypes.data_as(C.POINTER(q.entry)) if capacity else None, C.c_uint64(capacity))
        res = (offsets,) + _unpack(entries[: min(int(offsets[n]), capacity)], q.cols)
    else:
        out = _aligned_zeros((n,) + (q.tail if tail is None else tail), np.uint32)
        call(out.ctypes.data_as(C.POINTER(q.entry)))
        res = _unpack(out, q.cols)
    if not stats:
        return res
    return (res if isinstance(res, tuple) else (res,)) + (st.as_dict(),)


def closest_points_bvh4(tris, bvh4, points, r_max=None, stats=False, simple=False, brute_force=False):
    """Host twin of Context.closest_points (no GPU): the nearest triangle of `tris` to each point over the tree set_bvh4(bvh4) installs, with
    the device's bits.  bvh4 None needs brute_force=True.  Returns (dist, prim, u, v), and the counters as a dict in fifth place with stats=True."""
    return _twin(_CLOSEST, tris, bvh4, _point_records(points, r_max), (C.c_uint32(_flags(stats, simple, brute_force)),), stats)


def sweep_spheres_bvh4(tris, bvh4, origins, directions=None, radius=None, t_max=None, stats=False, simple=False, brute_force=False):
    """Host twin of Context.sweep_spheres (no GPU): the first contact of each moving sphere with `tris` over the tree set_bvh4(bvh4)
    installs, with the device's bits.  bvh4 None needs brute_force=True.  Returns (t, prim, u, v), and the counters as a dict in fifth place
    with stats=True."""
    return _twin(_SWEEP, tris, bvh4, _sweep_records(origins, directions, radius, t_max), (C.c_uint32(_flags(stats, simple, brute_force)),), stats)


def count_hits_bvh4(tris, bvh4, origins, directions=None, t_max=None, stats=False, simple=False, brute_force=False):
    """Host twin of Context.count_hits (no GPU): how many triangles of `tris` each ray crosses over the tree set_bvh4(bvh4) installs, with
    the device's counts.  bvh4 None needs brute_force=True.  Returns the (n,) uint32 counts, and the counters as a dict in second place
    with stats=True."""
    return _twin(_COUNT, tris, bvh4, _ray_records(origins, directions, t_max), (C.c_uint32(_flags(stats, simple, brute_force)),), stats)


def radius_search_bvh4(tris, bvh4, points, r_max=None, capacity=None, stats=False, simple=False, brute_force=False):
    """Host twin of Context.radius_search (no GPU): every triangle of `tris` within r_max of each point over the tree set_bvh4(bvh4) installs,
    with the device's bits and order.  bvh4 None needs brute_force=True.  Returns (offsets, dist, prim, u, v): offsets (n + 1,) uint64, the
    list of point i at offsets[i]:offsets[i + 1], in visit order (index order with brute_force).  capacity None: every entry (the twin runs
    twice, once for the total); else the first min(offsets[-1], capacity) entries, offsets complete.  The counters as a dict in sixth place
    with stats=True."""
    return _twin(_RADIUS, tris, bvh4, _point_records(points, r_max), (C.c_uint32(_flags(stats, simple, brute_force)),), stats, capacity=capacity)


def box_search_bvh4(tris, bvh4, lo, hi=None, capacity=None, stats=False, simple=False, brute_force=False):
    """Host twin of Context.box_search (no GPU): every triangle of `tris` that overlaps each box over the tree set_bvh4(bvh4) installs, with
    the device's words and order.  bvh4 None needs brute_force=True.  lo, hi: (n, 3) corners, or lo alone as (n, 8) PtBox records.  Returns
    (offsets, prim, verts_inside): offsets (n + 1,) uint64, the list of box i at offsets[i]:offsets[i + 1], in visit order (index order with
    brute_force).  capacity None: every entry (the twin runs twice, once for the total); else the first min(offsets[-1], capacity) entries,
    offsets complete.  The counters as a dict in fourth place with stats=True."""
    return _twin(_BOX, tris, bvh4, _box_records(lo, hi), (C.c_uint32(_flags(stats, simple, brute_force)),), stats, capacity=capacity)


def tri_search_bvh4(mesh, bvh4, tris, capacity=None, stats=False, simple=False, brute_force=False):
    """Host twin of Context.tri_search (no GPU): every triangle of `mesh` that each caller triangle cuts over the tree set_bvh4(bvh4)
    installs, with the device's words and order.  bvh4 None needs brute_force=True.  tris: (n, 3, 3) or (n, 9) vertices, or (n, 12) PtTri
    records.  Returns (offsets, prim, edges): offsets (n + 1,) uint64, the list of caller triangle i at offsets[i]:offsets[i + 1], in visit
    order (index order with brute_force).  capacity None: every entry (the twin runs twice, once for the total); else the first
    min(offsets[-1], capacity) entries, offsets complete.  The counters as a dict in fourth place with stats=True."""
    return _twin(_TRI, mesh, bvh4, _tri_records(tris), (C.c_uint32(_flags(stats, simple, brute_force)),), stats, capacity=capacity)


def cut_search_bvh4(tris, bvh4, normal, d=None, lo=None, hi=None, capacity=None, stats=False, simple=False, brute_force=False):
    """Host twin of Context.cut_search (no GPU): every triangle of `tris` that each plane cuts inside its window over the tree
    set_bvh4(bvh4) installs, with the device's words and order.  bvh4 None needs brute_force=True.  normal, d, lo, hi: as pack_cuts, or
    normal alone as (n, 12) PtCutPlane records.  Returns (offsets, prim, code, t0, t1): offsets (n + 1,) uint64, the list of plane i at
    offsets[i]:offsets[i + 1], in visit order (index order with brute_force).  capacity None: every entry (the twin runs twice, once for the
    total); else the first min(offsets[-1], capacity) entries, offsets complete.  The counters as a dict in sixth place with stats=True."""
    return _twin(_CUT, tris, bvh4, _cut_records(normal, d, lo, hi), (C.c_uint32(_flags(stats, simple, brute_force)),), stats, capacity=capacity)


def list_hits_bvh4(tris, bvh4, origins, directions=None, t_max=None, capacity=None, sort=False, stats=False, simple=False, brute_force=False):
    """Host twin of Context.list_hits (no GPU): every triangle of `tris` each ray crosses over the tree set_bvh4(bvh4) installs, with the
    device's bits and order.  bvh4 None needs brute_force=True.  Returns (offsets, t, prim, u, v): offsets (n + 1,) uint64, the list of ray i
    at offsets[i]:offsets[i + 1], in visit order (index order with brute_force; ascending (t, prim) with sort=True).  capacity None: every
    entry (the twin runs twice, once for the total); else the first min(offsets[-1], capacity) entries, offsets complete.  The counters as
    a dict in sixth place with stats=True."""
    return _twin(_HITS, tris, bvh4, _ray_records(origins, directions, t_max), (C.c_uint32(_flags(stats, simple, brute_force, sort)),), stats,
                 capacity=capacity)


def nearest_k_bvh4(tris, bvh4, points, k, r_max=None, stats=False, simple=False, brute_force=False):
    """Host twin of Context.nearest_k (no GPU): the k triangles of `tris` nearest to each point over the tree set_bvh4(bvh4) installs, with the
    device's bits and order.  bvh4 None needs brute_force=True.  Returns (dist, prim, u, v), each (n, k): row i in ascending order of
    distance, padded with dist = +inf and prim = 0xFFFFFFFF.  The counters as a dict in fifth place with stats=True."""
    k = int(k)                                          # (the rows are sized for a k in range; the C side refuses any other)
    return _twin(_NEAREST, tris, bvh4, _point_records(points, r_max), (C.c_uint32(k & 0xFFFFFFFF), C.c_uint32(_flags(stats, simple, brute_force))), stats,
                 tail=(min(max(k, 0), PT_NEAREST_MAX_K), 4))


def contains_bvh4(tris, bvh4, points, samples=3, seed=0, index_base=0, stats=False, simple=False):
    """Host twin of Context.contains (no GPU): (inside, odd, samples) per point, and the counters as a dict in fourth place with stats=True."""
    p = _contain_params(samples, seed, index_base, stats, simple)
    return _twin(_CONTAINS, tris, bvh4, _point_records(points, None), (C.byref(p),), stats)     # (r_max is ignored)


def refit_bvh2(tris, bvh2):
    """The BVH2 words Context.read_bvh2 returns after update_triangles(tris): leaf rule + the reference's propagateUp (a new array)."""
    tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
    out = np.array(bvh2, np.uint32).reshape(-1)
    _check(lib.pt_refit_bvh2(_p(tris, C.c_float), C.c_uint32(tris.size // 9), _p(out, C.c_uint32), C.c_uint64(out.size)))
    return out


def bvh4_cost(bvh4):
    """Host twin of Context.bvh_cost: sum over reachable internal nodes of halfArea(node) / halfArea(root), f64."""
    bvh4 = np.ascontiguousarray(bvh4, np.uint32).reshape(-1)
    cost = C.c_double()
    _check(lib.pt_bvh4_cost(_p(bvh4, C.c_uint32), C.c_uint64(bvh4.size), C.byref(cost)))
    return cost.value


def write_u32_file(path, words):
    words = np.ascontiguousarray(words, np.uint32)
    _check(lib.pt_file_write_u32(path.encode(), _p(words, C.c_uint32), C.c_uint64(words.size)))


def read_u32_file(path):
    n = C.c_uint64()
    _check(lib.pt_file_read_u32(path.encode(), None, C.c_uint64(0), C.byref(n)))
    out = np.zeros(n.value, np.uint32)
    _check(lib.pt_file_read_u32(path.encode(), _p(out, C.c_uint32), C.c_uint64(out.size), C.byref(n)))
    return out


def procedural_scene(kind, num_tris, seed=20260109):
    out = np.zeros(num_tris * 9, np.float32)
    _check(lib.pt_scene_procedural(C.c_uint32(kind), C.c_uint32(seed), C.c_uint32(num_tris), _p(out, C.c_float)))
    return out


PLAN_FIELDS = ("grid", "perm_rows", "perm_cols", "total_items", "chunk_items", "xcd_span", "shade_threshold", "fill_threshold", "quad_live", "fork_shadow", "slots", "setup_slots")


def debug_launch_plan_tuned(num_cus, frames, tile_count=1, launches_in_flight=0, traced_batches=1, batch_size=None, tune=None):
    """Diagnostics: the megakernel's launch plan (a dict over PLAN_FIELDS) for a launch shape under the knob overrides of `tune` ({name: value}), as a
    pure function: no GPU, no context.  Raises PtError where the host would refuse the launch."""
    tune = dict(tune or {})
    names = (C.c_char_p * max(len(tune), 1))(*[k.encode() for k in tune])
    values = (C.c_uint32 * max(len(tune), 1))(*[int(v) & 0xFFFFFFFF for v in tune.values()])
    out = (C.c_uint32 * 12)()
    _check(lib.pt_debug_launch_plan_tuned(C.c_uint32(num_cus), C.c_uint32(frames), C.c_uint32(tile_count), C.c_uint32(launches_in_flight), C.c_uint32(traced_batches),
                                          C.c_uint32(batch_size or frames), names, values, C.c_uint32(len(tune)), out))
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def tile_layout(width, height, rank, count):
    nt, fl = C.c_uint32(), C.c_uint64()
    _check(lib.pt_tile_layout(C.c_uint32(width), C.c_uint32(height), C.c_uint32(rank), C.c_uint32(count), C.byref(nt), C.byref(fl)))
    return nt.value, fl.value


def packed_layout(width, height, count, rect):
    """(largest packed share over the ranks in tiles, floats per frame of the gather) for the tile rectangle rect = (tx0, ty0, tx1, ty1)."""
    r = (C.c_uint32 * 4)(*rect); mt, fl = C.c_uint32(), C.c_uint64()
    _check(lib.pt_packed_layout(C.c_uint32(width), C.c_uint32(height), C.c_uint32(count), r, C.byref(mt), C.byref(fl)))
    return mt.value, fl.value


def packed_tile_ids(width, height, rank, count, rect):
    """Tile ids of the rank's packed share (its tiles inside rect), in packed-buffer order."""
    r = (C.c_uint32 * 4)(*rect); n = C.c_uint32()
    _check(lib.pt_packed_tile_ids(C.c_uint32(width), C.c_uint32(height), C.c_uint32(rank), C.c_uint32(count), r, None, C.c_uint32(0), C.byref(n)))
    ids = np.zeros(max(n.value, 1), np.uint32)
    _check(lib.pt_packed_tile_ids(C.c_uint32(width), C.c_uint32(height), C.c_uint32(rank), C.c_uint32(count), r, _p(ids, C.c_uint32), C.c_uint32(ids.size), C.byref(n)))
    return ids[: n.value]


def tile_ids(width, height, rank, count):
    """Tile ids (ty * ceil(W/8) + tx) of the rank's share, in compact-buffer order."""
    n = C.c_uint32()
    _check(lib.pt_tile_ids(C.c_uint32(width), C.c_uint32(height), C.c_uint32(rank), C.c_uint32(count), None, C.c_uint32(0), C.byref(n)))
    ids = np.zeros(max(n.value, 1), np.uint32)
    _check(lib.pt_tile_ids(C.c_uint32(width), C.c_uint32(height), C.c_uint32(rank), C.c_uint32(count), ids.ctypes.data_as(C.POINTER(C.c_uint32)), C.c_uint32(ids.size), C.byref(n)))
    return ids[: n.value]


# ---- device context -----------------------------------------------------------------------

class Context:
    """One GPU.  Thin, explicit wrapper over the pt_* entry points."""

    def __init__(self, device=-1):
        h = C.c_void_p()
        _check(lib.pt_create(C.c_int(device), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            lib.pt_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        _check(rc, self.h)

    def set_stream(self, stream_handle):
        self._ck(lib.pt_set_stream(self.h, C.c_void_p(stream_handle)))

    def get_stream(self):
        p = C.c_void_p()
        self._ck(lib.pt_get_stream(self.h, C.byref(p)))
        return p.value

    def synchronize(self):
        self._ck(lib.pt_synchronize(self.h))

    def set_triangles(self, tris):
        tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
        self._ck(lib.pt_set_triangles(self.h, _p(tris, C.c_float), C.c_uint32(tris.size // 9)))
        self.num_tris = tris.size // 9

    def update_triangles(self, tris):
        """New vertices for the same triangles: the tree keeps its topology and is refitted in place on the device (no rebuild, and on
        the device route no upload).  A numpy array takes the host route (returns when done).  A torch tensor on the context's GPU
        (float32, 9N elements) takes the device route: zero-copy when contiguous and 16-byte aligned, no host synchronisation, ordered
        with torch's current stream both ways; the tensor may be reused once synchronize() has returned."""
        if _is_torch(tris):
            _torch_route()
            import torch
            if tris.device.type != "cuda":
                raise ValueError("update_triangles: torch tensors must be on the context's GPU (got %s)" % tris.device)
            t = tris.reshape(-1)
            if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16:
                t = t.to(torch.float32).contiguous().clone()
            if t.numel() % 9:
                raise ValueError("update_triangles: 9 floats per triangle")
            self._on_context_stream(t.device, lambda: self.update_triangles_device(t.data_ptr(), t.numel() // 9))
            return
        tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
        self._ck(lib.pt_update_triangles(self.h, _p(tris, C.c_float), C.c_uint32(tris.size // 9)))

    def update_triangles_device(self, tris_ptr, num_tris):
        """Raw device route: f32[9 * num_tris] at tris_ptr (16-byte aligned, on the context's device), asynchronous on the context's stream."""
        self._ck(lib.pt_update_triangles_device(self.h, C.c_void_p(tris_ptr), C.c_uint32(num_tris)))

    def bvh_cost(self):
        """Quality of the current tree (grows as a refitted tree degrades): rebuild when it exceeds the cost at build by a factor you pick."""
        cost = C.c_double()
        self._ck(lib.pt_bvh_cost(self.h, C.byref(cost)))
        return cost.value

    def set_spheres(self, xyzr):
        xyzr = np.ascontiguousarray(xyzr, np.float32).reshape(-1)
        self._ck(lib.pt_set_spheres(self.h, _p(xyzr, C.c_float), C.c_uint32(xyzr.size // 4)))

    def build_bvh(self, accel=PT_ACCEL_REFERENCE):
        if accel == PT_ACCEL_REFERENCE:
            self._ck(lib.pt_build_bvh(self.h))
        else:
            self._ck(lib.pt_build_bvh_accel(self.h, C.c_uint32(accel)))

    def build_lbvh2(self, morton, tri_idx):
        morton = np.ascontiguousarray(morton, np.uint32); tri_idx = np.ascontiguousarray(tri_idx, np.uint32)
        self._ck(lib.pt_build_lbvh2(self.h, _p(morton, C.c_uint32), _p(tri_idx, C.c_uint32)))

    def read_bvh2(self):
        out = np.zeros(compute_bvh2_sizing(self.num_tris)["bytes"] // 4, np.uint32)
        self._ck(lib.pt_read_bvh2(self.h, _p(out, C.c_uint32), C.c_uint64(out.size * 4)))
        return out

    def set_bvh4(self, bvh4):
        bvh4 = np.ascontiguousarray(bvh4, np.uint32)
        self._ck(lib.pt_set_bvh4(self.h, _p(bvh4, C.c_uint32), C.c_uint64(bvh4.size)))

    def set_bvh2(self, bvh2):
        bvh2 = np.ascontiguousarray(bvh2, np.uint32)
        self._ck(lib.pt_set_bvh2(self.h, _p(bvh2, C.c_uint32), C.c_uint64(bvh2.size)))

    def scene_info(self):
        a, b, c = C.c_uint32(), C.c_uint32(), C.c_uint32()
        self._ck(lib.pt_scene_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return {"numTris": a.value, "numNodes2": b.value, "numNodes4": c.value}

    def read_bvh4(self):
        out = np.zeros(1 + 8 * self.scene_info()["numNodes4"], np.uint32)
        self._ck(lib.pt_read_bvh4(self.h, _p(out, C.c_uint32), C.c_uint64(out.size * 4)))
        return out

    def make_params(self, width, height, cam_pos=(0, 0, 2.5), cam_quat=(0, 0, 0, 1), mode=PT_MODE_REFERENCE, spp=1,
                    max_bounces=0, seed=1, frame=0, accumulate=False, tile_rank=0, tile_count=1, stats=False, num_tris=None, simple_kernel=False, brute_force=False):
        p = PtRenderParams()
        p.width, p.height = width, height
        p.focal, p.aspect = focal_aspect(width, height)
        p.cam_pos[:] = [float(np.float32(v)) for v in cam_pos]
        p.cam_quat[:] = [float(np.float32(v)) for v in cam_quat]
        p.num_tris = self.num_tris if num_tris is None else num_tris
        p.frame, p.mode, p.spp, p.max_bounces, p.seed = frame, mode, spp, max_bounces, seed
        p.accumulate = 1 if accumulate else 0
        p.tile_rank, p.tile_count = tile_rank, tile_count
        p.flags = (PT_FLAG_STATS if stats else 0) | (PT_FLAG_SIMPLE_KERNEL if simple_kernel else 0) | (PT_FLAG_BRUTE_FORCE if brute_force else 0)
        return p

    def render(self, params):
        self._ck(lib.pt_render(self.h, C.byref(params)))
        self._last = (params.width, params.height)

    def last_render_ms(self):
        ms = C.c_float()
        self._ck(lib.pt_last_render_ms(self.h, C.byref(ms)))
        return ms.value

    def set_batch(self, frames_per_launch):
        self._ck(lib.pt_set_batch(self.h, C.c_uint32(frames_per_launch)))

    def flush(self):
        self._ck(lib.pt_flush(self.h))

    def timing_begin(self, capacity):
        self._ck(lib.pt_timing_begin(self.h, C.c_uint32(capacity)))

    def timing_collect(self, capacity):
        ms = np.zeros(capacity, np.float32); n = C.c_uint32()
        self._ck(lib.pt_timing_collect(self.h, _p(ms, C.c_float), C.c_uint32(capacity), C.byref(n)))
        return ms[: n.value].copy()

    def debug_set_tune(self, name, value=None):
        """Diagnostics: override one launch heuristic of the megakernel on this context (None restores the default)."""
        self._ck(lib.pt_debug_set_tune(self.h, name.encode(), C.c_uint32(0xFFFFFFFF if value is None else value)))

    def debug_traced_tiles(self, params):
        """Diagnostics: (mask, rect_tiles, traced_tiles) -- mask[ty, tx] is True for the 8x8 tiles a megakernel launch of this frame traces;
        rect_tiles counts the owned tiles inside the root box's rectangle, traced_tiles those of them that the tile cover keeps."""
        tx, ty = (params.width + 7) // 8, (params.height + 7) // 8
        words = (tx * ty + 31) // 32
        bits = np.zeros(words, np.uint32); nr = C.c_uint32(); nt = C.c_uint32()
        self._ck(lib.pt_debug_traced_tiles(self.h, C.byref(params), _p(bits, C.c_uint32), C.c_uint32(words), C.byref(nr), C.byref(nt)))
        mask = np.unpackbits(bits.view(np.uint8), bitorder="little")[: tx * ty].astype(bool).reshape(ty, tx)
        return mask, nr.value, nt.value

    def debug_exposure(self, params=None, want_mask=True):
        """Diagnostics: the exposure mask.  params: compute it now for the current tree and that camera; None: the mask
        there is.  Returns a dict: valid, flagged, gave_up, listed, skipped, kernel_ms, mask (bool per triangle, or None), s_max, d_max, cam_max, used (the last megakernel launch read the mask).
        flagged, gave_up and mask are the first tier's; the second tier's (steeper hits only, a superset) are flagged2, gave_up2 (walks that ran
        out of budget after the first tier was settled as blocked) and mask2.  skipped counts the rays either tier skipped."""
        info = (C.c_uint32 * 7)(); ms = C.c_float(); bd = (C.c_double * 3)(); info2 = (C.c_uint32 * 2)()
        self._ck(lib.pt_debug_exposure(self.h, C.byref(params) if params is not None else None, info, bd, C.byref(ms), None, C.c_uint32(0)))
        self._ck(lib.pt_debug_exposure_tier2(self.h, info2, None, C.c_uint32(0)))
        mask = mask2 = None
        if want_mask and info[5]:
            bits = np.zeros(info[5], np.uint32)
            self._ck(lib.pt_debug_exposure(self.h, None, info, bd, C.byref(ms), _p(bits, C.c_uint32), C.c_uint32(info[5])))
            mask = np.unpackbits(bits.view(np.uint8), bitorder="little").astype(bool)
            self._ck(lib.pt_debug_exposure_tier2(self.h, info2, _p(bits, C.c_uint32), C.c_uint32(info[5])))
            mask2 = np.unpackbits(bits.view(np.uint8), bitorder="little").astype(bool)
        return {"valid": bool(info[0]), "flagged": info[1], "gave_up": info[2], "listed": info[3], "skipped": info[4], "kernel_ms": ms.value, "mask": mask,
                "s_max": bd[0], "d_max": bd[1], "cam_max": bd[2], "used": bool(info[6]), "flagged2": info2[0], "gave_up2": info2[1], "mask2": mask2}

    def timing_collect_spans(self, capacity):
        """(start_ms, dur_ms) of the launches recorded since timing_begin; starts are relative to the first launch."""
        st = np.zeros(capacity, np.float32); ms = np.zeros(capacity, np.float32); n = C.c_uint32()
        self._ck(lib.pt_timing_collect_spans(self.h, _p(st, C.c_float), _p(ms, C.c_float), C.c_uint32(capacity), C.byref(n)))
        return st[: n.value].copy(), ms[: n.value].copy()

    def set_compact_buffer(self, device_ptr, floats):
        self._ck(lib.pt_set_compact_buffer(self.h, C.c_void_p(device_ptr), C.c_uint64(floats)))

    def set_output_buffer(self, device_ptr, floats):
        self._ck(lib.pt_set_output_buffer(self.h, C.c_void_p(device_ptr), C.c_uint64(floats)))

    def stats(self):
        st = PtStats()
        self._ck(lib.pt_get_stats(self.h, C.byref(st)))
        return st.as_dict()

    def read_radiance(self, width=None, height=None):
        w, h = (width, height) if width else self._last
        out = np.zeros((h, w, 4), np.float32)
        self._ck(lib.pt_read_radiance(self.h, _p(out, C.c_float), C.c_uint64(out.size)))
        return out

    def read_rgba8(self):
        w, h = self._last
        out = np.zeros((h, w, 4), np.uint8)
        self._ck(lib.pt_read_rgba8(self.h, _p(out, C.c_uint8), C.c_uint64(out.size)))
        return out

    def read_tonemapped(self, from_rgba8=True):
        w, h = self._last
        out = np.zeros((h, w, 4), np.uint8)
        self._ck(lib.pt_read_tonemapped(self.h, C.c_int(int(from_rgba8)), _p(out, C.c_uint8), C.c_uint64(out.size)))
        return out

    def compact_radiance(self):
        ptr, fl = C.c_void_p(), C.c_uint64()
        self._ck(lib.pt_compact_radiance(self.h, C.byref(ptr), C.byref(fl)))
        return ptr.value, fl.value

    def deinterleave(self, gathered_device_ptr, stride_floats, width, height, tile_count):
        self._ck(lib.pt_deinterleave(self.h, C.c_void_p(gathered_device_ptr), C.c_uint64(stride_floats),
                                     C.c_uint32(width), C.c_uint32(height), C.c_uint32(tile_count)))
        self._last = (width, height)

    def deinterleave_batch(self, gathered_device_ptr, rank_stride_floats, frame_stride_floats, num_frames, width, height, tile_count, frames_out_ptr=0, out_stride_floats=0):
        self._ck(lib.pt_deinterleave_batch(self.h, C.c_void_p(gathered_device_ptr), C.c_uint64(rank_stride_floats), C.c_uint64(frame_stride_floats), C.c_uint32(num_frames),
                                           C.c_uint32(width), C.c_uint32(height), C.c_uint32(tile_count), C.c_void_p(frames_out_ptr or None), C.c_uint64(out_stride_floats)))
        self._last = (width, height)

    # ---- packed tile shares (what a sharded frame ships) ----
    def traced_tile_rect(self, params):
        r = (C.c_uint32 * 4)()
        self._ck(lib.pt_traced_tile_rect(self.h, C.byref(params), r))
        return tuple(int(v) for v in r)

    def pack_shares(self, compact_ptr, frame_stride_floats, num_frames, width, height, tile_rank, tile_count, rect, packed_ptr, packed_frame_stride_floats):
        self._ck(lib.pt_pack_shares(self.h, C.c_void_p(compact_ptr), C.c_uint64(frame_stride_floats), C.c_uint32(num_frames), C.c_uint32(width), C.c_uint32(height),
                                    C.c_uint32(tile_rank), C.c_uint32(tile_count), (C.c_uint32 * 4)(*rect), C.c_void_p(packed_ptr), C.c_uint64(packed_frame_stride_floats)))

    def unpack_batch(self, gathered_ptr, rank_stride_floats, frame_stride_floats, num_frames, width, height, tile_count, rect, spp, frames_out_ptr=0, out_stride_floats=0):
        self._ck(lib.pt_unpack_batch(self.h, C.c_void_p(gathered_ptr), C.c_uint64(rank_stride_floats), C.c_uint64(frame_stride_floats), C.c_uint32(num_frames),
                                     C.c_uint32(width), C.c_uint32(height), C.c_uint32(tile_count), (C.c_uint32 * 4)(*rect), C.c_uint32(spp),
                                     C.c_void_p(frames_out_ptr or None), C.c_uint64(out_stride_floats)))
        self._last = (width, height)

    # ---- checkpoint / resume of a progressive accumulation ----
    def accum_info(self):
        info = PtAccumInfo()
        self._ck(lib.pt_accum_info(self.h, C.byref(info)))
        return info

    def read_accum(self):
        """(PtAccumInfo, raw f32 dump: per-pixel sums in xyz, sample count in w) of the running accumulation."""
        info = self.accum_info()
        out = np.zeros(int(info.floats), np.float32)
        self._ck(lib.pt_read_accum(self.h, _p(out, C.c_float), C.c_uint64(out.size)))
        return info, out

    def set_accum(self, info, data):
        data = np.ascontiguousarray(data, np.float32).reshape(-1)
        assert data.size == info.floats
        self._ck(lib.pt_set_accum(self.h, C.byref(info), _p(data, C.c_float)))

    # ---- batched ray queries (an extension beyond the reference; include/mi355pt.h) ----
    def trace_rays(self, origins, directions=None, t_max=None, any_hit=False, stats=False, simple=False):
        """What does each ray hit?  Returns (t, prim, u, v): t = +inf and prim = 0xFFFFFFFF on a miss.

        origins, directions: (n, 3) float32, or origins alone as (n, 8) PtRay records (directions=None; t_max then comes from the records).
        numpy arrays take the host route (staged, returns when done).  torch tensors on the context's device take the device route:
        zero-copy for contiguous (n, 8) float32 records, no host synchronisation, ordered with torch's current stream both ways; the
        results are torch tensors (prim as torch.uint32).  stats: the counting kernel, counters in stats() afterwards."""
        flags = (PT_TRACE_ANY_HIT if any_hit else 0) | (PT_TRACE_STATS if stats else 0) | (PT_TRACE_SIMPLE_KERNEL if simple else 0)
        return self._run(_TRACE, _ray_records(origins, directions, t_max, "trace_rays"), C.c_uint32(flags))

    def trace_rays_device(self, rays_ptr, n, hits_ptr, flags=0):
        """Raw device route: n PtRay records at rays_ptr -> n PtHit records at hits_ptr (16-byte aligned device pointers).  Asynchronous on
        the context's stream (get_stream); the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_trace_rays(self.h, C.c_void_p(rays_ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(hits_ptr)))

    def camera_rays_device(self, params, rays_ptr):
        """Raw device route of camera_rays: width * height PtRay records at rays_ptr, asynchronous on the context's stream."""
        self._ck(lib.pt_camera_rays(self.h, C.byref(params), C.c_void_p(rays_ptr)))

    def _on_context_stream(self, device, launch):
        """Run launch() on the context's stream, ordered after and before torch's current stream on `device` (events only, no host wait)."""
        import torch
        cur = torch.cuda.current_stream(device)
        mine = self.get_stream()
        if cur.cuda_stream == mine:
            launch()
            return
        ext = torch.cuda.ExternalStream(mine, device=device)
        before = torch.cuda.Event(); before.record(cur); ext.wait_event(before)
        launch()
        after = torch.cuda.Event(); after.record(ext); cur.wait_event(after)

    def _run(self, q, rec, *extra, tail=None):
        """Query q (a _Query) over the n records `rec` as one call, extra being the ctypes arguments between the record count and the results."""
        return (self._run_host if isinstance(rec, np.ndarray) else self._run_torch)(q, rec, extra, q.tail if tail is None else tail)

    def _run_host(self, q, rec, extra, tail):
        """The host route: numpy records in, (n,) + tail result words out and unpacked; returns when done."""
        n = rec.shape[0]
        out = _aligned_zeros((n,) + tail, np.uint32)
        self._ck(q.host(self.h, rec.ctypes.data_as(C.POINTER(q.record)), C.c_uint64(n), *extra, out.ctypes.data_as(C.POINTER(q.entry))))
        return _unpack(out, q.cols)

    def _run_torch(self, q, rec, extra, tail):
        """The torch route: an int32 result tensor of shape (n,) + tail next to the records, the launch on the context's stream, ordered with
        torch's current stream both ways; no host wait."""
        import torch
        n = rec.shape[0]
        out = torch.empty((n,) + tail, dtype=torch.int32, device=rec.device)
        self._on_context_stream(rec.device, lambda: self._ck(q.device(self.h, C.c_void_p(rec.data_ptr()), C.c_uint64(n), *extra, C.c_void_p(out.data_ptr()))))
        return _unpack(out, q.cols)

    def camera_rays(self, params, device=None):
        """The rays PT_MODE_REFERENCE traces through each pixel centre of `params` (make_params): a torch (height * width, 8) float32 tensor of
        PtRay records on the context's GPU, row-major, ordered with torch's current stream.  Feed it to trace_rays for depth / id buffers or picking."""
        _torch_route()
        import torch
        dev = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        rays = torch.empty((params.height * params.width, 8), dtype=torch.float32, device=dev)
        self._on_context_stream(dev, lambda: self.camera_rays_device(params, rays.data_ptr()))
        return rays

    # ---- batched closest-point queries (an extension beyond the reference; include/mi355pt.h) ----
    def closest_points(self, points, r_max=None, stats=False, simple=False, brute_force=False):
        """Which triangle is nearest to each point?  Returns (dist, prim, u, v): dist = +inf and prim = 0xFFFFFFFF when nothing lies within
        r_max; the closest point is v0 + u * (v1 - v0) + v * (v2 - v0) of triangle prim.

        points: (n, 3) float32, or (n, 4) PtPoint records (r_max=None: taken from the records).  numpy arrays take the host route (staged,
        returns when done).  torch tensors on the context's device take the device route: zero-copy for contiguous (n, 4) float32 records,
        no host synchronisation, ordered with torch's current stream both ways; the results are torch tensors (prim as torch.uint32).
        stats: the counting kernel, counters in stats() afterwards; brute_force: every triangle in index order, no tree."""
        return self._run(_CLOSEST, _point_records(points, r_max, "closest_points"), C.c_uint32(_flags(stats, simple, brute_force)))

    def closest_points_device(self, ptr, n, out_ptr, flags=0):
        """Raw device route: n PtPoint records at ptr -> n PtClosest records at out_ptr (16-byte aligned device pointers).  Asynchronous on
        the context's stream (get_stream); the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_closest_points(self.h, C.c_void_p(ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(out_ptr)))

    # ---- sphere-cast queries (an extension beyond the reference; include/mi355pt.h) ----
    def sweep_spheres(self, origins, directions=None, radius=None, t_max=None, stats=False, simple=False, brute_force=False):
        """When does a sphere of `radius` that moves from each origin along its direction first touch the mesh, and where?  Returns
        (t, prim, u, v): t in units of the direction (0 for a sphere that overlaps at the start; +inf and prim = 0xFFFFFFFF on a miss); the
        contact point is v0 + u * (v1 - v0) + v * (v2 - v0) of triangle prim.

        origins, directions: (n, 3) float32 with radius a scalar or (n,), or origins alone as (n, 8) PtSweep records (pack_sweeps; radius,
        t_max None: taken from the records).  numpy arrays take the host route (staged, returns when done).  torch tensors on the context's
        device take the device route: zero-copy for contiguous (n, 8) float32 records, no host synchronisation, ordered with torch's
        current stream both ways; the results are torch tensors (prim as torch.uint32).
        stats: the counting kernel, counters in stats() afterwards; brute_force: every triangle in index order, no tree."""
        return self._run(_SWEEP, _sweep_records(origins, directions, radius, t_max, "sweep_spheres"), C.c_uint32(_flags(stats, simple, brute_force)))

    def sweep_spheres_device(self, ptr, n, out_ptr, flags=0):
        """Raw device route: n PtSweep records at ptr -> n PtHit records at out_ptr (16-byte aligned device pointers).  Asynchronous on the
        context's stream (get_stream); the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_sweep_spheres(self.h, C.c_void_p(ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(out_ptr)))

    # ---- batched ambient-occlusion queries (an extension beyond the reference; include/mi355pt.h) ----
    def occlusion(self, surfels, samples, seed=0, bias=1e-4, index_base=0, stats=False, simple=False):
        """How open is the hemisphere above each surfel?  Returns (visibility, unoccluded, samples) per surfel: `samples` cosine-distributed
        rays around the normal, walked any-hit up to r_max; all zero for a surfel that is not traced (a NaN, or r_max <= 0).

        surfels: (n, 8) float32 PtSurfel records (pack_surfels).  A numpy array takes the host route (staged, returns when done).  A torch
        tensor on the context's device takes the device route: zero-copy for contiguous float32 records, no host synchronisation, ordered
        with torch's current stream both ways; the results are torch tensors (the counts as torch.uint32).  stats: the counting kernel,
        counters in stats() afterwards; simple: the one-ray-per-thread kernel."""
        p = _occlusion_params(samples, seed, bias, index_base, stats, simple)
        return self._run(_OCCLUSION, _records8(surfels, "occlusion"), C.byref(p))

    def occlusion_device(self, surfels_ptr, n, params, out_ptr):
        """Raw device route: n PtSurfel records at surfels_ptr -> n PtOcclusion records at out_ptr (16-byte aligned device pointers; params:
        PtOcclusionParams).  Asynchronous on the context's stream (get_stream); the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_occlusion(self.h, C.c_void_p(surfels_ptr), C.c_uint64(n), C.byref(params), C.c_void_p(out_ptr)))

    def occlusion_rays(self, surfels, samples, seed=0, bias=1e-4, index_base=0):
        """The sample rays occlusion() walks, as (n * samples, 8) float32 PtRay records; sample s of surfel i is record i * samples + s.  A torch
        tensor of surfels takes the device route and gives a torch tensor on the same device (feed it to trace_rays); a numpy array is answered
        by the host twin, occlusion_rays_host, with the same bits.  Needs no scene."""
        if not _is_torch(surfels):
            return occlusion_rays_host(surfels, samples, seed, bias, index_base)
        import torch
        sf = _records8(surfels, "occlusion_rays")
        n = sf.shape[0]
        p = _occlusion_params(samples, seed, bias, index_base)
        rays = torch.empty((n * int(samples), 8), dtype=torch.float32, device=sf.device)
        self._on_context_stream(sf.device, lambda: self.occlusion_rays_device(sf.data_ptr(), n, p, rays.data_ptr()))
        return rays

    def occlusion_rays_device(self, surfels_ptr, n, params, rays_ptr):
        """Raw device route of occlusion_rays: n * params.samples PtRay records at rays_ptr, asynchronous on the context's stream."""
        self._ck(lib.pt_occlusion_rays(self.h, C.c_void_p(surfels_ptr), C.c_uint64(n), C.byref(params), C.c_void_p(rays_ptr)))

    def hit_surfels(self, rays, hits, r_max=float("inf")):
        """Rays + their hits -> (n, 8) float32 PtSurfel records: the hit point with the triangle's normal turned against the ray and r_max; a
        miss gives a surfel that is not traced.  rays: (n, 8) PtRay records; hits: (n, 4) PtHit records (int32 / uint32 / float32 words), or the
        (t, prim, u, v) tuple trace_rays returns.  numpy takes the host route, torch tensors the device route (nothing leaves the device)."""
        if isinstance(hits, (tuple, list)):
            t, prim, u, v = hits
            if _is_torch(rays):
                import torch
                hits = torch.stack([t.view(torch.int32), prim.view(torch.int32), u.view(torch.int32), v.view(torch.int32)], dim=1)
            else:
                hits = np.stack([np.asarray(t, np.float32).view(np.uint32), np.asarray(prim, np.uint32),
                                 np.asarray(u, np.float32).view(np.uint32), np.asarray(v, np.float32).view(np.uint32)], axis=1)
        r = _records8(rays, "hit_surfels")
        if (hits.element_size() if _is_torch(hits) else np.asarray(hits).dtype.itemsize) != 4:
            raise ValueError("hit_surfels: hits must be 4-byte words")
        if _is_torch(rays):
            import torch
            h = _torch_records(hits.reshape(-1, 4).view(torch.int32), "hit_surfels", dtype="int32")
        else:
            h = _records(np.asarray(hits).reshape(-1, 4).view(np.uint32))
        n = r.shape[0]
        if h.shape[0] != n:
            raise ValueError("hit_surfels: %d rays but %d hits" % (n, h.shape[0]))
        if _is_torch(rays):
            out = torch.empty((n, 8), dtype=torch.float32, device=r.device)
            self._on_context_stream(r.device, lambda: self.hit_surfels_device(r.data_ptr(), h.data_ptr(), n, r_max, out.data_ptr()))
            return out
        out = _aligned_zeros((n, 8), np.float32)
        self._ck(lib.pt_hit_surfels_host(self.h, r.ctypes.data_as(C.POINTER(PtRay)), h.ctypes.data_as(C.POINTER(PtHit)), C.c_uint64(n),
                                         C.c_float(r_max), out.ctypes.data_as(C.POINTER(PtSurfel))))
        return out

    def hit_surfels_device(self, rays_ptr, hits_ptr, n, r_max, surfels_ptr):
        """Raw device route of hit_surfels: n PtSurfel records at surfels_ptr, asynchronous on the context's stream."""
        self._ck(lib.pt_hit_surfels(self.h, C.c_void_p(rays_ptr), C.c_void_p(hits_ptr), C.c_uint64(n), C.c_float(r_max), C.c_void_p(surfels_ptr)))

    # ---- crossing counts, containment, signed distance (an extension beyond the reference; include/mi355pt.h) ----
    def count_hits(self, origins, directions=None, t_max=None, stats=False, simple=False, brute_force=False):
        """How many triangles does each ray cross (up to t_max)?  Returns the (n,) uint32 counts.

        origins, directions: (n, 3) float32, or origins alone as (n, 8) PtRay records (directions=None; t_max then comes from the records).
        numpy arrays take the host route (staged, returns when done).  torch tensors on the context's device take the device route:
        zero-copy for contiguous (n, 8) float32 records, no host synchronisation, ordered with torch's current stream both ways; the
        result is a torch.uint32 tensor.  stats: the counting kernel, counters in stats() afterwards; brute_force: every triangle, no tree."""
        return self._run(_COUNT, _ray_records(origins, directions, t_max, "count_hits"), C.c_uint32(_flags(stats, simple, brute_force)))

    def count_hits_device(self, rays_ptr, n, counts_ptr, flags=0):
        """Raw device route: n PtRay records at rays_ptr (16-byte aligned) -> n uint32 counts at counts_ptr.  Asynchronous on the context's
        stream (get_stream); the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_count_hits(self.h, C.c_void_p(rays_ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(counts_ptr)))

    def contains(self, points, samples=3, seed=0, index_base=0, stats=False, simple=False):
        """Is each point inside the mesh?  Crossing parity by majority vote over `samples` (odd, 1..255) rays per point: returns
        (inside, odd, samples) as uint32 -- on a closed mesh the point-in-solid test; on an open or self-intersecting mesh whatever the
        parity is, with odd / samples telling how much the rays disagreed.  All zero for a point with a NaN.

        points: (n, 3) float32 or (n, 4) PtPoint records (r_max is ignored).  numpy takes the host route; torch tensors on the context's
        device stay there, on the context's stream, with no host synchronisation."""
        p = _contain_params(samples, seed, index_base, stats, simple)
        return self._run(_CONTAINS, _point_records(points, None, "contains"), C.byref(p))        # (r_max is ignored)

    def contains_device(self, points_ptr, n, params, out_ptr):
        """Raw device route: n PtPoint records at points_ptr -> n PtContainment records at out_ptr (16-byte aligned device pointers; params:
        PtContainParams).  Asynchronous on the context's stream."""
        self._ck(lib.pt_contains(self.h, C.c_void_p(points_ptr), C.c_uint64(n), C.byref(params), C.c_void_p(out_ptr)))

    # ---- radius queries (an extension beyond the reference; include/mi355pt.h) ----
    def radius_count(self, points, r_max=None, stats=False, simple=False, brute_force=False):
        """How many triangles lie within r_max of each point?  Returns the (n,) uint32 counts (0 for a point with a NaN or r_max <= 0).

        points: (n, 3) float32, or (n, 4) PtPoint records (r_max=None: taken from the records).  numpy arrays take the host route (staged,
        returns when done).  torch tensors on the context's device stay there, on the context's stream, with no host synchronisation; the
        result is a torch.uint32 tensor.  stats: the counting kernel, counters in stats() afterwards (stack_drops > 0 means that triangles
        were lost at the 64-entry stack cap); brute_force: every triangle, no tree."""
        return self._run(_RADIUS_COUNT, _point_records(points, r_max, "radius_count"), C.c_uint32(_flags(stats, simple, brute_force)))

    def radius_count_device(self, points_ptr, n, counts_ptr, flags=0):
        """Raw device route: n PtPoint records at points_ptr (16-byte aligned) -> n uint32 counts at counts_ptr.  Asynchronous on the
        context's stream (get_stream); the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_radius_count(self.h, C.c_void_p(points_ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(counts_ptr)))

    def radius_search(self, points, r_max=None, capacity=None, stats=False, simple=False, brute_force=False):
        """Which triangles lie within r_max of each point -- all of them, each with its contact point?  Returns (offsets, dist, prim, u, v):
        the list of point i is entries offsets[i]:offsets[i + 1], in the walk's visit order (index order with brute_force); the contact point
        of an entry is v0 + u * (v1 - v0) + v * (v2 - v0) of triangle prim, at distance dist.  offsets has n + 1 elements and is always
        complete: offsets[-1] is the total, and offsets[-1] > capacity says that only the first `capacity` entries were written.

        points: as radius_count.  numpy arrays take the host route (staged, returns when done): offsets is uint64 and the entry arrays hold
        min(offsets[-1], capacity) elements; capacity=None starts with room for 16 entries per point and runs the query again when
        offsets[-1] says that this was too little.
        torch tensors on the context's device stay there, on the context's stream: offsets is int64, prim torch.uint32.  With `capacity` given
        the torch route waits for nothing on the host and the entry tensors hold `capacity` elements, of which those from offsets[-1] on are
        not written.  With capacity=None it reads offsets[-1] once to size the entries: that is the one host wait of this call (the counts
        are then walked a second time); pass a capacity to avoid it.
        stats: counters of the count walk in stats() afterwards -- stack_drops > 0 means that triangles were lost at the 64-entry stack cap,
        which large radii over deep trees reach sooner than any other query; brute_force lists every triangle within r_max regardless."""
        return self._list(_RADIUS, _point_records(points, r_max, "radius_search"), _flags(stats, simple, brute_force), capacity)

    def _list(self, q, rec, flags, capacity):
        """List query q over the n records `rec`: (offsets,) + the entry columns."""
        return (self._list_host if isinstance(rec, np.ndarray) else self._list_torch)(q, rec, flags, capacity)

    def _list_torch(self, q, rec, flags, capacity):
        """The torch route of a list query: with a capacity one call and no host wait; without, one for the offsets, the read of
        offsets[-1], and one for the entries."""
        import torch
        n, dev = rec.shape[0], rec.device
        offsets = torch.empty((n + 1,), dtype=torch.int64, device=dev)

        def call(entries_ptr, cap):
            self._on_context_stream(dev, lambda: self._ck(q.device(self.h, C.c_void_p(rec.data_ptr()), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(offsets.data_ptr()),
                                                                   C.c_void_p(entries_ptr) if cap else None, C.c_uint64(cap))))
        if capacity is None:
            call(0, 0)
            capacity = int(offsets[-1].item())          # the one host wait
        cap = int(capacity)
        entries = torch.empty((cap, 4), dtype=torch.int32, device=dev)
        call(entries.data_ptr(), cap)
        return (offsets,) + _unpack(entries, q.cols)

    def _list_host(self, q, rec, flags, capacity):
        """The host route of a list query.  capacity None: room for q.guess entries per record at first (16 for radius and box lists, 4 for
        hit lists), and a second run when offsets[n] says that this was too little."""
        n = rec.shape[0]
        offsets = np.zeros(n + 1, np.uint64)

        def call(entries, cap):
            self._ck(q.host(self.h, rec.ctypes.data_as(C.POINTER(q.record)), C.c_uint64(n), C.c_uint32(flags), _p(offsets, C.c_uint64),
                            entries.ctypes.data_as(C.POINTER(q.entry)) if cap else None, C.c_uint64(cap)))
        retry = capacity is None
        if retry:
            capacity = q.guess * n + 64             # a first guess; offsets[n] says how large the retry must be
        entries = _aligned_zeros((int(capacity), 4), np.uint32)
        call(entries, int(capacity))
        if retry and int(offsets[n]) > capacity:
            capacity = int(offsets[n])
            entries = _aligned_zeros((capacity, 4), np.uint32)
            call(entries, capacity)
        return (offsets,) + _unpack(entries[: min(int(offsets[n]), int(capacity))], q.cols)

    def radius_search_device(self, points_ptr, n, offsets_ptr, entries_ptr, capacity, flags=0):
        """Raw device route: n PtPoint records at points_ptr (16-byte aligned) -> n + 1 uint64 offsets at offsets_ptr (8-byte aligned) and up to
        `capacity` PtClosest records at entries_ptr (16-byte aligned; 0 with capacity 0: offsets only).  Three launches on the context's
        stream (get_stream), no host wait; the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_radius_search(self.h, C.c_void_p(points_ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(offsets_ptr),
                                      C.c_void_p(entries_ptr) if entries_ptr else None, C.c_uint64(capacity)))

    # ---- box-overlap queries (an extension beyond the reference; include/mi355pt.h) ----
    def box_count(self, lo, hi=None, stats=False, simple=False, brute_force=False):
        """How many triangles overlap each axis-aligned box?  Returns the (n,) uint32 counts (0 for a box with a NaN, an infinity or lo > hi).

        lo, hi: (n, 3) float32 corners, or lo alone as (n, 8) PtBox records (lo xyz, pad, hi xyz, pad).  numpy arrays take the host route
        (staged, returns when done).  torch tensors on the context's device stay there, on the context's stream, with no host
        synchronisation; the result is a torch.uint32 tensor.  stats: the counting kernel, counters in stats() afterwards (stack_drops > 0
        means that triangles were lost at the 64-entry stack cap); brute_force: every triangle, no tree."""
        return self._run(_BOX_COUNT, _box_records(lo, hi, "box_count"), C.c_uint32(_flags(stats, simple, brute_force)))

    def box_count_device(self, boxes_ptr, n, counts_ptr, flags=0):
        """Raw device route: n PtBox records at boxes_ptr (16-byte aligned) -> n uint32 counts at counts_ptr.  Asynchronous on the
        context's stream (get_stream); the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_box_count(self.h, C.c_void_p(boxes_ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(counts_ptr)))

    def box_search(self, lo, hi=None, capacity=None, stats=False, simple=False, brute_force=False):
        """Which triangles overlap each axis-aligned box -- all of them?  Returns (offsets, prim, verts_inside): the list of box i is entries
        offsets[i]:offsets[i + 1], in the walk's visit order (index order with brute_force); bit k of verts_inside says that vertex k of
        triangle prim lies in the closed box (7: the whole triangle is inside).  offsets has n + 1 elements and is always complete:
        offsets[-1] is the total, and offsets[-1] > capacity says that only the first `capacity` entries were written.  Touching counts.

        lo, hi: as box_count.  numpy arrays take the host route (staged, returns when done): offsets is uint64 and the entry arrays hold
        min(offsets[-1], capacity) elements; capacity=None starts with room for 16 entries per box and runs the query again when
        offsets[-1] says that this was too little.
        torch tensors on the context's device stay there, on the context's stream: offsets is int64, prim and verts_inside torch.uint32.
        With `capacity` given the torch route waits for nothing on the host and the entry tensors hold `capacity` elements, of which those
        from offsets[-1] on are not written.  With capacity=None it reads offsets[-1] once to size the entries: that is the one host wait
        of this call (the boxes are then counted a second time); pass a capacity to avoid it.
        stats: counters of the count walk in stats() afterwards -- stack_drops > 0 means that triangles were lost at the 64-entry stack cap,
        which large boxes over deep trees reach as large radii do; brute_force lists every overlapping triangle regardless."""
        return self._list(_BOX, _box_records(lo, hi, "box_search"), _flags(stats, simple, brute_force), capacity)

    def box_search_device(self, boxes_ptr, n, offsets_ptr, entries_ptr, capacity, flags=0):
        """Raw device route: n PtBox records at boxes_ptr (16-byte aligned) -> n + 1 uint64 offsets at offsets_ptr (8-byte aligned) and up to
        `capacity` PtOverlap records at entries_ptr (16-byte aligned; 0 with capacity 0: offsets only).  Three launches on the context's
        stream (get_stream), no host wait; the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_box_search(self.h, C.c_void_p(boxes_ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(offsets_ptr),
                                   C.c_void_p(entries_ptr) if entries_ptr else None, C.c_uint64(capacity)))

    # ---- triangle-overlap queries (an extension beyond the reference; include/mi355pt.h) ----
    def tri_count(self, tris, stats=False, simple=False, brute_force=False):
        """How many mesh triangles does each caller triangle cut?  Returns the (n,) uint32 counts (0 for a triangle with a NaN or an infinity).

        tris: (n, 3, 3) or (n, 9) float32 vertices, or (n, 12) PtTri records (v0 xyz, pad, v1 xyz, pad, v2 xyz, pad).  numpy arrays take the
        host route (staged, returns when done).  torch tensors on the context's device stay there, on the context's stream, with no host
        synchronisation; the result is a torch.uint32 tensor.  stats: the counting kernel, counters in stats() afterwards (stack_drops > 0
        means that triangles were lost at the 64-entry stack cap); brute_force: every triangle, no tree.  Coplanar pairs are not counted."""
        return self._run(_TRI_COUNT, _tri_records(tris, "tri_count"), C.c_uint32(_flags(stats, simple, brute_force)))

    def tri_count_device(self, tris_ptr, n, counts_ptr, flags=0):
        """Raw device route: n PtTri records at tris_ptr (16-byte aligned) -> n uint32 counts at counts_ptr.  Asynchronous on the
        context's stream (get_stream); the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_tri_count(self.h, C.c_void_p(tris_ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(counts_ptr)))

    def tri_search(self, tris, capacity=None, stats=False, simple=False, brute_force=False):
        """Which mesh triangles does each caller triangle cut -- all of them?  Returns (offsets, prim, edges): the list of caller triangle i
        is entries offsets[i]:offsets[i + 1], in the walk's visit order (index order with brute_force).  Bits 0-2 of edges say which of the
        caller's edges q0->q1, q1->q2, q2->q0 cross mesh triangle prim, bits 3-5 which of the mesh triangle's edges v0->v1, v1->v2, v0->v2
        cross the caller's triangle; in general position two bits are set, the end points of the intersection segment.  offsets has n + 1
        elements and is always complete: offsets[-1] is the total, and offsets[-1] > capacity says that only the first `capacity` entries
        were written.  Touching counts wherever the rounded f32 values say so.  COPLANAR PAIRS ARE NOT LISTED: run a 2-D test on the
        candidates of box_search for those.

        tris: as tri_count.  numpy arrays take the host route (staged, returns when done): offsets is uint64 and the entry arrays hold
        min(offsets[-1], capacity) elements; capacity=None starts with room for 16 entries per triangle and runs the query again when
        offsets[-1] says that this was too little.
        torch tensors on the context's device stay there, on the context's stream: offsets is int64, prim and edges torch.uint32.  With
        `capacity` given the torch route waits for nothing on the host and the entry tensors hold `capacity` elements, of which those from
        offsets[-1] on are not written.  With capacity=None it reads offsets[-1] once to size the entries: that is the one host wait of this
        call (the triangles are then counted a second time); pass a capacity to avoid it.
        stats: counters of the count walk in stats() afterwards -- stack_drops > 0 means that triangles were lost at the 64-entry stack cap;
        brute_force lists every cut triangle regardless."""
        return self._list(_TRI, _tri_records(tris, "tri_search"), _flags(stats, simple, brute_force), capacity)

    def tri_search_device(self, tris_ptr, n, offsets_ptr, entries_ptr, capacity, flags=0):
        """Raw device route: n PtTri records at tris_ptr (16-byte aligned) -> n + 1 uint64 offsets at offsets_ptr (8-byte aligned) and up to
        `capacity` PtCross records at entries_ptr (16-byte aligned; 0 with capacity 0: offsets only).  Three launches on the context's
        stream (get_stream), no host wait; the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_tri_search(self.h, C.c_void_p(tris_ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(offsets_ptr),
                                   C.c_void_p(entries_ptr) if entries_ptr else None, C.c_uint64(capacity)))

    def intersecting_pairs(self, tris, capacity=None):
        """tri_search flattened: returns (pairs, edges), pairs the (m, 2) int64 array of (caller triangle index, prim) of every entry that
        was written, in list order, and edges its edges column.  numpy in, numpy out; torch in, torch out (the torch route then reads the
        offsets on the host once, to expand them)."""
        offsets, prim, edges = self.tri_search(tris, capacity)
        if isinstance(offsets, np.ndarray):
            m = prim.shape[0]
            counts = np.diff(np.minimum(offsets, np.uint64(m)).astype(np.int64))
            return np.stack([np.repeat(np.arange(counts.size, dtype=np.int64), counts), prim.astype(np.int64)], axis=1), edges
        import torch
        m = min(int(offsets[-1].item()), prim.shape[0])
        counts = torch.diff(torch.clamp(offsets, max=m))
        caller = torch.repeat_interleave(torch.arange(counts.shape[0], dtype=torch.int64, device=offsets.device), counts)
        return torch.stack([caller, prim[:m].to(torch.int64)], dim=1), edges[:m]

    # ---- plane-cut queries (an extension beyond the reference; include/mi355pt.h) ----
    def cut_count(self, normal, d=None, lo=None, hi=None, stats=False, simple=False, brute_force=False):
        """How many mesh triangles does each plane n.x = d cut inside its window [lo, hi]?  Returns the (n,) uint32 counts (0 for a record
        with a NaN or an infinity, n = 0 or lo > hi).

        normal, d, lo, hi: one normal (3,) or (n, 3), d a scalar or (n,), the window's corners (3,) or (n, 3) each (None: [-32, 32]^3) -- or
        normal alone as (n, 12) PtCutPlane records (n xyz, d, lo xyz, pad, hi xyz, pad).  numpy arrays take the host route (staged,
        returns when done).  torch tensors on the context's device stay there, on the context's stream, with no host synchronisation;
        the result is a torch.uint32 tensor.  stats: the counting kernel, counters in stats() afterwards (stack_drops > 0 means that
        triangles were lost at the 64-entry stack cap); brute_force: every triangle, no tree."""
        return self._run(_CUT_COUNT, _cut_records(normal, d, lo, hi, "cut_count"), C.c_uint32(_flags(stats, simple, brute_force)))

    def cut_count_device(self, planes_ptr, n, counts_ptr, flags=0):
        """Raw device route: n PtCutPlane records at planes_ptr (16-byte aligned) -> n uint32 counts at counts_ptr.  Asynchronous on the
        context's stream (get_stream); the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_cut_count(self.h, C.c_void_p(planes_ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(counts_ptr)))

    def cut_search(self, normal, d=None, lo=None, hi=None, capacity=None, stats=False, simple=False, brute_force=False):
        """Which mesh triangles does each plane n.x = d cut inside its window, and where?  Returns (offsets, prim, code, t0, t1): the list
        of plane i is entries offsets[i]:offsets[i + 1], in the walk's visit order (index order with brute_force).  Bits 0-2 of code say
        which edges of mesh triangle prim cross the plane, v0-v1, v1-v2, v0-v2 (exactly two); bits 3-5 are the classes s_i >= 0 of its
        vertices, s = n.v - d.  t0 belongs to the lowest crossing edge, t1 to the highest, each measured from the edge's vertex below the
        plane: cut_segments turns them into points.  The rule is half-open: a triangle in the plane or touching it from the s >= 0 side is
        not listed, one touching it from below with one vertex is, as a zero-length segment.  The window does not clip: it filters on the
        triangle's bounding box, so a triangle whose box overlaps two windows is listed by both.  offsets has n + 1 elements and is always
        complete: offsets[-1] is the total, and offsets[-1] > capacity says that only the first `capacity` entries were written.

        normal, d, lo, hi: as cut_count.  numpy arrays take the host route (staged, returns when done): offsets is uint64 and the entry
        arrays hold min(offsets[-1], capacity) elements; capacity=None starts with room for 16 entries per plane and runs the query
        again when offsets[-1] says that this was too little.
        torch tensors on the context's device stay there, on the context's stream: offsets is int64, prim and code torch.uint32, t0 and
        t1 torch.float32.  With `capacity` given the torch route waits for nothing on the host and the entry tensors hold `capacity`
        elements, of which those from offsets[-1] on are not written.  With capacity=None it reads offsets[-1] once to size the entries:
        that is the one host wait of this call (the planes are then counted a second time); pass a capacity to avoid it.
        stats: counters of the count walk in stats() afterwards -- stack_drops > 0 means that triangles were lost at the 64-entry stack
        cap; brute_force lists every cut triangle regardless."""
        return self._list(_CUT, _cut_records(normal, d, lo, hi, "cut_search"), _flags(stats, simple, brute_force), capacity)

    def cut_search_device(self, planes_ptr, n, offsets_ptr, entries_ptr, capacity, flags=0):
        """Raw device route: n PtCutPlane records at planes_ptr (16-byte aligned) -> n + 1 uint64 offsets at offsets_ptr (8-byte aligned)
        and up to `capacity` PtCut records at entries_ptr (16-byte aligned; 0 with capacity 0: offsets only).  Three launches on the
        context's stream (get_stream), no host wait; the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_cut_search(self.h, C.c_void_p(planes_ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(offsets_ptr),
                                   C.c_void_p(entries_ptr) if entries_ptr else None, C.c_uint64(capacity)))

    def cross_section(self, tris, normal, d, grid=1):
        """The section of the mesh by the plane normal.x = d: returns (prim, code, segments), one row per cut triangle, segments the
        (m, 2, 3) float32 array of cut_segments.  tris: the mesh the context holds, as numpy vertices ((num_tris, 3, 3) or (num_tris, 9)).
        The mesh's bounding box is tiled into grid x grid windows over the two axes other than argmax |normal_k|, each with the box's full
        extent on that third axis, and all of them go through one cut_search call; a triangle that several windows list is kept once, at
        its first listing.  The segments are not stitched into polylines."""
        v = np.asarray(tris, np.float32).reshape(-1, 3)
        nrm = np.asarray(normal, np.float32).reshape(3)
        grid = int(grid)
        if grid < 1:
            raise ValueError("cross_section: grid must be at least 1, got %d" % grid)
        lo, hi = v.min(axis=0), v.max(axis=0)
        k = int(np.argmax(np.abs(nrm)))
        a, b = [ax for ax in range(3) if ax != k]
        steps = np.arange(grid + 1, dtype=np.float32) / np.float32(grid)
        edges = {ax: (lo[ax] + (hi[ax] - lo[ax]) * steps).astype(np.float32) for ax in (a, b)}
        for ax in (a, b):
            edges[ax][0], edges[ax][-1] = lo[ax], hi[ax]
            edges[ax] = np.maximum.accumulate(edges[ax])
        wlo = np.empty((grid, grid, 3), np.float32); whi = np.empty((grid, grid, 3), np.float32)
        wlo[..., k], whi[..., k] = lo[k], hi[k]
        wlo[..., a], whi[..., a] = edges[a][:-1, None], edges[a][1:, None]
        wlo[..., b], whi[..., b] = edges[b][None, :-1], edges[b][None, 1:]
        _, prim, code, t0, t1 = self.cut_search(nrm, np.float32(d), wlo.reshape(-1, 3), whi.reshape(-1, 3))
        _, first = np.unique(prim, return_index=True)
        first.sort()
        return prim[first], code[first], cut_segments(tris, prim[first], code[first], t0[first], t1[first])

    # ---- hit lists (an extension beyond the reference; include/mi355pt.h) ----
    def list_hits(self, origins, directions=None, t_max=None, capacity=None, sort=False, stats=False, simple=False, brute_force=False):
        """Which triangles does each ray cross (up to t_max), and where?  Returns (offsets, t, prim, u, v): the list of ray i is entries
        offsets[i]:offsets[i + 1] -- exactly the crossings count_hits counts -- in the walk's visit order (index order with brute_force), or
        with sort=True in ascending order of (t, prim); the point of an entry is org + t * dir = v0 + u * (v1 - v0) + v * (v2 - v0) of
        triangle prim.  offsets has n + 1 elements and is always complete: offsets[-1] is the total, and offsets[-1] > capacity says that
        only the first `capacity` entries were written (the one list that straddles the capacity is then left in visit order).

        origins, directions, t_max: as count_hits.  numpy arrays take the host route (staged, returns when done): offsets is uint64 and the
        entry arrays hold min(offsets[-1], capacity) elements; capacity=None starts with room for 4 entries per ray and runs the query again
        when offsets[-1] says that this was too little.
        torch tensors on the context's device stay there, on the context's stream: offsets is int64, prim torch.uint32.  With `capacity` given
        the torch route waits for nothing on the host and the entry tensors hold `capacity` elements, of which those from offsets[-1] on are
        not written.  With capacity=None it reads offsets[-1] once to size the entries: that is the one host wait of this call (the rays
        are then counted a second time); pass a capacity to avoid it.
        stats: counters of the count walk in stats() afterwards -- stack_drops > 0 means that crossings were lost at the 64-entry stack cap;
        brute_force lists every crossing regardless."""
        return self._list(_HITS, _ray_records(origins, directions, t_max, "list_hits"), _flags(stats, simple, brute_force, sort), capacity)

    def list_hits_device(self, rays_ptr, n, offsets_ptr, hits_ptr, capacity, flags=0):
        """Raw device route: n PtRay records at rays_ptr (16-byte aligned) -> n + 1 uint64 offsets at offsets_ptr (8-byte aligned) and up to
        `capacity` PtHit records at hits_ptr (16-byte aligned; 0 with capacity 0: offsets only).  Three launches on the context's stream
        (get_stream), four with PT_HITS_SORTED, no host wait; the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_list_hits(self.h, C.c_void_p(rays_ptr), C.c_uint64(n), C.c_uint32(flags), C.c_void_p(offsets_ptr),
                                  C.c_void_p(hits_ptr) if hits_ptr else None, C.c_uint64(capacity)))

    # ---- k-nearest queries (an extension beyond the reference; include/mi355pt.h) ----
    def nearest_k(self, points, k, r_max=None, stats=False, simple=False, brute_force=False):
        """Which k triangles are nearest to each point?  Returns (dist, prim, u, v), each of shape (n, k): row i holds the at most k
        triangles within r_max in ascending order of distance (equal distances in the walk's visit order; index order with brute_force),
        padded with dist = +inf and prim = 0xFFFFFFFF; the contact point of an entry is v0 + u * (v1 - v0) + v * (v2 - v0) of triangle prim.
        1 <= k <= PT_NEAREST_MAX_K (64).

        points: as closest_points.  numpy arrays take the host route (staged, returns when done).  torch tensors on the context's device take
        the device route: zero-copy for contiguous (n, 4) float32 records, no host synchronisation, ordered with torch's current stream both
        ways; the results are torch tensors (prim as torch.uint32).
        stats: the counting kernel, counters in stats() afterwards (stack_drops > 0 means that nearer triangles may be missing);
        brute_force: every triangle in index order, no tree."""
        k = int(k)        # (numpy rows for max(k, 0), torch rows for max(k, 1), both capped at 64: the C side refuses a k out of range)
        pts = _point_records(points, r_max, "nearest_k")
        return self._run(_NEAREST, pts, C.c_uint32(k & 0xFFFFFFFF), C.c_uint32(_flags(stats, simple, brute_force)),
                         tail=(min(max(k, 1 if _is_torch(pts) else 0), PT_NEAREST_MAX_K), 4))

    def nearest_k_device(self, ptr, n, k, out_ptr, flags=0):
        """Raw device route: n PtPoint records at ptr -> n * k PtClosest records at out_ptr, row i at record i * k (16-byte aligned device
        pointers).  Asynchronous on the context's stream (get_stream); the buffers must stay allocated until a later synchronize()."""
        self._ck(lib.pt_nearest_k(self.h, C.c_void_p(ptr), C.c_uint64(n), C.c_uint32(k & 0xFFFFFFFF), C.c_uint32(flags), C.c_void_p(out_ptr)))

    def signed_distance(self, points, r_max=None, samples=3, seed=0, index_base=0, simple=False):
        """closest_points with the sign of contains: returns (dist, prim, u, v), dist negative where the point is inside (-inf: inside, and
        nothing within r_max).  Arguments as closest_points and contains; three launches on the context's stream, no host wait."""
        p = _contain_params(samples, seed, index_base, False, simple)                  # (never the stats flag)
        return self._run(_SIGNED, _point_records(points, r_max, "signed_distance"), C.byref(p))

    def signed_distance_device(self, points_ptr, n, params, out_ptr):
        """Raw device route: n PtPoint records at points_ptr -> n PtClosest records at out_ptr (16-byte aligned; params: PtContainParams)."""
        self._ck(lib.pt_signed_distance(self.h, C.c_void_p(points_ptr), C.c_uint64(n), C.byref(params), C.c_void_p(out_ptr)))

    def buffer_busy(self, device_ptr, nbytes):
        b = C.c_int()
        self._ck(lib.pt_buffer_busy(self.h, C.c_void_p(device_ptr), C.c_uint64(nbytes), C.byref(b)))
        return bool(b.value)


PT_GROUP_TRANSPORT_RCCL, PT_GROUP_TRANSPORT_COPY = 0, 1


class Group:
    """Several GPUs, one image per render(): the pt_group_* entry points (one context per device inside this process, tile shares
    gathered on rank 0 over RCCL, de-interleaved there).  `devices=None` takes every visible device."""

    def __init__(self, devices=None, transport=PT_GROUP_TRANSPORT_RCCL):
        lib.pt_group_last_error.restype = C.c_char_p
        lib.pt_group_last_error.argtypes = [C.c_void_p]
        lib.pt_group_destroy.restype = None
        lib.pt_group_destroy.argtypes = [C.c_void_p]
        h = C.c_void_p()
        if devices is None:
            rc = lib.pt_group_create(None, C.c_uint32(0), C.c_uint32(transport), C.byref(h))
        else:
            arr = (C.c_int * len(devices))(*devices)
            rc = lib.pt_group_create(arr, C.c_uint32(len(devices)), C.c_uint32(transport), C.byref(h))
        if rc != 0:
            msg = lib.pt_group_last_error(None)
            raise PtError(rc, msg.decode() if msg else "")
        self.h = h
        self.num_tris = 0

    def _ck(self, rc):
        if rc != 0:
            msg = lib.pt_group_last_error(self.h)
            raise PtError(rc, msg.decode() if msg else "")

    def close(self):
        if getattr(self, "h", None):
            lib.pt_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def size(self):
        n = C.c_uint32()
        self._ck(lib.pt_group_size(self.h, C.byref(n)))
        return n.value

    def set_triangles(self, tris):
        tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
        self._ck(lib.pt_group_set_triangles(self.h, _p(tris, C.c_float), C.c_uint32(tris.size // 9)))
        self.num_tris = tris.size // 9

    def update_triangles(self, tris):
        tris = np.ascontiguousarray(tris, np.float32).reshape(-1)
        self._ck(lib.pt_group_update_triangles(self.h, _p(tris, C.c_float), C.c_uint32(tris.size // 9)))

    def build_bvh(self, accel=PT_ACCEL_REFERENCE):
        if accel == PT_ACCEL_REFERENCE:
            self._ck(lib.pt_group_build_bvh(self.h))
        else:
            self._ck(lib.pt_group_build_bvh_accel(self.h, C.c_uint32(accel)))

    def set_bvh4(self, bvh4):
        bvh4 = np.ascontiguousarray(bvh4, np.uint32)
        self._ck(lib.pt_group_set_bvh4(self.h, _p(bvh4, C.c_uint32), C.c_uint64(bvh4.size)))

    def set_bvh2(self, bvh2):
        bvh2 = np.ascontiguousarray(bvh2, np.uint32)
        self._ck(lib.pt_group_set_bvh2(self.h, _p(bvh2, C.c_uint32), C.c_uint64(bvh2.size)))

    def set_batch(self, frames_per_launch):
        self._ck(lib.pt_group_set_batch(self.h, C.c_uint32(frames_per_launch)))

    def make_params(self, *a, **kw):
        kw.setdefault("num_tris", self.num_tris)
        return Context.make_params(self, *a, **kw)

    def render(self, params):
        self._ck(lib.pt_group_render(self.h, C.byref(params)))
        self._last = (params.width, params.height)

    def flush(self):
        self._ck(lib.pt_group_flush(self.h))

    def synchronize(self):
        self._ck(lib.pt_group_synchronize(self.h))

    def read_radiance(self):
        w, h = self._last
        out = np.zeros((h, w, 4), np.float32)
        self._ck(lib.pt_group_read_radiance(self.h, _p(out, C.c_float), C.c_uint64(out.size)))
        return out

    def read_rgba8(self):
        w, h = self._last
        out = np.zeros((h, w, 4), np.uint8)
        self._ck(lib.pt_group_read_rgba8(self.h, _p(out, C.c_uint8), C.c_uint64(out.size)))
        return out


class PathTracer:
    """Python mirror of the reference's PathTracer class (src/libs/PathTracer.js): same method
    names, argument meaning and return shapes; `canvas` is any object with width/height."""

    def __init__(self, canvas, device=-1):
        self.canvas = canvas
        self.cameraPosition = [0.0, 0.0, 3.5]            # PathTracer.js:67
        self.cameraQuaternion = [0.0, 0.0, 0.0, 1.0]
        self.frameCount = 0
        self.trianglesData = np.array([                  # default tetrahedron, PathTracer.js:79-84
            1, 1, 1, -1, -1, 1, -1, 1, -1,
            1, 1, 1, -1, 1, -1, 1, -1, -1,
            1, 1, 1, 1, -1, -1, -1, -1, 1,
            -1, -1, 1, 1, -1, -1, -1, 1, -1], np.float32)
        self.options = {"mode": PT_MODE_REFERENCE, "spp": 1, "maxBounces": 0, "seed": 1, "accumulate": False}
        self._device = device
        self.ctx = None

    def initialize(self):                                 # PathTracer.js:97-102
        self.ctx = Context(self._device)

    def computeBVH2Sizing(self, numTris):                 # :227
        return compute_bvh2_sizing(numTris)

    def computeBVH4Sizing(self, numNodes4):               # :234
        return compute_bvh4_sizing(numNodes4)

    def buildMortonAndSort(self, trianglesData):          # :427
        m, t = morton_sort(trianglesData)
        return {"mortonSorted": m, "triIndexSorted": t}

    def collapseLBVH2ToBVH4(self, bvh2U32, numTris):      # :506
        b, n = collapse_lbvh2_to_bvh4(bvh2U32, numTris)
        return {"bvh4U32": b, "numNodes4": n}

    def readBVH2(self, nbytes=None):                      # :485
        out = self.ctx.read_bvh2()
        return out if nbytes is None else out[: max(4, nbytes) // 4]

    def buildBVH(self, trianglesData):                    # :671
        if self.ctx is None:
            return                                        # `if (!device) return`, :673
        self.ctx.set_triangles(trianglesData)
        self.ctx.build_bvh()

    def setScene(self, scene):                            # :751
        self.trianglesData = np.ascontiguousarray(scene.getTrianglesFloat32(), np.float32)
        self.buildBVH(self.trianglesData)

    def render(self):                                     # :756
        if self.ctx is None or not self.ctx.scene_info()["numNodes4"] and self.trianglesData.size:
            return
        o = self.options
        p = self.ctx.make_params(self.canvas.width, self.canvas.height, self.cameraPosition, self.cameraQuaternion,
                                 mode=o["mode"], spp=o["spp"], max_bounces=o["maxBounces"], seed=o["seed"],
                                 frame=self.frameCount, accumulate=o["accumulate"], num_tris=self.trianglesData.size // 9)
        self.ctx.render(p)

    def readRadiance(self):
        return self.ctx.read_radiance()

    def setCameraPosition(self, x, y, z):                 # :824
        self.cameraPosition = [x, y, z]

    def setCameraQuaternion(self, x, y, z, w):            # :828
        self.cameraQuaternion = [x, y, z, w]

    def setFrameCount(self, frameCount):                  # :832
        self.frameCount = frameCount
