/* addon.c -- thin N-API binding of the C ABI in include/mi355pt.h.
 *
 * This is the reference-side stub INTEGRATION.md describes: the reference's host is JavaScript
 * (src/libs/PathTracer.js drives WebGPU); here the same JS class drives libmi355pt through
 * these synchronous entry points.  Typed arrays in, typed arrays out, a non-zero PtStatus
 * becomes a thrown Error (the reference's error convention: exceptions / rejected Promises).
 * Pure N-API (ABI-stable, no V8 / nan), C only.
 */
#include <node_api.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <stdio.h>
#include <math.h>

#include "mi355pt.h"

#define NAPI_OK(call) do { if ((call) != napi_ok) { napi_throw_error(env, NULL, "N-API call failed: " #call); return NULL; } } while (0)

static napi_value throw_pt(napi_env env, PtContext* ctx, int rc, const char* where) {
    char msg[512];
    const char* e = pt_last_error(ctx);
    snprintf(msg, sizeof msg, "%s: libmi355pt error %d: %s", where, rc, e ? e : "");
    char code[16]; snprintf(code, sizeof code, "PT%d", rc);
    napi_throw_error(env, code, msg);
    return NULL;
}
#define PT_CALL(ctx, call, where) do { int rc__ = (call); if (rc__ != 0) return throw_pt(env, (ctx), rc__, (where)); } while (0)

static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value* argv) {
    size_t argc = want;
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < want) {
        napi_throw_type_error(env, NULL, "wrong number of arguments");
        return 0;
    }
    return 1;
}

static int get_typed(napi_env env, napi_value v, napi_typedarray_type want, void** data, size_t* length) {
    bool is = false;
    if (napi_is_typedarray(env, v, &is) != napi_ok || !is) { napi_throw_type_error(env, NULL, "expected a typed array"); return 0; }
    napi_typedarray_type t; napi_value ab; size_t off;
    if (napi_get_typedarray_info(env, v, &t, length, data, &ab, &off) != napi_ok) { napi_throw_type_error(env, NULL, "bad typed array"); return 0; }
    if (t != want) { napi_throw_type_error(env, NULL, "typed array of the wrong element type"); return 0; }
    return 1;
}

static napi_value make_typed(napi_env env, napi_typedarray_type t, size_t elem_size, size_t length, void** data) {
    napi_value ab, ta;
    if (napi_create_arraybuffer(env, length * elem_size, data, &ab) != napi_ok) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    if (napi_create_typedarray(env, t, length, ab, 0, &ta) != napi_ok) { napi_throw_error(env, NULL, "typed array creation failed"); return NULL; }
    return ta;
}

static PtContext* get_ctx(napi_env env, napi_value v) {
    void* p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p) { napi_throw_type_error(env, NULL, "expected a context handle"); return NULL; }
    return *(PtContext**)p;
}

static void finalize_ctx(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    PtContext** box = (PtContext**)data;
    if (*box) pt_destroy(*box);
    free(box);
}

static uint32_t get_u32(napi_env env, napi_value v) { uint32_t x = 0; napi_get_value_uint32(env, v, &x); return x; }
static double get_f64(napi_env env, napi_value v) { double x = 0; napi_get_value_double(env, v, &x); return x; }
static uint32_t prop_u32(napi_env env, napi_value obj, const char* name, uint32_t dflt) {
    napi_value v; bool has = false;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return dflt;
    napi_get_named_property(env, obj, name, &v);
    napi_valuetype t; napi_typeof(env, v, &t);
    if (t == napi_boolean) { bool b = false; napi_get_value_bool(env, v, &b); return b ? 1u : 0u; }
    if (t != napi_number) return dflt;
    double d = 0; napi_get_value_double(env, v, &d);
    return (uint32_t)d;
}
static double prop_f64(napi_env env, napi_value obj, const char* name, double dflt) {
    napi_value v; bool has = false;
    if (napi_has_named_property(env, obj, name, &has) != napi_ok || !has) return dflt;
    napi_get_named_property(env, obj, name, &v);
    napi_valuetype t; napi_typeof(env, v, &t);
    if (t != napi_number) return dflt;
    double d = 0; napi_get_value_double(env, v, &d);
    return d;
}
static void set_num(napi_env env, napi_value obj, const char* name, double v) {
    napi_value n; napi_create_double(env, v, &n); napi_set_named_property(env, obj, name, n);
}

/* ---- context --------------------------------------------------------------------- */

static napi_value fn_create(napi_env env, napi_callback_info info) {          /* PathTracer.initialize(), PathTracer.js:97 */
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    int32_t dev = -1; napi_get_value_int32(env, argv[0], &dev);
    PtContext** box = (PtContext**)calloc(1, sizeof(PtContext*));
    int rc = pt_create(dev, box);
    if (rc != 0) { free(box); return throw_pt(env, NULL, rc, "pt_create"); }
    napi_value ext;
    NAPI_OK(napi_create_external(env, box, finalize_ctx, NULL, &ext));
    return ext;
}

static napi_value fn_destroy(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    void* p = NULL;
    if (napi_get_value_external(env, argv[0], &p) == napi_ok && p) { PtContext** box = (PtContext**)p; if (*box) { pt_destroy(*box); *box = NULL; } }
    return NULL;
}

static napi_value fn_version(napi_env env, napi_callback_info info) {
    (void)info; napi_value s; NAPI_OK(napi_create_string_utf8(env, pt_version(), NAPI_AUTO_LENGTH, &s)); return s;
}

/* ---- host-side scene build -------------------------------------------------------- */

static napi_value fn_bvh2_sizing(napi_env env, napi_callback_info info) {     /* computeBVH2Sizing, PathTracer.js:227 */
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    double n = get_f64(env, argv[0]);
    uint32_t nn = 0; uint64_t bytes = 4;
    pt_compute_bvh2_sizing(n > 0 ? (uint32_t)n : 0u, &nn, &bytes);
    napi_value o; NAPI_OK(napi_create_object(env, &o));
    set_num(env, o, "numNodes2", nn); set_num(env, o, "bytes", (double)bytes);
    return o;
}
static napi_value fn_bvh4_sizing(napi_env env, napi_callback_info info) {     /* computeBVH4Sizing, PathTracer.js:234 */
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    double n = get_f64(env, argv[0]);
    uint64_t bytes = 4;
    pt_compute_bvh4_sizing(n > 0 ? (uint32_t)n : 0u, &bytes);
    napi_value o; NAPI_OK(napi_create_object(env, &o));
    set_num(env, o, "bytes", (double)bytes);
    return o;
}

static napi_value fn_morton_sort(napi_env env, napi_callback_info info) {     /* buildMortonAndSort, PathTracer.js:427 */
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    void* tris; size_t len; if (!get_typed(env, argv[0], napi_float32_array, &tris, &len)) return NULL;
    uint32_t n = (uint32_t)(len / 9);
    void *m, *t;
    napi_value ms = make_typed(env, napi_uint32_array, 4, n, &m); if (!ms) return NULL;
    napi_value ts = make_typed(env, napi_uint32_array, 4, n, &t); if (!ts) return NULL;
    PT_CALL(NULL, pt_morton_sort((const float*)tris, n, (uint32_t*)m, (uint32_t*)t), "pt_morton_sort");
    napi_value o; NAPI_OK(napi_create_object(env, &o));
    napi_set_named_property(env, o, "mortonSorted", ms); napi_set_named_property(env, o, "triIndexSorted", ts);
    return o;
}

static napi_value fn_collapse(napi_env env, napi_callback_info info) {        /* collapseLBVH2ToBVH4, PathTracer.js:506 */
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    void* b2; size_t len; if (!get_typed(env, argv[0], napi_uint32_array, &b2, &len)) return NULL;
    uint32_t n = get_u32(env, argv[1]);
    uint64_t need2 = n ? 1ull + 6ull * (2ull * n - 1ull) : 1ull;
    if (len < need2) { napi_throw_range_error(env, NULL, "BVH2 buffer shorter than 1 + 6*(2N-1) words"); return NULL; }
    uint64_t cap = n ? 1ull + 8ull * (2ull * n - 1ull) : 1ull;
    uint32_t* tmp = (uint32_t*)malloc(cap * 4);
    if (!tmp) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    uint32_t n4 = 0;
    int rc = pt_collapse_lbvh2_to_bvh4((const uint32_t*)b2, n, tmp, cap, &n4);
    if (rc != 0) { free(tmp); return throw_pt(env, NULL, rc, "pt_collapse_lbvh2_to_bvh4"); }
    size_t words = n ? 1 + 8 * (size_t)n4 : 1;
    void* out; napi_value ta = make_typed(env, napi_uint32_array, 4, words, &out);
    if (!ta) { free(tmp); return NULL; }
    memcpy(out, tmp, words * 4); free(tmp);
    napi_value o; NAPI_OK(napi_create_object(env, &o));
    napi_set_named_property(env, o, "bvh4U32", ta); set_num(env, o, "numNodes4", n4);
    return o;
}

static napi_value fn_bvh4_wide(napi_env env, napi_callback_info info) {       /* tests/test.cpp:106-196 */
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    void* b2; size_t len; if (!get_typed(env, argv[0], napi_uint32_array, &b2, &len)) return NULL;
    if (len < 1) { napi_throw_range_error(env, NULL, "empty BVH2 buffer"); return NULL; }
    size_t words = 1 + 8 * (size_t)((const uint32_t*)b2)[0];
    void* out; napi_value ta = make_typed(env, napi_uint32_array, 4, words, &out); if (!ta) return NULL;
    PT_CALL(NULL, pt_bvh2_to_bvh4_wide((const uint32_t*)b2, len, (uint32_t*)out, words), "pt_bvh2_to_bvh4_wide");
    return ta;
}

static napi_value fn_write_u32(napi_env env, napi_callback_info info) {       /* data/BVH2.bin writer, src/server/api.js:27-31 */
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    char path[4096]; size_t pl = 0; NAPI_OK(napi_get_value_string_utf8(env, argv[0], path, sizeof path, &pl));
    void* d; size_t len; if (!get_typed(env, argv[1], napi_uint32_array, &d, &len)) return NULL;
    PT_CALL(NULL, pt_file_write_u32(path, (const uint32_t*)d, len), "pt_file_write_u32");
    return NULL;
}
static napi_value fn_read_u32(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    char path[4096]; size_t pl = 0; NAPI_OK(napi_get_value_string_utf8(env, argv[0], path, sizeof path, &pl));
    uint64_t words = 0;
    PT_CALL(NULL, pt_file_read_u32(path, NULL, 0, &words), "pt_file_read_u32");
    void* out; napi_value ta = make_typed(env, napi_uint32_array, 4, (size_t)words, &out); if (!ta) return NULL;
    PT_CALL(NULL, pt_file_read_u32(path, (uint32_t*)out, words, &words), "pt_file_read_u32");
    return ta;
}

static napi_value fn_procedural(napi_env env, napi_callback_info info) {
    napi_value argv[3]; if (!get_args(env, info, 3, argv)) return NULL;
    uint32_t kind = get_u32(env, argv[0]), n = get_u32(env, argv[1]), seed = get_u32(env, argv[2]);
    void* out; napi_value ta = make_typed(env, napi_float32_array, 4, (size_t)n * 9, &out); if (!ta) return NULL;
    PT_CALL(NULL, pt_scene_procedural(kind, seed, n, (float*)out), "pt_scene_procedural");
    return ta;
}

/* ---- device scene state ----------------------------------------------------------- */

static napi_value fn_set_triangles(napi_env env, napi_callback_info info) {   /* writeBuffer(triangles), PathTracer.js:679 */
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    void* d; size_t len; if (!get_typed(env, argv[1], napi_float32_array, &d, &len)) return NULL;
    PT_CALL(ctx, pt_set_triangles(ctx, (const float*)d, (uint32_t)(len / 9)), "pt_set_triangles");
    return NULL;
}
/* new vertices, the same tree: refit in place (pt_update_triangles); the array is copied during the call */
static napi_value fn_update_triangles(napi_env env, napi_callback_info info) {
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    void* d; size_t len; if (!get_typed(env, argv[1], napi_float32_array, &d, &len)) return NULL;
    if (len % 9) { napi_throw_type_error(env, NULL, "updateTriangles: 9 floats per triangle"); return NULL; }
    PT_CALL(ctx, pt_update_triangles(ctx, (const float*)d, (uint32_t)(len / 9)), "pt_update_triangles");
    return NULL;
}
static napi_value fn_bvh_cost(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    double cost = 0; PT_CALL(ctx, pt_bvh_cost(ctx, &cost), "pt_bvh_cost");
    napi_value v; NAPI_OK(napi_create_double(env, cost, &v)); return v;
}
/* optional second argument of buildBVH / groupBuildBVH: the tree-quality level (PT_ACCEL_*), 0 when absent or undefined */
static int get_accel(napi_env env, napi_callback_info info, napi_value* argv, uint32_t* accel) {
    size_t argc = 2;
    if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < 1) { napi_throw_type_error(env, NULL, "wrong number of arguments"); return 0; }
    *accel = 0;
    if (argc >= 2) {
        napi_valuetype t; napi_typeof(env, argv[1], &t);
        if (t == napi_number) *accel = get_u32(env, argv[1]);
        else if (t != napi_undefined) { napi_throw_type_error(env, NULL, "accel must be a number"); return 0; }
    }
    return 1;
}
static napi_value fn_build_bvh(napi_env env, napi_callback_info info) {       /* buildBVH, PathTracer.js:671-749 */
    napi_value argv[2]; uint32_t accel; if (!get_accel(env, info, argv, &accel)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    if (accel == PT_ACCEL_REFERENCE) PT_CALL(ctx, pt_build_bvh(ctx), "pt_build_bvh");
    else PT_CALL(ctx, pt_build_bvh_accel(ctx, accel), "pt_build_bvh_accel");
    return NULL;
}
static napi_value fn_read_bvh2(napi_env env, napi_callback_info info) {       /* readBVH2, PathTracer.js:485 */
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    double bytes = get_f64(env, argv[1]);
    size_t size = bytes < 4 ? 4 : (size_t)bytes;                                /* Math.max(4, bytes), :486 */
    void* out; napi_value ta = make_typed(env, napi_uint32_array, 4, size / 4, &out); if (!ta) return NULL;
    PT_CALL(ctx, pt_read_bvh2(ctx, (uint32_t*)out, (size / 4) * 4), "pt_read_bvh2");
    return ta;
}
static napi_value fn_read_bvh4(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    uint32_t n4 = 0; pt_scene_info(ctx, NULL, NULL, &n4);
    size_t words = 1 + 8 * (size_t)n4;
    void* out; napi_value ta = make_typed(env, napi_uint32_array, 4, words, &out); if (!ta) return NULL;
    PT_CALL(ctx, pt_read_bvh4(ctx, (uint32_t*)out, words * 4), "pt_read_bvh4");
    return ta;
}
static napi_value fn_set_bvh4(napi_env env, napi_callback_info info) {        /* writeBuffer(BVH), PathTracer.js:739-740 */
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    void* d; size_t len; if (!get_typed(env, argv[1], napi_uint32_array, &d, &len)) return NULL;
    PT_CALL(ctx, pt_set_bvh4(ctx, (const uint32_t*)d, len), "pt_set_bvh4");
    return NULL;
}
static napi_value fn_set_bvh2(napi_env env, napi_callback_info info) {
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    void* d; size_t len; if (!get_typed(env, argv[1], napi_uint32_array, &d, &len)) return NULL;
    PT_CALL(ctx, pt_set_bvh2(ctx, (const uint32_t*)d, len), "pt_set_bvh2");
    return NULL;
}
static napi_value fn_set_spheres(napi_env env, napi_callback_info info) {     /* config C1 extension: (x,y,z,r) per sphere */
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    void* d; size_t len; if (!get_typed(env, argv[1], napi_float32_array, &d, &len)) return NULL;
    PT_CALL(ctx, pt_set_spheres(ctx, (const float*)d, (uint32_t)(len / 4)), "pt_set_spheres");
    return NULL;
}
static napi_value fn_scene_info(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    uint32_t a = 0, b = 0, c = 0; pt_scene_info(ctx, &a, &b, &c);
    napi_value o; NAPI_OK(napi_create_object(env, &o));
    set_num(env, o, "numTris", a); set_num(env, o, "numNodes2", b); set_num(env, o, "numNodes4", c);
    return o;
}

/* ---- the hot path ------------------------------------------------------------------ */

/* argv: the 16-float UBO exactly as PathTracer.js:764-787 packs it + the extension options */
static int params_from_ubo(napi_env env, napi_value ubo_v, napi_value opt, PtRenderParams* p) {
    void* u; size_t len; if (!get_typed(env, ubo_v, napi_float32_array, &u, &len)) return 0;
    if (len < 16) { napi_throw_range_error(env, NULL, "UBO must hold 16 floats"); return 0; }
    const float* ubo = (const float*)u;
    memset(p, 0, sizeof *p);
    p->width = (uint32_t)ubo[0]; p->height = (uint32_t)ubo[1];                  /* u32(ubo.resolution.xy), renderer.wgsl:357 */
    p->focal = ubo[2]; p->aspect = ubo[3];
    p->cam_pos[0] = ubo[4]; p->cam_pos[1] = ubo[5]; p->cam_pos[2] = ubo[6];
    p->num_tris = (uint32_t)ubo[7];                                             /* u32(camPosNumTris.w), renderer.wgsl:398 */
    p->cam_quat[0] = ubo[8]; p->cam_quat[1] = ubo[9]; p->cam_quat[2] = ubo[10]; p->cam_quat[3] = ubo[11];
    p->frame = (uint32_t)ubo[12];
    p->mode = prop_u32(env, opt, "mode", PT_MODE_REFERENCE);
    p->spp = prop_u32(env, opt, "spp", 1);
    p->max_bounces = prop_u32(env, opt, "maxBounces", 0);
    p->seed = prop_u32(env, opt, "seed", 1);
    p->accumulate = prop_u32(env, opt, "accumulate", 0);
    p->tile_rank = prop_u32(env, opt, "tileRank", 0);
    p->tile_count = prop_u32(env, opt, "tileCount", 1);
    p->flags = (prop_u32(env, opt, "stats", 0) ? PT_FLAG_STATS : 0u) | (prop_u32(env, opt, "simpleKernel", 0) ? PT_FLAG_SIMPLE_KERNEL : 0u) |
               (prop_u32(env, opt, "bruteForce", 0) ? PT_FLAG_BRUTE_FORCE : 0u);
    (void)prop_f64;
    return 1;
}

static napi_value fn_render(napi_env env, napi_callback_info info) {          /* PathTracer.render() compute pass, PathTracer.js:756-802 */
    napi_value argv[3]; if (!get_args(env, info, 3, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    PtRenderParams p; if (!params_from_ubo(env, argv[1], argv[2], &p)) return NULL;
    PT_CALL(ctx, pt_render(ctx, &p), "pt_render");
    return NULL;
}

/* ---- batched queries over the context's tree (extensions beyond the reference; include/mi355pt.h pt_*_host) ----------------------------- */

/* Every query takes a Float32Array of records and answers with 16-byte result records or with uint32 counts.  What differs is said once, here:
 *   traceRays       rays: 8 floats per ray (PtRay: org xyz, tMax, dir xyz, reserved); anyHit -> { t: Float32Array, prim: Uint32Array, u, v }
 *   closestPoints   points: 4 floats per point (PtPoint: x, y, z, rMax); flags: PT_CLOSEST_* -> { dist, prim, u, v }
 *   sweepSpheres    sweeps: 8 floats per sweep (PtSweep: org xyz, tMax, dir xyz, radius); flags: PT_SWEEP_* -> { t, prim, u, v }
 *   nearestK        points, k: 1 .. PT_NEAREST_MAX_K, flags: PT_NEAREST_* -> { k, dist: Float32Array of n * k, prim, u, v }: row i at
 *                   [i * k, i * k + k), ascending by dist, padded with dist = Infinity and prim = 0xFFFFFFFF
 *   signedDistance  points; opt as contains -> { dist, prim, u, v }, dist negative inside
 *   contains        points (rMax ignored); opt: { samples (3), seed, indexBase, simple } -> { inside: Uint32Array, odd, samples }
 *   occlusion       surfels: 8 floats per surfel (PtSurfel: p xyz, rMax, n xyz, reserved); opt: { samples (16), seed, bias, indexBase, simple }
 *                   -> { visibility: Float32Array, unoccluded: Uint32Array, samples: Uint32Array }
 *   countHits, radiusCount, boxCount   rays | points | boxes (8 floats per box: lo xyz, pad, hi xyz, pad); flags -> Uint32Array
 *   radiusSearch, boxSearch, listHits  the same records; flags -> { offsets: Float64Array of n + 1 (exact: the total is far below 2^53),
 *                   dist | t, prim, u, v } or, of boxes, { offsets, prim, vertsInside }: every entry.  The first call has room for 16 entries
 *                   per point or box and 4 per ray; when offsets[n] says that this was too little, the query runs again with room for all. */
typedef enum { Q_TRACE, Q_CLOSEST, Q_SWEEP, Q_NEAREST, Q_SIGNED, Q_CONTAINS, Q_OCCLUSION, Q_COUNT, Q_RADIUS_COUNT, Q_BOX_COUNT,
               Q_RADIUS, Q_BOX, Q_HITS, Q_SURFELS } Query;

/* floats per record, the range error of a partial record, throw_pt's label, the result columns and their types (f: Float32Array, u:
 * Uint32Array; none: counts), and of a list query the entries per record of the first call */
static const struct QueryKind { size_t floats; const char* partial; const char* label; const char* names[4]; const char* types; uint64_t guess; } KINDS[] = {
    [Q_TRACE]        = {8, "traceRays: 8 floats per ray", "pt_trace_rays_host", {"t", "prim", "u", "v"}, "fuff", 0},
    [Q_CLOSEST]      = {4, "closestPoints: 4 floats per point", "pt_closest_points_host", {"dist", "prim", "u", "v"}, "fuff", 0},
    [Q_SWEEP]        = {8, "sweepSpheres: 8 floats per sweep", "pt_sweep_spheres_host", {"t", "prim", "u", "v"}, "fuff", 0},
    [Q_NEAREST]      = {4, "nearestK: 4 floats per point", "pt_nearest_k_host", {"dist", "prim", "u", "v"}, "fuff", 0},
    [Q_SIGNED]       = {4, "signedDistance: 4 floats per point", "pt_signed_distance_host", {"dist", "prim", "u", "v"}, "fuff", 0},
    [Q_CONTAINS]     = {4, "contains: 4 floats per point", "pt_contains_host", {"inside", "odd", "samples"}, "uuu", 0},
    [Q_OCCLUSION]    = {8, "occlusion: 8 floats per surfel", "pt_occlusion_host", {"visibility", "unoccluded", "samples"}, "fuu", 0},
    [Q_COUNT]        = {8, "countHits: 8 floats per ray", "pt_count_hits_host", {0}, NULL, 0},
    [Q_RADIUS_COUNT] = {4, "radiusCount: 4 floats per point", "pt_radius_count_host", {0}, NULL, 0},
    [Q_BOX_COUNT]    = {8, "boxCount: 8 floats per box", "pt_box_count_host", {0}, NULL, 0},
    [Q_RADIUS]       = {4, "radiusSearch: 4 floats per point", "pt_radius_search_host", {"dist", "prim", "u", "v"}, "fuff", 16},
    [Q_BOX]          = {8, "boxSearch: 8 floats per box", "pt_box_search_host", {"prim", "vertsInside"}, "uu", 16},
    [Q_HITS]         = {8, "listHits: 8 floats per ray", "pt_list_hits_host", {"t", "prim", "u", "v"}, "fuff", 4},
};

/* the one place that calls the pt_*_host entry points, each with its own types */
static int call_host(Query q, PtContext* ctx, const void* rec, size_t n, uint32_t flags, uint32_t k, const void* params,
                     void* out, uint64_t* off, uint64_t cap) {
    switch (q) {
    case Q_TRACE:        return pt_trace_rays_host(ctx, (const PtRay*)rec, n, flags, (PtHit*)out);
    case Q_CLOSEST:      return pt_closest_points_host(ctx, (const PtPoint*)rec, n, flags, (PtClosest*)out);
    case Q_SWEEP:        return pt_sweep_spheres_host(ctx, (const PtSweep*)rec, n, flags, (PtHit*)out);
    case Q_NEAREST:      return pt_nearest_k_host(ctx, (const PtPoint*)rec, n, k, flags, (PtClosest*)out);
    case Q_SIGNED:       return pt_signed_distance_host(ctx, (const PtPoint*)rec, n, (const PtContainParams*)params, (PtClosest*)out);
    case Q_CONTAINS:     return pt_contains_host(ctx, (const PtPoint*)rec, n, (const PtContainParams*)params, (PtContainment*)out);
    case Q_OCCLUSION:    return pt_occlusion_host(ctx, (const PtSurfel*)rec, n, (const PtOcclusionParams*)params, (PtOcclusion*)out);
    case Q_COUNT:        return pt_count_hits_host(ctx, (const PtRay*)rec, n, flags, (uint32_t*)out);
    case Q_RADIUS_COUNT: return pt_radius_count_host(ctx, (const PtPoint*)rec, n, flags, (uint32_t*)out);
    case Q_BOX_COUNT:    return pt_box_count_host(ctx, (const PtBox*)rec, n, flags, (uint32_t*)out);
    case Q_RADIUS:       return pt_radius_search_host(ctx, (const PtPoint*)rec, n, flags, off, (PtClosest*)out, cap);
    case Q_BOX:          return pt_box_search_host(ctx, (const PtBox*)rec, n, flags, off, (PtOverlap*)out, cap);
    case Q_HITS:         return pt_list_hits_host(ctx, (const PtRay*)rec, n, flags, off, (PtHit*)out, cap);
    default:             return -1;
    }
}

/* The record intake: a Float32Array of `floats` per record -> a copy in 16-byte aligned host memory (a typed array's data need not be
 * aligned) and the record count; the caller frees it. */
static void* records_in(napi_env env, napi_value v, size_t floats, const char* partial, size_t* n) {
    void* d; size_t len; if (!get_typed(env, v, napi_float32_array, &d, &len)) return NULL;
    if (len % floats) { napi_throw_range_error(env, NULL, partial); return NULL; }
    *n = len / floats;
    void* rec = aligned_alloc(16, (*n ? *n : 1) * floats * sizeof(float));
    if (!rec) { napi_throw_error(env, NULL, "out of memory"); return NULL; }
    if (*n) memcpy(rec, d, *n * floats * sizeof(float));
    return rec;
}

/* The result builder: m 16-byte records -> an object of their leading columns, one typed array of m per letter of `types`, under `names`;
 * before them `k` when it is not 0 and `offsets` (n + 1 of them) when off is not NULL. */
static napi_value columns_out(napi_env env, const char* const* names, const char* types, const void* rec, size_t m,
                              uint32_t k, const uint64_t* off, size_t n) {
    napi_value o; NAPI_OK(napi_create_object(env, &o));
    if (k) { napi_value kv; NAPI_OK(napi_create_uint32(env, k, &kv)); napi_set_named_property(env, o, "k", kv); }
    if (off) {
        void* po; napi_value offs = make_typed(env, napi_float64_array, 8, n + 1, &po); if (!offs) return NULL;
        for (size_t i = 0; i <= n; ++i) ((double*)po)[i] = (double)off[i];
        napi_set_named_property(env, o, "offsets", offs);
    }
    for (size_t c = 0; types[c]; ++c) {
        void* p; napi_value col = make_typed(env, types[c] == 'f' ? napi_float32_array : napi_uint32_array, 4, m, &p); if (!col) return NULL;
        for (size_t i = 0; i < m; ++i) memcpy((char*)p + 4 * i, (const char*)rec + 16 * i + 4 * c, 4);
        napi_set_named_property(env, o, names[c], col);
    }
    return o;
}

/* A query that is one call: n records in, n (nearestK: n * k) result records out. */
static napi_value run_query(napi_env env, PtContext* ctx, Query q, napi_value records_v, uint32_t flags, uint32_t k, const void* params) {
    const struct QueryKind* kind = &KINDS[q];
    size_t n; void* rec = records_in(env, records_v, kind->floats, kind->partial, &n); if (!rec) return NULL;
    const size_t m = n * (k ? k : 1);
    napi_value result = NULL; void* out = NULL; int rc;
    if (q == Q_NEAREST && (k == 0 || k > PT_NEAREST_MAX_K)) napi_throw_range_error(env, NULL, "nearestK: k must be 1 .. 64");
    else if (!(out = aligned_alloc(16, (m ? m : 1) * 16))) napi_throw_error(env, NULL, "out of memory");
    else if ((rc = call_host(q, ctx, rec, n, flags, k, params, out, NULL, 0)) != 0) throw_pt(env, ctx, rc, kind->label);
    else result = columns_out(env, kind->names, kind->types, out, m, k, NULL, 0);
    free(rec); free(out);
    return result;
}

/* A count query: the counts go straight into the Uint32Array. */
static napi_value run_count(napi_env env, PtContext* ctx, Query q, napi_value records_v, uint32_t flags) {
    size_t n; void* rec = records_in(env, records_v, KINDS[q].floats, KINDS[q].partial, &n); if (!rec) return NULL;
    void* pc; napi_value counts = make_typed(env, napi_uint32_array, 4, n, &pc);
    uint32_t none = 0;                                                          /* an empty typed array may have no data pointer */
    const int rc = counts ? call_host(q, ctx, rec, n, flags, 0, NULL, n ? pc : (void*)&none, NULL, 0) : 0;
    free(rec);
    return rc != 0 ? throw_pt(env, ctx, rc, KINDS[q].label) : counts;
}

/* A list query: room for `guess` entries per record at first, and again with room for all when offsets[n] says that this was too little.
 * Every path leaves through `done`, which frees what there is. */
static napi_value run_list(napi_env env, PtContext* ctx, Query q, napi_value records_v, uint32_t flags) {
    const struct QueryKind* kind = &KINDS[q];
    size_t n; void* rec = records_in(env, records_v, kind->floats, kind->partial, &n); if (!rec) return NULL;
    napi_value result = NULL;
    uint64_t cap = kind->guess * (uint64_t)n + 64;
    uint64_t* off = (uint64_t*)malloc((n + 1) * sizeof(uint64_t));
    void* out = aligned_alloc(16, (size_t)cap * 16);
    if (!off || !out) { napi_throw_error(env, NULL, "out of memory"); goto done; }
    int rc = call_host(q, ctx, rec, n, flags, 0, NULL, out, off, cap);
    if (rc == 0 && off[n] > cap) {
        cap = off[n];
        free(out);
        out = aligned_alloc(16, (size_t)cap * 16);
        if (!out) { napi_throw_error(env, NULL, "out of memory"); goto done; }
        rc = call_host(q, ctx, rec, n, flags, 0, NULL, out, off, cap);
    }
    result = rc != 0 ? throw_pt(env, ctx, rc, kind->label) : columns_out(env, kind->names, kind->types, out, (size_t)off[n], 0, off, n);
done:
    free(rec); free(off); free(out);
    return result;
}

/* rays: Float32Array (8 floats per ray); t, prim, u, v: what traceRays resolved to; rMax -> Float32Array of 8 floats per surfel */
static napi_value hit_surfels_on(napi_env env, PtContext* ctx, napi_value* a) {
    void *d, *pt, *pp, *pu, *pv; size_t len, nt, np, nu, nv;
    if (!get_typed(env, a[0], napi_float32_array, &d, &len) || !get_typed(env, a[1], napi_float32_array, &pt, &nt) ||
        !get_typed(env, a[2], napi_uint32_array, &pp, &np) || !get_typed(env, a[3], napi_float32_array, &pu, &nu) ||
        !get_typed(env, a[4], napi_float32_array, &pv, &nv)) return NULL;
    const size_t n = len / 8;
    if (len % 8 || nt != n || np != n || nu != n || nv != n) { napi_throw_range_error(env, NULL, "hitSurfels: 8 floats per ray and one hit per ray"); return NULL; }
    const float r_max = (float)get_f64(env, a[5]);
    PtRay* rays = (PtRay*)aligned_alloc(16, (n ? n : 1) * sizeof(PtRay));
    PtHit* hits = (PtHit*)aligned_alloc(16, (n ? n : 1) * sizeof(PtHit));
    PtSurfel* sf = (PtSurfel*)aligned_alloc(16, (n ? n : 1) * sizeof(PtSurfel));
    if (!rays || !hits || !sf) { free(rays); free(hits); free(sf); napi_throw_error(env, NULL, "out of memory"); return NULL; }
    if (n) memcpy(rays, d, n * sizeof(PtRay));
    for (size_t i = 0; i < n; ++i) { hits[i].t = ((float*)pt)[i]; hits[i].prim = ((uint32_t*)pp)[i]; hits[i].u = ((float*)pu)[i]; hits[i].v = ((float*)pv)[i]; }
    int rc = pt_hit_surfels_host(ctx, rays, hits, n, r_max, sf);
    free(rays); free(hits);
    if (rc != 0) { free(sf); return throw_pt(env, ctx, rc, "pt_hit_surfels_host"); }
    void* out; napi_value ta = make_typed(env, napi_float32_array, 4, n * 8, &out);
    if (ta && n) memcpy(out, sf, n * sizeof(PtSurfel));
    free(sf);
    return ta;
}

/* The camera ray of PT_MODE_REFERENCE through the centre of pixel (x, y) of the UBO's camera, as one PtRay record (8 floats, t_max = +inf):
 * renderer.wgsl:387-395 in the operation order of pt_device.h::primary_ray -- correctly rounded f32 division and square root, fmaf where it
 * has fma, nothing contracted (-ffp-contract=off) -- so the same bits as the ray pt_camera_rays writes and mode 1 traces. */
static napi_value fn_camera_ray(napi_env env, napi_callback_info info) {      /* (UBO Float32Array[16], x, y) */
    napi_value argv[3]; if (!get_args(env, info, 3, argv)) return NULL;
    void* u; size_t len; if (!get_typed(env, argv[0], napi_float32_array, &u, &len)) return NULL;
    if (len < 16) { napi_throw_range_error(env, NULL, "UBO must hold 16 floats"); return NULL; }
    const float* ubo = (const float*)u;
    const float w = (float)(uint32_t)ubo[0], h = (float)(uint32_t)ubo[1], focal = ubo[2], aspect = ubo[3];
    const float fx = (float)get_u32(env, argv[1]) + 0.5f, fy = (float)get_u32(env, argv[2]) + 0.5f;
    const float px = fmaf(fx / w, 2.0f, -1.0f), py = fmaf(fy / h, 2.0f, -1.0f);
    float vx = px * aspect, vy = py, vz = -focal;
    const float inv = 1.0f / sqrtf((vx * vx + vy * vy) + vz * vz);
    vx = vx * inv; vy = vy * inv; vz = vz * inv;
    const float qx = ubo[8], qy = ubo[9], qz = ubo[10], qs = ubo[11];                       /* rotateVectorByQuat, renderer.wgsl:66-72 */
    const float ux = qy * vz - qz * vy, uy = qz * vx - qx * vz, uz = qx * vy - qy * vx;     /* cross(q.xyz, v) */
    const float wx = qy * uz - qz * uy, wy = qz * ux - qx * uz, wz = qx * uy - qy * ux;     /* cross(q.xyz, uv) */
    void* r; napi_value out = make_typed(env, napi_float32_array, 4, 8, &r); if (!out) return NULL;
    float* ray = (float*)r;
    ray[0] = ubo[4]; ray[1] = ubo[5]; ray[2] = ubo[6]; ray[3] = INFINITY;
    ray[4] = fmaf(2.0f, fmaf(qs, ux, wx), vx); ray[5] = fmaf(2.0f, fmaf(qs, uy, wy), vy); ray[6] = fmaf(2.0f, fmaf(qs, uz, wz), vz); ray[7] = 0.0f;
    return out;
}

static napi_value fn_set_batch(napi_env env, napi_callback_info info) {       /* frames per persistent launch (1..256) */
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    PT_CALL(ctx, pt_set_batch(ctx, get_u32(env, argv[1])), "pt_set_batch");
    return NULL;
}
static napi_value fn_flush(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    PT_CALL(ctx, pt_flush(ctx), "pt_flush");
    return NULL;
}
static napi_value fn_last_ms(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    float ms = 0; PT_CALL(ctx, pt_last_render_ms(ctx, &ms), "pt_last_render_ms");
    napi_value v; NAPI_OK(napi_create_double(env, ms, &v)); return v;
}
static napi_value fn_sync(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    PT_CALL(ctx, pt_synchronize(ctx), "pt_synchronize");
    return NULL;
}
static napi_value fn_stats(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    PtStats st; PT_CALL(ctx, pt_get_stats(ctx, &st), "pt_get_stats");
    napi_value o; NAPI_OK(napi_create_object(env, &o));
    set_num(env, o, "raysClosest", (double)st.rays_closest); set_num(env, o, "raysShadow", (double)st.rays_shadow);
    set_num(env, o, "nodesExamined", (double)st.nodes_examined); set_num(env, o, "trisTested", (double)st.tris_tested);
    set_num(env, o, "stackDrops", (double)st.stack_drops); set_num(env, o, "maxStack", (double)st.max_stack);
    set_num(env, o, "samples", (double)st.samples);
    return o;
}
static napi_value fn_read_radiance(napi_env env, napi_callback_info info) {
    napi_value argv[3]; if (!get_args(env, info, 3, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    size_t n = (size_t)get_u32(env, argv[1]) * get_u32(env, argv[2]) * 4;
    void* out; napi_value ta = make_typed(env, napi_float32_array, 4, n, &out); if (!ta) return NULL;
    PT_CALL(ctx, pt_read_radiance(ctx, (float*)out, n), "pt_read_radiance");
    return ta;
}
static napi_value read_u8(napi_env env, napi_callback_info info, int which) {
    napi_value argv[4]; if (!get_args(env, info, which == 2 ? 4 : 3, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    size_t n = (size_t)get_u32(env, argv[1]) * get_u32(env, argv[2]) * 4;
    void* out; napi_value ta = make_typed(env, napi_uint8_array, 1, n, &out); if (!ta) return NULL;
    if (which == 1) PT_CALL(ctx, pt_read_rgba8(ctx, (uint8_t*)out, n), "pt_read_rgba8");
    else { bool q = true; napi_get_value_bool(env, argv[3], &q); PT_CALL(ctx, pt_read_tonemapped(ctx, q ? 1 : 0, (uint8_t*)out, n), "pt_read_tonemapped"); }
    return ta;
}
/* checkpoint of a progressive accumulation (pt_read_accum): { width, height, tileRank, tileCount, compact, samples, data: Float32Array } */
static napi_value fn_read_accum(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    PtAccumInfo ai; PT_CALL(ctx, pt_accum_info(ctx, &ai), "pt_accum_info");
    if (ai.floats == 0) { napi_throw_error(env, "PT4", "readAccumulation: no running accumulation (render with accumulate first)"); return NULL; }
    void* out; napi_value ta = make_typed(env, napi_float32_array, 4, (size_t)ai.floats, &out); if (!ta) return NULL;
    PT_CALL(ctx, pt_read_accum(ctx, (float*)out, ai.floats), "pt_read_accum");
    napi_value o; NAPI_OK(napi_create_object(env, &o));
    set_num(env, o, "width", ai.width); set_num(env, o, "height", ai.height); set_num(env, o, "tileRank", ai.tile_rank); set_num(env, o, "tileCount", ai.tile_count);
    set_num(env, o, "compact", ai.compact); set_num(env, o, "samples", ai.samples);
    napi_set_named_property(env, o, "data", ta);
    return o;
}
static napi_value fn_set_accum(napi_env env, napi_callback_info info) {          /* (ctx, the object readAccumulation returned) */
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtContext* ctx = get_ctx(env, argv[0]); if (!ctx) return NULL;
    PtAccumInfo ai; memset(&ai, 0, sizeof ai);
    ai.width = prop_u32(env, argv[1], "width", 0); ai.height = prop_u32(env, argv[1], "height", 0); ai.tile_rank = prop_u32(env, argv[1], "tileRank", 0);
    ai.tile_count = prop_u32(env, argv[1], "tileCount", 1); ai.compact = prop_u32(env, argv[1], "compact", 0); ai.samples = prop_u32(env, argv[1], "samples", 0);
    napi_value dv; bool has = false;
    if (napi_has_named_property(env, argv[1], "data", &has) != napi_ok || !has) { napi_throw_type_error(env, NULL, "restoreAccumulation: no `data`"); return NULL; }
    napi_get_named_property(env, argv[1], "data", &dv);
    void* d; size_t len; if (!get_typed(env, dv, napi_float32_array, &d, &len)) return NULL;
    ai.floats = len;
    PT_CALL(ctx, pt_set_accum(ctx, &ai, (const float*)d), "pt_set_accum");
    return NULL;
}
static napi_value fn_read_rgba8(napi_env env, napi_callback_info info) { return read_u8(env, info, 1); }       /* outputTex, PathTracer.js:163-172 */
static napi_value fn_read_tonemapped(napi_env env, napi_callback_info info) { return read_u8(env, info, 2); }  /* tonemapper.wgsl */


/* ---- several GPUs, one image per render(): pt_group_* (include/mi355pt.h) --------------------------------------- */

static void finalize_group(napi_env env, void* data, void* hint) {
    (void)env; (void)hint;
    PtGroup** box = (PtGroup**)data;
    if (*box) pt_group_destroy(*box);
    free(box);
}
static PtGroup* get_group(napi_env env, napi_value v) {
    void* p = NULL;
    if (napi_get_value_external(env, v, &p) != napi_ok || !p || !*(PtGroup**)p) { napi_throw_type_error(env, NULL, "expected a group handle"); return NULL; }
    return *(PtGroup**)p;
}
static napi_value throw_group(napi_env env, PtGroup* g, int rc, const char* where) {
    char msg[640];
    const char* e = pt_group_last_error(g);
    snprintf(msg, sizeof msg, "%s: libmi355pt error %d: %s", where, rc, e ? e : "");
    char code[16]; snprintf(code, sizeof code, "PT%d", rc);
    napi_throw_error(env, code, msg);
    return NULL;
}
#define PTG_CALL(g, call, where) do { int rc__ = (call); if (rc__ != 0) return throw_group(env, (g), rc__, (where)); } while (0)

/* Every query is registered under two names (init): `traceRays` takes a context as its first argument, `groupTraceRays` a group, and runs
 * on the group's member 0, which holds the whole scene.  The function's data pointer says which. */
static const struct QueryName { const char* name; Query q; int group; } QUERY_NAMES[] = {
    {"traceRays", Q_TRACE, 0}, {"groupTraceRays", Q_TRACE, 1}, {"closestPoints", Q_CLOSEST, 0}, {"groupClosestPoints", Q_CLOSEST, 1},
    {"sweepSpheres", Q_SWEEP, 0}, {"groupSweepSpheres", Q_SWEEP, 1}, {"nearestK", Q_NEAREST, 0}, {"groupNearestK", Q_NEAREST, 1},
    {"signedDistance", Q_SIGNED, 0}, {"groupSignedDistance", Q_SIGNED, 1}, {"contains", Q_CONTAINS, 0}, {"groupContains", Q_CONTAINS, 1},
    {"occlusion", Q_OCCLUSION, 0}, {"groupOcclusion", Q_OCCLUSION, 1}, {"countHits", Q_COUNT, 0}, {"groupCountHits", Q_COUNT, 1},
    {"radiusCount", Q_RADIUS_COUNT, 0}, {"groupRadiusCount", Q_RADIUS_COUNT, 1}, {"boxCount", Q_BOX_COUNT, 0}, {"groupBoxCount", Q_BOX_COUNT, 1},
    {"radiusSearch", Q_RADIUS, 0}, {"groupRadiusSearch", Q_RADIUS, 1}, {"boxSearch", Q_BOX, 0}, {"groupBoxSearch", Q_BOX, 1},
    {"listHits", Q_HITS, 0}, {"groupListHits", Q_HITS, 1}, {"hitSurfels", Q_SURFELS, 0}, {"groupHitSurfels", Q_SURFELS, 1},
};

/* (ctx | group, records, the query's own arguments): anyHit | flags | k, flags | options; hitSurfels: (ctx | group, rays, t, prim, u, v, rMax) */
static napi_value fn_query(napi_env env, napi_callback_info info) {
    napi_value argv[7]; size_t argc = 7; void* data = NULL;
    const napi_status got = napi_get_cb_info(env, info, &argc, argv, NULL, &data);
    const struct QueryName* name = (const struct QueryName*)data;
    const Query q = name->q;
    if (got != napi_ok || argc < (q == Q_SURFELS ? 7u : q == Q_NEAREST ? 4u : 3u)) { napi_throw_type_error(env, NULL, "wrong number of arguments"); return NULL; }
    PtContext* ctx = NULL;
    if (name->group) {
        PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
        int rc = pt_group_context(g, 0, &ctx); if (rc != 0) return throw_group(env, g, rc, "pt_group_context");
    } else if (!(ctx = get_ctx(env, argv[0]))) return NULL;
    const napi_value opt = argv[2];
    switch (q) {
    case Q_SURFELS: return hit_surfels_on(env, ctx, argv + 1);
    case Q_TRACE: { bool any = false; napi_get_value_bool(env, opt, &any); return run_query(env, ctx, q, argv[1], any ? PT_TRACE_ANY_HIT : 0u, 0, NULL); }
    case Q_NEAREST: return run_query(env, ctx, q, argv[1], get_u32(env, argv[3]), get_u32(env, argv[2]), NULL);
    case Q_OCCLUSION: {
        PtOcclusionParams p; memset(&p, 0, sizeof p);
        p.samples = prop_u32(env, opt, "samples", 16); p.seed = prop_u32(env, opt, "seed", 0); p.index_base = prop_u32(env, opt, "indexBase", 0);
        p.bias = (float)prop_f64(env, opt, "bias", 1e-4);
        p.flags = prop_u32(env, opt, "simple", 0) ? PT_OCCLUSION_SIMPLE_KERNEL : 0u;
        return run_query(env, ctx, q, argv[1], 0, 0, &p);
    }
    case Q_CONTAINS: case Q_SIGNED: {
        PtContainParams p; memset(&p, 0, sizeof p);
        p.samples = prop_u32(env, opt, "samples", 3); p.seed = prop_u32(env, opt, "seed", 0); p.index_base = prop_u32(env, opt, "indexBase", 0);
        p.flags = prop_u32(env, opt, "simple", 0) ? PT_CONTAIN_SIMPLE_KERNEL : 0u;
        return run_query(env, ctx, q, argv[1], 0, 0, &p);
    }
    case Q_COUNT: case Q_RADIUS_COUNT: case Q_BOX_COUNT: return run_count(env, ctx, q, argv[1], get_u32(env, opt));
    case Q_RADIUS: case Q_BOX: case Q_HITS: return run_list(env, ctx, q, argv[1], get_u32(env, opt));
    default: return run_query(env, ctx, q, argv[1], get_u32(env, opt), 0, NULL);           /* closestPoints, sweepSpheres */
    }
}

static napi_value fn_group_create(napi_env env, napi_callback_info info) {    /* (Int32Array devices | number of devices, transport) */
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    bool is_ta = false; napi_is_typedarray(env, argv[0], &is_ta);
    const int* devs = NULL; uint32_t n = 0;
    if (is_ta) { void* d; size_t len; if (!get_typed(env, argv[0], napi_int32_array, &d, &len)) return NULL; devs = (const int*)d; n = (uint32_t)len; }
    else n = get_u32(env, argv[0]);
    PtGroup** box = (PtGroup**)calloc(1, sizeof(PtGroup*));
    int rc = pt_group_create(devs, n, get_u32(env, argv[1]), box);
    if (rc != 0) { free(box); return throw_group(env, NULL, rc, "pt_group_create"); }
    napi_value ext;
    NAPI_OK(napi_create_external(env, box, finalize_group, NULL, &ext));
    return ext;
}
static napi_value fn_group_destroy(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    void* p = NULL;
    if (napi_get_value_external(env, argv[0], &p) == napi_ok && p) { PtGroup** box = (PtGroup**)p; if (*box) { pt_group_destroy(*box); *box = NULL; } }
    return NULL;
}
static napi_value fn_group_size(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    uint32_t n = 0; PTG_CALL(g, pt_group_size(g, &n), "pt_group_size");
    napi_value v; NAPI_OK(napi_create_uint32(env, n, &v)); return v;
}
static napi_value fn_group_set_triangles(napi_env env, napi_callback_info info) {
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    void* d; size_t len; if (!get_typed(env, argv[1], napi_float32_array, &d, &len)) return NULL;
    PTG_CALL(g, pt_group_set_triangles(g, (const float*)d, (uint32_t)(len / 9)), "pt_group_set_triangles");
    return NULL;
}
static napi_value fn_group_update_triangles(napi_env env, napi_callback_info info) {
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    void* d; size_t len; if (!get_typed(env, argv[1], napi_float32_array, &d, &len)) return NULL;
    if (len % 9) { napi_throw_type_error(env, NULL, "updateTriangles: 9 floats per triangle"); return NULL; }
    PTG_CALL(g, pt_group_update_triangles(g, (const float*)d, (uint32_t)(len / 9)), "pt_group_update_triangles");
    return NULL;
}
static napi_value fn_group_bvh_cost(napi_env env, napi_callback_info info) {      /* member 0: every member holds the same tree */
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    PtContext* ctx = NULL; PTG_CALL(g, pt_group_context(g, 0, &ctx), "pt_group_context");
    double cost = 0; PT_CALL(ctx, pt_bvh_cost(ctx, &cost), "pt_bvh_cost");
    napi_value v; NAPI_OK(napi_create_double(env, cost, &v)); return v;
}
static napi_value fn_group_build_bvh(napi_env env, napi_callback_info info) {
    napi_value argv[2]; uint32_t accel; if (!get_accel(env, info, argv, &accel)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    if (accel == PT_ACCEL_REFERENCE) PTG_CALL(g, pt_group_build_bvh(g), "pt_group_build_bvh");
    else PTG_CALL(g, pt_group_build_bvh_accel(g, accel), "pt_group_build_bvh_accel");
    return NULL;
}
static napi_value group_set_bvh(napi_env env, napi_callback_info info, int four) {
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    void* d; size_t len; if (!get_typed(env, argv[1], napi_uint32_array, &d, &len)) return NULL;
    if (four) PTG_CALL(g, pt_group_set_bvh4(g, (const uint32_t*)d, len), "pt_group_set_bvh4");
    else PTG_CALL(g, pt_group_set_bvh2(g, (const uint32_t*)d, len), "pt_group_set_bvh2");
    return NULL;
}
static napi_value fn_group_set_bvh4(napi_env env, napi_callback_info info) { return group_set_bvh(env, info, 1); }
static napi_value fn_group_set_bvh2(napi_env env, napi_callback_info info) { return group_set_bvh(env, info, 0); }
static napi_value fn_group_read_bvh2(napi_env env, napi_callback_info info) {  /* readBVH2 of rank 0 (every member holds the same buffer) */
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    PtContext* c0 = NULL; PTG_CALL(g, pt_group_context(g, 0, &c0), "pt_group_context");
    double bytes = get_f64(env, argv[1]);
    size_t size = bytes < 4 ? 4 : (size_t)bytes;
    void* out; napi_value ta = make_typed(env, napi_uint32_array, 4, size / 4, &out); if (!ta) return NULL;
    PT_CALL(c0, pt_read_bvh2(c0, (uint32_t*)out, (size / 4) * 4), "pt_read_bvh2");
    return ta;
}
static napi_value fn_group_set_batch(napi_env env, napi_callback_info info) {
    napi_value argv[2]; if (!get_args(env, info, 2, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    PTG_CALL(g, pt_group_set_batch(g, get_u32(env, argv[1])), "pt_group_set_batch");
    return NULL;
}
static napi_value fn_group_render(napi_env env, napi_callback_info info) {
    napi_value argv[3]; if (!get_args(env, info, 3, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    PtRenderParams p; if (!params_from_ubo(env, argv[1], argv[2], &p)) return NULL;
    PTG_CALL(g, pt_group_render(g, &p), "pt_group_render");
    return NULL;
}
static napi_value fn_group_flush(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    PTG_CALL(g, pt_group_flush(g), "pt_group_flush");
    return NULL;
}
static napi_value fn_group_sync(napi_env env, napi_callback_info info) {
    napi_value argv[1]; if (!get_args(env, info, 1, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    PTG_CALL(g, pt_group_synchronize(g), "pt_group_synchronize");
    return NULL;
}
static napi_value fn_group_read_radiance(napi_env env, napi_callback_info info) {
    napi_value argv[3]; if (!get_args(env, info, 3, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    size_t n = (size_t)get_u32(env, argv[1]) * get_u32(env, argv[2]) * 4;
    void* out; napi_value ta = make_typed(env, napi_float32_array, 4, n, &out); if (!ta) return NULL;
    PTG_CALL(g, pt_group_read_radiance(g, (float*)out, n), "pt_group_read_radiance");
    return ta;
}
static napi_value group_read_u8(napi_env env, napi_callback_info info, int which) {
    napi_value argv[4]; if (!get_args(env, info, which == 2 ? 4 : 3, argv)) return NULL;
    PtGroup* g = get_group(env, argv[0]); if (!g) return NULL;
    size_t n = (size_t)get_u32(env, argv[1]) * get_u32(env, argv[2]) * 4;
    void* out; napi_value ta = make_typed(env, napi_uint8_array, 1, n, &out); if (!ta) return NULL;
    if (which == 1) PTG_CALL(g, pt_group_read_rgba8(g, (uint8_t*)out, n), "pt_group_read_rgba8");
    else { bool q = true; napi_get_value_bool(env, argv[3], &q); PTG_CALL(g, pt_group_read_tonemapped(g, q ? 1 : 0, (uint8_t*)out, n), "pt_group_read_tonemapped"); }
    return ta;
}
static napi_value fn_group_read_rgba8(napi_env env, napi_callback_info info) { return group_read_u8(env, info, 1); }
static napi_value fn_group_read_tonemapped(napi_env env, napi_callback_info info) { return group_read_u8(env, info, 2); }

static napi_value init(napi_env env, napi_value exports) {
    static const struct { const char* name; napi_callback fn; } fns[] = {
        {"create", fn_create}, {"destroy", fn_destroy}, {"version", fn_version},
        {"computeBVH2Sizing", fn_bvh2_sizing}, {"computeBVH4Sizing", fn_bvh4_sizing},
        {"mortonSort", fn_morton_sort}, {"collapse", fn_collapse}, {"bvh4Wide", fn_bvh4_wide},
        {"writeU32File", fn_write_u32}, {"readU32File", fn_read_u32}, {"proceduralScene", fn_procedural},
        {"setTriangles", fn_set_triangles}, {"updateTriangles", fn_update_triangles}, {"bvhCost", fn_bvh_cost}, {"buildBVH", fn_build_bvh}, {"readBVH2", fn_read_bvh2}, {"readBVH4", fn_read_bvh4},
        {"setBVH4", fn_set_bvh4}, {"setBVH2", fn_set_bvh2}, {"setSpheres", fn_set_spheres}, {"sceneInfo", fn_scene_info},
        {"render", fn_render}, {"setBatch", fn_set_batch}, {"flush", fn_flush}, {"lastRenderMs", fn_last_ms}, {"synchronize", fn_sync}, {"getStats", fn_stats},
        {"readRadiance", fn_read_radiance}, {"readRGBA8", fn_read_rgba8}, {"readTonemapped", fn_read_tonemapped},
        {"readAccumulation", fn_read_accum}, {"restoreAccumulation", fn_set_accum},
        {"cameraRay", fn_camera_ray},
        {"groupCreate", fn_group_create}, {"groupDestroy", fn_group_destroy}, {"groupSize", fn_group_size},
        {"groupSetTriangles", fn_group_set_triangles}, {"groupUpdateTriangles", fn_group_update_triangles}, {"groupBvhCost", fn_group_bvh_cost}, {"groupBuildBVH", fn_group_build_bvh}, {"groupSetBVH4", fn_group_set_bvh4}, {"groupSetBVH2", fn_group_set_bvh2},
        {"groupReadBVH2", fn_group_read_bvh2}, {"groupSetBatch", fn_group_set_batch}, {"groupRender", fn_group_render}, {"groupFlush", fn_group_flush},
        {"groupSynchronize", fn_group_sync}, {"groupReadRadiance", fn_group_read_radiance}, {"groupReadRGBA8", fn_group_read_rgba8}, {"groupReadTonemapped", fn_group_read_tonemapped},
    };
    for (size_t i = 0; i < sizeof fns / sizeof fns[0]; ++i) {
        napi_value f;
        if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok) return NULL;
        if (napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) return NULL;
    }
    for (size_t i = 0; i < sizeof QUERY_NAMES / sizeof QUERY_NAMES[0]; ++i) {
        napi_value f;
        if (napi_create_function(env, QUERY_NAMES[i].name, NAPI_AUTO_LENGTH, fn_query, (void*)&QUERY_NAMES[i], &f) != napi_ok) return NULL;
        if (napi_set_named_property(env, exports, QUERY_NAMES[i].name, f) != napi_ok) return NULL;
    }
    return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
