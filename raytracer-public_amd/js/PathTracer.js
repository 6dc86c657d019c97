// PathTracer.js -- Node host class with the API of the reference's src/libs/PathTracer.js,
// driving libmi355pt (HIP, MI355X) through the N-API addon instead of WebGPU.
// Node-12-safe CommonJS (no ??, ?., top-level await).  Method names, arity, return shapes and
// Promise-ness follow the reference (cited per method); the extension options (mode, spp,
// maxBounces, seed, accumulate) default to the reference's behaviour: one primary ray per pixel.
"use strict";
const path = require("path");

// overlapped frame slots need more than ROCm's default 4 hardware queues (read at HIP runtime init)
if (process.env.GPU_MAX_HW_QUEUES === undefined) process.env.GPU_MAX_HW_QUEUES = "12";
let addon = null;
function native() {
  if (!addon) addon = require(path.join(__dirname, "..", "napi", "mi355pt.node"));   // throws loudly when not built
  return addon;
}

const MODE_REFERENCE_PACKET = 0, MODE_REFERENCE = 1, MODE_PATH = 2;
const FLAG_SIMPLE_KERNEL = 2, FLAG_BRUTE_FORCE = 4, HITS_SORTED = 8;

class PathTracer {
  // reference: constructor(canvas), PathTracer.js:60-95 -- uses only canvas.width / canvas.height
  constructor(canvas, options) {
    this.canvas = canvas;
    this.device = null;                         // the reference's GPUDevice slot: here the native context handle
    this.cameraPosition = [0.0, 0.0, 3.5];      // :67
    this.cameraQuaternion = [0.0, 0.0, 0.0, 1.0];
    this.buffers = {};                          // kept for shape compatibility; device buffers live in the context
    this.frameCount = 0;
    this.trianglesData = new Float32Array([     // default tetrahedron, :79-84
      1, 1, 1, -1, -1, 1, -1, 1, -1,
      1, 1, 1, -1, 1, -1, 1, -1, -1,
      1, 1, 1, 1, -1, -1, -1, -1, 1,
      -1, -1, 1, 1, -1, -1, -1, 1, -1,
    ]);
    const o = options || {};
    this.options = {
      device: o.device === undefined ? -1 : o.device,
      mode: o.mode === undefined ? MODE_REFERENCE : o.mode,
      spp: o.spp || 1, maxBounces: o.maxBounces || 0, seed: o.seed === undefined ? 1 : o.seed,
      accumulate: !!o.accumulate, stats: !!o.stats, bruteForce: !!o.bruteForce,
      // tree quality of buildBVH (include/mi355pt.h PT_ACCEL_*): 0 = the reference's tree; 1 = area-guided collapse; 2 = PLOC + area-guided collapse
      accel: o.accel || 0,
    };
    // Several GPUs, still one image per render(): `gpus: N` (devices 0..N-1) or `devices: [..]` makes this PathTracer drive a
    // group of contexts -- pixel tiles interleaved over the GPUs, gathered on the first one over RCCL (pt_group_*, include/mi355pt.h).
    // `transport: "copy"` swaps the collective for peer copies (members may then share a GPU: rehearsals on a one-GPU machine).
    this.groupDevices = o.devices ? Int32Array.from(o.devices) : (o.gpus && o.gpus > 1 ? Int32Array.from({ length: o.gpus }, (_, i) => i) : null);
    this.groupTransport = o.transport === "copy" ? 1 : 0;
    this.group = null;
    this._hasBVH = false;
  }

  // :97-102 (adapter/device/shaders/buffers/pipelines) -> one native context per GPU
  async initialize() {
    if (this.groupDevices) { this.group = native().groupCreate(this.groupDevices, this.groupTransport); this.device = this.group; }
    else this.device = native().create(this.options.device);
  }

  computeBVH2Sizing(numTris) { return native().computeBVH2Sizing(numTris); }      // :227
  computeBVH4Sizing(numNodes4) { return native().computeBVH4Sizing(numNodes4); }  // :234

  buildMortonAndSort(trianglesData) {            // :427 -> { mortonSorted, triIndexSorted }
    return native().mortonSort(trianglesData);
  }

  async readBVH2(bytes) {                        // :485 -> fresh Uint32Array copy
    return this.group ? native().groupReadBVH2(this.group, bytes) : native().readBVH2(this.device, bytes);
  }

  collapseLBVH2ToBVH4(bvh2U32, numTris) {        // :506 -> { bvh4U32, numNodes4 }
    return native().collapse(bvh2U32, numTris);
  }

  async buildBVH(trianglesData) {                // :671-749
    if (!this.device) return;                    // `if (!device) return`, :673
    const t0 = Date.now();
    if (this.group) { native().groupSetTriangles(this.group, trianglesData); native().groupBuildBVH(this.group, this.options.accel); }
    else { native().setTriangles(this.device, trianglesData); native().buildBVH(this.device, this.options.accel); }
    this._hasBVH = true;
    console.log("BVH Build Time:", Date.now() - t0, "ms");   // :745-748 prints timings
  }

  async setScene(scene) {                        // :751-754
    this.trianglesData = scene.getTrianglesFloat32();
    await this.buildBVH(this.trianglesData);
  }

  // config C1 extension: brute-force scene = uploaded triangles + analytic spheres, no BVH
  setBruteForceScene(trianglesData, spheresXYZR) {
    if (this.group) throw new Error("brute-force scenes (config C1) render on one GPU");
    this.trianglesData = trianglesData;
    native().setTriangles(this.device, trianglesData);
    native().setSpheres(this.device, spheresXYZR);
    this.options.bruteForce = true; this._hasBVH = true;
  }

  // setScene for a scene whose BVH2 was built before (data/BVH2.bin, what src/main.js:27-46 dumps): upload the triangles, install the
  // BVH2 through the reference's own route (collapseLBVH2ToBVH4, then the BVH4 the renderer traverses) -- no rebuild
  async setSceneWithBVH2(scene, bvh2U32) {
    if (!this.device) return;
    this.trianglesData = scene.getTrianglesFloat32();
    if (this.group) native().groupSetTriangles(this.group, this.trianglesData); else native().setTriangles(this.device, this.trianglesData);
    this.setBVH2(bvh2U32);
  }

  // ---- animated geometry: an extension beyond the reference (include/mi355pt.h pt_update_triangles, DESIGN.md section 14) ----
  // New vertices for the same triangles (a Float32Array of the same length): the tree keeps its topology and is refitted in place on
  // the GPU -- no rebuild.  Frames rendered before show the old geometry, frames after the new.
  updateTriangles(trianglesData) {
    if (!this.device) return;
    if (this.group) native().groupUpdateTriangles(this.group, trianglesData); else native().updateTriangles(this.device, trianglesData);
    this.trianglesData = trianglesData;
  }
  // Quality of the current tree: sum over internal nodes of halfArea(node) / halfArea(root).  It grows as a refitted tree degrades:
  // rebuild (buildBVH) when it exceeds the cost at build by a factor of your choice.  On a group: member 0 (every member holds the same tree).
  bvhCost() { return this.group ? native().groupBvhCost(this.group) : native().bvhCost(this.device); }

  // install a prebuilt BVH (data/BVH2.bin or data/BVH4_wide.bin) instead of rebuilding
  setBVH2(bvh2U32) { if (this.group) native().groupSetBVH2(this.group, bvh2U32); else native().setBVH2(this.device, bvh2U32); this._hasBVH = true; }
  setBVH4(bvh4U32) { if (this.group) native().groupSetBVH4(this.group, bvh4U32); else native().setBVH4(this.device, bvh4U32); this._hasBVH = true; }

  _ubo() {
    const numTriangles = (this.trianglesData.length / 9) | 0;
    const fov = (70.0 * Math.PI) / 180;          // :761
    const focal = 1.0 / Math.tan(0.5 * fov);
    return new Float32Array([                    // :764-787, same 16 floats in the same order
      this.canvas.width, this.canvas.height, focal, this.canvas.width / this.canvas.height,
      this.cameraPosition[0], this.cameraPosition[1], this.cameraPosition[2], numTriangles,
      this.cameraQuaternion[0], this.cameraQuaternion[1], this.cameraQuaternion[2], this.cameraQuaternion[3],
      this.frameCount, 0, 0, 0,
    ]);
  }

  async render() {                               // :756-822
    if (!this._hasBVH) return;                   // `if (!this.buffers.BVH) return`, :757
    const UBO = this._ubo();
    if (this.group) native().groupRender(this.group, UBO, this.options);   // every GPU traces its tiles; the gather follows on their streams
    else native().render(this.device, UBO, this.options);                  // asynchronous on the GPU, like queue.submit (:821)
  }

  // The batched queries below run on this context or, on a group, on member 0, which holds the whole scene: the addon registers each
  // under two names, `traceRays(context, ...)` and `groupTraceRays(group, ...)`.
  _query(name, ...args) {
    return this.group ? native()["group" + name[0].toUpperCase() + name.slice(1)](this.group, ...args) : native()[name](this.device, ...args);
  }
  // options -> the flag word of a query (include/mi355pt.h PT_*_SIMPLE_KERNEL, PT_*_BRUTE_FORCE: the same bits in every query)
  _flags(options) {
    const o = options || {};
    return (o.simple ? FLAG_SIMPLE_KERNEL : 0) | (o.bruteForce ? FLAG_BRUTE_FORCE : 0);
  }

  // ---- batched ray queries: an extension beyond the reference (include/mi355pt.h pt_trace_rays, DESIGN.md section 13) ----
  // rays: Float32Array, 8 floats per ray (origin xyz, tMax, direction xyz, 0).  Resolves to { t, prim, u, v } (Float32Array / Uint32Array):
  // the closest hit (anyHit: the first hit in traversal order) over the current tree; a miss has t = Infinity, prim = 0xFFFFFFFF, u = v = 0.
  // Triangles only (the spheres of a brute-force scene take no part).  On a group: member 0, which holds the whole scene.
  async traceRays(rays, options) {
    return this._query("traceRays", rays, !!(options && options.anyHit));
  }
  // What is under pixel (x, y) of the current camera (setCameraPosition / setCameraQuaternion)?  The ray render() traces through the
  // pixel's centre in mode 1 (row 0 at the bottom of the image, as in the radiance); resolves to { hit, t, prim, point }, point = origin + t * direction.
  async pick(x, y) {
    const ray = native().cameraRay(this._ubo(), x, y);
    const r = await this.traceRays(ray);
    const hit = r.prim[0] !== 0xFFFFFFFF, t = r.t[0];
    const point = hit ? [0, 1, 2].map((k) => Math.fround(ray[k] + Math.fround(t * ray[4 + k]))) : null;
    return { hit: hit, t: t, prim: r.prim[0], point: point };
  }

  // ---- batched closest-point queries: an extension beyond the reference (include/mi355pt.h pt_closest_points, DESIGN.md section 15) ----
  // points: Float32Array, 4 floats per point (x, y, z, rMax; rMax = Infinity for no limit).  Resolves to { dist, prim, u, v } (Float32Array /
  // Uint32Array): the nearest triangle within rMax over the current tree and the closest point on it as v0 + u (v1 - v0) + v (v2 - v0);
  // nothing within rMax: dist = Infinity, prim = 0xFFFFFFFF, u = v = 0.  options.bruteForce: every triangle, no tree; options.simple: the
  // one-point-per-thread kernel.  Triangles only.  On a group: member 0, which holds the whole scene.
  async closestPoints(points, options) {
    return this._query("closestPoints", points, this._flags(options));
  }
  // The nearest triangle to (x, y, z): resolves to { found, dist, prim, u, v, point }.  point = v0 + u (v1 - v0) + v (v2 - v0) from
  // `trianglesData`, the Float32Array the scene was built from (9 floats per triangle), when the caller passes it; null without it or
  // when nothing is found (this object does not keep a copy of what every route uploaded).
  async nearest(x, y, z, trianglesData) {
    const r = await this.closestPoints(Float32Array.of(x, y, z, Infinity));
    const found = r.prim[0] !== 0xFFFFFFFF;
    let point = null;
    if (found && trianglesData) {
      const t = trianglesData, o = r.prim[0] * 9, u = r.u[0], v = r.v[0];
      point = [0, 1, 2].map((k) => t[o + k] + u * Math.fround(t[o + 3 + k] - t[o + k]) + v * Math.fround(t[o + 6 + k] - t[o + k]));
    }
    return { found: found, dist: r.dist[0], prim: r.prim[0], u: r.u[0], v: r.v[0], point: point };
  }

  // ---- crossing counts, containment, signed distance: an extension beyond the reference (include/mi355pt.h pt_count_hits, DESIGN.md section 17) ----
  // rays: Float32Array, 8 floats per ray (origin xyz, tMax, direction xyz, 0).  Resolves to a Uint32Array: how many triangles each ray
  // crosses before tMax -- every one, not only the first.  options.bruteForce: every triangle, no tree; options.simple: the
  // one-ray-per-thread kernel.  Triangles only.  On a group: member 0, which holds the whole scene.
  async countHits(rays, options) {
    return this._query("countHits", rays, this._flags(options));
  }
  // points: Float32Array, 4 floats per point (x, y, z, ignored).  options: { samples (3; odd, 1..255), seed (0), indexBase (0), simple }.
  // Resolves to { inside, odd, samples } (Uint32Array): crossing parity by majority vote over `samples` rays per point -- on a closed mesh
  // the point-in-solid test; on an open or self-intersecting mesh whatever the parity is, odd / samples telling how much the rays disagreed.
  async contains(points, options) {
    return this._query("contains", points, options || {});
  }
  // ---- sphere-cast queries: an extension beyond the reference (include/mi355pt.h pt_sweep_spheres, DESIGN.md section 22) ----
  // sweeps: Float32Array, 8 floats per sweep (origin xyz, tMax, direction xyz, radius).  Resolves to { t, prim, u, v } (Float32Array /
  // Uint32Array): the first contact of the moving sphere with the mesh over the current tree, t in units of the direction (0 for a sphere
  // that overlaps at the start) and the contact point as v0 + u (v1 - v0) + v (v2 - v0); a miss has t = Infinity, prim = 0xFFFFFFFF,
  // u = v = 0.  options.bruteForce: every triangle, no tree; options.simple: the one-sweep-per-thread kernel.  Triangles only.  On a
  // group: member 0, which holds the whole scene.
  async sweepSpheres(sweeps, options) {
    return this._query("sweepSpheres", sweeps, this._flags(options));
  }
  // One sphere of radius r from (ox, oy, oz) along (dx, dy, dz): resolves to { hit, t, prim, u, v, center }, center = origin + t * direction.
  async sweep(ox, oy, oz, dx, dy, dz, r) {
    const q = await this.sweepSpheres(Float32Array.of(ox, oy, oz, Infinity, dx, dy, dz, r));
    const hit = q.prim[0] !== 0xFFFFFFFF, t = q.t[0];
    return { hit: hit, t: t, prim: q.prim[0], u: q.u[0], v: q.v[0], center: hit ? [ox + t * dx, oy + t * dy, oz + t * dz] : null };
  }

  // closestPoints with the sign of contains: { dist, prim, u, v }, dist negative inside (-Infinity: inside, and nothing within rMax)
  async signedDistance(points, options) {
    return this._query("signedDistance", points, options || {});
  }
  // Is (x, y, z) inside the mesh?  Resolves to { inside, odd, samples }.
  async inside(x, y, z, options) {
    const r = await this.contains(Float32Array.of(x, y, z, Infinity), options);
    return { inside: r.inside[0] !== 0, odd: r.odd[0], samples: r.samples[0] };
  }

  // ---- radius queries: an extension beyond the reference (include/mi355pt.h pt_radius_search, DESIGN.md section 18) ----
  // points: Float32Array, 4 floats per point (x, y, z, rMax); a number rMax replaces the fourth float of every point (the caller's array is
  // not written).  radiusSearch resolves to { offsets, dist, prim, u, v }: the triangles within rMax of point i are entries
  // offsets[i] .. offsets[i + 1] - 1 (offsets: Float64Array of n + 1 exact integers), each with its distance and its contact point
  // v0 + u (v1 - v0) + v (v2 - v0), in the order the walk meets them (triangle order with options.bruteForce).  radiusCount resolves to a
  // Uint32Array of the list lengths alone.  A point with a NaN or rMax <= 0 has an empty list.  options.bruteForce: every triangle, no
  // tree; options.simple: the one-point-per-thread kernels.  A radius that covers much of a deep tree can lose triangles at the
  // 64-entry stack cap (the header says when); bruteForce never does.  Triangles only.  On a group: member 0, which holds the whole scene.
  _radiusPoints(points, rMax) {
    if (rMax === undefined || rMax === null) return points;
    const p = Float32Array.from(points);
    for (let i = 3; i < p.length; i += 4) p[i] = rMax;
    return p;
  }
  async radiusSearch(points, rMax, options) {
    return this._query("radiusSearch", this._radiusPoints(points, rMax), this._flags(options));
  }
  async radiusCount(points, rMax, options) {
    return this._query("radiusCount", this._radiusPoints(points, rMax), this._flags(options));
  }
  // The triangles within r of (x, y, z): resolves to { count, dist, prim, u, v }.
  async within(x, y, z, r, options) {
    const s = await this.radiusSearch(Float32Array.of(x, y, z, r), undefined, options);
    return { count: s.prim.length, dist: s.dist, prim: s.prim, u: s.u, v: s.v };
  }

  // ---- box-overlap queries: an extension beyond the reference (include/mi355pt.h pt_box_search, DESIGN.md section 21) ----
  // boxes: Float32Array, 8 floats per box (lo xyz, 0, hi xyz, 0).  boxSearch resolves to { offsets, prim, vertsInside }: the triangles that
  // overlap box i (touching counts) are entries offsets[i] .. offsets[i + 1] - 1 (offsets: Float64Array of n + 1 exact integers), in the
  // order the walk meets them (triangle order with options.bruteForce); bit k of vertsInside says that vertex k lies in the closed box
  // (7: the whole triangle is inside).  boxCount resolves to a Uint32Array of the list lengths alone.  A box with a NaN, an infinity or
  // lo > hi on an axis has an empty list.  options.bruteForce: every triangle, no tree; options.simple: the one-box-per-thread kernels.
  // A box that covers much of a deep tree can lose triangles at the 64-entry stack cap (the header says when); bruteForce never does.
  // Triangles only.  On a group: member 0, which holds the whole scene.
  async boxSearch(boxes, options) {
    return this._query("boxSearch", boxes, this._flags(options));
  }
  async boxCount(boxes, options) {
    return this._query("boxCount", boxes, this._flags(options));
  }
  // The triangles that overlap the box lo = [x, y, z] .. hi = [x, y, z]: resolves to { count, prim, vertsInside }.
  async overlapping(lo, hi, options) {
    const s = await this.boxSearch(Float32Array.of(lo[0], lo[1], lo[2], 0, hi[0], hi[1], hi[2], 0), options);
    return { count: s.prim.length, prim: s.prim, vertsInside: s.vertsInside };
  }

  // ---- hit lists: an extension beyond the reference (include/mi355pt.h pt_list_hits, DESIGN.md section 20) ----
  // rays: Float32Array, 8 floats per ray (origin xyz, tMax, direction xyz, 0).  Resolves to { offsets, t, prim, u, v }: the triangles ray i
  // crosses before tMax -- the ones countHits counts -- are entries offsets[i] .. offsets[i + 1] - 1 (offsets: Float64Array of n + 1 exact
  // integers), each with its distance t and its barycentrics u, v, in the order the walk meets them (triangle order with
  // options.bruteForce), or with options.sort in ascending order of t (equal t: ascending prim).  A ray with a NaN or tMax <= 0 has an
  // empty list.  options.simple: the one-ray-per-thread kernels.  A ray through a very deep tree can lose crossings at the 64-entry stack
  // cap (the header says when); bruteForce never does.  Triangles only.  On a group: member 0, which holds the whole scene.
  async listHits(rays, options) {
    return this._query("listHits", rays, this._flags(options) | (options && options.sort ? HITS_SORTED : 0));
  }
  // Every crossing of the ray from (ox, oy, oz) along (dx, dy, dz), nearest first: resolves to { count, t, prim, u, v }.  options.tMax
  // (default: no limit), options.simple, options.bruteForce.
  async hitsAlong(ox, oy, oz, dx, dy, dz, options) {
    const o = options || {}, tMax = o.tMax === undefined ? Infinity : o.tMax;
    const s = await this.listHits(Float32Array.of(ox, oy, oz, tMax, dx, dy, dz, 0), Object.assign({}, o, { sort: true }));
    return { count: s.prim.length, t: s.t, prim: s.prim, u: s.u, v: s.v };
  }
  // A thickness frame of the current camera: camera rays -> listHits(sort) -> t[1] - t[0].  Resolves to a Float32Array of width * height
  // distances between the first and the second crossing, row-major like the radiance; 0 where the camera ray has fewer than two crossings.
  async thickness(options) {
    const w = this.canvas.width, h = this.canvas.height, ubo = this._ubo();
    const rays = new Float32Array(w * h * 8);
    for (let y = 0; y < h; y++) for (let x = 0; x < w; x++) rays.set(native().cameraRay(ubo, x, y), (y * w + x) * 8);
    const s = await this.listHits(rays, Object.assign({}, options || {}, { sort: true }));
    const out = new Float32Array(w * h);
    for (let i = 0; i < w * h; i++) { const a = s.offsets[i]; if (s.offsets[i + 1] - a >= 2) out[i] = Math.fround(s.t[a + 1] - s.t[a]); }
    return out;
  }

  // ---- k-nearest queries: an extension beyond the reference (include/mi355pt.h pt_nearest_k, DESIGN.md section 19) ----
  // points: Float32Array, 4 floats per point (x, y, z, rMax; rMax = Infinity for no limit); k: 1 .. 64.  Resolves to { k, dist, prim, u, v }
  // (Float32Array / Uint32Array of n * k): row i at [i * k, i * k + k) holds the at most k triangles within rMax in ascending order of
  // distance, each with its contact point v0 + u (v1 - v0) + v (v2 - v0), padded with dist = Infinity, prim = 0xFFFFFFFF, u = v = 0.
  // options.rMax: a number that replaces the fourth float of every point (the caller's array is not written); options.bruteForce: every
  // triangle, no tree; options.simple: the one-point-per-thread kernel.  Triangles only.  On a group: member 0, which holds the whole scene.
  async nearestK(points, k, options) {
    return this._query("nearestK", this._radiusPoints(points, options && options.rMax), k, this._flags(options));
  }
  // The k triangles nearest to (x, y, z): resolves to { count, dist, prim, u, v } without the padding, nearest first.
  async kNearest(x, y, z, k, options) {
    const r = await this.nearestK(Float32Array.of(x, y, z, Infinity), k, options);
    let count = 0;
    while (count < r.prim.length && r.prim[count] !== 0xFFFFFFFF) ++count;
    return { count: count, dist: r.dist.slice(0, count), prim: r.prim.slice(0, count), u: r.u.slice(0, count), v: r.v.slice(0, count) };
  }

  // ---- batched ambient-occlusion queries: an extension beyond the reference (include/mi355pt.h pt_occlusion, DESIGN.md section 16) ----
  // surfels: Float32Array, 8 floats per surfel (point xyz, rMax, unit normal xyz, 0).  options: { samples (16), seed (0), bias (1e-4),
  // indexBase (0), simple }.  Resolves to { visibility: Float32Array, unoccluded: Uint32Array, samples: Uint32Array }: of `samples`
  // cosine-distributed rays around the normal, how many reach nothing within rMax; all zero for a surfel that is not traced (a NaN, rMax <= 0).
  // On a group: member 0, which holds the whole scene.
  async occlusion(surfels, options) {
    return this._query("occlusion", surfels, options || {});
  }
  // rays + what traceRays resolved to for them -> Float32Array of surfels (8 floats each): the hit point, rMax, the triangle's normal turned
  // against the ray; a miss gives a surfel that occlusion() does not trace.
  async hitSurfels(rays, hits, rMax) {
    return this._query("hitSurfels", rays, hits.t, hits.prim, hits.u, hits.v, rMax === undefined ? Infinity : rMax);
  }
  // An ambient-occlusion frame of the current camera: camera rays -> traceRays -> hitSurfels -> occlusion.  Resolves to a Float32Array of
  // width * height visibilities, row-major like the radiance; 0 where the camera ray misses.
  async ambientOcclusion(samples, rMax, options) {
    const w = this.canvas.width, h = this.canvas.height, ubo = this._ubo();
    const rays = new Float32Array(w * h * 8);
    for (let y = 0; y < h; y++) for (let x = 0; x < w; x++) rays.set(native().cameraRay(ubo, x, y), (y * w + x) * 8);
    const surfels = await this.hitSurfels(rays, await this.traceRays(rays), rMax);
    return (await this.occlusion(surfels, Object.assign({ samples: samples }, options || {}))).visibility;
  }

  setCameraPosition(x, y, z) { this.cameraPosition = [x, y, z]; }           // :824
  setCameraQuaternion(x, y, z, w) { this.cameraQuaternion = [x, y, z, w]; } // :828
  setFrameCount(frameCount) { this.frameCount = frameCount; }               // :832

  // queue `n` (1..256) consecutive render() calls into one persistent GPU launch; read-backs flush a partial batch
  setBatch(n) { if (this.group) native().groupSetBatch(this.group, n); else native().setBatch(this.device, n); }
  flush() { if (this.group) native().groupFlush(this.group); else native().flush(this.device); }

  // ---- results (the reference presents to a canvas; a Node host reads them back) ----
  readRadiance() { const w = this.canvas.width, h = this.canvas.height; return this.group ? native().groupReadRadiance(this.group, w, h) : native().readRadiance(this.device, w, h); }
  readRGBA8() { const w = this.canvas.width, h = this.canvas.height; return this.group ? native().groupReadRGBA8(this.group, w, h) : native().readRGBA8(this.device, w, h); }      // outputTex equivalent, :163-172
  readTonemapped(fromRGBA8) {                                                                                                      // tonemapper.wgsl
    const w = this.canvas.width, h = this.canvas.height, q = fromRGBA8 !== false;
    return this.group ? native().groupReadTonemapped(this.group, w, h, q) : native().readTonemapped(this.device, w, h, q);
  }
  // Checkpoint / resume of a progressive accumulation (options.accumulate): the raw running sums (f32 RGB sums + sample count per pixel).
  // readAccumulation() -> { width, height, tileRank, tileCount, compact, samples, data: Float32Array }; restoreAccumulation(that object) on a
  // PathTracer with the same scene continues bit for bit with the next render() (frame counts go on where the dumped run stopped).
  readAccumulation() { if (this.group) throw new Error("readAccumulation: per-context state; on a group use the member contexts"); return native().readAccumulation(this.device); }
  restoreAccumulation(dump) { if (this.group) throw new Error("restoreAccumulation: per-context state; on a group use the member contexts"); native().restoreAccumulation(this.device, dump); }
  lastRenderMs() { if (this.group) throw new Error("lastRenderMs: per-context timing; not available on a group"); return native().lastRenderMs(this.device); }
  getStats() { if (this.group) throw new Error("getStats: per-context counters; not available on a group"); return native().getStats(this.device); }
  synchronize() { if (this.group) native().groupSynchronize(this.group); else native().synchronize(this.device); }
  gpuCount() { return this.group ? native().groupSize(this.group) : 1; }
  destroy() {
    if (this.group) { native().groupDestroy(this.group); this.group = null; this.device = null; }
    else if (this.device) { native().destroy(this.device); this.device = null; }
  }
}

// The drivers' `--animate AMP` displacement (tools/README.md): every vertex of `base` moves in y by AMP times a triangle wave of its own x,
//   u = (2 x + 0.25) + 0.125 frame;   y += AMP (4 |u - floor(u) - 0.5| - 1),
// every step rounded to f32 (Math.fround), in that order -- add, multiply, floor and abs only, so numpy float32 gives the same bits.
function animateWave(base, amp, frame, out) {
  const f = Math.fround, a = f(amp), phase = f(f(0.125) * f(frame));
  for (let i = 0; i < base.length; i += 3) {
    const u = f(f(f(2 * base[i]) + 0.25) + phase);
    const tri = f(f(4 * Math.abs(f(f(u - Math.floor(u)) - 0.5))) - 1);
    out[i] = base[i]; out[i + 1] = f(base[i + 1] + f(a * tri)); out[i + 2] = base[i + 2];
  }
  return out;
}

module.exports = { PathTracer, animateWave, MODE_REFERENCE_PACKET, MODE_REFERENCE, MODE_PATH, native };
