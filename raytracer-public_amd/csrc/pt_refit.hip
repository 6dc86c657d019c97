// pt_refit.hip -- animated geometry: new vertices, the same tree.  pt_update_triangles keeps the topology of the context's
// BVH4 (whatever installed it) and recomputes every box from the new triangles, in place, with the arithmetic of the build:
//
//   BVH4 leaf       min / max of the three vertices, rounded to f16 and stepped one f16 outwards (BVHBuilder.wgsl:63-102)
//   BVH4 internal   js_min_f / js_max_f over the exactly decoded child boxes in slot order, packed with half_trunc
//                   (PathTracer.js:640-661, what collapse_up_kernel computes)
//   wide arena      the 64-byte record of every internal node, as wide_nodes_kernel writes it from the refitted BVH4
//   BVH2            leaves by the leaf rule, internal nodes by the reference's propagateUp (BVHBuilder.wgsl:242-275)
//
// One launch refits the BVH4: a thread per node starts at every leaf and climbs; the thread that completes a node's arrival
// count unions the children, stores the node's box and goes on to the parent.  A second launch writes the wide records from the
// refitted BVH4 (the climbing thread holds the four child boxes in registers and could store the record itself, but those 64 bytes
// then sit inside the climb's dependent chain, ahead of the next s_waitcnt: measured 6..18 % slower, profiles/refit_fused_wide_ab.json).
// Coherence across the eight XCD L2s as in lbvh2_leaves_kernel (pt_kernels.hip): bounds words
// travel as agent-scope stores and loads, a thread's stores have left the CU (s_waitcnt vmcnt(0)) before it counts itself in, and
// the loads of the children's words depend on the returned count.  The thread that completes a count also zeroes it, so the
// counters need no reset between updates.
//
// The climb needs what the reference's BVH4 does not store: parent links.  A prepare pass derives them once per installed tree.
// Host twins: pt_host.cpp (refit_bvh4, refit_bvh2, bvh4_cost), on the arithmetic the kernels compile, pt_bounds.h.
#include "pt_kernels.h"
#include "pt_device.h"
#include "pt_bounds.h"

namespace ptk {

namespace {

inline uint32_t blocks(uint32_t n) { return (n + 255u) / 256u; }

__device__ __forceinline__ uint32_t load_agent(const uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void store_agent(uint32_t* p, uint32_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ------------------------------------------------------------------------------------
// prepare, for a tree this library built itself: every node is reachable, ids are the pre-order, wide_index is the internal scan
// (launch_internal_scan).  A thread per node writes its own kind and wide index, its children's parent links, and the packed
// references of its wide record -- everything of that record that no update changes.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void refit_prepare4_kernel(const uint32_t* __restrict__ bvh4, uint32_t m, const uint32_t* __restrict__ wide_index,
                                                              uint32_t num_tris, uint32_t node_base16, uint2* __restrict__ up, uint2* __restrict__ self,
                                                              uint4* __restrict__ child_ref) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t* r = bvh4 + 1 + (size_t)i * 8;
    if (i == 0u) up[0] = make_uint2(kInvalidRef, 0u);
    if (r[7] & kLeaf) { self[i] = make_uint2(kRefitLeaf, kInvalidRef); return; }
    uint32_t ref[4], valid = 0u;
    for (uint32_t s = 0; s < 4u; ++s) {
        ref[s] = kInvalidRef;
        const uint32_t c = r[3 + s];
        if (c == kInvalidRef || c >= m) continue;
        const uint32_t w7 = bvh4[1 + (size_t)c * 8 + 7];
        ref[s] = (w7 & kLeaf) ? ptbd::packed_leaf_ref(w7 & 0x7fffffffu, num_tris) : node_base16 + 4u * wide_index[c];
        up[c] = make_uint2(i, s);
        ++valid;
    }
    const uint32_t w = wide_index[i];
    self[i] = make_uint2(valid, w);
    child_ref[w] = make_uint4(ref[0], ref[1], ref[2], ref[3]);
}

// ------------------------------------------------------------------------------------
// One internal node from its children: the BVH4 box (PathTracer.js:640-661) and the wide record (wide_nodes_kernel's rule: the
// inverted box for an empty slot, kDegenerateRef and the inverted box for a child whose box is degenerate).  AGENT: the children
// were written by other threads of this launch.
// ------------------------------------------------------------------------------------
template <bool AGENT, bool BOX, bool WIDE>
__device__ __forceinline__ void finish_node(uint32_t* bvh4, uint32_t node, uint4 cref, uint4* __restrict__ wide_rec) {
    uint32_t* rec = bvh4 + 1 + (size_t)node * 8;
    const uint32_t ref[4] = {cref.x, cref.y, cref.z, cref.w};
    uint32_t cw[4][3];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        cw[s][0] = kEmptyBox0; cw[s][1] = kEmptyBox1; cw[s][2] = kEmptyBox2;
        if (ref[s] == kInvalidRef) continue;
        const uint32_t* cr = bvh4 + 1 + (size_t)rec[3 + s] * 8;
        if (AGENT) { cw[s][0] = load_agent(cr + 0); cw[s][1] = load_agent(cr + 1); cw[s][2] = load_agent(cr + 2); }
        else       { cw[s][0] = cr[0]; cw[s][1] = cr[1]; cw[s][2] = cr[2]; }
    }
    if (BOX) {
        const float inf = __uint_as_float(0x7f800000u);
        float mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (ref[s] == kInvalidRef) continue;
            using ptbd::js_min_f; using ptbd::js_max_f; using ptbd::half_exact;
            const uint32_t b0 = cw[s][0], b1 = cw[s][1], b2 = cw[s][2];
            mn[0] = js_min_f(mn[0], half_exact(b0 & 0xffffu)); mn[1] = js_min_f(mn[1], half_exact(b0 >> 16)); mn[2] = js_min_f(mn[2], half_exact(b1 & 0xffffu));
            mx[0] = js_max_f(mx[0], half_exact(b1 >> 16)); mx[1] = js_max_f(mx[1], half_exact(b2 & 0xffffu)); mx[2] = js_max_f(mx[2], half_exact(b2 >> 16));
        }
        store_agent(rec + 0, ptbd::pack_trunc_word(mn[0], mn[1], mn[2], mx[0], mx[1], mx[2], 0));
        store_agent(rec + 1, ptbd::pack_trunc_word(mn[0], mn[1], mn[2], mx[0], mx[1], mx[2], 1));
        store_agent(rec + 2, ptbd::pack_trunc_word(mn[0], mn[1], mn[2], mx[0], mx[1], mx[2], 2));
    }
    if (WIDE) {
        uint4 o[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const bool degenerate = ref[s] != kInvalidRef && ptbd::box_degenerate(cw[s][0], cw[s][1], cw[s][2]);
            o[s] = degenerate ? make_uint4(kEmptyBox0, kEmptyBox1, kEmptyBox2, kDegenerateRef) : make_uint4(cw[s][0], cw[s][1], cw[s][2], ref[s]);
        }
        wide_rec[0] = o[0]; wide_rec[1] = o[1]; wide_rec[2] = o[2]; wide_rec[3] = o[3];     // child-major (pt_host.h::WideNode)
    }
}

// One thread per BVH4 node; the threads of leaves (and of internal nodes without a valid child, which keep their words) climb.
__global__ __launch_bounds__(256) void refit4_kernel(const float* __restrict__ tris, uint32_t num_tris, uint32_t* bvh4, uint32_t m,
                                                      const uint2* __restrict__ up, const uint2* __restrict__ self, const uint4* __restrict__ child_ref,
                                                      uint32_t* arrive) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint32_t kind = self[i].x;
    if (kind != kRefitLeaf && kind != 0u) return;               // an internal node with children is finished by its last child; kRefitDead: not reachable
    if (kind == kRefitLeaf) {
        uint32_t* rec = bvh4 + 1 + (size_t)i * 8;
        const uint32_t t = rec[7] & 0x7fffffffu;
        if (t < num_tris) {                                     // a leaf beyond the triangle count keeps its words
            uint32_t w[3];
            ptbd::leaf_box_words(tris + (size_t)t * 9, w);
            store_agent(rec + 0, w[0]); store_agent(rec + 1, w[1]); store_agent(rec + 2, w[2]);
        }
    }
    uint32_t cur = i;
    for (;;) {
        const uint32_t par = up[cur].x;
        if (par == kInvalidRef) break;
        const uint2 ps = self[par];                             // (valid children, wide index)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t old = __hip_atomic_fetch_add(&arrive[par], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old + 1u != ps.x) break;
        store_agent(&arrive[par], 0u);                          // the last to arrive: nobody else touches the count before the next update
        finish_node<true, true, false>(bvh4, par, child_ref[ps.y], nullptr);
        cur = par;
    }
}

// the wide records, from the refitted BVH4
__global__ __launch_bounds__(256) void refit_wide_kernel(uint32_t* bvh4, uint32_t m, const uint2* __restrict__ self, const uint4* __restrict__ child_ref, uint4* __restrict__ wide) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const uint2 s = self[i];
    if (s.x > 4u) return;                                       // leaf or not reachable
    finish_node<false, false, true>(bvh4, i, child_ref[s.y], wide + (size_t)s.y * 4);
}

// ------------------------------------------------------------------------------------
// BVH2: parent links from the child words of every internal node (a tree installed by pt_set_bvh2 has none on the device), then
// lbvh2_leaves_kernel's walk over them.  A node is finished by the second of its two children to arrive.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void refit_prepare2_kernel(const uint32_t* __restrict__ bvh2, uint32_t nn2, uint32_t* __restrict__ parent2) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nn2) return;
    const uint32_t* p = bvh2 + 1 + (size_t)i * 6;
    if (p[5] & kLeaf) return;
    const uint32_t l = p[3], r = p[4];
    if (l >= nn2 || r >= nn2 || l == r) return;                 // such a node is never finished: it keeps its words
    parent2[l] = i; parent2[r] = i;
}

__global__ __launch_bounds__(256) void refit2_kernel(const float* __restrict__ tris, uint32_t num_tris, uint32_t* bvh2, uint32_t nn2,
                                                      const uint32_t* __restrict__ parent2, uint32_t* arrive) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nn2) return;
    uint32_t* p = bvh2 + 1 + (size_t)i * 6;
    const uint32_t w5 = p[5];
    if (!(w5 & kLeaf)) return;
    const uint32_t t = w5 & 0x7fffffffu;
    if (t < num_tris) {
        uint32_t w[3];
        ptbd::leaf_box_words(tris + (size_t)t * 9, w);
        store_agent(p + 0, w[0]); store_agent(p + 1, w[1]); store_agent(p + 2, w[2]);
    }
    uint32_t cur = i;
    for (;;) {
        const uint32_t par = parent2[cur];
        if (par >= nn2) break;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t old = __hip_atomic_fetch_add(&arrive[par], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (old == 0u) break;
        store_agent(&arrive[par], 0u);
        uint32_t* pp = bvh2 + 1 + (size_t)par * 6;
        const uint32_t* lp = bvh2 + 1 + (size_t)pp[3] * 6; const uint32_t* rp = bvh2 + 1 + (size_t)pp[4] * 6;
        const uint32_t l0 = load_agent(lp + 0), l1 = load_agent(lp + 1), l2 = load_agent(lp + 2);
        const uint32_t r0 = load_agent(rp + 0), r1 = load_agent(rp + 1), r2 = load_agent(rp + 2);
        // propagateUp (BVHBuilder.wgsl:242-275): the union, stepped outwards once more by store_bounds2
        const ptbd::Box u = {{wmin(half_lo(l0), half_lo(r0)), wmin(half_hi(l0), half_hi(r0)), wmin(half_lo(l1), half_lo(r1))},
                             {wmax(half_hi(l1), half_hi(r1)), wmax(half_lo(l2), half_lo(r2)), wmax(half_hi(l2), half_hi(r2))}};
        ptbd::store_bounds2(u, [&](int k, uint32_t w) { store_agent(pp + k, w); });
        cur = par;
    }
}

// ------------------------------------------------------------------------------------
// Tree quality (pt_bvh_cost): sum over the reachable internal nodes of halfArea(node) / halfArea(root), boxes decoded exactly,
// f64 throughout (pt_bounds.h::half_area).  Host twin: pt::bvh4_cost.  A degenerate box or one with a NaN bound has half-area 0.
// ------------------------------------------------------------------------------------
using ptbd::half_area;

__global__ __launch_bounds__(256) void bvh_cost_kernel(const uint32_t* __restrict__ bvh4, uint32_t m, const uint2* __restrict__ self, double* __restrict__ out) {
    __shared__ double part[4];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const double root = half_area(bvh4[1], bvh4[2], bvh4[3]);
    double term = 0.0;
    if (i < m && self[i].x <= 4u && root > 0.0 && root < __longlong_as_double(0x7ff0000000000000ll)) {
        const uint32_t* r = bvh4 + 1 + (size_t)i * 8;
        term = half_area(r[0], r[1], r[2]) / root;
    }
    for (int off = 32; off > 0; off >>= 1) term += __shfl_xor(term, off);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = term;
    __syncthreads();
    if (threadIdx.x == 0u) {
        const double s = (part[0] + part[1]) + (part[2] + part[3]);
        if (s != 0.0) atomicAdd(out, s);
    }
}

} // namespace

hipError_t launch_refit_prepare4(const uint32_t* bvh4, uint32_t m, const uint32_t* wide_index, uint32_t num_tris, uint32_t node_base16, const RefitBuffers& R, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(refit_prepare4_kernel, dim3(blocks(m)), dim3(256), 0, stream, bvh4, m, wide_index, num_tris, node_base16, R.up, R.self, R.child_ref);
    return hipGetLastError();
}

hipError_t launch_refit4(const float* tris9, uint32_t num_tris, uint32_t* bvh4, uint32_t m, const RefitBuffers& R, uint4* wide, hipStream_t stream) {
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(refit4_kernel, dim3(blocks(m)), dim3(256), 0, stream, tris9, num_tris, bvh4, m, R.up, R.self, R.child_ref, R.arrive);
    hipLaunchKernelGGL(refit_wide_kernel, dim3(blocks(m)), dim3(256), 0, stream, bvh4, m, R.self, R.child_ref, wide);
    return hipGetLastError();
}

hipError_t launch_refit_prepare2(const uint32_t* bvh2, uint32_t nn2, uint32_t* parent2, hipStream_t stream) {
    if (nn2 == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(parent2, 0xFF, sizeof(uint32_t) * nn2, stream); if (e != hipSuccess) return e;
    hipLaunchKernelGGL(refit_prepare2_kernel, dim3(blocks(nn2)), dim3(256), 0, stream, bvh2, nn2, parent2);
    return hipGetLastError();
}

hipError_t launch_refit2(const float* tris9, uint32_t num_tris, uint32_t* bvh2, uint32_t nn2, const uint32_t* parent2, uint32_t* arrive, hipStream_t stream) {
    if (nn2 == 0) return hipSuccess;
    hipLaunchKernelGGL(refit2_kernel, dim3(blocks(nn2)), dim3(256), 0, stream, tris9, num_tris, bvh2, nn2, parent2, arrive);
    return hipGetLastError();
}

hipError_t launch_bvh_cost(const uint32_t* bvh4, uint32_t m, const uint2* self, double* out, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(out, 0, sizeof(double), stream); if (e != hipSuccess) return e;
    if (m == 0) return hipSuccess;
    hipLaunchKernelGGL(bvh_cost_kernel, dim3(blocks(m)), dim3(256), 0, stream, bvh4, m, self, out);
    return hipGetLastError();
}

} // namespace ptk
