// component_kernels.h - connected components of an indexed triangle mesh on the device: labels, per-component statistics.  The rules
// (which faces count, the area, the union-find loops) are component_rules.h's; the contract is the components section of
// include/vmapstep.h.
//
//   comp_init          parent[v] = v
//   comp_hook          one face per lane: unite(corner 0, corner 1), then that union's root with corner 2; a face with an index out of range is
//                      skipped whole.  Lock-free union-find: the only coherent operations are the device-scope compare-and-swap of a
//                      root and the device-scope atomicMin that shortens a path.  Loads of parent are PLAIN loads: this CU's L1 is
//                      never refreshed by another CU's atomics, so a load may return a value of any age - an older parent is a
//                      larger-or-equal ancestor, which costs hops and failed swaps, never correctness (the swap returns the
//                      current value).  Measured against relaxed agent-scope loads, which go to L2: 0.72 - 0.80 against 1.02 - 1.06 ms
//                      per label_components on the 896 k-face mesh (HISTORY.md).  No lane waits for another: the loops' termination
//                      is an argument about two falling integers (component_rules.h), not about progress elsewhere.
//   comp_flatten       a launch of its own: the kernel boundary makes parent visible to plain loads.  labels[v] = the root of v, found
//                      by plain loads and written to `labels`, never into parent, so it races with nothing; and the block's roots
//                      (root == v) for the numbering.
//   comp_scan          one workgroup: exclusive scan of the blocks' root counts; the total -> counts[0] = C
//   comp_root_emit     block scan + block offset -> dense[v] at every root v: roots in ascending order are numbered 0 .. C - 1, and a
//                      root is its component's smallest vertex
//   comp_relabel       labels[v] = dense[labels[v]] (a lane reads and writes its own entry)
//   comp_face_stats    per valid face: 1 and area_q to the component of its corner 0
//   comp_vertex_stats  per vertex: 1 to its component
// The statistics are integer sums only: any order gives the same bits.  The main surface owns nearly every face, so the adds are
// combined before they reach memory: inside the wave (broadcast one lane's component, ballot the lanes that match, reduce over
// them, one lane carries the run, loop over what is left - ingest_kernels.h's idiom), then the workgroup's sixteen waves in an LDS
// table keyed by component, then one set of global atomics per workgroup and table row.
#pragma once
#include <hip/hip_runtime.h>

#include "component_rules.h"
#include "launch_geometry.h"
#include "scan_ops.h"

#ifndef VCC_PLAIN_LOADS
#define VCC_PLAIN_LOADS 1                  // comp_hook reads parent by plain loads; 0: relaxed agent-scope loads (L2), measurement builds only
#endif
#ifndef VCC_SHORTEN
#define VCC_SHORTEN 1                      // comp_hook shortens paths by atomicMin(parent[x], grandparent); 0: measurement builds only
#endif

namespace vcc {

// parent as comp_hook sees it, while other waves change it
struct HookAccess {
    int* parent;
    __device__ __forceinline__ int load(int x) const {
#if VCC_PLAIN_LOADS
        return parent[x];                                  // may be served by this CU's L1, however old: an ancestor all the same
#else
        return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#endif
    }
    __device__ __forceinline__ int cas(int x, int expect, int desired) { return atomicCAS(parent + x, expect, desired); }      // device scope
    __device__ __forceinline__ void shorten(int x, int to) {
        if (VCC_SHORTEN) atomicMin(parent + x, to);        // monotone: parent[x] only ever falls, to an ancestor
    }
};

// parent after the hooking kernel has ended: nobody writes it any more
struct SettledAccess {
    const int* parent;
    __device__ __forceinline__ int load(int x) const { return parent[x]; }
    __device__ __forceinline__ void shorten(int, int) {}
};

struct LabelArgs {
    const int* faces;                      // [n_faces][3]
    long long n_faces;
    long long n_vertices;
    int nvb;
    int* parent;                           // workspace: [n_vertices]
    int* dense;                            // workspace: [n_vertices], written at roots
    long long* vblk;                       // workspace: [nvb] roots per block, then their exclusive prefix
    int* labels;                           // [n_vertices]: the root after comp_flatten, the component number after comp_relabel
    long long* counts;                     // device int64[1]: C
};

__global__ void __launch_bounds__(kCompWG) comp_init(LabelArgs a) {
    const long long v = (long long)blockIdx.x * kCompWG + threadIdx.x;
    if (v < a.n_vertices) a.parent[v] = (int)v;
}

__global__ void __launch_bounds__(kCompWG) comp_hook(LabelArgs a) {
    const long long face = (long long)blockIdx.x * kCompWG + threadIdx.x;
    if (face >= a.n_faces) return;
    const int v0 = a.faces[3 * face], v1 = a.faces[3 * face + 1], v2 = a.faces[3 * face + 2];
    if (!kr::face_valid(v0, v1, v2, a.n_vertices)) return;
    HookAccess acc{a.parent};
    const int r = kr::unite(acc, v0, v1);                  // a root of corners 0 and 1: corner 1's own walk is not made twice
    kr::unite(acc, r, v2);
}

__global__ void __launch_bounds__(kCompWG) comp_flatten(LabelArgs a) {
    __shared__ int wsum[kCompWG / 64];
    const long long v = (long long)blockIdx.x * kCompWG + threadIdx.x;
    int is_root = 0;
    if (v < a.n_vertices) {
        SettledAccess acc{a.parent};
        const int root = kr::find_root(acc, (int)v);
        a.labels[v] = root;
        is_root = root == (int)v ? 1 : 0;
    }
    int total;
    (void)vscan::wg_exclusive_scan<kCompWG>(is_root, wsum, total);
    if (threadIdx.x == 0) a.vblk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kCompScanWG) comp_scan(LabelArgs a) {
    __shared__ long long wsum[kCompScanWG / 64];
    const long long c = vscan::wg_scan_totals<kCompScanWG>(
        a.nvb, wsum, [&](long long b) { return a.vblk[b]; }, [&](long long b, long long ex) { a.vblk[b] = ex; });
    if (threadIdx.x == 0) a.counts[0] = c;
}

__global__ void __launch_bounds__(kCompWG) comp_root_emit(LabelArgs a) {
    __shared__ int wsum[kCompWG / 64];
    const long long v = (long long)blockIdx.x * kCompWG + threadIdx.x;
    const int is_root = v < a.n_vertices && a.labels[v] == (int)v ? 1 : 0;
    int total;
    const long long at = a.vblk[blockIdx.x] + vscan::wg_exclusive_scan<kCompWG>(is_root, wsum, total);
    if (is_root) a.dense[v] = (int)at;
}

__global__ void __launch_bounds__(kCompWG) comp_relabel(LabelArgs a) {
    const long long v = (long long)blockIdx.x * kCompWG + threadIdx.x;
    if (v < a.n_vertices) a.labels[v] = a.dense[a.labels[v]];      // labels[v] is a root: a vertex, and dense is written there
}

struct StatsArgs {
    const float* vertices;                 // [n_vertices][3] or null: areas stay 0
    const int* faces;                      // [n_faces][3]
    long long n_faces;
    const int* labels;                     // [n_vertices]
    long long n_vertices;
    long long n_components;                // the capacity of the three outputs: a label outside [0, n_components) is not counted
    int* comp_vertices;                    // [n_components]
    unsigned long long* comp_faces;        // [n_components] (int64 to the caller)
    unsigned long long* comp_area_q;       // [n_components] (int64 to the caller: sums wrap like int64's)
};

// The wave's lanes grouped by component: for every distinct c among the lanes with `counted`, one lane calls run(c, lanes, sum of q
// over them).  Wave-uniform control flow; every lane of the wave calls it.
template <bool kWithSum, typename Run>
__device__ __forceinline__ void wave_runs(bool counted, int c, unsigned long long q, Run run) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(counted);
    while (todo != 0) {                                    // one round per distinct component among the wave's lanes
        const int leader = __ffsll((long long)todo) - 1;
        const int lc = __shfl(c, leader, 64);
        const bool mine = counted && c == lc;
        const unsigned long long m = __ballot(mine);
        unsigned long long s = 0;
        if (kWithSum) {
            s = mine ? q : 0ull;
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        }
        if (lane == leader) run(lc, __popcll(m), s);
        todo &= ~m;
    }
}

__global__ void __launch_bounds__(kStatsWG) comp_face_stats(StatsArgs a) {
    __shared__ int key[kStatsSlots];
    __shared__ unsigned long long acc[kStatsSlots][2];
    if (threadIdx.x < kStatsSlots) { key[threadIdx.x] = -1; acc[threadIdx.x][0] = 0; acc[threadIdx.x][1] = 0; }
    __syncthreads();
    const long long face = (long long)blockIdx.x * kStatsWG + threadIdx.x;
    int c = -1;
    unsigned long long q = 0;
    if (face < a.n_faces) {
        const int v0 = a.faces[3 * face], v1 = a.faces[3 * face + 1], v2 = a.faces[3 * face + 2];
        if (kr::face_valid(v0, v1, v2, a.n_vertices)) {
            c = a.labels[v0];
            if (!(c >= 0 && c < a.n_components)) c = -1;
            else if (a.vertices) q = (unsigned long long)kr::quantise_area(kr::triangle_area(a.vertices + 3ll * v0, a.vertices + 3ll * v1, a.vertices + 3ll * v2));
        }
    }
    auto run = [&](int lc, int n, unsigned long long s) {
        const int slot = lc & (kStatsSlots - 1);
        const int was = atomicCAS(&key[slot], -1, lc);
        if (was == -1 || was == lc) {
            atomicAdd(&acc[slot][0], (unsigned long long)n);
            if (s != 0) atomicAdd(&acc[slot][1], s);
        } else {                                           // the row belongs to another component of this workgroup
            atomicAdd(a.comp_faces + lc, (unsigned long long)n);
            if (s != 0) atomicAdd(a.comp_area_q + lc, s);
        }
    };
    if (a.vertices) wave_runs<true>(c >= 0, c, q, run);    // kernel-uniform
    else wave_runs<false>(c >= 0, c, q, run);
    __syncthreads();
    if (threadIdx.x < kStatsSlots && key[threadIdx.x] >= 0) {
        const int lc = key[threadIdx.x];
        atomicAdd(a.comp_faces + lc, acc[threadIdx.x][0]);
        if (acc[threadIdx.x][1] != 0) atomicAdd(a.comp_area_q + lc, acc[threadIdx.x][1]);
    }
}

__global__ void __launch_bounds__(kStatsWG) comp_vertex_stats(StatsArgs a) {
    __shared__ int key[kStatsSlots];
    __shared__ int acc[kStatsSlots];
    if (threadIdx.x < kStatsSlots) { key[threadIdx.x] = -1; acc[threadIdx.x] = 0; }
    __syncthreads();
    const long long v = (long long)blockIdx.x * kStatsWG + threadIdx.x;
    int c = -1;
    if (v < a.n_vertices) {
        c = a.labels[v];
        if (!(c >= 0 && c < a.n_components)) c = -1;
    }
    wave_runs<false>(c >= 0, c, 0ull, [&](int lc, int n, unsigned long long) {
        const int slot = lc & (kStatsSlots - 1);
        const int was = atomicCAS(&key[slot], -1, lc);
        if (was == -1 || was == lc) atomicAdd(&acc[slot], n);
        else atomicAdd(a.comp_vertices + lc, n);
    });
    __syncthreads();
    if (threadIdx.x < kStatsSlots && key[threadIdx.x] >= 0) atomicAdd(a.comp_vertices + key[threadIdx.x], acc[threadIdx.x]);
}

}  // namespace vcc
