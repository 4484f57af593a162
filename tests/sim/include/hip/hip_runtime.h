// TEST INFRASTRUCTURE: stand-in for <hip/hip_runtime.h> when the kernel headers are compiled for the CPU
// SIMT executor (tests/sim).  Only what the kernel headers under vmap_amd/csrc use.
#pragma once
#include <cmath>
#include <cstdint>

#include "sim_runtime.h"

#define __global__
#define __device__
#define __host__
#define __forceinline__ inline __attribute__((always_inline))
#define __launch_bounds__(...)
#define __restrict__
// a workgroup's fibers all run on one OS thread and a thread runs one workgroup at a time: thread-local statics are per workgroup.
// (They are NOT re-poisoned between workgroups: a kernel that reads shared memory it never wrote sees the previous workgroup's.)
#define __shared__ static thread_local
#define __constant__ static const

struct sim_tid_proxy { unsigned x, y, z; };
#define threadIdx (sim_tid_proxy{sim::tid(), 0u, 0u})
#define blockIdx (sim::g_blockIdx)
#define blockDim (sim::g_blockDim)
#define gridDim (sim::g_gridDim)

inline void __syncthreads() { sim::block_barrier(); }
inline float atomicAdd(float* p, float v) { float o = *p; *p = o + v; return o; }
inline int atomicOr(int* p, int v) { int o = *p; *p = o | v; return o; }
inline int atomicMax(int* p, int v) {                       // workgroups run on several OS threads: a real atomic
    int o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v > o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}

inline int min(int a, int b) { return a < b ? a : b; }
inline int max(int a, int b) { return a > b ? a : b; }
#include <cstring>
inline unsigned __float_as_uint(float x) { unsigned u; std::memcpy(&u, &x, 4); return u; }
inline float __uint_as_float(unsigned u) { float x; std::memcpy(&x, &u, 4); return x; }

// ---- what the mesh, evaluation and bounds families use (mesh_kernels.h, eval_kernels.h, bounds_kernels.h, scan_ops.h) ----
struct float3 { float x, y, z; };
struct alignas(16) float4 { float x, y, z, w; };
inline float3 make_float3(float x, float y, float z) { return float3{x, y, z}; }
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }
inline int __popc(unsigned x) { return __builtin_popcount(x); }

// __shfl_up over the 64 lanes of a wave, as a rendezvous: every lane publishes, one wave barrier, every lane reads.  Two
// buffers used in turn make the single barrier enough: a buffer is rewritten two shuffles later, when every lane has passed the
// barrier of the shuffle in between and so has finished reading.  A partial last wave reads its own value from absent lanes.
template <typename T>
inline T __shfl_up(T v, unsigned delta, int width = 64) {
    static_assert(sizeof(T) == 4 || sizeof(T) == 8, "4- and 8-byte types");
    (void)width;
    const int w = sim::wave_id(), l = sim::lane_id();
    unsigned long long (*buf)[sim::kWave] = sim::g_block->x8[sim::g_cur->shfl_turn++ & 1u];
    unsigned long long bits = 0;
    std::memcpy(&bits, &v, sizeof(T));
    buf[w][l] = bits;
    sim::wave_barrier();
    const int src = l - (int)delta;
    if (src >= 0) std::memcpy(&v, &buf[w][src], sizeof(T));
    return v;
}

// workgroups run on several OS threads: real atomics
template <typename T>
inline T sim_atomic_min(T* p, T v) {
    T o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v < o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
template <typename T>
inline T sim_atomic_max(T* p, T v) {
    T o = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (v > o && !__atomic_compare_exchange_n(p, &o, v, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    return o;
}
inline unsigned atomicMin(unsigned* p, unsigned v) { return sim_atomic_min(p, v); }
inline unsigned atomicMax(unsigned* p, unsigned v) { return sim_atomic_max(p, v); }
inline unsigned long long atomicMin(unsigned long long* p, unsigned long long v) { return sim_atomic_min(p, v); }
inline unsigned long long atomicMax(unsigned long long* p, unsigned long long v) { return sim_atomic_max(p, v); }
