// eval_kernels.h - mesh evaluation on the device: what the reference's metric/eval_3D_obj.py:8-41 and metric/metrics.py do on the
// host with trimesh and scipy (crop to the GT box, area-weighted surface samples, KD-tree nearest neighbours).
//
// Three families, none of which lets the dispatch order decide a result (the output is bit-identical from call to call and does
// not depend on the launch geometry):
//   nearest neighbour  nn_plan     one workgroup: per set, (query blocks x ref chunks) work items, exclusive prefix to the workspace
//                                  (scan_ops.h's scan of totals)
//                      nn_init     the packed (squared distance bits, ref index) key of every query = all ones
//                      nn_search   one item per workgroup (its set: the segment of the item in that prefix): kNnQ queries per lane in registers, the item's refs staged through LDS
//                                  kNnTile at a time and broadcast to the wave; per query the running (min, first index), then one
//                                  64-bit atomic min of the packed key.  A squared distance is >= 0, so its float bits order as the
//                                  value; the low word breaks ties to the smallest ref index; min is order-independent
//                      nn_finalize dist = sqrtf(min squared distance), index = the key's low word
//   surface sampling   surface_cdf     one workgroup per set: float64 face areas, inclusive per-set cumulative sum (a scan of its
//                                      own, in a fixed order of additions)
//                      surface_sample  per point: u0 -> searchsorted_left(cdf, u0 * total), (r1, r2) folded, v0 + r1 e1 + r2 e2
//   box clipping       clip_count  per face: triangles left after Sutherland-Hodgman against the box's 6 half-spaces; per-block
//                                  totals to the workspace
//                      clip_scan   one workgroup: exclusive scan of the block totals, the grand total to a device int64
//                      clip_emit   per face again: block scan + block offset -> its first output triangle; the fan from vertex 0
//                                  (the block scans and the scan of the totals are scan_ops.h's: wave shuffles, one LDS word per wave)
// Distances are always taken from coordinate differences (dx*dx + dy*dy + dz*dz), never from |a|^2 + |b|^2 - 2 a.b, which loses
// millimetres at room scale exactly where the completion ratio at 1 cm is decided.
#pragma once
#include <hip/hip_runtime.h>

#include "launch_geometry.h"
#include "scan_ops.h"

namespace ve {

constexpr int kCdfWG = 256;                // surface_cdf
constexpr int kCdfPer = 4;                 // faces per lane and round of surface_cdf

struct NnArgs {
    const float* q;                        // [n][3]
    const float* r;                        // [m][3]
    const long long* qo;                   // [n_sets + 1]
    const long long* ro;                   // [n_sets + 1]
    int n_sets;
    long long rchunk;                      // refs per work item, a multiple of kNnTile
    long long* prefix;                     // workspace: [n_sets + 1] exclusive prefix of the work items
    unsigned long long* keys;              // workspace: [n] (only [q_begin, q_end) is used)
    long long q_begin, q_end;
    float* dist;
    int* index;                            // may be null
};

__device__ __forceinline__ long long nn_items(const NnArgs& a, int s) {
    const long long nq = a.qo[s + 1] - a.qo[s], nr = a.ro[s + 1] - a.ro[s];
    if (nq <= 0 || nr <= 0) return 0;
    return ((nq + kNnQB - 1) / kNnQB) * ((nr + a.rchunk - 1) / a.rchunk);
}

__global__ void __launch_bounds__(kPlanWG) nn_plan(NnArgs a) {
    __shared__ long long wsum[kPlanWG / 64];
    const long long items = vscan::wg_scan_totals<kPlanWG>(
        a.n_sets, wsum, [&](long long s) { return nn_items(a, (int)s); }, [&](long long s, long long ex) { a.prefix[s] = ex; });
    if (threadIdx.x == 0) a.prefix[a.n_sets] = items;
}

__global__ void __launch_bounds__(kEvalWG) nn_init(NnArgs a) {
    const long long i = a.q_begin + (long long)blockIdx.x * kEvalWG + threadIdx.x;
    if (i < a.q_end) a.keys[i] = ~0ull;
}

__global__ void __launch_bounds__(kNnWG) nn_search(NnArgs a) {
    __shared__ float4 tile[kNnTile];
    const long long item = blockIdx.x;
    const int s = vscan::segment_of(a.prefix, a.n_sets, item);      // sets without items share their successor's prefix
    const long long q0 = a.qo[s], q1 = a.qo[s + 1], r0 = a.ro[s], r1 = a.ro[s + 1];
    const long long nrc = (r1 - r0 + a.rchunk - 1) / a.rchunk;
    const long long local = item - a.prefix[s];
    const long long qb = q0 + (local / nrc) * kNnQB;
    const long long rb = r0 + (local % nrc) * a.rchunk;
    const long long re = rb + a.rchunk < r1 ? rb + a.rchunk : r1;

    float qx[kNnQ], qy[kNnQ], qz[kNnQ], best[kNnQ];
    int bi[kNnQ];
#pragma unroll
    for (int j = 0; j < kNnQ; ++j) {
        const long long i = qb + j * kNnWG + threadIdx.x;
        const bool ok = i < q1;
        qx[j] = ok ? a.q[3 * i] : 0.0f;
        qy[j] = ok ? a.q[3 * i + 1] : 0.0f;
        qz[j] = ok ? a.q[3 * i + 2] : 0.0f;
        best[j] = __builtin_inff();
        bi[j] = (int)rb;
    }
    for (long long t0 = rb; t0 < re; t0 += kNnTile) {
        const int n = (int)(re - t0 < kNnTile ? re - t0 : kNnTile);
        const int n4 = (n + 3) & ~3;
        __syncthreads();
        for (int k = threadIdx.x; k < n4; k += kNnWG) {
            // padding refs at infinity: their distance is +inf and never replaces a finite minimum under the strict <
            const float inf = __builtin_inff();
            const long long g = t0 + k;
            tile[k] = k < n ? make_float4(a.r[3 * g], a.r[3 * g + 1], a.r[3 * g + 2], 0.0f) : make_float4(inf, inf, inf, 0.0f);
        }
        __syncthreads();
        const int base = (int)t0;
#pragma unroll 4
        for (int k = 0; k < n4; ++k) {
            const float4 p = tile[k];            // one address per wave: an LDS broadcast
#pragma unroll
            for (int j = 0; j < kNnQ; ++j) {
                const float dx = qx[j] - p.x, dy = qy[j] - p.y, dz = qz[j] - p.z;
                const float d = __builtin_fmaf(dz, dz, __builtin_fmaf(dy, dy, dx * dx));
                if (d < best[j]) { best[j] = d; bi[j] = base + k; }      // strict: the first (smallest) index keeps a tie
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kNnQ; ++j) {
        const long long i = qb + j * kNnWG + threadIdx.x;
        if (i < q1) {
            const unsigned long long key = ((unsigned long long)__float_as_uint(best[j]) << 32) | (unsigned)bi[j];
            atomicMin(a.keys + i, key);
        }
    }
}

__global__ void __launch_bounds__(kEvalWG) nn_finalize(NnArgs a) {
    const long long i = a.q_begin + (long long)blockIdx.x * kEvalWG + threadIdx.x;
    if (i >= a.q_end) return;
    const unsigned long long key = a.keys[i];
    a.dist[i] = sqrtf(__uint_as_float((unsigned)(key >> 32)));
    if (a.index) a.index[i] = (int)(unsigned)(key & 0xffffffffu);
}

// ---- surface sampling (trimesh.sample.sample_surface) ----------------------------------------------------------------------------

struct U4 { unsigned x, y, z, w; };

// Philox4x32-10, the same function as the ray sampler's (sample_kernels.h); the streams are disjoint from the sampler's by use
__device__ __forceinline__ U4 philox4x32_10(U4 c, unsigned k0, unsigned k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const unsigned long long p0 = 0xD2511F53ull * c.x, p1 = 0xCD9E8D57ull * c.z;
        const U4 n = {(unsigned)(p1 >> 32) ^ c.y ^ k0, (unsigned)p1, (unsigned)(p0 >> 32) ^ c.w ^ k1, (unsigned)p0};
        c = n;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

struct SurfArgs {
    const float* v;                        // [V][3]
    long long n_vertices;
    const int* f;                          // [F][3], indices into v
    const long long* fo;                   // [n_sets + 1] faces of each set
    const long long* oo;                   // [n_sets + 1] output points of each set
    int n_sets;
    double* cdf;                           // workspace: [F] inclusive per-set cumulative area
    long long o_begin, o_end;
    float* out;                            // [N][3]
    int* face_index;                       // may be null
    const double* u0;                      // test mode (both or neither): [N]
    const float* r;                        //                              [N][2]
    unsigned seed_lo, seed_hi, stream;
    int set_base;
};

// a vertex of face f; an index outside [0, V) reads as the origin (never out of bounds)
__device__ __forceinline__ float3 face_vertex(const float* v, long long nv, const int* f, long long face, int c) {
    const int i = f[3 * face + c];
    if (i < 0 || i >= nv) return make_float3(0.0f, 0.0f, 0.0f);
    return make_float3(v[3 * (long long)i], v[3 * (long long)i + 1], v[3 * (long long)i + 2]);
}

// 0.5 |(v1 - v0) x (v2 - v0)| in float64 (trimesh's area_faces on float64 vertices)
__device__ __forceinline__ double face_area(const SurfArgs& a, long long face) {
    const float3 p0 = face_vertex(a.v, a.n_vertices, a.f, face, 0), p1 = face_vertex(a.v, a.n_vertices, a.f, face, 1),
                 p2 = face_vertex(a.v, a.n_vertices, a.f, face, 2);
    const double ax = (double)p1.x - p0.x, ay = (double)p1.y - p0.y, az = (double)p1.z - p0.z;
    const double bx = (double)p2.x - p0.x, by = (double)p2.y - p0.y, bz = (double)p2.z - p0.z;
    const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
    return 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
}

// Inclusive scan of one float64 per lane over the kCdfWG lanes (Hillis-Steele in LDS); every lane gets the total as well.  Not
// scan_ops.h's shuffle scan: this tree fixes the order of the float64 additions, and the cumulative areas decide a sample's face.
__device__ __forceinline__ double cdf_inclusive_scan(double v, double* lds, double& total) {
    const int t = threadIdx.x;
    lds[t] = v;
    __syncthreads();
#pragma unroll
    for (int off = 1; off < kCdfWG; off <<= 1) {
        const double add = t >= off ? lds[t - off] : 0.0;
        __syncthreads();
        lds[t] += add;
        __syncthreads();
    }
    const double out = lds[t];
    total = lds[kCdfWG - 1];
    __syncthreads();
    return out;
}

__global__ void __launch_bounds__(kCdfWG) surface_cdf(SurfArgs a) {
    __shared__ double lds[kCdfWG];
    const int s = blockIdx.x;
    const long long f0 = a.fo[s], f1 = a.fo[s + 1];
    double carry = 0.0;
    for (long long base = f0; base < f1; base += (long long)kCdfWG * kCdfPer) {
        const long long mine = base + (long long)threadIdx.x * kCdfPer;
        double part[kCdfPer], sum = 0.0;
#pragma unroll
        for (int c = 0; c < kCdfPer; ++c) {
            part[c] = mine + c < f1 ? face_area(a, mine + c) : 0.0;
            sum += part[c];
            part[c] = sum;
        }
        double total;
        const double incl = cdf_inclusive_scan(sum, lds, total);
        const double excl = carry + (incl - sum);
#pragma unroll
        for (int c = 0; c < kCdfPer; ++c)
            if (mine + c < f1) a.cdf[mine + c] = excl + part[c];
        carry += total;
    }
}

__global__ void __launch_bounds__(kEvalWG) surface_sample(SurfArgs a) {
    const long long j = a.o_begin + (long long)blockIdx.x * kEvalWG + threadIdx.x;
    if (j >= a.o_end) return;
    const int s = vscan::segment_of(a.oo, a.n_sets, j);             // the set of point j
    double u0;
    float r1, r2;
    if (a.u0) {
        u0 = a.u0[j];
        r1 = a.r[2 * j];
        r2 = a.r[2 * j + 1];
    } else {
        const U4 w = philox4x32_10({(unsigned)(j - a.oo[s]), (unsigned)(a.set_base + s), a.stream, 0u}, a.seed_lo, a.seed_hi);
        u0 = (double)(((unsigned long long)w.x << 21) | (w.y >> 11)) * 0x1p-53;
        r1 = (float)(w.z >> 8) * 0x1p-24f;
        r2 = (float)(w.w >> 8) * 0x1p-24f;
    }
    if ((double)r1 + (double)r2 > 1.0) { r1 = 1.0f - r1; r2 = 1.0f - r2; }
    const long long f0 = a.fo[s], f1 = a.fo[s + 1];
    const double target = u0 * a.cdf[f1 - 1];
    long long l = f0, h = f1;                       // searchsorted(..., side='left'): the first face with cdf >= target
    while (l < h) {
        const long long m = (l + h) >> 1;
        if (a.cdf[m] < target) l = m + 1; else h = m;
    }
    const long long face = l < f1 ? l : f1 - 1;
    const float3 p0 = face_vertex(a.v, a.n_vertices, a.f, face, 0), p1 = face_vertex(a.v, a.n_vertices, a.f, face, 1),
                 p2 = face_vertex(a.v, a.n_vertices, a.f, face, 2);
    a.out[3 * j] = p0.x + __builtin_fmaf(r1, p1.x - p0.x, r2 * (p2.x - p0.x));
    a.out[3 * j + 1] = p0.y + __builtin_fmaf(r1, p1.y - p0.y, r2 * (p2.y - p0.y));
    a.out[3 * j + 2] = p0.z + __builtin_fmaf(r1, p1.z - p0.z, r2 * (p2.z - p0.z));
    if (a.face_index) a.face_index[j] = (int)face;
}

// ---- cropping to an oriented box (trimesh's slice_plane against the 6 faces of the box) -------------------------------------------

constexpr int kClipMax = 9;                // a triangle cut by 6 planes keeps at most 3 + 6 vertices

struct ClipArgs {
    const float* v;
    long long n_vertices;
    const int* f;
    long long n_faces;
    int nblk;
    float c[3];                            // box centre
    float ax[3][3];                        // ax[k] = the box's k-th axis (column k of R)
    float h[3];                            // half extents
    long long* blk;                        // workspace: [nblk] triangles per block, then (after clip_scan) their exclusive prefix
    long long* count;                      // device int64[1]: all triangles
    float* out;                            // [cap][3][3]
    long long cap;
};

// Sutherland-Hodgman of face `face` against the half-spaces h_k -+ ax_k . (p - c) >= 0; returns the polygon's vertex count
__device__ __forceinline__ int clip_face(const ClipArgs& a, long long face, float (&px)[kClipMax], float (&py)[kClipMax], float (&pz)[kClipMax]) {
    int n = 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float3 p = face_vertex(a.v, a.n_vertices, a.f, face, c);
        px[c] = p.x; py[c] = p.y; pz[c] = p.z;
    }
    for (int pl = 0; pl < 6 && n > 0; ++pl) {
        const int k = pl >> 1;
        const float sg = (pl & 1) ? 1.0f : -1.0f;
        float sd[kClipMax];
        for (int i = 0; i < n; ++i)
            sd[i] = a.h[k] + sg * (a.ax[k][0] * (px[i] - a.c[0]) + a.ax[k][1] * (py[i] - a.c[1]) + a.ax[k][2] * (pz[i] - a.c[2]));
        bool all_in = true;
        for (int i = 0; i < n; ++i) all_in &= sd[i] >= 0.0f;
        if (all_in) continue;                      // the polygon unchanged (a triangle inside the box stays bit-identical)
        float ox[kClipMax], oy[kClipMax], oz[kClipMax];
        int m = 0;
        for (int i = 0; i < n; ++i) {
            const int pv = i == 0 ? n - 1 : i - 1;
            const bool in_c = sd[i] >= 0.0f, in_p = sd[pv] >= 0.0f;
            if (in_c != in_p && m < kClipMax) {
                // p = the previous vertex, q = the current one: p + (s_p / (s_p - s_q)) (q - p)
                const float t = sd[pv] / (sd[pv] - sd[i]);
                ox[m] = px[pv] + t * (px[i] - px[pv]);
                oy[m] = py[pv] + t * (py[i] - py[pv]);
                oz[m] = pz[pv] + t * (pz[i] - pz[pv]);
                ++m;
            }
            if (in_c && m < kClipMax) { ox[m] = px[i]; oy[m] = py[i]; oz[m] = pz[i]; ++m; }
        }
        n = m;
        for (int i = 0; i < n; ++i) { px[i] = ox[i]; py[i] = oy[i]; pz[i] = oz[i]; }
    }
    return n;
}

__global__ void __launch_bounds__(kEvalWG) clip_count(ClipArgs a) {
    __shared__ int wsum[kEvalWG / 64];
    const long long face = (long long)blockIdx.x * kEvalWG + threadIdx.x;
    int t = 0;                                 // at most kClipMax - 2 per face: a block's sums fit an int
    if (face < a.n_faces) {
        float px[kClipMax], py[kClipMax], pz[kClipMax];
        const int n = clip_face(a, face, px, py, pz);
        t = n >= 3 ? n - 2 : 0;
    }
    int total;
    (void)vscan::wg_exclusive_scan<kEvalWG>(t, wsum, total);
    if (threadIdx.x == 0) a.blk[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kPlanWG) clip_scan(ClipArgs a) {
    __shared__ long long wsum[kPlanWG / 64];
    const long long all = vscan::wg_scan_totals<kPlanWG>(
        a.nblk, wsum, [&](long long b) { return a.blk[b]; }, [&](long long b, long long ex) { a.blk[b] = ex; });
    if (threadIdx.x == 0) a.count[0] = all;
}

__global__ void __launch_bounds__(kEvalWG) clip_emit(ClipArgs a) {
    __shared__ int wsum[kEvalWG / 64];
    const long long face = (long long)blockIdx.x * kEvalWG + threadIdx.x;
    float px[kClipMax], py[kClipMax], pz[kClipMax];
    int n = 0;
    if (face < a.n_faces) n = clip_face(a, face, px, py, pz);
    const int t = n >= 3 ? n - 2 : 0;
    int total;
    const long long first = a.blk[blockIdx.x] + vscan::wg_exclusive_scan<kEvalWG>(t, wsum, total);
    for (int k = 0; k < t; ++k) {
        const long long o = first + k;
        if (o >= a.cap) break;
        float* w = a.out + 9 * o;
        const int id[3] = {0, k + 1, k + 2};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            w[3 * c] = px[id[c]];
            w[3 * c + 1] = py[id[c]];
            w[3 * c + 2] = pz[id[c]];
        }
    }
}

}  // namespace ve
