// bounds_kernels.h - object bounds on the device: what the reference's sceneObject.get_bound (vmap.py:270-315) does on the host with
// Open3D (unprojection of every keyframe) and trimesh / qhull (oriented_bounds).
//
// Three families, none of which lets the dispatch order decide a result (no float atomics on sums anywhere; what blocks combine is
// a minimum, a maximum or an integer count, so the output is bit-identical from call to call and for any launch geometry):
//   unprojection   unproject_init   the encoded coordinate minimum / maximum of every object = (+inf, -inf)
//                  unproject_count  one block per (object, keyframe) pair and 1024 pixels: pixels with inst == the object's id and
//                                   depth > 0; the per-block total to the workspace, the block's coordinate minimum / maximum into
//                                   the object's by an integer atomic min / max of the order-preserving encoding
//                  unproject_scan   one workgroup: exclusive scan of the block totals; the per-object offsets and decoded bounds
//                  unproject_emit   per block again: block scan + block offset -> each pixel's output row; the same point function
//                                   (the block scans and the scan of the totals are scan_ops.h's: wave shuffles, one LDS word per
//                                   wave; a pair's object is the segment of the pair in first_pair)
//   box search     obb_init         lo = enc(+inf), hi = enc(-inf) for every (object, candidate, axis)
//                  obb_extents      the hot kernel.  A block = (1024 candidates, one chunk of one object's points).  Lanes own
//                                   candidates: kObbCand per lane, each 9 rotation entries and 6 running extremes in registers.  The
//                                   chunk is staged through LDS kObbTile points at a time (centred while staged) and read back one
//                                   point per iteration at a single address for the whole wave - an LDS broadcast, no bank
//                                   conflict, no cross-lane traffic: 9 multiply-adds and 6 min / max per (point, candidate).
//                                   Chunks meet in global memory by integer atomic min / max of the encoding
//                  obb_decode       the encoding back to float32, in place
//   moments        cloud_moments    one workgroup per object: float64 sums of the centred coordinates and their products, every lane
//                                   over a fixed stride, then a fixed tree in LDS - the order depends on the object alone, so the
//                                   covariance of an object is bit-identical whatever else is in the batch
// The encoding of a float32 as uint32 (sign bit set: all bits flipped, else the sign bit set) orders as the value does.
#pragma once
#include <hip/hip_runtime.h>

#include "launch_geometry.h"
#include "scan_ops.h"

namespace vb {

__device__ __forceinline__ unsigned enc_f32(float v) {
    const unsigned b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float dec_f32(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// ---- unprojection (vmap.py:272-282: Open3D's float-image path, no depth scale, no truncation) -------------------------------------

struct UnprojArgs {
    const float* depth;                    // [n_slots][W][H]
    const int* inst;                       // [n_slots][W][H]
    const float* t_wc;                     // [n_slots][4][4]
    int n_slots, width, height;
    float fx, fy, cx, cy;
    const int* pairs;                      // [n_pairs][2]: (store slot, instance id) of every (object, keyframe), objects in order
    const int* first_pair;                 // [n_obj + 1]: the pairs of object o are [first_pair[o], first_pair[o + 1])
    int n_obj, n_pairs, nb;                // nb = blocks per frame
    long long* blk;                        // workspace: [n_pairs * nb] points per block, then (after unproject_scan) their exclusive prefix
    unsigned* enc;                         // workspace: [n_obj][6] encoded (min xyz, max xyz)
    long long* offsets;                    // [n_obj + 1]
    float* bounds;                         // [n_obj][6]
    float* out;                            // [cap][3]
    long long cap;
};

// t_wc . ((w - cx) / fx . d, (h - cy) / fy . d, d, 1): every product and sum written out, so that both passes round alike
__device__ __forceinline__ float3 unproject_pixel(const UnprojArgs& a, const float* T, int w, int h, float d) {
    const float xc = (((float)w - a.cx) / a.fx) * d;
    const float yc = (((float)h - a.cy) / a.fy) * d;
    float3 p;
    p.x = __builtin_fmaf(T[0], xc, __builtin_fmaf(T[1], yc, __builtin_fmaf(T[2], d, T[3])));
    p.y = __builtin_fmaf(T[4], xc, __builtin_fmaf(T[5], yc, __builtin_fmaf(T[6], d, T[7])));
    p.z = __builtin_fmaf(T[8], xc, __builtin_fmaf(T[9], yc, __builtin_fmaf(T[10], d, T[11])));
    return p;
}

// the valid pixels of this lane (bit c of the result: pixel c of its kPixPer); a slot outside the store counts nothing
__device__ __forceinline__ int unproject_lane(const UnprojArgs& a, int pair, long long pix0, float (&d)[kPixPer]) {
    const int slot = a.pairs[2 * pair], id = a.pairs[2 * pair + 1];
    const long long npix = (long long)a.width * a.height;
    int mask = 0;
    if (slot < 0 || slot >= a.n_slots) return 0;
#pragma unroll
    for (int c = 0; c < kPixPer; ++c) {
        const long long pix = pix0 + c;
        d[c] = 0.0f;
        if (pix < npix) {
            const long long g = (long long)slot * npix + pix;
            d[c] = a.depth[g];
            if (a.inst[g] == id && d[c] > 0.0f) mask |= 1 << c;
        }
    }
    return mask;
}

__global__ void __launch_bounds__(kBoundsWG) unproject_init(UnprojArgs a) {
    const int i = blockIdx.x * kBoundsWG + threadIdx.x;
    if (i < a.n_obj * 6) a.enc[i] = enc_f32(i % 6 < 3 ? __builtin_inff() : -__builtin_inff());
}

__global__ void __launch_bounds__(kBoundsWG) unproject_count(UnprojArgs a) {
    __shared__ int wsum[kBoundsWG / 64];
    __shared__ unsigned ext[6];
    const int pair = blockIdx.y;
    const long long pix0 = ((long long)blockIdx.x * kBoundsWG + threadIdx.x) * kPixPer;
    if (threadIdx.x < 6) ext[threadIdx.x] = enc_f32(threadIdx.x < 3 ? __builtin_inff() : -__builtin_inff());
    float d[kPixPer];
    const int mask = unproject_lane(a, pair, pix0, d);
    int total;                                 // at most kPixBlock
    (void)vscan::wg_exclusive_scan<kBoundsWG>(__builtin_popcount(mask), wsum, total);
    if (threadIdx.x == 0) a.blk[(long long)pair * a.nb + blockIdx.x] = total;
    if (total == 0) return;                    // uniform over the block
    __syncthreads();                           // ext[] is initialised before any lane's atomics reach it
    if (mask) {
        const float* T = a.t_wc + 16 * (long long)a.pairs[2 * pair];
        const float inf = __builtin_inff();
        float lo[3] = {inf, inf, inf}, hi[3] = {-inf, -inf, -inf};
#pragma unroll
        for (int c = 0; c < kPixPer; ++c)
            if (mask >> c & 1) {
                const long long pix = pix0 + c;
                const float3 p = unproject_pixel(a, T, (int)(pix / a.height), (int)(pix % a.height), d[c]);
                lo[0] = fminf(lo[0], p.x); lo[1] = fminf(lo[1], p.y); lo[2] = fminf(lo[2], p.z);
                hi[0] = fmaxf(hi[0], p.x); hi[1] = fmaxf(hi[1], p.y); hi[2] = fmaxf(hi[2], p.z);
            }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            atomicMin(&ext[k], enc_f32(lo[k] + 0.0f));           // + 0.0f: a zero of either sign enters as +0
            atomicMax(&ext[3 + k], enc_f32(hi[k] + 0.0f));
        }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        unsigned* e = a.enc + 6 * vscan::segment_of(a.first_pair, a.n_obj, pair) + threadIdx.x;      // the object of this pair
        if (threadIdx.x < 3) atomicMin(e, ext[threadIdx.x]); else atomicMax(e, ext[threadIdx.x]);
    }
}

__global__ void __launch_bounds__(kScanWG) unproject_scan(UnprojArgs a) {
    __shared__ long long wsum[kScanWG / 64];
    const long long n = (long long)a.n_pairs * a.nb;
    const long long carry = vscan::wg_scan_totals<kScanWG>(
        n, wsum, [&](long long b) { return a.blk[b]; }, [&](long long b, long long ex) { a.blk[b] = ex; });
    __syncthreads();                           // the offsets below read prefixes other lanes stored
    for (int o = threadIdx.x; o <= a.n_obj; o += kScanWG) {
        const long long b = (long long)a.first_pair[o] * a.nb;
        a.offsets[o] = b < n ? a.blk[b] : carry;
    }
    for (int i = threadIdx.x; i < a.n_obj * 6; i += kScanWG) a.bounds[i] = dec_f32(a.enc[i]);
}

__global__ void __launch_bounds__(kBoundsWG) unproject_emit(UnprojArgs a) {
    __shared__ int wsum[kBoundsWG / 64];
    const int pair = blockIdx.y;
    const long long pix0 = ((long long)blockIdx.x * kBoundsWG + threadIdx.x) * kPixPer;
    float d[kPixPer];
    const int mask = unproject_lane(a, pair, pix0, d);
    int total;
    long long o = a.blk[(long long)pair * a.nb + blockIdx.x] + vscan::wg_exclusive_scan<kBoundsWG>(__builtin_popcount(mask), wsum, total);
    if (!mask) return;
    const float* T = a.t_wc + 16 * (long long)a.pairs[2 * pair];
#pragma unroll
    for (int c = 0; c < kPixPer; ++c)
        if (mask >> c & 1) {
            const long long pix = pix0 + c;
            const float3 p = unproject_pixel(a, T, (int)(pix / a.height), (int)(pix % a.height), d[c]);
            if (o >= 0 && o < a.cap) {
                a.out[3 * o] = p.x;
                a.out[3 * o + 1] = p.y;
                a.out[3 * o + 2] = p.z;
            }
            ++o;
        }
}

// ---- oriented box search: extents of a cloud along the axes of many candidate frames -----------------------------------------------

struct ObbArgs {
    const float* p;                        // [N][3]
    const long long* po;                   // [n_obj + 1]
    const float* center;                   // [n_obj][3] subtracted from every point while staged; may be null
    const float* rot;                      // [n_sets][K][9] row-major, rows = box axes
    long long set_stride;                  // floats between the sets of two objects; 0 = one set shared by all
    int n_obj, K, chunks;
    unsigned* lo;                          // [n_obj][K][3]: encoded while the launch runs, float32 after obb_decode
    unsigned* hi;
    double* moments;                       // cloud_moments: [n_obj][9] (x, y, z, xx, xy, xz, yy, yz, zz)
};

__global__ void __launch_bounds__(kBoundsWG) obb_init(ObbArgs a) {
    const long long i = (long long)blockIdx.x * kBoundsWG + threadIdx.x;
    if (i < (long long)a.n_obj * a.K * 3) {
        a.lo[i] = enc_f32(__builtin_inff());
        a.hi[i] = enc_f32(-__builtin_inff());
    }
}

__global__ void __launch_bounds__(kBoundsWG) obb_decode(ObbArgs a) {
    const long long i = (long long)blockIdx.x * kBoundsWG + threadIdx.x;
    if (i < (long long)a.n_obj * a.K * 3) {
        a.lo[i] = __float_as_uint(dec_f32(a.lo[i]));
        a.hi[i] = __float_as_uint(dec_f32(a.hi[i]));
    }
}

__global__ void __launch_bounds__(kBoundsWG) obb_extents(ObbArgs a) {
    __shared__ float4 tile[kObbTile];
    const int o = blockIdx.z;
    const long long p0 = a.po[o], p1 = a.po[o + 1];
    // this block's chunk: the object's points cut into a.chunks runs of whole tiles
    long long per = (p1 - p0 + a.chunks - 1) / a.chunks;
    per = (per + kObbTile - 1) / kObbTile * kObbTile;
    const long long b = p0 + (long long)blockIdx.y * per;
    if (b >= p1) return;                   // uniform over the block
    const long long e = b + per < p1 ? b + per : p1;

    float cxyz[3] = {0.0f, 0.0f, 0.0f};
    if (a.center) { cxyz[0] = a.center[3 * o]; cxyz[1] = a.center[3 * o + 1]; cxyz[2] = a.center[3 * o + 2]; }
    const float* rot = a.rot + (long long)o * a.set_stride;
    float r[kObbCand][9], lo[kObbCand][3], hi[kObbCand][3];
#pragma unroll
    for (int j = 0; j < kObbCand; ++j) {
        const int k = blockIdx.x * kObbBlock + j * kBoundsWG + threadIdx.x;
#pragma unroll
        for (int i = 0; i < 9; ++i) r[j][i] = k < a.K ? rot[9 * (long long)k + i] : 0.0f;
#pragma unroll
        for (int i = 0; i < 3; ++i) { lo[j][i] = __builtin_inff(); hi[j][i] = -__builtin_inff(); }
    }
    for (long long t0 = b; t0 < e; t0 += kObbTile) {
        const int n = (int)(e - t0 < kObbTile ? e - t0 : kObbTile);
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += kBoundsWG) {
            const long long g = t0 + k;
            tile[k] = make_float4(a.p[3 * g] - cxyz[0], a.p[3 * g + 1] - cxyz[1], a.p[3 * g + 2] - cxyz[2], 0.0f);
        }
        __syncthreads();
#pragma unroll 4
        for (int k = 0; k < n; ++k) {
            const float4 p = tile[k];            // one address per wave: an LDS broadcast
#pragma unroll
            for (int j = 0; j < kObbCand; ++j)
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    const float u = __builtin_fmaf(r[j][3 * i + 2], p.z, __builtin_fmaf(r[j][3 * i + 1], p.y, r[j][3 * i] * p.x));
                    lo[j][i] = fminf(lo[j][i], u);
                    hi[j][i] = fmaxf(hi[j][i], u);
                }
        }
    }
#pragma unroll
    for (int j = 0; j < kObbCand; ++j) {
        const int k = blockIdx.x * kObbBlock + j * kBoundsWG + threadIdx.x;
        if (k < a.K) {
            const long long at = ((long long)o * a.K + k) * 3;
#pragma unroll
            for (int i = 0; i < 3; ++i) {
                atomicMin(a.lo + at + i, enc_f32(lo[j][i] + 0.0f));      // + 0.0f: a zero of either sign enters as +0
                atomicMax(a.hi + at + i, enc_f32(hi[j][i] + 0.0f));
            }
        }
    }
}

__global__ void __launch_bounds__(kScanWG) cloud_moments(ObbArgs a) {
    __shared__ double lds[kScanWG];
    const int o = blockIdx.x;
    const long long p0 = a.po[o], p1 = a.po[o + 1];
    double c[3] = {0.0, 0.0, 0.0};
    if (a.center) { c[0] = a.center[3 * o]; c[1] = a.center[3 * o + 1]; c[2] = a.center[3 * o + 2]; }
    double s[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (long long g = p0 + threadIdx.x; g < p1; g += kScanWG) {
        const double x = (double)a.p[3 * g] - c[0], y = (double)a.p[3 * g + 1] - c[1], z = (double)a.p[3 * g + 2] - c[2];
        s[0] += x; s[1] += y; s[2] += z;
        s[3] += x * x; s[4] += x * y; s[5] += x * z;
        s[6] += y * y; s[7] += y * z; s[8] += z * z;
    }
    for (int m = 0; m < 9; ++m) {
        __syncthreads();
        lds[threadIdx.x] = s[m];
        __syncthreads();
        for (int off = kScanWG / 2; off > 0; off >>= 1) {
            if ((int)threadIdx.x < off) lds[threadIdx.x] += lds[threadIdx.x + off];
            __syncthreads();
        }
        if (threadIdx.x == 0) a.moments[9 * o + m] = lds[0];
    }
}

}  // namespace vb
