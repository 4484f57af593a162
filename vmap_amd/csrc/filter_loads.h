// filter_loads.h - the argument block of the filter kernels and their loads of a decoded frame: one pixel of either input type, and
// four consecutive pixels with one instruction where the pointers are 16-byte aligned.  Shared by the filter kernels
// (filter_kernels.h) and the track kernels (track_kernels.h), which fill a FilterArgs with the fields the loads read.
#pragma once
#include <hip/hip_runtime.h>

#include "filter_rules.h"
#include "launch_geometry.h"

namespace vf {

struct FilterArgs {
    fr::Rules rules;
    int label_i32, depth_f32;              // input types: labels int32 (else uint16), depth float32 (else uint16)
    int vec_ok;                            // depth, inst and labels_out are 16-byte aligned
    const void* depth;                     // [H][W]
    const void* inst;                      // [H][W]
    const void* sem;                       // [H][W]
    const float* box_table;                // [max_ids][fr::kBoxFloats]
    int* status;                           // [max_ids]
    int* rows_out;                         // fr::kHeadInts, then [n_rows][fr::kRowInts]
    unsigned long long* keys_out;          // [n_pix]
    int* labels_out;                       // [H][W]
    int* overflow;                         // workspace
    int* table;                            // workspace: [kReplicas][max_ids][kTableInts]
    unsigned char* flags;                  // workspace: [n_pix]
    int* blk;                              // workspace: [n_blk][2]
    int n_blk;
    long long n_pix;
};

constexpr int kIntMax = 2147483647, kIntMin = -2147483647 - 1;

__device__ __forceinline__ int stat_identity(int field) { return field == 1 ? kIntMax : field == 2 ? kIntMin : 0; }

__device__ __forceinline__ int load_label(const void* p, long long i, int is_i32) {
    return is_i32 ? static_cast<const int*>(p)[i] : (int)static_cast<const unsigned short*>(p)[i];
}
__device__ __forceinline__ float load_depth(const void* p, long long i, int is_f32) {
    return is_f32 ? static_cast<const float*>(p)[i] : (float)static_cast<const unsigned short*>(p)[i];
}

// kPixPer consecutive pixels from pix0 (a multiple of kPixPer): one load where all of them exist and the pointer is aligned
__device__ __forceinline__ void load_labels4(const FilterArgs& a, const void* p, long long pix0, int (&out)[kPixPer]) {
    if (a.vec_ok && pix0 + kPixPer <= a.n_pix) {
        if (a.label_i32) {
            const int4 v = *reinterpret_cast<const int4*>(static_cast<const int*>(p) + pix0);
            out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
        } else {
            const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(p) + pix0);
            out[0] = (int)(v.x & 0xffffu); out[1] = (int)(v.x >> 16); out[2] = (int)(v.y & 0xffffu); out[3] = (int)(v.y >> 16);
        }
    } else {
#pragma unroll
        for (int c = 0; c < kPixPer; ++c) out[c] = pix0 + c < a.n_pix ? load_label(p, pix0 + c, a.label_i32) : 0;
    }
}
__device__ __forceinline__ void load_depths4(const FilterArgs& a, long long pix0, float (&out)[kPixPer]) {
    if (a.vec_ok && pix0 + kPixPer <= a.n_pix) {
        if (a.depth_f32) {
            const float4 v = *reinterpret_cast<const float4*>(static_cast<const float*>(a.depth) + pix0);
            out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
        } else {
            const uint2 v = *reinterpret_cast<const uint2*>(static_cast<const unsigned short*>(a.depth) + pix0);
            out[0] = (float)(v.x & 0xffffu); out[1] = (float)(v.x >> 16); out[2] = (float)(v.y & 0xffffu); out[3] = (float)(v.y >> 16);
        }
    } else {
#pragma unroll
        for (int c = 0; c < kPixPer; ++c) out[c] = pix0 + c < a.n_pix ? load_depth(a.depth, pix0 + c, a.depth_f32) : 0.0f;
    }
}

}  // namespace vf
