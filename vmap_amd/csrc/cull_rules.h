// cull_rules.h - the rule of visibility culling: whether a world point was seen by a keyframe.  Plain inline C++ with no HIP include:
// the cull kernels (cull_kernels.h) and the host program of the tests (tests/tools/cull_rules_host.cpp) compile the same functions, so
// that the host program's output is what the device must produce bit for bit.
//
// The rounding contract (include/vmapstep.h, the cull section): float32 throughout; every fma below is ONE fused operation, every
// other operation is rounded on its own - contraction is switched off per function (clang: the pragma; other compilers build with
// -ffp-contract=off), divisions are IEEE, rintf rounds half to even (the default rounding mode is assumed).
//
// The camera convention is view_geometry.h's: T = rows 0..2 of the camera-to-world matrix (row-major, 12 floats), a pixel (w, h) looks
// along ((w - cx) / fx, (h - cy) / fy, 1), so z is depth along the optical axis.  The rotation is ASSUMED orthonormal: the camera
// frame of a point is R^T (p - t), the transpose standing in for the inverse; nothing checks it.  An all-zero T (an unused slot of
// a FrameStore) gives z = 0, which no min_depth >= 0 lets through: such a frame sees nothing.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define CR_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define CR_FN inline
#endif
#if defined(__clang__)
#define CR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define CR_NO_CONTRACT
#endif

namespace cr {

struct Rules {
    float fx, fy, cx, cy;
    float min_depth;                       // >= 0: a point is in front of the camera iff z > min_depth
    float eps;                             // occlusion tolerance in metres (use_depth only)
    int width, height;                     // depth images are [width][height], width-major
    int margin;                            // pixels at the image border that do not count
    int use_depth;                         // 0: frustum only, the depth image is not read
};

// The pixel p falls on in the frame of pose T, and its depth z along the optical axis: false where p is not in front of the camera
// or its pixel is outside the image less the margin.  A NaN anywhere fails (every comparison is written so that it does).
//   q = p - t;  c_i = fma(T[8 + i], q2, fma(T[4 + i], q1, T[i] * q0))           (R^T q, box_segment's fma shape)
//   u = fma(fx, c_0 / z, cx), v = fma(fy, c_1 / z, cy);  w = rintf(u), h = rintf(v)
// The bounds are compared as floats before the conversion, so nothing out of an int's range is ever converted.
CR_FN bool project(const Rules& r, const float* T, float px, float py, float pz, int& w, int& h, float& z) {
    CR_NO_CONTRACT
    const float q0 = px - T[3], q1 = py - T[7], q2 = pz - T[11];
    const float c0 = __builtin_fmaf(T[8], q2, __builtin_fmaf(T[4], q1, T[0] * q0));
    const float c1 = __builtin_fmaf(T[9], q2, __builtin_fmaf(T[5], q1, T[1] * q0));
    const float c2 = __builtin_fmaf(T[10], q2, __builtin_fmaf(T[6], q1, T[2] * q0));
    z = c2;
    if (!(z > r.min_depth)) return false;
    const float u = __builtin_fmaf(r.fx, c0 / z, r.cx);
    const float v = __builtin_fmaf(r.fy, c1 / z, r.cy);
    const float wf = __builtin_rintf(u), hf = __builtin_rintf(v);
    const float lo = (float)r.margin, w_hi = (float)(r.width - 1 - r.margin), h_hi = (float)(r.height - 1 - r.margin);
    if (!(wf >= lo && wf <= w_hi && hf >= lo && hf <= h_hi)) return false;
    w = (int)wf;
    h = (int)hf;
    return true;
}

// the occlusion test against the depth d the frame measured at the pixel: one rounded add; d <= 0 and a NaN d are no measurement
CR_FN bool not_occluded(float z, float d, float eps) {
    CR_NO_CONTRACT
    return d > 0.0f && z <= d + eps;
}

// element (w, h) of a [width][height] image
CR_FN long long pixel_offset(const Rules& r, int w, int h) { return (long long)w * r.height + h; }

// p is seen by the frame of pose T; depth = the frame's image, not read (may be null) unless r.use_depth
CR_FN bool seen_by(const Rules& r, const float* T, const float* depth, float px, float py, float pz) {
    int w = 0, h = 0;
    float z = 0.0f;
    if (!project(r, T, px, py, pz, w, h, z)) return false;
    if (!r.use_depth) return true;
    return not_occluded(z, depth[pixel_offset(r, w, h)], r.eps);
}

// a face is kept iff at least min_seen of its three corners are seen (a repeated index counts once per corner)
CR_FN bool face_kept(int s0, int s1, int s2, int min_seen) { return (s0 != 0) + (s1 != 0) + (s2 != 0) >= min_seen; }

}  // namespace cr
