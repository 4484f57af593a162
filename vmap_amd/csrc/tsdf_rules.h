// tsdf_rules.h - the rule of TSDF fusion: how one posed depth frame changes one voxel of a truncated signed distance volume.  Plain
// inline C++ with no HIP include: the kernel (tsdf_kernels.h) and the host program of the tests (tests/tools/tsdf_rules_host.cpp)
// compile the same functions, so that the host program's output is what the device must produce bit for bit.
//
// The rounding contract (include/vmapstep.h, the tsdf section): float32 throughout; every fma below is ONE fused operation, every
// other operation is rounded on its own - contraction is switched off per function (clang: the pragma; other compilers build with
// -ffp-contract=off), divisions are IEEE.  Projection is cull_rules.h's cr::project: its camera convention, its half-to-even pixel
// and its margin are the ones pinned there.
//
// The two properties the tests hold:
//   1. A voxel is owned by one lane and updated sequentially over the frames, with no atomics: the result depends on the ORDER of the
//      frames only, never on the launch geometry (workgroup size, voxels per lane, frames per LDS chunk).
//   2. The state after a frame is exactly what the volume stores (float32 D, W and r, g, b, wc; nothing else is carried), so
//      integrate(frames 0 .. K) equals integrate(0 .. a) followed by integrate(a .. K) bit for bit.
#pragma once

#include "cull_rules.h"

namespace tr {

struct Rules {
    cr::Rules cam;                         // fx, fy, cx, cy, min_depth, width, height, margin (eps and use_depth are not read)
    float max_depth;                       // a measurement d is usable iff d > min_depth && d <= max_depth (NaN, inf, <= min_depth fail)
    float trunc;                           // > 0, metres
    float max_weight;                      // >= 1: the cap of both weights
    int obj_id;                            // >= 0: only pixels whose instance id equals it; < 0: the instance image is not read
};

// the centre of voxel (i, j, k) under the affine A ([3,4] rows, index -> world): mesh_grid_points' arithmetic
CR_FN void voxel_center(const float* A, int i, int j, int k, float& x, float& y, float& z) {
    CR_NO_CONTRACT
    const float fi = (float)i, fj = (float)j, fk = (float)k;
    x = __builtin_fmaf(A[2], fk, __builtin_fmaf(A[1], fj, __builtin_fmaf(A[0], fi, A[3])));
    y = __builtin_fmaf(A[6], fk, __builtin_fmaf(A[5], fj, __builtin_fmaf(A[4], fi, A[7])));
    z = __builtin_fmaf(A[10], fk, __builtin_fmaf(A[9], fj, __builtin_fmaf(A[8], fi, A[11])));
}

// The signed distance a frame measures for a voxel that projects onto pixel `pix` (cr::pixel_offset) at depth z along the optical axis;
// depth / inst: the frame's own images.  false = no update: no usable measurement, another instance's pixel, or farther than trunc
// behind the surface.  sdf = d - z is one rounded subtraction.
CR_FN bool measure(const Rules& r, const float* depth, const int* inst, long long pix, float z, float& sdf) {
    CR_NO_CONTRACT
    const float d = depth[pix];
    if (!(d > r.cam.min_depth && d <= r.max_depth)) return false;
    if (r.obj_id >= 0 && inst[pix] != r.obj_id) return false;
    sdf = d - z;
    return sdf >= -r.trunc;
}

// D <- (D W + s) / (W + 1) with s = min(1, sdf / trunc); W <- min(W + 1, max_weight)
CR_FN void update(const Rules& r, float sdf, float& D, float& W) {
    CR_NO_CONTRACT
    const float s = __builtin_fminf(1.0f, sdf / r.trunc);
    const float W1 = W + 1.0f;
    D = __builtin_fmaf(D, W, s) / W1;
    W = __builtin_fminf(W1, r.max_weight);
}

// colour is updated only inside the band (measure() has already passed sdf >= -trunc)
CR_FN bool in_band(const Rules& r, float sdf) { return sdf <= r.trunc; }

// c = (r, g, b, wc) on the 0 .. 255 scale; px = the pixel's bytes (its first three are read)
CR_FN void update_color(const Rules& r, const unsigned char* px, float* c) {
    CR_NO_CONTRACT
    const float wc = c[3], wc1 = wc + 1.0f;
    c[0] = __builtin_fmaf(c[0], wc, (float)px[0]) / wc1;
    c[1] = __builtin_fmaf(c[1], wc, (float)px[1]) / wc1;
    c[2] = __builtin_fmaf(c[2], wc, (float)px[2]) / wc1;
    c[3] = __builtin_fminf(wc1, r.max_weight);
}

// One frame (pose T = 12 floats, images depth / rgbx / inst of that frame; rgbx may be null with c null) applied to one voxel at
// (px, py, pz).  Returns whether D, W (and c) were updated.  The kernel runs the same three steps, with a wave-wide vote between
// the projection and the gather.
CR_FN bool integrate_frame(const Rules& r, const float* T, const float* depth, const unsigned char* rgbx, const int* inst, float px, float py,
                           float pz, float& D, float& W, float* c) {
    int w = 0, h = 0;
    float z = 0.0f, sdf = 0.0f;
    if (!cr::project(r.cam, T, px, py, pz, w, h, z)) return false;
    const long long pix = cr::pixel_offset(r.cam, w, h);
    if (!measure(r, depth, inst, pix, z, sdf)) return false;
    update(r, sdf, D, W);
    if (c && in_band(r, sdf)) update_color(r, rgbx + 4 * pix, c);
    return true;
}

}  // namespace tr
