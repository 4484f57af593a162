// view_geometry.h - the geometry of view rendering: the ray of a pixel, the segment a ray spends inside an oriented box, the depth
// and the field-frame point of a sample.  Plain inline C++ with no HIP include: the view kernels (view_kernels.h,
// query_split_kernels.h) and the host program of the tests (tests/tools/view_geometry_host.cpp) compile the same functions, so that
// the host program's output is what the device must produce bit for bit.
//
// The rounding contract (include/vmapstep.h, the view section): float32 throughout; every fma below is ONE fused operation, every
// other operation is rounded on its own - contraction is switched off per function (clang: the pragma; other compilers build with
// -ffp-contract=off), divisions are IEEE.  The ray convention is the reference's (vmap.py:31-41, 507-516: direction z = 1, so t is
// depth along the optical axis), the point is (o + d * t) - center (vmap.py:452-454), as load_point of step_kernels.h rebuilds it.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define VG_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define VG_FN inline
#endif
#if defined(__clang__)
#define VG_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define VG_NO_CONTRACT
#endif

namespace vg {

constexpr int kMaxHits = 16;               // VMAPSTEP_VIEW_MAX_HITS: boxes composited per pixel

struct Camera {
    float fx, fy, cx, cy;
    float T[12];                           // camera-to-world, rows 0..2 of the 4 x 4 (row-major)
    float min_depth;
    int width, height, samples;
};

struct Ray {
    float o[3], d[3];
};

// one hit of one box by one pixel's ray, as view_emit writes it: 16 bytes
struct alignas(16) Pair {
    int pixel;                             // w * height + h
    float t_near, dt;
    int zero;
};

// pixel (w, h): dc = ((w - cx) / fx, (h - cy) / fy, 1), d = R dc by two fmas per row, o = the translation
VG_FN Ray pixel_ray(const Camera& c, int w, int h) {
    VG_NO_CONTRACT
    const float x = ((float)w - c.cx) / c.fx;
    const float y = ((float)h - c.cy) / c.fy;
    Ray r;
    for (int i = 0; i < 3; ++i) {
        r.d[i] = __builtin_fmaf(c.T[4 * i], x, __builtin_fmaf(c.T[4 * i + 1], y, c.T[4 * i + 2]));
        r.o[i] = c.T[4 * i + 3];
    }
    return r;
}

// The segment of the ray inside box = centre[3], R[9] (row-major, columns = the box's axes), full extent[3], cut at min_depth and
// into S samples: true iff t_far > t_near; t_near and dt = (t_far - t_near) / S.  fminf / fmaxf drop a NaN operand (a ray parallel
// to a slab and on its face: 0 / 0).  A zero t_near is +0 whatever the signs of the zeros that met (the "+ 0.0f").
VG_FN bool box_segment(const Ray& r, const float* box, float min_depth, int S, float& t_near, float& dt) {
    VG_NO_CONTRACT
    const float* R = box + 3;
    const float q0 = r.o[0] - box[0], q1 = r.o[1] - box[1], q2 = r.o[2] - box[2];
    float near = -__builtin_inff(), far = __builtin_inff();
    for (int i = 0; i < 3; ++i) {
        const float ob = __builtin_fmaf(R[6 + i], q2, __builtin_fmaf(R[3 + i], q1, R[i] * q0));
        const float db = __builtin_fmaf(R[6 + i], r.d[2], __builtin_fmaf(R[3 + i], r.d[1], R[i] * r.d[0]));
        const float h = 0.5f * box[12 + i];
        const float ta = (-h - ob) / db, tb = (h - ob) / db;
        near = __builtin_fmaxf(near, __builtin_fminf(ta, tb));
        far = __builtin_fminf(far, __builtin_fmaxf(ta, tb));
    }
    t_near = __builtin_fmaxf(min_depth, near) + 0.0f;
    dt = (far - t_near) / (float)S;
    return far > t_near;
}

// depth of sample s: fma(s + 0.5, dt, t_near)
VG_FN float sample_depth(float t_near, float dt, int s) {
    VG_NO_CONTRACT
    return __builtin_fmaf((float)s + 0.5f, dt, t_near);
}

// the sample in the object's field frame: (o + d * t) - center, three roundings per coordinate
VG_FN void sample_point(const Ray& r, float t, const float* center, float (&p)[3]) {
    VG_NO_CONTRACT
    for (int i = 0; i < 3; ++i) p[i] = (r.o[i] + r.d[i] * t) - center[i];
}

}  // namespace vg
