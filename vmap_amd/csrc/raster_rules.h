// raster_rules.h - the rules of the mesh rasteriser: which faces take part in a view, how a corner is snapped to the sub-pixel grid,
// which pixel centres a face covers, the depth it has there, the key the z-buffer minimises, and the comparison of two depth images.
// Plain inline C++ with no HIP include: the raster kernels (raster_kernels.h) and the host program of the tests
// (tests/tools/raster_rules_host.cpp) compile the same functions, so that the host program's output is what the device must produce
// bit for bit.  The contract is the raster section of include/vmapstep.h.
//
// The rounding contract.  The camera is cull_rules.h's, in float32: every fma below is ONE fused operation, every other operation is
// rounded on its own (contraction is switched off per function: clang by the pragma, other compilers build with -ffp-contract=off),
// divisions are IEEE, rintf rounds half to even.  Coverage is integer arithmetic and exact (see kGuard).  The depth of a covered
// pixel is float64 with NO fused operation, in the order depth_at spells out, and one rounding to float32 at the end.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define RR_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define RR_FN inline
#endif
#if defined(__clang__)
#define RR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define RR_NO_CONTRACT
#endif

namespace rr {

// The guard band: a corner takes part only with |u|, |v| <= kGuard pixels.  With kSubBits sub-pixel bits a snapped coordinate is at
// most 2^22 in magnitude, and so is 256 * a pixel index (width, height <= kMaxSide); differences stay at or below 2^23 and every
// product of an edge function at or below 2^46: all of coverage is exact in int64.
constexpr float kGuard = 16384.0f;
constexpr int kSubBits = 8;
constexpr float kSubScale = 256.0f;
constexpr int kMaxSide = 16384;
constexpr int kTile = 8;                   // the tile path draws kTile x kTile pixel centres per (view, face, tile) pair
constexpr int kSmallSide = 4;              // a face whose box holds at most kSmallSide x kSmallSide centres is drawn by one lane
constexpr unsigned long long kEmptyKey = ~0ull;
constexpr long long kCompareClamp = 1ll << 40;         // the most one pixel adds to sum_q, in units of 2^-20 m (a million metres)

struct Camera {
    float fx, fy, cx, cy;
    float min_depth;                       // > 0: a corner takes part iff z > min_depth; a pixel is written iff its z > min_depth
    float max_depth;                       // > 0: a pixel whose z > max_depth is not written; <= 0: no far bound
    int width, height;                     // images are [width][height], width-major
};

// One corner: the camera point R^T (p - t) in the fma shape of cr::project, u = fma(fx, c0 / z, cx), v = fma(fy, c1 / z, cy), then
// X = (int)rintf(u * 256), Y likewise (the product is exact; half to even).  false where z is not > min_depth or |u| or |v| is
// not <= kGuard - compared as floats before the conversion, so that a NaN fails and nothing out of range is ever converted.
RR_FN bool snap_corner(const Camera& c, const float* T, const float* p, int& X, int& Y, float& z) {
    RR_NO_CONTRACT
    const float q0 = p[0] - T[3], q1 = p[1] - T[7], q2 = p[2] - T[11];
    const float c0 = __builtin_fmaf(T[8], q2, __builtin_fmaf(T[4], q1, T[0] * q0));
    const float c1 = __builtin_fmaf(T[9], q2, __builtin_fmaf(T[5], q1, T[1] * q0));
    const float c2 = __builtin_fmaf(T[10], q2, __builtin_fmaf(T[6], q1, T[2] * q0));
    z = c2;
    if (!(z > c.min_depth)) return false;
    const float u = __builtin_fmaf(c.fx, c0 / z, c.cx);
    const float v = __builtin_fmaf(c.fy, c1 / z, c.cy);
    if (!(__builtin_fabsf(u) <= kGuard && __builtin_fabsf(v) <= kGuard)) return false;
    X = (int)__builtin_rintf(u * kSubScale);
    Y = (int)__builtin_rintf(v * kSubScale);
    return true;
}

// A face that takes part in a view, oriented: A >= 0, corners 1 and 2 swapped (with their depths) where the input's A was negative,
// so both windings of a triangle are one and the same Face.  A == 0 covers nothing.
struct Face {
    int X[3], Y[3];
    float z[3];
    long long A;                           // (X1 - X0)(Y2 - Y0) - (Y1 - Y0)(X2 - X0) >= 0
};

RR_FN long long edge_fn(int ax, int ay, int bx, int by, int px, int py) {
    return (long long)(bx - ax) * (long long)(py - ay) - (long long)(by - ay) * (long long)(px - ax);
}

// false: the face is dropped for this view (a corner behind min_depth, outside the guard band, or not a number)
RR_FN bool setup_face(const Camera& c, const float* T, const float* p0, const float* p1, const float* p2, Face& f) {
    if (!snap_corner(c, T, p0, f.X[0], f.Y[0], f.z[0])) return false;
    if (!snap_corner(c, T, p1, f.X[1], f.Y[1], f.z[1])) return false;
    if (!snap_corner(c, T, p2, f.X[2], f.Y[2], f.z[2])) return false;
    f.A = edge_fn(f.X[0], f.Y[0], f.X[1], f.Y[1], f.X[2], f.Y[2]);
    if (f.A < 0) {
        const int x = f.X[1], y = f.Y[1];
        const float z = f.z[1];
        f.X[1] = f.X[2]; f.Y[1] = f.Y[2]; f.z[1] = f.z[2];
        f.X[2] = x; f.Y[2] = y; f.z[2] = z;
        f.A = -f.A;
    }
    return true;
}

// The pixel centres a face can cover: w0 <= w <= w1, h0 <= h <= h1, the bounding box of the snapped corners rounded inwards to
// whole pixels and clipped to the image; empty (w0 > w1 or h0 > h1) where no centre is inside, and for A == 0.
struct Box {
    int w0, w1, h0, h1;
};
RR_FN int min3(int a, int b, int c) { return a < b ? (a < c ? a : c) : (b < c ? b : c); }
RR_FN int max3(int a, int b, int c) { return a > b ? (a > c ? a : c) : (b > c ? b : c); }
RR_FN Box pixel_box(const Camera& c, const Face& f) {
    Box b;
    if (f.A == 0) { b.w0 = b.h0 = 0; b.w1 = b.h1 = -1; return b; }
    const int mask = (1 << kSubBits) - 1;
    b.w0 = (min3(f.X[0], f.X[1], f.X[2]) + mask) >> kSubBits;          // arithmetic shifts: ceiling and floor of X / 256
    b.w1 = max3(f.X[0], f.X[1], f.X[2]) >> kSubBits;
    b.h0 = (min3(f.Y[0], f.Y[1], f.Y[2]) + mask) >> kSubBits;
    b.h1 = max3(f.Y[0], f.Y[1], f.Y[2]) >> kSubBits;
    b.w0 = b.w0 < 0 ? 0 : b.w0;
    b.h0 = b.h0 < 0 ? 0 : b.h0;
    b.w1 = b.w1 > c.width - 1 ? c.width - 1 : b.w1;
    b.h1 = b.h1 > c.height - 1 ? c.height - 1 : b.h1;
    return b;
}
RR_FN bool box_empty(const Box& b) { return b.w0 > b.w1 || b.h0 > b.h1; }
RR_FN bool box_small(const Box& b) { return b.w1 - b.w0 < kSmallSide && b.h1 - b.h0 < kSmallSide; }

// the tie rule: a centre exactly on the edge a -> b belongs to the face iff the edge's direction is lexicographically positive
RR_FN bool edge_owns_ties(int ax, int ay, int bx, int by) {
    const int dx = bx - ax, dy = by - ay;
    return dy > 0 || (dy == 0 && dx > 0);
}

// Whether the face covers the centre of pixel (w, h), P = (256 w, 256 h); E[i] = the edge function of the edge opposite corner i
// (1 -> 2, 2 -> 0, 0 -> 1), E[0] + E[1] + E[2] == A.  Covered iff every E > 0, or E == 0 on an edge that owns its ties.
RR_FN bool covers(const Face& f, int w, int h, long long (&E)[3]) {
    if (f.A == 0) return false;
    const int px = w << kSubBits, py = h << kSubBits;
    bool in = true;
#if defined(__clang__)
#pragma unroll
#endif
    for (int i = 0; i < 3; ++i) {
        const int a = (i + 1) % 3, b = (i + 2) % 3;
        E[i] = edge_fn(f.X[a], f.Y[a], f.X[b], f.Y[b], px, py);
        in = in && (E[i] > 0 || (E[i] == 0 && edge_owns_ties(f.X[a], f.Y[a], f.X[b], f.Y[b])));
    }
    return in;
}

// The depth of a covered pixel, perspective-correct, a function of (face, pixel) alone.  In float64, every operation rounded on its own:
//   i_k = 1.0 / (double)z_k;  l_k = (double)E_k / (double)A   (both conversions exact);  r = (l_0 i_0 + l_1 i_1) + l_2 i_2;
//   z = (float)(1.0 / r)
RR_FN float depth_at(const Face& f, const long long (&E)[3]) {
    RR_NO_CONTRACT
    const double A = (double)f.A;
    const double i0 = 1.0 / (double)f.z[0], i1 = 1.0 / (double)f.z[1], i2 = 1.0 / (double)f.z[2];
    const double l0 = (double)E[0] / A, l1 = (double)E[1] / A, l2 = (double)E[2] / A;
    const double t0 = l0 * i0, t1 = l1 * i1, t2 = l2 * i2;
    const double t01 = t0 + t1;
    const double r = t01 + t2;
    return (float)(1.0 / r);
}

// a pixel is written iff its depth is finite, > min_depth and - with max_depth > 0 - not > max_depth
RR_FN bool depth_written(const Camera& c, float z) {
    if (!(z > c.min_depth && z <= 3.402823466e+38f)) return false;
    return !(c.max_depth > 0.0f && z > c.max_depth);
}

// The z-buffer key: the smallest wins.  The bits of a positive float order as the float does; equal depths go to the smaller face.
RR_FN unsigned long long make_key(float z, int face) {
    unsigned bits;
    __builtin_memcpy(&bits, &z, sizeof(bits));
    return ((unsigned long long)bits << 32) | (unsigned)face;
}
RR_FN float key_depth(unsigned long long key) {
    const unsigned bits = (unsigned)(key >> 32);
    float z;
    __builtin_memcpy(&z, &bits, sizeof(z));
    return key == kEmptyKey ? 0.0f : z;
}
RR_FN int key_face(unsigned long long key) { return key == kEmptyKey ? -1 : (int)(unsigned)(key & 0xffffffffull); }

// ---- the comparison of two depth values of a pixel: > 0 means measured (a NaN is not) -------------------------------------------------
enum { kBoth = 0, kAOnly = 1, kBOnly = 2, kNeither = 3 };
RR_FN int compare_class(float a, float b) {
    const bool ma = a > 0.0f, mb = b > 0.0f;
    return ma ? (mb ? kBoth : kAOnly) : (mb ? kBOnly : kNeither);
}
// |a - b| of a pixel both measured, in units of 2^-20 m: one rounded float32 subtraction, then rint((double)x * 2^20), half to even
// (the product is exact); a difference that is not finite counts 0, one pixel is clamped at kCompareClamp.
RR_FN long long compare_q(float a, float b) {
    RR_NO_CONTRACT
    const float d = __builtin_fabsf(a - b);
    if (!(d <= 3.402823466e+38f)) return 0;
    const double q = (double)d * 0x1p20;
    if (q >= (double)kCompareClamp) return kCompareClamp;
    return (long long)__builtin_rint(q);
}

}  // namespace rr
