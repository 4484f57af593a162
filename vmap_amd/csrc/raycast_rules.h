// raycast_rules.h - the rule of the TSDF ray cast: what one pixel of a depth, normal and colour image of a truncated signed distance
// volume (tsdf_rules.h) holds.  Plain inline C++ with no HIP include: the kernels (raycast_kernels.h) and the host program of the tests
// (tests/tools/raycast_rules_host.cpp) compile the same functions, so that the host program's output is what the device must produce
// bit for bit.  This header is the definition; the raycast section of include/vmapstep.h repeats it in prose.
//
// The rounding contract is cull_rules.h's: float32 throughout; every fma below is ONE fused operation, every other operation is rounded
// on its own (contraction is switched off per function), divisions and square roots are IEEE, rintf rounds half to even.
//
// Ray.  Pixel (w, h) of a [width][height] image looks along ((w - cx) / fx, (h - cy) / fy, 1) = (u, v, 1) in the camera frame - the
// inverse of cr::project's convention - and is parameterised by z, the depth along the optical axis, which is what a depth image
// stores.  The host composes M = A^-1 T_wc in float64 (A: the volume's affine made 4 x 4, voxel index -> world) and rounds it ONCE to
// 12 float32 per view (rows [R | o]).  The contract starts from those 12 floats: the index-space origin is o = M[:, 3], the
// index-space direction per unit z is d_r = fma(M[4r+1], v, fma(M[4r], u, M[4r+2])).  A view whose 12 floats are all zero is an unused
// slot: every pixel is a miss.
//
// Range.  A slab test of o + d z against [0, nx-1] x [0, ny-1] x [0, nz-1], intersected with [min_depth, max_depth].  An axis with
// d == 0 takes its own branch: o outside on that axis is a miss, otherwise no constraint; no infinity is relied on.
//
// Samples.  z_n = fma((float)n, dz, z0), n = 0, 1, ... (never accumulated), dz = step / sqrt(fma(u, u, fma(v, v, 1))): `step` is
// metres ALONG THE RAY.  The ray has left the range at the first n with !(z_n <= z1); it takes at most max_steps (< 2^24: (float)n is
// exact) samples.
//
// Value at a sample p = fma(d, z, o) per axis.  A p outside [0, n-1] on some axis (rounding at the slab's faces, or a NaN) is an invalid
// sample.  Otherwise trilinear over the cell i0 = min((int)floor(p), n - 2), t = p - (float)i0 per axis, every lerp written
// fma(t, b - a, a), along k, then j, then i: a cell whose eight values are exactly 1.0 yields exactly 1.0 (b - a = 0).  The sample is
// VALID iff all eight corners have weight >= min_weight (a NaN weight fails).
//
// The march keeps ONE piece of state: the previous sample, if it was valid and > 0.
//   invalid sample                     -> the state is cleared
//   valid, f <= 0, state set           -> HIT at z* = fma(z_n - z_prev, f_prev / (f_prev - f), z_prev)
//   valid, f < 0, no state             -> the ray ends BEHIND a surface: what lies beyond is not seen
//   valid, f == 0 (or NaN), no state   -> the state stays cleared and the ray goes on: a zero is neither in front of a surface nor behind
//   valid, f > 0                       -> the state is set to (f, z_n)
//
// Brick classes (exact empty-space skipping).  The cells are cut into bricks of 8 x 8 x 8: cell (i, j, k) belongs to brick
// (i >> 3, j >> 3, k >> 3); brick (a, b, c) spans voxels 8a .. min(8a + 8, nx - 1) and so on (the apron voxel is shared with the
// neighbour).  One byte per brick, [bx][by][bz] in C order, b_ = ceil((n_ - 1) / 8):
//   EMPTY  no cell of the brick has eight valid corners           -> every sample in it is invalid
//   FREE   every voxel of the brick is valid and exactly 1.0f     -> every sample in it is valid and exactly 1.0 (the lerp form above)
//   MIXED  anything else                                          -> sampled in full
// sample_classed takes the result from the class and gathers nothing in an EMPTY or FREE brick.  THE property: march() with a class
// table and with none (null) produce the same bits for every output, whatever the volume holds.  No leap over several samples is made:
// every sample n is visited, a classed one costs one byte.
#pragma once

#include "cull_rules.h"

namespace rc {

enum Status : unsigned char { MISS = 0, HIT = 1, LEFT = 2, BEHIND = 3, STEPS = 4 };
enum BrickClass : unsigned char { MIXED = 0, EMPTY = 1, FREE = 2 };
constexpr int kBrickShift = 3;             // bricks of 8 x 8 x 8 cells
constexpr int kMaxStepsLimit = 1 << 24;    // max_steps < this: (float)n is exact

struct Rules {
    float fx, fy, cx, cy;
    float min_depth, max_depth;            // the ray is cast over min_depth <= z <= max_depth
    float step;                            // metres along the ray between samples, > 0
    float min_weight;                      // a voxel is valid iff weight >= min_weight
    int width, height;                     // images are [width][height], width-major
    int max_steps;                         // 1 .. 2^24 - 1
    int nx, ny, nz;                        // the volume, each >= 2
    float N[9];                            // float32 rounding of A^-T (rows): index-space gradient -> world normal
};

struct Volume {
    const float* tsdf;                     // [nx][ny][nz]
    const float* weight;                   // [nx][ny][nz]
    const float* color;                    // [nx*ny*nz][4] r, g, b, wc, or null
};

CR_FN int brick_dim(int n) { return (n - 1 + 7) >> kBrickShift; }
CR_FN bool voxel_valid(float w, float min_weight) { return w >= min_weight; }
CR_FN bool voxel_free(float d) { return d == 1.0f; }
// the class of a brick from two facts: some cell of it has eight valid corners; every voxel of it is valid and exactly 1.0f
CR_FN unsigned char classify(bool any_cell, bool all_free) { return !any_cell ? (unsigned char)EMPTY : all_free ? (unsigned char)FREE : (unsigned char)MIXED; }

CR_FN bool unused_view(const float* M) {
    bool any = false;
    for (int e = 0; e < 12; ++e) any = any || M[e] != 0.0f;
    return !any;
}

struct Ray {
    float o[3], d[3];                      // index space: p(z) = o + d z
    float z0, z1, dz;
};

// false = a miss: the unused slot, the slab test or the depth range
CR_FN bool make_ray(const Rules& r, const float* M, int w, int h, Ray& ray) {
    CR_NO_CONTRACT
    if (unused_view(M)) return false;
    const float u = ((float)w - r.cx) / r.fx, v = ((float)h - r.cy) / r.fy;
    float z0 = r.min_depth, z1 = r.max_depth;
    const int dims[3] = {r.nx, r.ny, r.nz};
    for (int a = 0; a < 3; ++a) {
        const float o = M[4 * a + 3];
        const float d = __builtin_fmaf(M[4 * a + 1], v, __builtin_fmaf(M[4 * a], u, M[4 * a + 2]));
        const float hi = (float)(dims[a] - 1);
        ray.o[a] = o;
        ray.d[a] = d;
        if (d == 0.0f) {
            if (!(o >= 0.0f && o <= hi)) return false;
            continue;
        }
        const float ta = (0.0f - o) / d, tb = (hi - o) / d;
        z0 = __builtin_fmaxf(z0, __builtin_fminf(ta, tb));
        z1 = __builtin_fminf(z1, __builtin_fmaxf(ta, tb));
    }
    if (!(z0 <= z1)) return false;
    ray.z0 = z0;
    ray.z1 = z1;
    ray.dz = r.step / __builtin_sqrtf(__builtin_fmaf(u, u, __builtin_fmaf(v, v, 1.0f)));
    return true;
}

struct Cell {
    int i, j, k;
    float ti, tj, tk;
};

// false = p is outside the volume (or a NaN)
CR_FN bool locate_axis(float p, int n, int& i0, float& t) {
    CR_NO_CONTRACT
    if (!(p >= 0.0f && p <= (float)(n - 1))) return false;
    const int f = (int)__builtin_floorf(p);
    i0 = f < n - 2 ? f : n - 2;
    t = p - (float)i0;
    return true;
}

CR_FN bool locate(const Rules& r, float px, float py, float pz, Cell& c) {
    return locate_axis(px, r.nx, c.i, c.ti) && locate_axis(py, r.ny, c.j, c.tj) && locate_axis(pz, r.nz, c.k, c.tk);
}

CR_FN long long voxel_offset(const Rules& r, int i, int j, int k) { return ((long long)i * r.ny + j) * r.nz + k; }

// the trilinear value of a located cell; false = one of the eight corners is not valid
CR_FN bool sample_cell(const Rules& r, const Volume& vol, const Cell& c, float& f) {
    CR_NO_CONTRACT
    const long long p = voxel_offset(r, c.i, c.j, c.k), sj = r.nz, si = (long long)r.ny * r.nz;
    const long long at[4] = {p, p + sj, p + si, p + si + sj};
    float line[4];
    bool ok = true;
    for (int e = 0; e < 4; ++e) {
        ok = ok && voxel_valid(vol.weight[at[e]], r.min_weight) && voxel_valid(vol.weight[at[e] + 1], r.min_weight);
        const float a = vol.tsdf[at[e]], b = vol.tsdf[at[e] + 1];
        line[e] = __builtin_fmaf(c.tk, b - a, a);
    }
    if (!ok) return false;
    const float f0 = __builtin_fmaf(c.tj, line[1] - line[0], line[0]);
    const float f1 = __builtin_fmaf(c.tj, line[3] - line[2], line[2]);
    f = __builtin_fmaf(c.ti, f1 - f0, f0);
    return true;
}

// the plain sample: valid and its value
CR_FN bool sample(const Rules& r, const Volume& vol, float px, float py, float pz, float& f) {
    Cell c;
    return locate(r, px, py, pz, c) && sample_cell(r, vol, c, f);
}

// the class-aware sample; bricks == null is the plain one
CR_FN bool sample_classed(const Rules& r, const Volume& vol, const unsigned char* bricks, float px, float py, float pz, float& f) {
    Cell c;
    if (!locate(r, px, py, pz, c)) return false;
    if (bricks) {
        const unsigned char cls =
            bricks[((c.i >> kBrickShift) * brick_dim(r.ny) + (c.j >> kBrickShift)) * brick_dim(r.nz) + (c.k >> kBrickShift)];
        if (cls == EMPTY) return false;
        if (cls == FREE) {
            f = 1.0f;
            return true;
        }
    }
    return sample_cell(r, vol, c, f);
}

struct March {
    int n;                                 // the next sample
    bool have;                             // the previous sample was valid and > 0
    float f_prev, z_prev;
};

CR_FN void march_begin(March& m) {
    m.n = 0;
    m.have = false;
    m.f_prev = m.z_prev = 0.0f;
}

// One sample of the march: -1 = go on, otherwise the ray's status; z_hit is set with HIT.  The kernel calls this per lane under a
// wave-wide vote, march() below in a loop: the same function.
CR_FN int march_step(const Rules& r, const Volume& vol, const unsigned char* bricks, const Ray& ray, March& m, float& z_hit) {
    CR_NO_CONTRACT
    const float z = __builtin_fmaf((float)m.n, ray.dz, ray.z0);
    if (!(z <= ray.z1)) return LEFT;
    if (m.n >= r.max_steps) return STEPS;
    m.n += 1;
    const float px = __builtin_fmaf(ray.d[0], z, ray.o[0]), py = __builtin_fmaf(ray.d[1], z, ray.o[1]), pz = __builtin_fmaf(ray.d[2], z, ray.o[2]);
    float f = 0.0f;
    if (!sample_classed(r, vol, bricks, px, py, pz, f)) {
        m.have = false;
        return -1;
    }
    if (m.have && f <= 0.0f) {
        z_hit = __builtin_fmaf(z - m.z_prev, m.f_prev / (m.f_prev - f), m.z_prev);
        return HIT;
    }
    if (f > 0.0f) {
        m.have = true;
        m.f_prev = f;
        m.z_prev = z;
        return -1;
    }
    m.have = false;
    return f < 0.0f ? (int)BEHIND : -1;
}

// the whole ray; bricks may be null
CR_FN int march(const Rules& r, const Volume& vol, const unsigned char* bricks, const Ray& ray, float& z_hit) {
    March m;
    march_begin(m);
    for (;;) {
        const int s = march_step(r, vol, bricks, ray, m, z_hit);
        if (s >= 0) return s;
    }
}

// The world normal at the hit: central differences of six plain samples at p* +- 1 voxel along each index axis, g_a = f(+) - f(-),
// mapped by N (n_r = fma(N[3r+2], g2, fma(N[3r+1], g1, N[3r] * g0))) and divided by its length sqrt(fma(n0, n0, fma(n1, n1, n2 * n2))).
// All zero when one of the six samples is invalid or outside, or when the length is not > 0.  It points to increasing TSDF: free space.
CR_FN void hit_normal(const Rules& r, const Volume& vol, const Ray& ray, float z, float* out) {
    CR_NO_CONTRACT
    out[0] = out[1] = out[2] = 0.0f;
    const float p[3] = {__builtin_fmaf(ray.d[0], z, ray.o[0]), __builtin_fmaf(ray.d[1], z, ray.o[1]), __builtin_fmaf(ray.d[2], z, ray.o[2])};
    float g[3];
    for (int a = 0; a < 3; ++a) {
        float q[3] = {p[0], p[1], p[2]};
        float fp = 0.0f, fm = 0.0f;
        q[a] = p[a] + 1.0f;
        if (!sample(r, vol, q[0], q[1], q[2], fp)) return;
        q[a] = p[a] - 1.0f;
        if (!sample(r, vol, q[0], q[1], q[2], fm)) return;
        g[a] = fp - fm;
    }
    float n[3];
    for (int a = 0; a < 3; ++a) n[a] = __builtin_fmaf(r.N[3 * a + 2], g[2], __builtin_fmaf(r.N[3 * a + 1], g[1], r.N[3 * a] * g[0]));
    const float len = __builtin_sqrtf(__builtin_fmaf(n[0], n[0], __builtin_fmaf(n[1], n[1], n[2] * n[2])));
    if (!(len > 0.0f)) return;
    for (int a = 0; a < 3; ++a) out[a] = n[a] / len;
}

// The colour at the hit: over the corners of p*'s cell whose colour weight wc > 0, in the order (di, dj, dk) with dk fastest, the
// trilinear weight q = (qi * qj) * qk (q_ = t or 1 - t) accumulates s = s + q and c = fma(q, colour, c) per channel; the byte is
// rintf(c / s) clamped to 0 .. 255, byte 3 is 255.  All zero when no corner has colour, when s is not > 0, or when p* is outside.
CR_FN void hit_color(const Rules& r, const Volume& vol, const Ray& ray, float z, unsigned char* out) {
    CR_NO_CONTRACT
    out[0] = out[1] = out[2] = out[3] = 0;
    Cell c;
    if (!locate(r, __builtin_fmaf(ray.d[0], z, ray.o[0]), __builtin_fmaf(ray.d[1], z, ray.o[1]), __builtin_fmaf(ray.d[2], z, ray.o[2]), c)) return;
    const float qi[2] = {1.0f - c.ti, c.ti}, qj[2] = {1.0f - c.tj, c.tj}, qk[2] = {1.0f - c.tk, c.tk};
    float s = 0.0f, acc[3] = {0.0f, 0.0f, 0.0f};
    for (int e = 0; e < 8; ++e) {
        const int di = e >> 2, dj = (e >> 1) & 1, dk = e & 1;
        const float* px = vol.color + 4 * voxel_offset(r, c.i + di, c.j + dj, c.k + dk);
        if (!(px[3] > 0.0f)) continue;
        const float q = (qi[di] * qj[dj]) * qk[dk];
        s = s + q;
        for (int ch = 0; ch < 3; ++ch) acc[ch] = __builtin_fmaf(q, px[ch], acc[ch]);
    }
    if (!(s > 0.0f)) return;
    for (int ch = 0; ch < 3; ++ch) out[ch] = (unsigned char)__builtin_fminf(255.0f, __builtin_fmaxf(0.0f, __builtin_rintf(acc[ch] / s)));
    out[3] = 255;
}

// One pixel, whole: what the kernel's lane and the host program both do.  normal / color_out may be null (color_out needs vol.color).
CR_FN void cast_pixel(const Rules& r, const Volume& vol, const unsigned char* bricks, const float* M, int w, int h, float& depth,
                      unsigned char& status, float* normal, unsigned char* color_out) {
    Ray ray;
    float z = 0.0f;
    const int s = make_ray(r, M, w, h, ray) ? march(r, vol, bricks, ray, z) : (int)MISS;
    status = (unsigned char)s;
    depth = s == HIT ? z : 0.0f;
    if (normal) {
        normal[0] = normal[1] = normal[2] = 0.0f;
        if (s == HIT) hit_normal(r, vol, ray, z, normal);
    }
    if (color_out) {
        color_out[0] = color_out[1] = color_out[2] = color_out[3] = 0;
        if (s == HIT) hit_color(r, vol, ray, z, color_out);
    }
}

// The class of brick (a, b, c), cell by cell: the definition the tsdf_bricks kernel is held to.
CR_FN unsigned char brick_class(const Rules& r, const Volume& vol, int a, int b, int c) {
    const int i1 = 8 * a + 8 < r.nx - 1 ? 8 * a + 8 : r.nx - 1, j1 = 8 * b + 8 < r.ny - 1 ? 8 * b + 8 : r.ny - 1,
              k1 = 8 * c + 8 < r.nz - 1 ? 8 * c + 8 : r.nz - 1;
    bool any_cell = false, all_free = true;
    for (int i = 8 * a; i <= i1; ++i)
        for (int j = 8 * b; j <= j1; ++j)
            for (int k = 8 * c; k <= k1; ++k) {
                const long long p = voxel_offset(r, i, j, k);
                all_free = all_free && voxel_valid(vol.weight[p], r.min_weight) && voxel_free(vol.tsdf[p]);
                if (i == i1 || j == j1 || k == k1) continue;       // the last voxel of an axis starts no cell of this brick
                bool cell = true;
                for (int e = 0; e < 8; ++e)
                    cell = cell && voxel_valid(vol.weight[voxel_offset(r, i + (e >> 2), j + ((e >> 1) & 1), k + (e & 1))], r.min_weight);
                any_cell = any_cell || cell;
            }
    return classify(any_cell, all_free);
}

}  // namespace rc
