// filter_rules.h - the rules of the instance filter (ScanNet's box_filter, utils.py:112-208): what a pixel's id, depth, world point and
// voxel key are, whether a point lies inside a registered box, and what becomes of an instance id given the statistics of its
// pixels.  Plain inline C++ with no HIP include: the filter kernels (filter_kernels.h) and the host program of the tests
// (tests/tools/filter_rules_host.cpp) compile the same functions, so that the host program's output is what the device must produce
// bit for bit.  Every product that feeds a sum is written out as __builtin_fmaf, as bounds_kernels.h::unproject_pixel does, so that
// no compiler decides where a rounding falls.  The filter section of include/vmapstep.h is the contract.
#pragma once

#include "ingest_rules.h"

namespace fr {

constexpr int kMaxClasses = ir::kMaxClasses;
constexpr int kRowInts = 8;                // a result row: id, status, class, pixels, valid, inside, eroded, eroded_valid
constexpr int kHeadInts = 4;               // in front of the rows: n_rows, overflow, n_keys, out_of_grid
constexpr int kBoxFloats = 16;             // a box-table row: centre[3], axis a[3], axis b[3], axis c[3], half extent[3], known flag
constexpr int kMaxIds = 32767;             // the id takes the 15 bits above bit 48 of a key
constexpr int kMaxRadius = 8;
constexpr int kKeyBias = 32768;            // a voxel coordinate lies in [-32768, 32767]

enum Status : int {
    ABSENT = 0,                            // no pixel carries the id
    NEW = 1,                               // registered by this frame: label = id
    MERGED = 2,                            // known, and some of its points lie inside its box: -1 where valid and outside, else id
    UNSURE = 3,                            // known, and none of its points lies inside its box: -1 everywhere
    BACKGROUND = 4,                        // its class is in the background list, or the id is 0: label 0
    FEW_POINTS = 5,                        // valid <= min_points: label 0
    SMALL = 6,                             // new, and its eroded mask has fewer than min_pixels pixels: label 0
    MIXED = 7,                             // its pixels carry more than one class: an error for the caller
    NEW_NO_BOX = 8,                        // new, but its cloud has no box (the host's verdict after the search): label 0
};

enum Flag : int { VALID = 1, INSIDE = 2, ERODED = 4 };     // the per-pixel flags filter_stats leaves for filter_emit

struct Camera {
    float fx, fy, cx, cy;
    float T[12];                           // rows 0..2 of t_wc
};

struct Rules {
    int width, height;
    float depth_scale, max_depth;
    Camera cam;
    float voxel;
    int id_shift, min_pixels, min_points, erode_radius, max_ids;
    int n_background;
    int background[kMaxClasses];
};

// The statistics of one id over the frame.
struct Stats {
    int pixels, c_min, c_max, valid, inside, eroded, eroded_valid;
};

struct Point {
    float x, y, z;
};

// raw + id_shift as a table row, or -1 where the id has none (the sum is taken in 64 bits: any int32 label is safe)
IR_FN int shifted_id(int raw, int id_shift, int max_ids) {
    const long long id = (long long)raw + (long long)id_shift;
    return id >= 0 && id < (long long)max_ids ? (int)id : -1;
}

// a NaN is not valid
IR_FN bool valid_depth(float d) { return d > 0.0f; }

// t_wc . ((u - cx) / fx . d, (v - cy) / fy . d, d, 1), u the column and v the row: unproject_pixel's expression order
IR_FN Point world_point(const Camera& c, int u, int v, float d) {
    const float xc = (((float)u - c.cx) / c.fx) * d;
    const float yc = (((float)v - c.cy) / c.fy) * d;
    Point p;
    p.x = __builtin_fmaf(c.T[0], xc, __builtin_fmaf(c.T[1], yc, __builtin_fmaf(c.T[2], d, c.T[3])));
    p.y = __builtin_fmaf(c.T[4], xc, __builtin_fmaf(c.T[5], yc, __builtin_fmaf(c.T[6], d, c.T[7])));
    p.z = __builtin_fmaf(c.T[8], xc, __builtin_fmaf(c.T[9], yc, __builtin_fmaf(c.T[10], d, c.T[11])));
    return p;
}

// floor(p / voxel) where it lies in [-32768, 32767] (compared as floats before the conversion, so that nothing out of an int's range
// is ever converted; a NaN fails)
IR_FN bool voxel_coord(float p, float voxel, int* k) {
    const float f = __builtin_floorf(p / voxel);
    if (!(f >= -32768.0f && f <= 32767.0f)) return false;
    *k = (int)f;
    return true;
}

IR_FN unsigned long long pack_key(int id, int kx, int ky, int kz) {
    return ((unsigned long long)id << 48) | ((unsigned long long)(kx + kKeyBias) << 32) | ((unsigned long long)(ky + kKeyBias) << 16) |
           (unsigned long long)(kz + kKeyBias);
}

// the key of point p of instance id; false where a coordinate leaves the grid (the point is then counted, not inserted)
IR_FN bool voxel_key(int id, const Point& p, float voxel, unsigned long long* key) {
    int kx = 0, ky = 0, kz = 0;
    const bool ok = voxel_coord(p.x, voxel, &kx) & voxel_coord(p.y, voxel, &ky) & voxel_coord(p.z, voxel, &kz);
    if (ok) *key = pack_key(id, kx, ky, kz);
    return ok;
}

IR_FN int key_id(unsigned long long key) { return (int)(key >> 48); }
IR_FN int key_coord(unsigned long long key, int axis) { return (int)((key >> (32 - 16 * axis)) & 0xffffull) - kKeyBias; }

// a key stands for the centre of its voxel
IR_FN float voxel_centre(int k, float voxel) { return __builtin_fmaf((float)k, voxel, 0.5f * voxel); }

IR_FN bool box_known(const float* row) { return row[15] != 0.0f; }

// |(p - centre) . axis| <= half extent on all three axes of a box-table row
IR_FN bool inside_box(const float* row, const Point& p) {
    const float dx = p.x - row[0], dy = p.y - row[1], dz = p.z - row[2];
    bool in = true;
    for (int a = 0; a < 3; ++a) {
        const float* ax = row + 3 + 3 * a;
        const float proj = __builtin_fmaf(ax[0], dx, __builtin_fmaf(ax[1], dy, ax[2] * dz));
        in = in && __builtin_fabsf(proj) <= row[12 + a];
    }
    return in;
}

// the conditions in the reference's order (utils.py:119, 126, 129-161, 181-185); the class test comes first, as in the loader
IR_FN int decide(const Rules& r, int id, const Stats& s, bool known) {
    if (s.pixels <= 0) return ABSENT;
    bool background = false;
    for (int k = 0; k < r.n_background; ++k) background = background || r.background[k] == s.c_min;
    if (s.c_min != s.c_max) return MIXED;
    if (background || id == 0) return BACKGROUND;
    if (s.valid <= r.min_points) return FEW_POINTS;
    if (known) return s.inside == 0 ? UNSURE : MERGED;
    return s.eroded < r.min_pixels ? SMALL : NEW;
}

// the label of a pixel of instance id: `valid` and `inside` (against the OLD box) matter for MERGED alone
IR_FN int label_of(int id, int status, bool valid, bool inside) {
    if (status == NEW) return id;
    if (status == UNSURE) return -1;
    if (status == MERGED) return valid && !inside ? -1 : id;
    return 0;
}

// whether a pixel's point goes to the cloud of its id
IR_FN bool emits(int status, int flags) {
    return (status == NEW && (flags & (VALID | ERODED)) == (VALID | ERODED)) || (status == MERGED && (flags & (VALID | INSIDE)) == (VALID | INSIDE));
}

}  // namespace fr
