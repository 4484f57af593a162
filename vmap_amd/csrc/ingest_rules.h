// ingest_rules.h - the rules of frame ingest: what becomes of an instance id given the statistics of its pixels (kept with an enlarged
// 2-D box, or relabelled to background), and what becomes of a pixel's depth and label.  Plain inline C++ with no HIP include: the
// ingest kernels (ingest_kernels.h) and the host program of the tests (tests/tools/ingest_rules_host.cpp) compile the same functions,
// so that the host program's output is what the device must produce bit for bit.
//
// The arithmetic is the reference's (dataset.py:93-133, utils.py:36-57, image_transforms.py:13-33) in [W, H] terms: u = column index,
// v = row index of the [H, W] image the files hold.  All of it is integer except the margin, which the reference computes on 0-dim
// int64 tensors and torch therefore evaluates in float32: trunc(float32(0.5 * scale) * float32(extent)); and the depth, one float32
// product.  The ingest section of include/vmapstep.h is the contract.
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define IR_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define IR_FN inline
#endif

namespace ir {

constexpr int kMaxClasses = 64;            // background classes a call can name (vmapstep_ingest_cfg::background_classes)
constexpr int kRowInts = 8;                // a result row: id, status, count, box[4], class

enum Status : int {
    ABSENT = 0,                            // no pixel carries the id (only id 0 is reported in this state)
    KEPT = 1,
    BACKGROUND = 2,                        // its class is in the background list
    SMALL = 3,                             // an extent <= min_box
    ZERO_MARGIN = 4,                       // the enlargement margin truncates to 0 along u or v
    MIXED = 5,                             // its pixels carry more than one class
};

struct Rules {
    int width, height;
    float half_scale;                      // float32(0.5 * bbox_scale)
    int min_box;                           // < 0: no size test
    int n_background;
    int background[kMaxClasses];
    float depth_scale, max_depth;
};

// The statistics of one id over the frame: pixel count, inclusive extremes of u and v, extremes of the class.
struct Stats {
    int count, u_min, u_max, v_min, v_max, c_min, c_max;
};

struct Decision {
    int status;
    int box[4];                            // u low, u high, v low, v high (ObjectKeyframes.write's order)
    int cls;
};

IR_FN int margin_of(float half_scale, int extent) { return (int)(half_scale * (float)extent); }

IR_FN int clip_to(int x, int hi) { return x < 0 ? 0 : x > hi ? hi : x; }

// id 0 always reports the full-frame box (dataset.py:133), whatever its status; an id that is not KEPT reports the box of zeros.
IR_FN Decision decide(const Rules& r, int id, const Stats& s) {
    Decision d;
    d.status = ABSENT;
    d.box[0] = d.box[1] = d.box[2] = d.box[3] = 0;
    d.cls = 0;
    if (s.count > 0) {
        const int u0 = s.u_min, u1 = s.u_max + 1, v0 = s.v_min, v1 = s.v_max + 1;
        d.cls = s.c_min;
        bool background = false;
        for (int k = 0; k < r.n_background; ++k) background = background || r.background[k] == s.c_min;
        const int mu = margin_of(r.half_scale, u1 - u0), mv = margin_of(r.half_scale, v1 - v0);
        if (s.c_min != s.c_max) d.status = MIXED;
        else if (background) d.status = BACKGROUND;
        else if (u1 - u0 <= r.min_box || v1 - v0 <= r.min_box) d.status = SMALL;
        else if (mu == 0 || mv == 0) d.status = ZERO_MARGIN;
        else {
            d.status = KEPT;
            d.box[0] = clip_to(u0 - mu, r.width - 1);
            d.box[1] = clip_to(u1 + mu, r.width - 1);
            d.box[2] = clip_to(v0 - mv, r.height - 1);
            d.box[3] = clip_to(v1 + mv, r.height - 1);
        }
    }
    if (id == 0) {
        d.box[0] = 0; d.box[1] = r.width; d.box[2] = 0; d.box[3] = r.height;
    }
    return d;
}

// image_transforms.py:13-33: scale, then zero what lies beyond max_depth (a NaN stays a NaN, as the comparison leaves it)
IR_FN float depth_of(float raw, float depth_scale, float max_depth) {
    const float d = raw * depth_scale;
    return d > max_depth ? 0.0f : d;
}

// dataset.py:130: an instance that is not kept becomes background
IR_FN int label_of(int id, int status) { return status == KEPT ? id : 0; }

}  // namespace ir
