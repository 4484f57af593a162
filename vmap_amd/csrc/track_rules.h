// track_rules.h - the rules of the instance tracker (the reference's track_instance, utils.py:274-382): what becomes of a detection
// of one frame given the statistics of its pixels and, for every known instance of its class, the number of its points inside that
// instance's box.  Plain inline C++ with no HIP include: the track kernels (track_kernels.h) and the host program of the tests
// (tests/tools/track_rules_host.cpp) compile the same functions.  What a pixel's row, depth, world point and voxel key are, the
// erosion rule and the inside test are filter_rules.h's and are not repeated here.  The track section of include/vmapstep.h is the
// contract.
#pragma once

#include "filter_rules.h"

namespace tr {

constexpr int kRowInts = 9;                // a result row: d, status, class, persistent id, pixels, valid, inside, eroded, eroded_valid
constexpr int kHeadInts = 4;               // in front of the rows: n_rows, overflow, n_keys, out_of_grid
constexpr int kStatInts = 4;               // pixels, valid, eroded, eroded_valid
constexpr int kMaxDet = 4096;              // detection rows of one frame
constexpr int kMaxPairs = 65536;           // (detection, candidate) pairs of one frame
constexpr int kRatioOne = 65536;           // match_ratio = 1 as ratio_q

// The statuses are the filter's numbers (UNSURE and MIXED do not occur): one label rule and one emit rule serve both.
enum Status : int {
    ABSENT = fr::ABSENT,                   // no pixel carries the row
    NEW = fr::NEW,                         // no candidate matched: registered under id next_id + rank: label = id
    MERGED = fr::MERGED,                   // the first candidate past the ratio: -1 where valid and outside its old box, else its id
    BACKGROUND = fr::BACKGROUND,           // row 0, or its class is in the background list: label 0
    FEW_POINTS = fr::FEW_POINTS,           // eroded_valid <= min_points: label 0
    SMALL = fr::SMALL,                     // eroded <= min_pixels: label 0
    NEW_NO_BOX = fr::NEW_NO_BOX,           // new, but its cloud has no box (the host's verdict after the search): label 0
};

// frame: the filter's rules of the frame, with id_shift = det_shift and max_ids = max_det, so that fr::shifted_id is the detection row
struct Rules {
    fr::Rules frame;
    int max_ids;                           // persistent ids lie in [1, max_ids)
    int ratio_q;                           // round(match_ratio * 65536)
    int next_id;                           // the id of the frame's first NEW detection
    int n_det;                             // rows [0, n_det) have a class
};

// The statistics of one detection row over the frame.
struct Stats {
    int pixels, valid, eroded, eroded_valid;
};

// inside / valid > match_ratio, in integers: counts near 2^31 need the 64-bit products
IR_FN bool matches(int inside, int valid, int ratio_q) { return ((long long)inside << 16) > (long long)ratio_q * (long long)valid; }

// The conditions in the reference's order (utils.py:284-340).  inside[j]: the row's valid pixels inside the box of candidate j, the
// candidates in ascending id; *match = the first candidate past the ratio (the reference's break), or -1.
IR_FN int decide(const Rules& r, int d, int cls, const Stats& s, const int* inside, int n_cand, int* match) {
    *match = -1;
    if (s.pixels <= 0) return ABSENT;
    bool background = d == 0;
    for (int k = 0; k < r.frame.n_background; ++k) background = background || r.frame.background[k] == cls;
    if (background) return BACKGROUND;
    if (s.eroded <= r.frame.min_pixels) return SMALL;
    if (s.eroded_valid <= r.frame.min_points) return FEW_POINTS;
    for (int j = 0; j < n_cand; ++j)
        if (matches(inside[j], s.valid, r.ratio_q)) {
            *match = j;
            return MERGED;
        }
    return NEW;
}

// the label of a pixel of a detection with persistent id `id`: `valid` and `inside` (against the matched instance's OLD box) matter
// for MERGED alone; every status that is not the tracker's gives 0
IR_FN int label_of(int id, int status, bool valid, bool inside) {
    return status == NEW || status == MERGED ? fr::label_of(id, status, valid, inside) : 0;
}

// whether a pixel's point goes to the cloud of its detection's persistent id; INSIDE is against the matched instance's old box
IR_FN bool emits(int status, int flags) { return fr::emits(status, flags); }

}  // namespace tr
