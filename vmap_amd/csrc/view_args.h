// view_args.h - the argument block of the view kernels (view_kernels.h: view_count, view_scan, view_emit, view_plan, view_composite;
// query_split_kernels.h: field_query_seg_s32; query_kernels.h: field_query_seg_gen).  Plain C++: the C ABI unit fills it, the two
// kernel units launch with it.
#pragma once
#include "launch_geometry.h"
#include "view_geometry.h"

namespace vv {

struct ViewArgs {
    vg::Camera cam;                        // cam.samples: the launched group's sample count (field kernels); a one-group view's S
    int n_obj, nb;                         // nb = blocks of kViewBlock pixels in [pix_begin, pix_end)
    long long pix_begin, pix_end;          // the call's pixel range (pixel index w * height + h)
    const float* boxes;                    // [n_obj][15] centre, R (row-major, columns = axes), full extent
    const float* centers;                  // [n_obj][3] field-frame centres
    const float* scale; long long scale_so;   // pe.scale of object k = scale[k * scale_so]
    const char* wimg;                      // workspace: [n_obj] parameter images (Img32s at hidden 32)
    long long* blk;                        // workspace: [n_obj * nb] hits per block, then their exclusive prefix
    int* plan;                             // workspace: [plan_cap][4] (object, first chunk, end chunk, 0)
    int plan_cap;                          // entries the plan section holds (vl::SceneLayout)
    long long* offsets;                    // [n_obj + 1] pair offsets
    vg::Pair* pairs; long long cap;        // [cap] pair records, ordered by (object, pixel)
    float* occ;                            // [samples of all pairs]
    float* rgb;                            // [samples of all pairs][3]
    float* depth; float* color; float* opacity; int* instance;      // [width * height] (x 3)
    int* overflow;                         // [1] pixels that hit more than kViewMaxHits boxes (added to)
    // Field groups, read by view_count / _emit / _plan / _composite.  Objects [g_end[g - 1], g_end[g]) belong to group g (unused
    // groups: n_obj, so a view of one group is g_end = {n, n, n, n}); an object's sample count is its group's; sample s of pair pr of
    // group g is element pr * g_samples[g] + g_shift[g] + s of occ; a plan entry of group g holds g_per[g] chunks.
    // The field kernels never read these: each group's launch gets an argument block of its own (vl::view_field).
    int g_end[kViewMaxGroups], g_samples[kViewMaxGroups];
    long long g_shift[kViewMaxGroups], g_per[kViewMaxGroups];
};

}  // namespace vv
