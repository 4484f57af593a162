// wave_reduce.h - many sums of products over a half wave at once: a transposing (reduce-scatter) butterfly.
//
// half_sum32_hi_row (wave_ops.h) sums ONE value over the 32 lanes of a half wave and leaves the sum on every lane of the half's
// second row.  A caller that wants sixteen such sums and keeps each on one lane only (step_main_s32's B_layer.weight gradient:
// value c on lane c of that row) pays sixteen full butterflies for it.  half_dots32_scatter16 walks the SAME sum tree per value,
// but from the second step on a lane keeps one value of a pair and hands the other to its partner (two selects and one add that
// takes the partner's value through DPP): 16 + 8 + 4 + 2 steps instead of 64.
//
// The tree, and why the bits are those of the per-value form.  The values are products d * t.  Step 1 of the per-value form,
// x + x[l ^ 1] with x = d * t, is compiled as ONE fused multiply-add, fma(d, t, x[l ^ 1]): the two partners of a pair then hold
// DIFFERENT sums (each has its own product unrounded, the partner's rounded), and so, after the steps l ^ 2, 7 - l (row_half_mirror)
// and 15 - l (row_mirror), do the lanes of the two classes  k1 = l0 ^ l2 = 0 / 1  (l0..l3: the bits of lane & 15; both mirrors pair
// lanes of one class).  The per-value form keeps value c from lane c of the second row, i.e. class k1(c), and adds lane 15 of the
// first row (row_bcast:15), i.e. class 0.  Here:
//   * step 1 is the same fused multiply-add on every lane for every value (spelled as one, so that it does not depend on
//     what the compiler contracts);
//   * steps 2..4 use the same partners and halve the set of values with the keys  k2 = l1 ^ l2, k3 = l2 ^ l3, k4 = l3  (each key
//     differs between the two partners of its step and agrees between the partners of the later steps and of step 1's pairs).
//     Addition commutes bit for bit, so each kept sum is the one the per-value form has on that lane;
//   * two values are left per lane, the register slots b0 + 2 k2 + 4 k3 + 8 k4, b0 = 0 / 1: the lane's own class picks the one
//     it keeps (slot rs_slot(c) on lane c: the caller's value c is put there at compile time); the first row hands over, for the
//     same value, the sum of its class-0 lane (its own, or the one of lane l ^ 1) through v_permlane16_swap.
//
// Device body: DPP.  Host body (the CPU SIMT executor of tests/sim): wv::shfl with the same partners.
#pragma once
#include <wave_ops.h>   // resolved through -I: csrc/ (device) or tests/sim/ (CPU SIMT executor)

namespace wv {

// register slot whose value lane c (0..15) of a row ends up with
constexpr int rs_slot(int c) {
    return (((c >> 0) ^ (c >> 2)) & 1) | ((((c >> 1) ^ (c >> 2)) & 1) << 1) | ((((c >> 2) ^ (c >> 3)) & 1) << 2) | (((c >> 3) & 1) << 3);
}

#ifdef __HIP__
#define WV_RS_FN __device__ __forceinline__
// x of the partner lane; every lane of the row is a valid source under these controls, so bound_ctrl changes nothing and lets
// the move fold into the add that consumes it
template <int CTRL>
WV_RS_FN float rs_partner(float x, int) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(__float_as_uint(x), __float_as_uint(x), CTRL, 0xf, 0xf, true));
}
// x of the same lane of the row below (rows 1 / 3 <- rows 0 / 2): v_permlane16_swap exchanges the odd rows of its first operand
// with the even rows of its second
WV_RS_FN float rs_row_below(float x, int) {
    const unsigned u = __float_as_uint(x);
    const auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    return __uint_as_float(r[0]);
}
// x of lane 15 of the row below, on rows 1 / 3 (DPP row_bcast:15 under row mask 0xA; rows 0 / 2 keep x)
WV_RS_FN float rs_row_below15(float x, int) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(__float_as_uint(x), __float_as_uint(x), 0x142, 0xA, 0xF, false));
}
#else
#define WV_RS_FN inline
template <int CTRL>
WV_RS_FN float rs_partner(float x, int l) {
    return shfl(x, CTRL == 0xB1 ? l ^ 1 : CTRL == 0x4E ? l ^ 2 : CTRL == 0x141 ? (l & ~7) + (7 - (l & 7)) : (l & ~15) + (15 - (l & 15)));
}
WV_RS_FN float rs_row_below(float x, int l) { return shfl(x, l ^ 16); }
WV_RS_FN float rs_row_below15(float x, int l) { return shfl(x, (l & 16) ? (l & ~31) + 15 : l); }
#endif

// step 1 of either form: this lane's product unrounded + the partner's product
WV_RS_FN float rs_first(float d, float t, int lane) { return __builtin_fmaf(d, t, rs_partner<0xB1>(d * t, lane)); }

// one halving step on slot bit 1: N values -> N / 2; a lane whose key is set keeps the slots with the bit set and sends the others
template <int N, int CTRL>
WV_RS_FN void rs_step(float (&a)[16], bool key, int lane) {
    float o[N / 2];
#pragma unroll
    for (int q = 0; q < N / 4; ++q) {
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const float keep = key ? a[4 * q + 2 + b] : a[4 * q + b];
            const float send = key ? a[4 * q + b] : a[4 * q + 2 + b];
            o[2 * q + b] = keep + rs_partner<CTRL>(send, lane);
        }
    }
#pragma unroll
    for (int i = 0; i < N / 2; ++i) a[i] = o[i];
}

// sum of d * t over the 32 lanes of this lane's half of the wave, valid on the lanes of the half's second 16-lane row: the
// per-value form (half_sum32_hi_row of wave_ops.h with its first step spelled as the fused multiply-add it is compiled to)
WV_RS_FN float half_dot32_hi_row(float d, float t, int lane) {
    float x = rs_first(d, t, lane);
    x += rs_partner<0x4E>(x, lane);      // quad_perm [2,3,0,1]
    x += rs_partner<0x141>(x, lane);     // row_half_mirror
    x += rs_partner<0x140>(x, lane);     // row_mirror
    return x + rs_row_below15(x, lane);  // own row's sum first (rows 0 / 2: x + x, not a result)
}

// val(c, d, t), c = 0..15, sets the two factors of sixteen per-lane products.  Returns, on lane c of the second 16-lane row of each
// half of the wave (lane & 16), the sum of product c over the 32 lanes of that half - the bits half_dot32_hi_row(d, t) has on that
// lane; other lanes: unspecified.
template <class F>
WV_RS_FN float half_dots32_scatter16(F&& val, int lane) {
    float a[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
        float d, t;
        val(c, d, t);
        a[rs_slot(c)] = rs_first(d, t, lane);                              // quad_perm [1,0,3,2]
    }
    rs_step<16, 0x4E>(a, (((lane >> 1) ^ (lane >> 2)) & 1) != 0, lane);    // quad_perm [2,3,0,1]
    rs_step<8, 0x141>(a, (((lane >> 2) ^ (lane >> 3)) & 1) != 0, lane);    // row_half_mirror
    rs_step<4, 0x140>(a, ((lane >> 3) & 1) != 0, lane);                    // row_mirror
    const bool k1 = ((lane ^ (lane >> 2)) & 1) != 0;
    const float mine = k1 ? a[1] : a[0];
    const float from_class0 = rs_partner<0xB1>(a[1], lane);                // (every lane takes part in an exchange)
    const float for_above = k1 ? from_class0 : a[0];                       // the class-0 lane's sum of the value the lane above keeps
    return mine + rs_row_below(for_above, lane);                           // own row's sum first, as the per-value form
}

#undef WV_RS_FN

}  // namespace wv
