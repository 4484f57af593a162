// icp_rules.h - the rules of the depth tracker: frame-to-model projective ICP (point-to-plane, coarse to fine) of a depth image against
// a model depth image.  Plain inline C++ with no HIP include: the icp kernels (icp_kernels.h) and the host program of the tests
// (tests/tools/icp_rules_host.cpp) compile the same functions, so that the host program's output is what the device must produce bit
// for bit.  The numpy checker (tests/icp_oracle.py) is written from THIS text, not from the kernels.
//
// The rounding contract is cull_rules.h's: contraction is switched off per function (clang: the pragma; other compilers build with
// -ffp-contract=off); every fma below is ONE fused operation and is written out, every other operation is rounded on its own, in the
// order the expression is written (left to right); divisions and square roots are IEEE; rint rounds half to even (the default rounding
// mode is assumed).  "f32" / "f64" below name the format an operation is carried out in.
//
// Images are [width][height], width-major (h is the fast axis), pixel (w, h) at offset w * height + h; pixel (w, h) looks along
// ((w - cx) / fx, (h - cy) / fy, 1) and z is depth along the optical axis (view_geometry.h's camera).
//
// 1. Pyramid.  A depth d is VALID iff  d > min_depth && d <= max_depth  (min_depth >= 0 and max_depth finite are checked by the
//    caller, so a valid depth is finite and positive; a NaN fails both comparisons).  Level 0 is the input with every invalid pixel
//    replaced by 0.  Level l + 1 has size ceil(W_l / 2) x ceil(H_l / 2); its pixel (w, h) is made of the level-l pixels
//    (2w, 2h), (min(2w + 1, W_l - 1), 2h), (2w, min(2h + 1, H_l - 1)), (min(2w + 1, W_l - 1), min(2h + 1, H_l - 1)), in THAT order (a
//    clamped pixel counts again): s = the f32 sum of the valid ones in that order, n their number, mn / mx their minimum / maximum.
//    The pixel is s / float(n) if n >= 1 and  mx - mn <= band  (one rounded f32 subtraction), else 0: no mean across a depth edge.
//    The camera of level l (f32):  fx_l = fx / 2^l,  cx_l = (cx - (2^l - 1) / 2) / 2^l, likewise fy_l, cy_l; 2^l and (2^l - 1) / 2 are
//    exact, so each is one rounded subtraction (cx, cy) and one division by a power of two.
// 2. Vertex and normal maps, per level, camera frame, f32.  V(w, h) = (((float)w - cx) / fx * d, ((float)h - cy) / fy * d, d): a
//    subtraction, a division and a multiplication, each rounded.  The normal of (w, h) exists iff 1 <= w <= W - 2, 1 <= h <= H - 2, the
//    pixel and its four neighbours (w - 1, h), (w + 1, h), (w, h - 1), (w, h + 1) are valid, and |d(w + 1, h) - d(w - 1, h)| <= band +
//    band and |d(w, h + 1) - d(w, h - 1)| <= band + band.  Then a = V(w + 1, h) - V(w - 1, h), b = V(w, h + 1) - V(w, h - 1),
//    c = (a1 * b2 - a2 * b1, a2 * b0 - a0 * b2, a0 * b1 - a1 * b0) (two rounded products and one rounded subtraction each),
//    len = sqrtf(c0 * c0 + c1 * c1 + c2 * c2); no normal unless len > 0; n = c / len (three divisions); if n0 * V0 + n1 * V1 + n2 * V2
//    > 0 (V of the pixel itself) every component is negated: n . V <= 0, towards the camera.  A pixel without a normal stores
//    (0, 0, 0); a pixel's MAP entry is the four floats (n0, n1, n2, d), which is all either side of a correspondence reads.
// 3. Correspondence.  T = (float)T64[k], k = 0 .. 11: rows 0 .. 2 of the source-camera -> model-camera matrix, each entry of the f64
//    state rounded to f32 once.  For a source pixel (w, h) with a normal n and p = V(w, h):
//      p'_i = fma(T[4i + 2], p2, fma(T[4i + 1], p1, T[4i] * p0)) + T[4i + 3],   n'_i = fma(T[4i + 2], n2, fma(T[4i + 1], n1, T[4i] * n0))
//      z = p'_2, required > min_depth;  u = fma(fx, p'_0 / z, cx), v = fma(fy, p'_1 / z, cy);  wm = rintf(u), hm = rintf(v), compared
//      as floats against [0, W - 1] x [0, H - 1] before the conversion (cr::project's arithmetic and rounding, margin 0).
//    With the model's entry (m0, m1, m2, dm) at (wm, hm) and q = V(wm, hm) from dm, the pair is an INLIER iff, first failure named:
//      NO_MODEL   (m0, m1, m2) is not all zero
//      FAR        fabsf(z - dm) <= dist_thresh                                       (f32)
//      ANGLE      n'_0 * m0 + n'_1 * m1 + n'_2 * m2 >= cos_thresh                    (f32)
//      GUARD      |r| <= 64 and every |J_k| <= 64, where, in f64 from the f32 values:
//                 e = p' - q;  r = m0 * e0 + m1 * e1 + m2 * e2;  J = (m0, m1, m2, p'_1 * m2 - p'_2 * m1, p'_2 * m0 - p'_0 * m2,
//                 p'_0 * m1 - p'_1 * m0)     (the linearisation r(x) = r + J . x of x = (v, omega): p' moves to p' + omega x p' + v)
// 4. Sums.  29 int64: [0] the inlier count; [1 .. 21] the upper triangle of J J^T row by row ((0,0), (0,1) .. (0,5), (1,1) .. (5,5));
//    [22 .. 27] J_k * r; [28] r * r.  Each product is formed in f64 (one rounding), multiplied by 2^30 (exact) and rounded with rint
//    to an integer, which is added.  Integer addition is associative: the sums do not depend on the order of the pixels.
//    NO OVERFLOW: the guard gives |J_i * J_j|, |J_k * r|, r * r <= 64 * 64 = 2^12, so every addend is at most 2^42 in magnitude; a
//    level has at most kMaxPixels = 2^20 pixels (the caller refuses larger images), so |sum| <= 2^62 < 2^63.  The bound is reached -
//    2^20 pixels with r = 64 give [28] = 2^62 exactly - and not passed.
// 5. Solve and update, f64, no fma anywhere.  A_ij = double(sums[..]) * 2^-30 (symmetric), A_ii += damping, b_k = double(sums[22 + k])
//    * 2^-30.  DEGENERATE if sums[0] < min_inliers.  Else LDL^T without pivoting, thresh = pivot_rel * max_i A_ii:
//      for j = 0 .. 5:  w_k = L_jk * D_k (k < j);  D_j = A_jj - L_j0 * w_0 - .. - L_j,j-1 * w_j-1 (subtracted in that order);
//                       DEGENERATE unless D_j > thresh;  L_ij = (A_ij - L_i0 * w_0 - .. - L_i,j-1 * w_j-1) / D_j  (i > j)
//    y_i = -b_i - L_i0 * y_0 - .. ;  z_i = y_i / D_i;  x_i = z_i - L_i+1,i * x_i+1 - .. - L_5,i * x_5 (i = 5 .. 0, ascending k).
//    x = (v, omega); |x|^2 = x_0 * x_0 + .. + x_5 * x_5, and a |x|^2 that is not finite is DEGENERATE too.  On DEGENERATE the pose does
//    not move and |x|^2 is logged as 0.  Else a = 0.5 * omega, s = a0 * a0 + a1 * a1 +
//    a2 * a2, den = 1 + s, c = 1 - s, and the rotation is the Cayley map, rational and so bit-equal everywhere:
//      dR_ii = (c + 2 * (a_i * a_i)) / den;  dR_ij = (2 * (a_i * a_j) + 2 * k_ij) / den with k = [a]x: k_01 = -a2, k_02 = a1, k_10 = a2,
//      k_12 = -a0, k_20 = -a1, k_21 = a0.
//    T <- dT . T:  R'_ij = dR_i0 * R_0j + dR_i1 * R_1j + dR_i2 * R_2j,  t'_i = dR_i0 * t_0 + dR_i1 * t_1 + dR_i2 * t_2 + v_i.
//    |x|^2 = x_0 * x_0 + .. + x_5 * x_5; the level is finished once |x|^2 < eps * eps.
#pragma once

#include "cull_rules.h"

namespace icp {

constexpr int kMaxLevels = 4;
constexpr int kSums = 29;
constexpr long long kMaxPixels = 1ll << 20;
constexpr double kQuant = 1073741824.0;    // 2^30
constexpr double kGuard = 64.0;
constexpr int kLogCols = 4;                // a log row: count, sum r^2, status, |x|^2

enum Status : int { OK = 0, DEGENERATE = 1, SKIPPED = 2 };
enum Reject : int { INLIER = 0, NO_NORMAL = 1, OUTSIDE = 2, NO_MODEL = 3, FAR = 4, ANGLE = 5, GUARD = 6 };

struct Camera {
    float fx, fy, cx, cy;
    int width, height;
};

struct Rules {
    float min_depth, max_depth, band, dist_thresh, cos_thresh;
};

struct Solve {
    double damping, pivot_rel, eps;
    int min_inliers;
};

CR_FN int half_up(int n) { return (n + 1) / 2; }

CR_FN Camera level_camera(const Camera& c0, int level) {
    CR_NO_CONTRACT
    Camera c = c0;
    for (int k = 0; k < level; ++k) {
        c.width = half_up(c.width);
        c.height = half_up(c.height);
    }
    const float s = (float)(1 << level);
    const float off = (float)((1 << level) - 1) * 0.5f;
    c.fx = c0.fx / s;
    c.fy = c0.fy / s;
    c.cx = (c0.cx - off) / s;
    c.cy = (c0.cy - off) / s;
    return c;
}

CR_FN bool valid(const Rules& r, float d) { return d > r.min_depth && d <= r.max_depth; }

CR_FN float clean(const Rules& r, float d) { return valid(r, d) ? d : 0.0f; }

// a pixel of level l + 1 from its 2 x 2 block of level l, in the order of section 1
CR_FN float down(const Rules& r, float d0, float d1, float d2, float d3) {
    CR_NO_CONTRACT
    const float v[4] = {d0, d1, d2, d3};
    float s = 0.0f, mn = 0.0f, mx = 0.0f;
    int n = 0;
    for (int k = 0; k < 4; ++k) {
        if (!valid(r, v[k])) continue;
        if (n == 0) {
            s = mn = mx = v[k];
        } else {
            s = s + v[k];
            mn = v[k] < mn ? v[k] : mn;
            mx = v[k] > mx ? v[k] : mx;
        }
        ++n;
    }
    if (n == 0) return 0.0f;
    if (!(mx - mn <= r.band)) return 0.0f;
    return s / (float)n;
}

CR_FN void vertex(const Camera& c, int w, int h, float d, float* V) {
    CR_NO_CONTRACT
    V[0] = ((float)w - c.cx) / c.fx * d;
    V[1] = ((float)h - c.cy) / c.fy * d;
    V[2] = d;
}

// the normal of pixel (w, h) of depth d; dwm / dwp = the depths at (w - 1, h) / (w + 1, h), dhm / dhp at (w, h - 1) / (w, h + 1) (not
// looked at for a border pixel).  n = (0, 0, 0) and false where there is none.
CR_FN bool normal(const Rules& r, const Camera& c, int w, int h, float d, float dwm, float dwp, float dhm, float dhp, float* n) {
    CR_NO_CONTRACT
    n[0] = n[1] = n[2] = 0.0f;
    if (!(w >= 1 && h >= 1 && w <= c.width - 2 && h <= c.height - 2)) return false;
    if (!(valid(r, d) && valid(r, dwm) && valid(r, dwp) && valid(r, dhm) && valid(r, dhp))) return false;
    const float two = r.band + r.band;
    if (!(__builtin_fabsf(dwp - dwm) <= two && __builtin_fabsf(dhp - dhm) <= two)) return false;
    float P[3], Wp[3], Wm[3], Hp[3], Hm[3];
    vertex(c, w, h, d, P);
    vertex(c, w + 1, h, dwp, Wp);
    vertex(c, w - 1, h, dwm, Wm);
    vertex(c, w, h + 1, dhp, Hp);
    vertex(c, w, h - 1, dhm, Hm);
    const float a0 = Wp[0] - Wm[0], a1 = Wp[1] - Wm[1], a2 = Wp[2] - Wm[2];
    const float b0 = Hp[0] - Hm[0], b1 = Hp[1] - Hm[1], b2 = Hp[2] - Hm[2];
    const float c0 = a1 * b2 - a2 * b1, c1 = a2 * b0 - a0 * b2, c2 = a0 * b1 - a1 * b0;
    const float len = __builtin_sqrtf(c0 * c0 + c1 * c1 + c2 * c2);
    if (!(len > 0.0f)) return false;
    float n0 = c0 / len, n1 = c1 / len, n2 = c2 / len;
    if (n0 * P[0] + n1 * P[1] + n2 * P[2] > 0.0f) {
        n0 = -n0;
        n1 = -n1;
        n2 = -n2;
    }
    n[0] = n0;
    n[1] = n1;
    n[2] = n2;
    return n0 != 0.0f || n1 != 0.0f || n2 != 0.0f;
}

CR_FN void pose_rows(const double* T64, float* T) {
    for (int k = 0; k < 12; ++k) T[k] = (float)T64[k];
}

// the first half of a correspondence: the source pixel (w, h) with map entry s = (n0, n1, n2, d) under T -> p', n' and the model pixel
CR_FN int project(const Rules& r, const Camera& c, const float* T, int w, int h, const float* s, float* pp, float* np, int& wm, int& hm) {
    CR_NO_CONTRACT
    if (s[0] == 0.0f && s[1] == 0.0f && s[2] == 0.0f) return NO_NORMAL;
    float p[3];
    vertex(c, w, h, s[3], p);
    for (int i = 0; i < 3; ++i) {
        pp[i] = __builtin_fmaf(T[4 * i + 2], p[2], __builtin_fmaf(T[4 * i + 1], p[1], T[4 * i] * p[0])) + T[4 * i + 3];
        np[i] = __builtin_fmaf(T[4 * i + 2], s[2], __builtin_fmaf(T[4 * i + 1], s[1], T[4 * i] * s[0]));
    }
    const float z = pp[2];
    if (!(z > r.min_depth)) return OUTSIDE;
    const float u = __builtin_fmaf(c.fx, pp[0] / z, c.cx);
    const float v = __builtin_fmaf(c.fy, pp[1] / z, c.cy);
    const float wf = __builtin_rintf(u), hf = __builtin_rintf(v);
    if (!(wf >= 0.0f && wf <= (float)(c.width - 1) && hf >= 0.0f && hf <= (float)(c.height - 1))) return OUTSIDE;
    wm = (int)wf;
    hm = (int)hf;
    return INLIER;
}

struct Pair {
    double r;
    double J[6];
};

// the second half: against the model's entry m = (m0, m1, m2, dm) at (wm, hm)
CR_FN int residual(const Rules& r, const Camera& c, const float* pp, const float* np, int wm, int hm, const float* m, Pair& out) {
    CR_NO_CONTRACT
    if (m[0] == 0.0f && m[1] == 0.0f && m[2] == 0.0f) return NO_MODEL;
    if (!(__builtin_fabsf(pp[2] - m[3]) <= r.dist_thresh)) return FAR;
    if (!(np[0] * m[0] + np[1] * m[1] + np[2] * m[2] >= r.cos_thresh)) return ANGLE;
    float q[3];
    vertex(c, wm, hm, m[3], q);
    const double p0 = pp[0], p1 = pp[1], p2 = pp[2], m0 = m[0], m1 = m[1], m2 = m[2];
    const double e0 = p0 - (double)q[0], e1 = p1 - (double)q[1], e2 = p2 - (double)q[2];
    out.r = m0 * e0 + m1 * e1 + m2 * e2;
    out.J[0] = m0;
    out.J[1] = m1;
    out.J[2] = m2;
    out.J[3] = p1 * m2 - p2 * m1;
    out.J[4] = p2 * m0 - p0 * m2;
    out.J[5] = p0 * m1 - p1 * m0;
    bool ok = __builtin_fabs(out.r) <= kGuard;
    for (int k = 0; k < 6; ++k) ok = ok && __builtin_fabs(out.J[k]) <= kGuard;
    return ok ? INLIER : GUARD;
}

// |x| <= 2^12 by the guard: x * 2^30 is exact and at most 2^42
CR_FN long long quant(double x) {
    CR_NO_CONTRACT
    return (long long)__builtin_rint(x * kQuant);
}

CR_FN void accumulate(const Pair& p, long long* s) {
    CR_NO_CONTRACT
    s[0] += 1;
    int at = 1;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) s[at++] += quant(p.J[i] * p.J[j]);
    for (int k = 0; k < 6; ++k) s[22 + k] += quant(p.J[k] * p.r);
    s[28] += quant(p.r * p.r);
}

struct Step {
    int status;
    int finished;                          // |x|^2 < eps^2
    double x[6];
    double x2;
};

// section 5: the 29 sums -> the step; T (12 doubles) is updated in place unless the step is DEGENERATE
CR_FN void solve(const Solve& p, const long long* sums, double* T, Step& st) {
    CR_NO_CONTRACT
    const double inv = 1.0 / kQuant;
    st.status = DEGENERATE;
    st.finished = 0;
    st.x2 = 0.0;
    for (int k = 0; k < 6; ++k) st.x[k] = 0.0;
    if (sums[0] < (long long)p.min_inliers) return;
    double A[6][6], b[6], L[6][6], D[6], w[6];
    int at = 1;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) {
            A[i][j] = (double)sums[at++] * inv;
            A[j][i] = A[i][j];
        }
    for (int k = 0; k < 6; ++k) {
        A[k][k] = A[k][k] + p.damping;
        b[k] = (double)sums[22 + k] * inv;
    }
    double top = A[0][0];
    for (int k = 1; k < 6; ++k) top = A[k][k] > top ? A[k][k] : top;
    const double thresh = p.pivot_rel * top;
    for (int j = 0; j < 6; ++j) {
        double d = A[j][j];
        for (int k = 0; k < j; ++k) {
            w[k] = L[j][k] * D[k];
            d = d - L[j][k] * w[k];
        }
        if (!(d > thresh)) return;
        D[j] = d;
        for (int i = j + 1; i < 6; ++i) {
            double s = A[i][j];
            for (int k = 0; k < j; ++k) s = s - L[i][k] * w[k];
            L[i][j] = s / d;
        }
    }
    double y[6], x[6];
    for (int i = 0; i < 6; ++i) {
        double s = -b[i];
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s;
    }
    for (int i = 5; i >= 0; --i) {
        double s = y[i] / D[i];
        for (int k = i + 1; k < 6; ++k) s = s - L[k][i] * x[k];
        x[i] = s;
    }
    double x2 = 0.0;
    for (int k = 0; k < 6; ++k) {
        st.x[k] = x[k];
        x2 = k == 0 ? x[0] * x[0] : x2 + x[k] * x[k];
    }
    if (!(x2 == x2 && x2 - x2 == 0.0)) return;         // a NaN or an overflow in the solve: the pose does not move
    const double a0 = 0.5 * x[3], a1 = 0.5 * x[4], a2 = 0.5 * x[5];
    const double ss = a0 * a0 + a1 * a1 + a2 * a2;
    const double den = 1.0 + ss, c = 1.0 - ss;
    double R[3][3];
    R[0][0] = (c + 2.0 * (a0 * a0)) / den;
    R[0][1] = (2.0 * (a0 * a1) + 2.0 * -a2) / den;
    R[0][2] = (2.0 * (a0 * a2) + 2.0 * a1) / den;
    R[1][0] = (2.0 * (a1 * a0) + 2.0 * a2) / den;
    R[1][1] = (c + 2.0 * (a1 * a1)) / den;
    R[1][2] = (2.0 * (a1 * a2) + 2.0 * -a0) / den;
    R[2][0] = (2.0 * (a2 * a0) + 2.0 * -a1) / den;
    R[2][1] = (2.0 * (a2 * a1) + 2.0 * a0) / den;
    R[2][2] = (c + 2.0 * (a2 * a2)) / den;
    double N[12];
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) N[4 * i + j] = R[i][0] * T[j] + R[i][1] * T[4 + j] + R[i][2] * T[8 + j];
        N[4 * i + 3] = R[i][0] * T[3] + R[i][1] * T[7] + R[i][2] * T[11] + x[i];
    }
    for (int k = 0; k < 12; ++k) T[k] = N[k];
    st.status = OK;
    st.x2 = x2;
    st.finished = x2 < p.eps * p.eps ? 1 : 0;
}

}  // namespace icp
