// component_rules.h - the rules of mesh components: which faces count, the area of a triangle and its quantisation, the keep
// decision, and the union-find loops.  Plain inline C++ with no HIP include: the component kernels (component_kernels.h) and the
// host programs of the tests (tests/tools/component_rules_host.cpp, single-threaded under the address sanitizer and four threads
// under the thread sanitizer) compile the same functions, so that what the host programs print is what the device must produce
// bit for bit.  The contract is the components section of include/vmapstep.h.
//
// The rounding contract of the area: float32 throughout, NO fused operation - every subtraction, product, sum and the square root
// is rounded on its own (contraction is switched off per function: clang by the pragma, other compilers build with
// -ffp-contract=off), the square root is IEEE (correctly rounded), denormals are kept, rint rounds half to even (the default rounding
// mode is assumed).
#pragma once

#if defined(__HIP__) || defined(__HIPCC__)
#define KR_FN __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define KR_FN inline
#endif
#if defined(__clang__)
#define KR_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define KR_NO_CONTRACT
#endif

namespace kr {

constexpr long long kAreaClamp = 1ll << 62;            // the most one face adds, in units of 2^-40 m^2

// a face counts iff every index names a vertex; a face that holds one index outside [0, n_vertices) is ignored whole (a repeated
// index is fine: the face still connects its distinct corners and still counts as a face)
KR_FN bool face_valid(int v0, int v1, int v2, long long n_vertices) {
    return v0 >= 0 && v0 < n_vertices && v1 >= 0 && v1 < n_vertices && v2 >= 0 && v2 < n_vertices;
}

// The area of the triangle p0 p1 p2 (three floats each) in float32:
//   a = p1 - p0, b = p2 - p0                                   (six rounded subtractions)
//   c = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0)           (two rounded products and one rounded subtraction each)
//   area = 0.5 * sqrt((c0 c0 + c1 c1) + c2 c2)                  (three products, two sums in this order, IEEE sqrt; the half is exact)
KR_FN float triangle_area(const float* p0, const float* p1, const float* p2) {
    KR_NO_CONTRACT
    const float a0 = p1[0] - p0[0], a1 = p1[1] - p0[1], a2 = p1[2] - p0[2];
    const float b0 = p2[0] - p0[0], b1 = p2[1] - p0[1], b2 = p2[2] - p0[2];
    const float m0 = a1 * b2, n0 = a2 * b1, m1 = a2 * b0, n1 = a0 * b2, m2 = a0 * b1, n2 = a1 * b0;
    const float c0 = m0 - n0, c1 = m1 - n1, c2 = m2 - n2;
    const float s0 = c0 * c0, s1 = c1 * c1, s2 = c2 * c2;
    const float s01 = s0 + s1;
    const float s = s01 + s2;
    return 0.5f * __builtin_sqrtf(s);
}

// An area in units of 2^-40 m^2: rint((double)area * 2^40), half to even (the product is exact: a power of two times a float).
// NaN, an infinity, zero and anything negative count 0; one face is clamped at 2^62 units.
KR_FN long long quantise_area(float area) {
    if (!(area > 0.0f && area <= 3.402823466e+38f)) return 0;      // NaN fails both comparisons, an infinity the second
    const double q = (double)area * 0x1p40;
    if (q >= 0x1p62) return kAreaClamp;
    return (long long)__builtin_rint(q);
}

// the area threshold of the keep decision in the same units: rint(min_area * 2^40), half to even, clamped to [0, 2^62]
KR_FN long long area_threshold(double min_area) {
    if (!(min_area > 0.0)) return 0;
    const double q = min_area * 0x1p40;
    if (q >= 0x1p62) return kAreaClamp;
    return (long long)__builtin_rint(q);
}

// A component is kept iff it has enough faces, enough area and - where largest >= 0 - is among the `largest` largest by area_q;
// rank = how many components come before it in that order (a larger area_q first, ties to the lower component number).
KR_FN bool component_kept(long long n_faces, long long area_q, long long min_faces, long long min_area_q, long long rank, long long largest) {
    return n_faces >= min_faces && area_q >= min_area_q && (largest < 0 || rank < largest);
}

// ---- union-find over an access policy -------------------------------------------------------------------------------------------------
// Access: int load(int x) - the parent of x, possibly a stale (older) one; int cas(int x, int expect, int desired) - an atomic
// compare-and-swap of parent[x] that returns the value it found (== expect iff it swapped); void shorten(int x, int to) - an atomic
// minimum of parent[x] with `to`, or nothing at all.
//
// The invariant (kept by unite, which alone turns a root into a non-root, and by shorten, which only ever lowers the parent of a
// non-root to one of its ancestors): parent[x] <= x, equal only while x is a root, and parent[x] never rises.  So the value a load
// returns - fresh or stale - is x or an ancestor of x that is smaller than x, a tree's root is its smallest member, and the final
// root of a component is its smallest vertex whatever the order of arrival.

// Walks up from x until a load says "root".  Terminates: every hop strictly lowers x, a non-negative integer - whatever other lanes
// do meanwhile and however stale a load is.  The result was a root at the time of its load, and is in x's tree.
template <class Access>
KR_FN int find_root(Access& acc, int x) {
    int p = acc.load(x);
    while (p != x) {
        const int g = acc.load(p);
        if (g == p) return p;                              // p said "root"
        acc.shorten(x, g);                                 // g is p's parent: an ancestor of x below p
        x = p;                                             // x > p > g: one load per hop - g is a value parent[p] has held, which
        p = g;                                             // is all a load of it could promise
    }
    return x;
}

// Joins the trees of a and b: the larger root is linked under the smaller.  A failed compare-and-swap means someone else linked the
// larger root first; the loop then continues from the value the swap returned - that root's new parent, strictly smaller and in the
// same tree - and the other value in hand, NOT from the original endpoints.
// Terminates by construction: every pass of this loop either returns or strictly lowers hi while lo stays (find_root never raises
// either), so hi + lo, a non-negative integer, strictly falls from pass to pass.  Nothing here waits for another lane, and nothing
// depends on a load being fresh: a stale load only returns an older, larger-or-equal ancestor.
// Returns a vertex of the joined tree that was its root when last seen: a face's second union starts there and not at a corner.
template <class Access>
KR_FN int unite(Access& acc, int a, int b) {
    for (;;) {
        a = find_root(acc, a);
        b = find_root(acc, b);
        if (a == b) return a;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int found = acc.cas(hi, hi, lo);             // parent[hi]: hi -> lo, only while hi is still a root
        if (found == hi) return lo;
        a = found;                                         // found < hi: hi's parent by now
        b = lo;
    }
}

// a plain array, one thread (the host program's sequential mode; `shorten` as the kernels have it)
struct SequentialAccess {
    int* parent;
    bool shortening;
    int load(int x) const { return parent[x]; }
    int cas(int x, int expect, int desired) {
        const int found = parent[x];
        if (found == expect) parent[x] = desired;
        return found;
    }
    void shorten(int x, int to) {
        if (shortening && to < parent[x]) parent[x] = to;
    }
};

}  // namespace kr
