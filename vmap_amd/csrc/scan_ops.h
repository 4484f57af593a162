// scan_ops.h - the device primitives the count -> scan -> emit families share (mesh_kernels.h, eval_kernels.h, bounds_kernels.h):
// the workgroup scan of integers, the one-workgroup scan of per-block totals, and the lookup of a segment in CSR offsets.
// Integer sums only: any order of the additions gives the same bits, which is what lets all three families use one scan.  (The
// float64 scan of surface_cdf is not one of these: its order is part of its output, see eval_kernels.h.)
#pragma once
#include <hip/hip_runtime.h>

namespace vscan {

// Exclusive scan of one integer per lane over a workgroup of WG lanes (whole waves of 64; T = int, long long, unsigned long long):
// a shuffle scan inside each wave, the waves' sums through one LDS word per wave.  Returns the sum of the lanes before this one;
// total = the workgroup's sum, in every lane.
// Barrier contract: every lane of the workgroup calls it, and it holds ONE barrier, between writing wsum[WG / 64] and reading it.
// There is none after the reads, so the caller owes a barrier before anything writes the same wsum again - a second call included
// (two scans in a row take two arrays, as mesh_count does; a loop ends its round with __syncthreads(), as wg_scan_totals does).
// That one barrier orders nothing else for the caller: LDS of the caller's own needs the caller's own barrier.
template <int WG, typename T>
__device__ __forceinline__ T wg_exclusive_scan(T x, T* wsum, T& total) {
    static_assert(WG % 64 == 0 && WG <= 1024, "whole waves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T s = x;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(s, d, 64);
        if (lane >= d) s += y;
    }
    if (lane == 63) wsum[wave] = s;
    __syncthreads();
    T before = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < WG / 64; ++w) {
        const T t = wsum[w];
        before += w < wave ? t : T(0);
        sum += t;
    }
    total = sum;
    return before + s - x;
}

// One workgroup of WG lanes scans n per-block totals in chunks of WG with a running carry: store(i, the sum of load(0 .. i - 1)) for
// every i in [0, n); returns the grand total in every lane.  load and store may name the same memory (each lane reads and writes
// its own i).  Ends every chunk with a barrier, so wsum[WG / 64] is free on return.
template <int WG, typename T, typename Load, typename Store>
__device__ __forceinline__ T wg_scan_totals(long long n, T* wsum, Load load, Store store) {
    T carry = 0;
    for (long long base = 0; base < n; base += WG) {
        const long long i = base + threadIdx.x;
        const T x = i < n ? load(i) : T(0);
        T total;
        const T ex = wg_exclusive_scan<WG>(x, wsum, total);
        if (i < n) store(i, carry + ex);
        carry += total;
        __syncthreads();      // wsum is rewritten by the next chunk
    }
    return carry;
}

// The segment of x in CSR offsets: the last s in [0, n) with offsets[s] <= x (empty segments share their successor's offset and are
// never returned for an x inside [offsets[0], offsets[n])).
template <typename T>
__device__ __forceinline__ int segment_of(const T* offsets, int n, T x) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= x) lo = mid; else hi = mid;
    }
    return lo;
}

}  // namespace vscan
