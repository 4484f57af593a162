// TEST INFRASTRUCTURE: csrc/component_rules.h compiled for the host - the same functions the component kernels compile - so that
// tests/test_components.py can hold them to the numpy checker (tests/components_oracle.py).  Reads the file named on the command line:
//   n_vertices n_faces shortening min_faces largest           (decimal; shortening 0 / 1; largest < 0: no such rule)
//   min_area                                                   (the hexadecimal of its float64 bits)
//   n_faces x 3 indices                                        (decimal; the order given is the order of the unions)
//   n_vertices x 3 floats                                      (the hexadecimal of their float32 bits)
// and prints six lines: the labels, C, and per component its vertices, its faces, its area_q and 1 / 0 for kept.
// Built twice: plainly (one thread over kr::SequentialAccess; address and undefined-behaviour sanitizers), and with -DKR_THREADS=4
// (four std::threads hook interleaved quarters of the faces over __atomic builtins, the access the kernels have; thread sanitizer).
// parent lives in a vector of exactly n_vertices entries: an index the rules should not have followed aborts the first build.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#ifdef KR_THREADS
#include <thread>
#endif

#include "component_rules.h"

#ifdef KR_THREADS
struct AtomicAccess {
    int* parent;
    bool shortening;
    int load(int x) const { return __atomic_load_n(parent + x, __ATOMIC_RELAXED); }
    int cas(int x, int expect, int desired) {
        __atomic_compare_exchange_n(parent + x, &expect, desired, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED);
        return expect;                                     // the value found: unchanged iff it swapped
    }
    void shorten(int x, int to) {
        if (!shortening) return;
        int cur = __atomic_load_n(parent + x, __ATOMIC_RELAXED);      // an atomic minimum
        while (to < cur && !__atomic_compare_exchange_n(parent + x, &cur, to, false, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) {}
    }
};
#endif

template <class Access>
static void hook(Access acc, const std::vector<int>& faces, long long n_vertices, size_t begin, size_t step) {
    for (size_t f = begin; 3 * f < faces.size(); f += step) {
        const int v0 = faces[3 * f], v1 = faces[3 * f + 1], v2 = faces[3 * f + 2];
        if (!kr::face_valid(v0, v1, v2, n_vertices)) continue;
        const int r = kr::unite(acc, v0, v1);
        kr::unite(acc, r, v2);
    }
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = std::fopen(argv[1], "r");
    if (!fh) return 2;
    long long nv = 0, nf = 0, min_faces = 0, largest = -1;
    int shortening = 0;
    unsigned long long area_bits = 0;
    if (std::fscanf(fh, "%lld %lld %d %lld %lld %llx", &nv, &nf, &shortening, &min_faces, &largest, &area_bits) != 6) return 3;
    if (nv < 0 || nf < 0 || nv >= (1ll << 31)) return 3;
    double min_area = 0.0;
    std::memcpy(&min_area, &area_bits, sizeof(double));
    std::vector<int> faces((size_t)nf * 3);
    std::vector<float> vertices((size_t)nv * 3);
    for (int& x : faces)
        if (std::fscanf(fh, "%d", &x) != 1) return 3;
    for (float& x : vertices) {
        uint32_t b = 0;
        if (std::fscanf(fh, "%x", &b) != 1) return 3;
        std::memcpy(&x, &b, sizeof(float));
    }
    std::fclose(fh);

    std::vector<int> parent((size_t)nv), labels((size_t)nv);
    for (long long v = 0; v < nv; ++v) parent[(size_t)v] = (int)v;
#ifdef KR_THREADS
    {
        std::vector<std::thread> pool;
        for (int t = 0; t < KR_THREADS; ++t)
            pool.emplace_back([&, t] { hook(AtomicAccess{parent.data(), shortening != 0}, faces, nv, (size_t)t, (size_t)KR_THREADS); });
        for (std::thread& th : pool) th.join();
    }
#else
    hook(kr::SequentialAccess{parent.data(), shortening != 0}, faces, nv, 0, 1);
#endif
    // flatten, number the roots in ascending order, relabel: what comp_flatten .. comp_relabel do
    kr::SequentialAccess settled{parent.data(), false};
    std::vector<int> dense((size_t)nv, -1);
    for (long long v = 0; v < nv; ++v) labels[(size_t)v] = kr::find_root(settled, (int)v);
    long long C = 0;
    for (long long v = 0; v < nv; ++v)
        if (labels[(size_t)v] == v) dense[(size_t)v] = (int)C++;
    for (long long v = 0; v < nv; ++v) labels[(size_t)v] = dense[(size_t)labels[(size_t)v]];

    std::vector<long long> cv((size_t)C, 0), cf((size_t)C, 0);
    std::vector<unsigned long long> ca((size_t)C, 0);
    for (long long v = 0; v < nv; ++v) ++cv[(size_t)labels[(size_t)v]];
    for (long long f = 0; f < nf; ++f) {
        const int v0 = faces[3 * (size_t)f], v1 = faces[3 * (size_t)f + 1], v2 = faces[3 * (size_t)f + 2];
        if (!kr::face_valid(v0, v1, v2, nv)) continue;
        const size_t c = (size_t)labels[(size_t)v0];
        ++cf[c];
        ca[c] += (unsigned long long)kr::quantise_area(kr::triangle_area(&vertices[3 * (size_t)v0], &vertices[3 * (size_t)v1], &vertices[3 * (size_t)v2]));
    }
    const long long thr = kr::area_threshold(min_area);
    for (long long v = 0; v < nv; ++v) std::printf(v ? " %d" : "%d", labels[(size_t)v]);
    std::printf("\n%lld\n", C);
    for (long long c = 0; c < C; ++c) std::printf(c ? " %lld" : "%lld", cv[(size_t)c]);
    std::printf("\n");
    for (long long c = 0; c < C; ++c) std::printf(c ? " %lld" : "%lld", cf[(size_t)c]);
    std::printf("\n");
    for (long long c = 0; c < C; ++c) std::printf(c ? " %lld" : "%lld", (long long)ca[(size_t)c]);
    std::printf("\n");
    for (long long c = 0; c < C; ++c) {
        long long rank = 0;
        for (long long o = 0; o < C; ++o)
            rank += (long long)ca[(size_t)o] > (long long)ca[(size_t)c] || (ca[(size_t)o] == ca[(size_t)c] && o < c);
        std::printf("%d", kr::component_kept(cf[(size_t)c], (long long)ca[(size_t)c], min_faces, thr, rank, largest) ? 1 : 0);
    }
    std::printf("\n");
    return 0;
}
