// TEST INFRASTRUCTURE: csrc/icp_rules.h compiled for the host - the same functions the icp kernels compile - so that tests/test_icp.py
// can hold them to the numpy checker (tests/icp_oracle.py) bit for bit.  Built with -fsanitize=address,undefined: an access out of
// bounds or undefined arithmetic in the rules aborts it.  Reads commands from the file named on the command line; float32 values travel
// as 8 hex digits, float64 values as 16:
//   R min_depth max_depth band dist_thresh cos_thresh          the rules from here on (no answer)
//   C fx fy cx cy W H                                          the level-0 camera from here on (no answer)
//   K level                                                    -> fx fy cx cy W H of the level
//   M levels, then W * H depths                                -> per level "level l W H", then one line "n0 n1 n2 d" per pixel
//   F level T[12], then W_l * H_l source entries and as many model entries (4 floats each)
//                                                              -> per pixel "reason r J0 .. J5", then "sums s0 .. s28"
//   S damping pivot_rel eps min_inliers s0 .. s28 T[12]        -> "status finished x2 x0 .. x5 T0 .. T11"
//   Q x n                                                      -> quant(x) added n times (int64; an overflow aborts under the sanitizer)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "icp_rules.h"

static bool rf(FILE* fh, float& v) {
    unsigned u = 0;
    if (std::fscanf(fh, "%x", &u) != 1) return false;
    std::memcpy(&v, &u, 4);
    return true;
}
static bool rd(FILE* fh, double& v) {
    unsigned long long u = 0;
    if (std::fscanf(fh, "%llx", &u) != 1) return false;
    std::memcpy(&v, &u, 8);
    return true;
}
static unsigned hf(float v) {
    unsigned u;
    std::memcpy(&u, &v, 4);
    return u;
}
static unsigned long long hd(double v) {
    unsigned long long u;
    std::memcpy(&u, &v, 8);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = std::fopen(argv[1], "r");
    if (!fh) return 2;
    icp::Rules rules;
    icp::Camera cam0;
    std::memset(&rules, 0, sizeof(rules));
    std::memset(&cam0, 0, sizeof(cam0));
    char cmd[8];
    while (std::fscanf(fh, "%7s", cmd) == 1) {
        if (cmd[0] == 'R') {
            if (!(rf(fh, rules.min_depth) && rf(fh, rules.max_depth) && rf(fh, rules.band) && rf(fh, rules.dist_thresh) && rf(fh, rules.cos_thresh))) return 3;
        } else if (cmd[0] == 'C') {
            if (!(rf(fh, cam0.fx) && rf(fh, cam0.fy) && rf(fh, cam0.cx) && rf(fh, cam0.cy)) || std::fscanf(fh, "%d %d", &cam0.width, &cam0.height) != 2) return 3;
            if (cam0.width < 1 || cam0.height < 1 || (long long)cam0.width * cam0.height > icp::kMaxPixels) return 3;
        } else if (cmd[0] == 'K') {
            int level = 0;
            if (std::fscanf(fh, "%d", &level) != 1 || level < 0 || level >= icp::kMaxLevels) return 3;
            const icp::Camera c = icp::level_camera(cam0, level);
            std::printf("%08x %08x %08x %08x %d %d\n", hf(c.fx), hf(c.fy), hf(c.cx), hf(c.cy), c.width, c.height);
        } else if (cmd[0] == 'M') {
            int levels = 0;
            if (std::fscanf(fh, "%d", &levels) != 1 || levels < 1 || levels > icp::kMaxLevels) return 3;
            std::vector<float> D((size_t)cam0.width * cam0.height);          // exactly the level: a read past it is the sanitizer's to find
            for (float& v : D) {
                if (!rf(fh, v)) return 3;
                v = icp::clean(rules, v);
            }
            for (int l = 0; l < levels; ++l) {
                const icp::Camera c = icp::level_camera(cam0, l);
                if (l > 0) {
                    const icp::Camera b = icp::level_camera(cam0, l - 1);
                    std::vector<float> N((size_t)c.width * c.height);
                    for (int w = 0; w < c.width; ++w)
                        for (int h = 0; h < c.height; ++h) {
                            const int wa = 2 * w, ha = 2 * h, wb = wa + 1 < b.width ? wa + 1 : b.width - 1, hb = ha + 1 < b.height ? ha + 1 : b.height - 1;
                            N[(size_t)w * c.height + h] = icp::down(rules, D[(size_t)wa * b.height + ha], D[(size_t)wb * b.height + ha],
                                                                    D[(size_t)wa * b.height + hb], D[(size_t)wb * b.height + hb]);
                        }
                    D.swap(N);
                }
                std::printf("level %d %d %d\n", l, c.width, c.height);
                for (int w = 0; w < c.width; ++w)
                    for (int h = 0; h < c.height; ++h) {
                        const bool inner = w >= 1 && h >= 1 && w <= c.width - 2 && h <= c.height - 2;
                        const size_t at = (size_t)w * c.height + h;
                        float n[3];
                        icp::normal(rules, c, w, h, D[at], inner ? D[at - c.height] : 0.0f, inner ? D[at + c.height] : 0.0f, inner ? D[at - 1] : 0.0f,
                                    inner ? D[at + 1] : 0.0f, n);
                        std::printf("%08x %08x %08x %08x\n", hf(n[0]), hf(n[1]), hf(n[2]), hf(D[at]));
                    }
            }
        } else if (cmd[0] == 'F') {
            int level = 0;
            double T64[12];
            if (std::fscanf(fh, "%d", &level) != 1 || level < 0 || level >= icp::kMaxLevels) return 3;
            for (double& v : T64)
                if (!rd(fh, v)) return 3;
            const icp::Camera c = icp::level_camera(cam0, level);
            const size_t n = (size_t)c.width * c.height;
            std::vector<float> src(n * 4), model(n * 4);
            for (float& v : src)
                if (!rf(fh, v)) return 3;
            for (float& v : model)
                if (!rf(fh, v)) return 3;
            float T[12];
            icp::pose_rows(T64, T);
            long long sums[icp::kSums] = {0};
            for (int w = 0; w < c.width; ++w)
                for (int h = 0; h < c.height; ++h) {
                    float pp[3], np[3];
                    int wm = -1, hm = -1;
                    icp::Pair p;
                    std::memset(&p, 0, sizeof(p));
                    int reason = icp::project(rules, c, T, w, h, &src[((size_t)w * c.height + h) * 4], pp, np, wm, hm);
                    if (reason == icp::INLIER) reason = icp::residual(rules, c, pp, np, wm, hm, &model[((size_t)wm * c.height + hm) * 4], p);
                    if (reason == icp::INLIER) icp::accumulate(p, sums);
                    std::printf("%d %016llx", reason, hd(p.r));
                    for (double j : p.J) std::printf(" %016llx", hd(j));
                    std::printf("\n");
                }
            std::printf("sums");
            for (long long s : sums) std::printf(" %lld", s);
            std::printf("\n");
        } else if (cmd[0] == 'S') {
            icp::Solve p;
            long long sums[icp::kSums];
            double T[12];
            if (!(rd(fh, p.damping) && rd(fh, p.pivot_rel) && rd(fh, p.eps)) || std::fscanf(fh, "%d", &p.min_inliers) != 1) return 3;
            for (long long& s : sums)
                if (std::fscanf(fh, "%lld", &s) != 1) return 3;
            for (double& v : T)
                if (!rd(fh, v)) return 3;
            icp::Step st;
            icp::solve(p, sums, T, st);
            std::printf("%d %d %016llx", st.status, st.finished, hd(st.x2));
            for (double v : st.x) std::printf(" %016llx", hd(v));
            for (double v : T) std::printf(" %016llx", hd(v));
            std::printf("\n");
        } else if (cmd[0] == 'Q') {
            double x = 0.0;
            long long n = 0, sum = 0;
            if (!rd(fh, x) || std::fscanf(fh, "%lld", &n) != 1 || n < 0 || n > icp::kMaxPixels) return 3;
            for (long long k = 0; k < n; ++k) sum += icp::quant(x);
            std::printf("%lld\n", sum);
        } else {
            return 3;
        }
    }
    std::fclose(fh);
    return 0;
}
