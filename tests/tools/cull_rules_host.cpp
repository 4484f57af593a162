// TEST INFRASTRUCTURE: csrc/cull_rules.h compiled for the host - the same functions the cull kernels compile - so that
// tests/test_cull.py can hold them to the numpy checker (tests/cull_oracle.py).  Reads the file named on the command line, floats as
// the hexadecimal of their float32 bits:
//   fx fy cx cy min_depth eps
//   width height margin use_depth n_frames n_points          (decimal)
//   n_frames x 12 floats                                      rows 0..2 of every pose
//   n_frames x width x height floats                          the depth images, width-major (only when use_depth)
//   n_points x 3 floats
// and prints one line of n_points characters, '1' where any frame sees the point.  The depth images live in a vector of exactly
// their size: the address sanitizer turns an offset outside an image's array into an abort.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cull_rules.h"

static bool read_floats(FILE* fh, float* out, size_t n) {
    for (size_t k = 0; k < n; ++k) {
        uint32_t b = 0;
        if (std::fscanf(fh, "%x", &b) != 1) return false;
        std::memcpy(&out[k], &b, sizeof(float));
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = std::fopen(argv[1], "r");
    if (!fh) return 2;
    cr::Rules r;
    std::memset(&r, 0, sizeof(r));
    float head[6];
    int n_frames = 0, n_points = 0;
    if (!read_floats(fh, head, 6)) return 3;
    if (std::fscanf(fh, "%d %d %d %d %d %d", &r.width, &r.height, &r.margin, &r.use_depth, &n_frames, &n_points) != 6) return 3;
    if (r.width < 1 || r.height < 1 || n_frames < 0 || n_points < 0) return 3;
    r.fx = head[0]; r.fy = head[1]; r.cx = head[2]; r.cy = head[3]; r.min_depth = head[4]; r.eps = head[5];
    const size_t pixels = (size_t)r.width * r.height;
    std::vector<float> poses((size_t)n_frames * 12), depth(r.use_depth ? (size_t)n_frames * pixels : 0), points((size_t)n_points * 3);
    if (!read_floats(fh, poses.data(), poses.size()) || !read_floats(fh, depth.data(), depth.size()) || !read_floats(fh, points.data(), points.size()))
        return 3;
    std::fclose(fh);
    std::string out((size_t)n_points, '0');
    for (int i = 0; i < n_points; ++i)
        for (int k = 0; k < n_frames && out[i] == '0'; ++k)
            if (cr::seen_by(r, &poses[(size_t)k * 12], r.use_depth ? &depth[(size_t)k * pixels] : nullptr, points[3 * (size_t)i], points[3 * (size_t)i + 1],
                            points[3 * (size_t)i + 2]))
                out[i] = '1';
    std::printf("%s\n", out.c_str());
    return 0;
}
