// TEST INFRASTRUCTURE: csrc/raster_rules.h compiled for the host - the same functions the raster kernels compile - so that
// tests/test_raster.py can hold them to the numpy checker (tests/raster_oracle.py).  Floats travel as the hexadecimal of their
// float32 bits.
//
//   raster_rules_host raster FILE      FILE:  fx fy cx cy min_depth max_depth
//                                             width height n_views n_vertices n_faces            (decimal)
//                                             n_views x 12 floats                                rows 0..2 of every pose
//                                             n_vertices x 3 floats
//                                             n_faces x 3 indices                                (decimal)
//                                      prints per view "view K dropped D", then one line per pixel, width-major:
//                                      depth bits, face, how many faces cover the pixel's centre (before any depth cut)
//   raster_rules_host compare FILE     FILE:  n, then n pairs of floats;  prints per pair the class (0 both, 1 a only, 2 b only,
//                                      3 neither) and the quantised difference
// The key image and the coverage counts live in vectors of exactly their size: the address sanitizer turns a pixel outside the image
// into an abort, the undefined-behaviour sanitizer a conversion or a shift out of range.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "raster_rules.h"

static bool read_floats(FILE* fh, float* out, size_t n) {
    for (size_t k = 0; k < n; ++k) {
        uint32_t b = 0;
        if (std::fscanf(fh, "%x", &b) != 1) return false;
        std::memcpy(&out[k], &b, sizeof(float));
    }
    return true;
}

static int run_raster(FILE* fh) {
    rr::Camera cam;
    std::memset(&cam, 0, sizeof(cam));
    float head[6];
    int n_views = 0, n_vertices = 0, n_faces = 0;
    if (!read_floats(fh, head, 6)) return 3;
    if (std::fscanf(fh, "%d %d %d %d %d", &cam.width, &cam.height, &n_views, &n_vertices, &n_faces) != 5) return 3;
    if (cam.width < 1 || cam.height < 1 || cam.width > rr::kMaxSide || cam.height > rr::kMaxSide || n_views < 0 || n_vertices < 0 || n_faces < 0) return 3;
    cam.fx = head[0]; cam.fy = head[1]; cam.cx = head[2]; cam.cy = head[3]; cam.min_depth = head[4]; cam.max_depth = head[5];
    std::vector<float> poses((size_t)n_views * 12), vertices((size_t)n_vertices * 3);
    std::vector<int> faces((size_t)n_faces * 3);
    if (!read_floats(fh, poses.data(), poses.size()) || !read_floats(fh, vertices.data(), vertices.size())) return 3;
    for (int& i : faces)
        if (std::fscanf(fh, "%d", &i) != 1) return 3;
    const size_t pixels = (size_t)cam.width * cam.height;
    for (int k = 0; k < n_views; ++k) {
        std::vector<unsigned long long> keys(pixels, rr::kEmptyKey);
        std::vector<int> covered(pixels, 0);
        long long dropped = 0;
        for (int f = 0; f < n_faces; ++f) {
            const int v0 = faces[3 * (size_t)f], v1 = faces[3 * (size_t)f + 1], v2 = faces[3 * (size_t)f + 2];
            rr::Face face;
            if (!(v0 >= 0 && v0 < n_vertices && v1 >= 0 && v1 < n_vertices && v2 >= 0 && v2 < n_vertices) ||
                !rr::setup_face(cam, &poses[(size_t)k * 12], &vertices[3 * (size_t)v0], &vertices[3 * (size_t)v1], &vertices[3 * (size_t)v2], face)) {
                ++dropped;
                continue;
            }
            const rr::Box box = rr::pixel_box(cam, face);
            for (int w = box.w0; w <= box.w1; ++w)
                for (int h = box.h0; h <= box.h1; ++h) {
                    long long E[3];
                    if (!rr::covers(face, w, h, E)) continue;
                    const size_t at = (size_t)w * cam.height + h;
                    covered.at(at) += 1;
                    const float z = rr::depth_at(face, E);
                    if (!rr::depth_written(cam, z)) continue;
                    const unsigned long long key = rr::make_key(z, f);
                    if (key < keys.at(at)) keys.at(at) = key;
                }
        }
        std::printf("view %d dropped %lld\n", k, dropped);
        for (size_t at = 0; at < pixels; ++at) {
            const float z = rr::key_depth(keys[at]);
            uint32_t bits;
            std::memcpy(&bits, &z, sizeof(bits));
            std::printf("%08x %d %d\n", bits, rr::key_face(keys[at]), covered[at]);
        }
    }
    return 0;
}

static int run_compare(FILE* fh) {
    int n = 0;
    if (std::fscanf(fh, "%d", &n) != 1 || n < 0) return 3;
    std::vector<float> v((size_t)n * 2);
    if (!read_floats(fh, v.data(), v.size())) return 3;
    for (int i = 0; i < n; ++i) {
        const int c = rr::compare_class(v[2 * (size_t)i], v[2 * (size_t)i + 1]);
        std::printf("%d %lld\n", c, c == rr::kBoth ? rr::compare_q(v[2 * (size_t)i], v[2 * (size_t)i + 1]) : 0ll);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fh = std::fopen(argv[2], "r");
    if (!fh) return 2;
    int rc = 2;
    if (std::strcmp(argv[1], "raster") == 0) rc = run_raster(fh);
    else if (std::strcmp(argv[1], "compare") == 0) rc = run_compare(fh);
    std::fclose(fh);
    return rc;
}
