// TEST INFRASTRUCTURE: csrc/raycast_rules.h compiled for the host - the same functions the raycast kernels compile - so that
// tests/test_raycast.py can hold them to the numpy checker (tests/raycast_oracle.py) bit for bit.  Built with
// -fsanitize=address,undefined: an access out of bounds or undefined arithmetic in the rules aborts it.
// Usage: raycast_rules_host IN OUT, both raw little-endian files.
//   IN:  int32 nx ny nz width height max_steps n_views has_color; float32 fx fy cx cy min_depth max_depth step min_weight N[9];
//        float32 views[n_views][12]; float32 tsdf[n], weight[n], color[n][4] (has_color)
//   OUT: uint8 classes[bx*by*bz]; then twice - the plain march (no class table), then the class-aware one - float32 depth[K][W][H],
//        uint8 status[K][W][H], float32 normal[K][W][H][3], uint8 color[K][W][H][4] (has_color)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "raycast_rules.h"

template <class T>
static bool rd(FILE* fh, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, fh) == n;
}

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fh = std::fopen(argv[1], "rb");
    if (!fh) return 2;
    std::vector<int32_t> head;
    std::vector<float> fl;
    if (!rd(fh, head, 8) || !rd(fh, fl, 17)) return 3;
    rc::Rules r;
    std::memset(&r, 0, sizeof(r));
    r.nx = head[0]; r.ny = head[1]; r.nz = head[2]; r.width = head[3]; r.height = head[4]; r.max_steps = head[5];
    const int n_views = head[6];
    const bool has_color = head[7] != 0;
    r.fx = fl[0]; r.fy = fl[1]; r.cx = fl[2]; r.cy = fl[3]; r.min_depth = fl[4]; r.max_depth = fl[5]; r.step = fl[6]; r.min_weight = fl[7];
    std::memcpy(r.N, fl.data() + 8, sizeof(r.N));
    if (r.nx < 2 || r.ny < 2 || r.nz < 2 || r.width < 1 || r.height < 1 || n_views < 0 || r.max_steps < 1 || r.max_steps >= rc::kMaxStepsLimit) return 3;
    const size_t n = (size_t)r.nx * r.ny * r.nz, pixels = (size_t)r.width * r.height;
    std::vector<float> views, D, W, C;
    if (!rd(fh, views, (size_t)n_views * 12) || !rd(fh, D, n) || !rd(fh, W, n)) return 3;
    if (has_color && !rd(fh, C, n * 4)) return 3;
    std::fclose(fh);
    rc::Volume vol;
    vol.tsdf = D.data(); vol.weight = W.data(); vol.color = has_color ? C.data() : nullptr;
    const int bx = rc::brick_dim(r.nx), by = rc::brick_dim(r.ny), bz = rc::brick_dim(r.nz);
    std::vector<unsigned char> classes((size_t)bx * by * bz);
    for (int a = 0; a < bx; ++a)
        for (int b = 0; b < by; ++b)
            for (int c = 0; c < bz; ++c) classes[((size_t)a * by + b) * bz + c] = rc::brick_class(r, vol, a, b, c);
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::fwrite(classes.data(), 1, classes.size(), out);
    for (int form = 0; form < 2; ++form) {
        std::vector<float> depth(n_views * pixels), normal(n_views * pixels * 3);
        std::vector<unsigned char> status(n_views * pixels), color(has_color ? n_views * pixels * 4 : 0);
        for (int v = 0; v < n_views; ++v)
            for (int w = 0; w < r.width; ++w)
                for (int h = 0; h < r.height; ++h) {
                    const size_t pix = ((size_t)v * r.width + w) * r.height + h;
                    rc::cast_pixel(r, vol, form ? classes.data() : nullptr, views.data() + 12 * v, w, h, depth[pix], status[pix], normal.data() + 3 * pix,
                                   has_color ? color.data() + 4 * pix : nullptr);
                }
        std::fwrite(depth.data(), 4, depth.size(), out);
        std::fwrite(status.data(), 1, status.size(), out);
        std::fwrite(normal.data(), 4, normal.size(), out);
        if (has_color) std::fwrite(color.data(), 1, color.size(), out);
    }
    return std::fclose(out) == 0 ? 0 : 2;
}
