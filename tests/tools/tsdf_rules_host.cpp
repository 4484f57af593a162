// TEST INFRASTRUCTURE: csrc/tsdf_rules.h compiled for the host - the same functions the tsdf kernel compiles - so that tests/test_tsdf.py
// can hold them to the numpy checker (tests/tsdf_oracle.py) bit for bit.  Built with -fsanitize=address,undefined: an access out of
// bounds or undefined arithmetic in the rules aborts it.  Usage: tsdf_rules_host IN OUT, both raw little-endian files.
//   IN:  int32 nx ny nz obj_id width height margin n_slots n_frames has_color has_inst; float32 affine[12] fx fy cx cy min_depth
//        max_depth trunc max_weight; int32 slots[n_frames]; float32 poses[n_slots][16]; float32 depth[n_slots][W][H];
//        uint8 rgbx[n_slots][W][H][4] (has_color); int32 inst[n_slots][W][H] (has_inst); float32 tsdf[n], weight[n], color[n][4] (has_color)
//   OUT: float32 centres[n][3], tsdf[n], weight[n], color[n][4] (has_color)
// Every voxel is updated sequentially over the frames in the order given, as one lane of the kernel does.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "tsdf_rules.h"

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
    if (!rd(fh, head, 11) || !rd(fh, fl, 20)) return 3;
    const int nx = head[0], ny = head[1], nz = head[2], n_slots = head[7], n_frames = head[8];
    const bool has_color = head[9] != 0, has_inst = head[10] != 0;
    tr::Rules r;
    std::memset(&r, 0, sizeof(r));
    r.obj_id = head[3];
    r.cam.width = head[4]; r.cam.height = head[5]; r.cam.margin = head[6];
    const float* A = fl.data();
    r.cam.fx = fl[12]; r.cam.fy = fl[13]; r.cam.cx = fl[14]; r.cam.cy = fl[15];
    r.cam.min_depth = fl[16]; r.max_depth = fl[17]; r.trunc = fl[18]; r.max_weight = fl[19];
    if (nx < 1 || ny < 1 || nz < 1 || n_slots < 0 || n_frames < 0 || r.cam.width < 1 || r.cam.height < 1 || (r.obj_id >= 0 && !has_inst)) return 3;
    const size_t n = (size_t)nx * ny * nz, pixels = (size_t)r.cam.width * r.cam.height;
    std::vector<int32_t> slots, inst;
    std::vector<float> poses, depth, D, W, C;
    std::vector<unsigned char> rgbx;
    if (!rd(fh, slots, n_frames) || !rd(fh, poses, (size_t)n_slots * 16) || !rd(fh, depth, n_slots * pixels)) return 3;
    if (has_color && !rd(fh, rgbx, n_slots * pixels * 4)) return 3;
    if (has_inst && !rd(fh, inst, n_slots * pixels)) return 3;
    if (!rd(fh, D, n) || !rd(fh, W, n)) return 3;
    if (has_color && !rd(fh, C, n * 4)) return 3;
    std::fclose(fh);
    for (int s : slots)
        if (s < 0 || s >= n_slots) return 3;
    std::vector<float> centres(n * 3);
    for (size_t p = 0; p < n; ++p) {
        const int k = (int)(p % nz), row = (int)(p / nz);
        float x, y, z;
        tr::voxel_center(A, row / ny, row % ny, k, x, y, z);
        centres[3 * p] = x; centres[3 * p + 1] = y; centres[3 * p + 2] = z;
        for (int f = 0; f < n_frames; ++f) {
            const size_t s = (size_t)slots[f];
            tr::integrate_frame(r, poses.data() + 16 * s, depth.data() + s * pixels, has_color ? rgbx.data() + 4 * s * pixels : nullptr,
                                has_inst ? inst.data() + s * pixels : nullptr, x, y, z, D[p], W[p], has_color ? C.data() + 4 * p : nullptr);
        }
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) return 2;
    std::fwrite(centres.data(), 4, centres.size(), out);
    std::fwrite(D.data(), 4, n, out);
    std::fwrite(W.data(), 4, n, out);
    if (has_color) std::fwrite(C.data(), 4, C.size(), out);
    return std::fclose(out) == 0 ? 0 : 2;
}
