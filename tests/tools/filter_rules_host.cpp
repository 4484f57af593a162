// TEST INFRASTRUCTURE: csrc/filter_rules.h compiled for the host - the same functions the filter kernels compile - so that
// tests/test_filter.py can hold them to the numpy checker (tests/filter_oracle.py).  Reads commands from the file named on the
// command line, one per line, floats as the hexadecimal of their float32 bits, and prints one answer per command:
//   B n c0 .. c(n-1)                                  the background list from here on (no answer)
//   C fx fy cx cy t0 .. t11                           the camera from here on: intrinsics and rows 0..2 of t_wc (no answer)
//   T r0 .. r15                                       the box-table row from here on (no answer)
//   S raw id_shift max_ids                            ->  the shifted id (-1: no table row)
//   D raw scale max                                   ->  the depth's bits, then whether it is valid
//   P u v depth                                       ->  the world point's bits x y z
//   K id voxel x y z                                  ->  1 and the key, or 0
//   X key                                             ->  id kx ky kz
//   V k voxel                                         ->  the centre's bits
//   I x y z                                           ->  whether the point is inside the box row
//   R id min_pixels min_points known pixels cmin cmax valid inside eroded   ->  status
//   L id status valid inside                          ->  the label
//   E status flags                                    ->  whether the pixel's point joins the cloud
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "filter_rules.h"

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, sizeof(f));
    return f;
}
static uint32_t to_bits(float f) {
    uint32_t b;
    std::memcpy(&b, &f, sizeof(b));
    return b;
}
static bool read_floats(FILE* fh, float* out, int n) {
    for (int k = 0; k < n; ++k) {
        uint32_t b = 0;
        if (std::fscanf(fh, "%x", &b) != 1) return false;
        out[k] = from_bits(b);
    }
    return true;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = std::fopen(argv[1], "r");
    if (!fh) return 2;
    fr::Rules rules;
    std::memset(&rules, 0, sizeof(rules));
    float box[fr::kBoxFloats] = {0};
    char cmd[8];
    while (std::fscanf(fh, "%7s", cmd) == 1) {
        if (cmd[0] == 'B') {
            int n = 0;
            if (std::fscanf(fh, "%d", &n) != 1 || n < 0 || n > fr::kMaxClasses) return 3;
            rules.n_background = n;
            for (int k = 0; k < n; ++k)
                if (std::fscanf(fh, "%d", &rules.background[k]) != 1) return 3;
        } else if (cmd[0] == 'C') {
            float v[16];
            if (!read_floats(fh, v, 16)) return 3;
            rules.cam.fx = v[0]; rules.cam.fy = v[1]; rules.cam.cx = v[2]; rules.cam.cy = v[3];
            for (int k = 0; k < 12; ++k) rules.cam.T[k] = v[4 + k];
        } else if (cmd[0] == 'T') {
            if (!read_floats(fh, box, fr::kBoxFloats)) return 3;
        } else if (cmd[0] == 'S') {
            int raw = 0, shift = 0, max_ids = 0;
            if (std::fscanf(fh, "%d %d %d", &raw, &shift, &max_ids) != 3) return 3;
            std::printf("%d\n", fr::shifted_id(raw, shift, max_ids));
        } else if (cmd[0] == 'D') {
            float v[3];
            if (!read_floats(fh, v, 3)) return 3;
            const float d = ir::depth_of(v[0], v[1], v[2]);
            std::printf("%08x %d\n", to_bits(d), fr::valid_depth(d) ? 1 : 0);
        } else if (cmd[0] == 'P') {
            int u = 0, v = 0;
            float d;
            if (std::fscanf(fh, "%d %d", &u, &v) != 2 || !read_floats(fh, &d, 1)) return 3;
            const fr::Point p = fr::world_point(rules.cam, u, v, d);
            std::printf("%08x %08x %08x\n", to_bits(p.x), to_bits(p.y), to_bits(p.z));
        } else if (cmd[0] == 'K') {
            int id = 0;
            float v[4];
            if (std::fscanf(fh, "%d", &id) != 1 || !read_floats(fh, v, 4)) return 3;
            unsigned long long key = 0;
            const fr::Point p = {v[1], v[2], v[3]};
            if (fr::voxel_key(id, p, v[0], &key)) std::printf("1 %llu\n", key);
            else std::printf("0\n");
        } else if (cmd[0] == 'X') {
            unsigned long long key = 0;
            if (std::fscanf(fh, "%llu", &key) != 1) return 3;
            std::printf("%d %d %d %d\n", fr::key_id(key), fr::key_coord(key, 0), fr::key_coord(key, 1), fr::key_coord(key, 2));
        } else if (cmd[0] == 'V') {
            int k = 0;
            float voxel;
            if (std::fscanf(fh, "%d", &k) != 1 || !read_floats(fh, &voxel, 1)) return 3;
            std::printf("%08x\n", to_bits(fr::voxel_centre(k, voxel)));
        } else if (cmd[0] == 'I') {
            float v[3];
            if (!read_floats(fh, v, 3)) return 3;
            const fr::Point p = {v[0], v[1], v[2]};
            std::printf("%d\n", fr::inside_box(box, p) ? 1 : 0);
        } else if (cmd[0] == 'R') {
            int id = 0, known = 0;
            fr::Stats s;
            std::memset(&s, 0, sizeof(s));
            if (std::fscanf(fh, "%d %d %d %d %d %d %d %d %d %d", &id, &rules.min_pixels, &rules.min_points, &known, &s.pixels, &s.c_min, &s.c_max,
                            &s.valid, &s.inside, &s.eroded) != 10)
                return 3;
            std::printf("%d\n", fr::decide(rules, id, s, known != 0));
        } else if (cmd[0] == 'L') {
            int id = 0, status = 0, valid = 0, inside = 0;
            if (std::fscanf(fh, "%d %d %d %d", &id, &status, &valid, &inside) != 4) return 3;
            std::printf("%d\n", fr::label_of(id, status, valid != 0, inside != 0));
        } else if (cmd[0] == 'E') {
            int status = 0, flags = 0;
            if (std::fscanf(fh, "%d %d", &status, &flags) != 2) return 3;
            std::printf("%d\n", fr::emits(status, flags) ? 1 : 0);
        } else {
            return 3;
        }
    }
    std::fclose(fh);
    return 0;
}
