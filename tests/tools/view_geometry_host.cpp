// view_geometry_host.cpp - the geometry of view rendering (vmap_amd/csrc/view_geometry.h) on the host: the very functions the view
// kernels compile, so what this prints is what view_emit must write bit for bit.  Built by tests/view_oracle.py with
//   g++ -O2 -ffp-contract=off -I vmap_amd/csrc
// Input (a text file, argv[1]; floats in any form strtof reads - the tests write hexadecimal floats, which are exact):
//   width height samples n_obj   fx fy cx cy min_depth   t_wc[16] (row-major)   then n_obj boxes of 15 floats (centre, R, extent)
// Output (stdout): one line per (object, pixel) in that order, pixel = w * height + h:  hit  bits(t_near)  bits(dt)  (hexadecimal).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "view_geometry.h"

static bool read_float(FILE* f, float& v) {
    char tok[128];
    if (fscanf(f, "%127s", tok) != 1) return false;
    char* end = nullptr;
    v = strtof(tok, &end);
    return end != tok && *end == '\0';
}

static uint32_t bits(float v) {
    uint32_t u;
    memcpy(&u, &v, sizeof(u));
    return u;
}

int main(int argc, char** argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s scene.txt\n", argv[0]);
        return 2;
    }
    FILE* f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    vg::Camera cam;
    int n_obj = 0;
    if (fscanf(f, "%d %d %d %d", &cam.width, &cam.height, &cam.samples, &n_obj) != 4 || cam.width < 1 || cam.height < 1 || cam.width > 16384 ||
        cam.height > 16384 || cam.samples < 1 || n_obj < 0 || n_obj > 65536) {
        fprintf(stderr, "bad header\n");
        return 2;
    }
    float t_wc[16];
    bool ok = read_float(f, cam.fx) && read_float(f, cam.fy) && read_float(f, cam.cx) && read_float(f, cam.cy) && read_float(f, cam.min_depth);
    for (int i = 0; i < 16 && ok; ++i) ok = read_float(f, t_wc[i]);
    for (int i = 0; i < 12; ++i) cam.T[i] = t_wc[i];
    std::vector<float> boxes((size_t)n_obj * 15);
    for (size_t i = 0; i < boxes.size() && ok; ++i) ok = read_float(f, boxes[i]);
    fclose(f);
    if (!ok) {
        fprintf(stderr, "bad or missing number\n");
        return 2;
    }
    for (int k = 0; k < n_obj; ++k)
        for (int w = 0; w < cam.width; ++w)
            for (int h = 0; h < cam.height; ++h) {
                const vg::Ray r = vg::pixel_ray(cam, w, h);
                float t_near, dt;
                const bool hit = vg::box_segment(r, boxes.data() + 15 * (size_t)k, cam.min_depth, cam.samples, t_near, dt);
                printf("%d %08x %08x\n", hit ? 1 : 0, bits(t_near), bits(dt));
            }
    return 0;
}
