// TEST INFRASTRUCTURE: csrc/ingest_rules.h compiled for the host - the same functions the ingest kernels compile - so that
// tests/test_ingest.py can hold them to the numpy checker (tests/ingest_oracle.py).  Reads commands from the file named on the
// command line, one per line, floats as the hexadecimal of their float32 bits, and prints one answer per command:
//   B n c0 .. c(n-1)                                                  the background list from here on (no answer)
//   R W H half_scale_bits min_box id count umin umax vmin vmax cmin cmax   ->  status box0 box1 box2 box3 class
//   M half_scale_bits extent                                          ->  margin
//   D raw_bits scale_bits max_bits                                    ->  the depth's bits
//   L id status                                                       ->  the label
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "ingest_rules.h"

static float from_bits(uint32_t b) {
    float f;
    std::memcpy(&f, &b, sizeof(f));
    return f;
}

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = std::fopen(argv[1], "r");
    if (!fh) return 2;
    std::vector<int> background;
    char cmd[8];
    while (std::fscanf(fh, "%7s", cmd) == 1) {
        if (cmd[0] == 'B') {
            int n = 0;
            if (std::fscanf(fh, "%d", &n) != 1 || n < 0 || n > ir::kMaxClasses) return 3;
            background.assign(n, 0);
            for (int k = 0; k < n; ++k)
                if (std::fscanf(fh, "%d", &background[k]) != 1) return 3;
        } else if (cmd[0] == 'R') {
            ir::Rules r;
            std::memset(&r, 0, sizeof(r));
            uint32_t hs = 0;
            int id = 0;
            ir::Stats s;
            if (std::fscanf(fh, "%d %d %x %d %d %d %d %d %d %d %d %d", &r.width, &r.height, &hs, &r.min_box, &id, &s.count, &s.u_min, &s.u_max,
                            &s.v_min, &s.v_max, &s.c_min, &s.c_max) != 12)
                return 3;
            r.half_scale = from_bits(hs);
            r.n_background = (int)background.size();
            for (size_t k = 0; k < background.size(); ++k) r.background[k] = background[k];
            const ir::Decision d = ir::decide(r, id, s);
            std::printf("%d %d %d %d %d %d\n", d.status, d.box[0], d.box[1], d.box[2], d.box[3], d.cls);
        } else if (cmd[0] == 'M') {
            uint32_t hs = 0;
            int extent = 0;
            if (std::fscanf(fh, "%x %d", &hs, &extent) != 2) return 3;
            std::printf("%d\n", ir::margin_of(from_bits(hs), extent));
        } else if (cmd[0] == 'D') {
            uint32_t raw = 0, sc = 0, mx = 0;
            if (std::fscanf(fh, "%x %x %x", &raw, &sc, &mx) != 3) return 3;
            const float d = ir::depth_of(from_bits(raw), from_bits(sc), from_bits(mx));
            uint32_t bits;
            std::memcpy(&bits, &d, sizeof(bits));
            std::printf("%08x\n", bits);
        } else if (cmd[0] == 'L') {
            int id = 0, status = 0;
            if (std::fscanf(fh, "%d %d", &id, &status) != 2) return 3;
            std::printf("%d\n", ir::label_of(id, status));
        } else {
            return 3;
        }
    }
    std::fclose(fh);
    return 0;
}
