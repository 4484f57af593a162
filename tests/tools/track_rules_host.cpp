// TEST INFRASTRUCTURE: csrc/track_rules.h compiled for the host - the same functions the track kernels compile - so that
// tests/test_track.py can hold them to the numpy checker (tests/track_oracle.py).  Reads commands from the file named on the command
// line, one per line, and prints one answer per command:
//   B n c0 .. c(n-1)                                  the background list from here on (no answer)
//   M inside valid ratio_q                            ->  whether the pair is past the ratio
//   R d cls min_pixels min_points ratio_q pixels valid eroded eroded_valid n i0 .. i(n-1)   ->  status and the matched candidate
//   L id status valid inside                          ->  the label
//   E status flags                                    ->  whether the pixel's point joins the cloud
#include <cstdio>
#include <cstring>
#include <vector>

#include "track_rules.h"

int main(int argc, char** argv) {
    if (argc != 2) return 2;
    FILE* fh = std::fopen(argv[1], "r");
    if (!fh) return 2;
    tr::Rules rules;
    std::memset(&rules, 0, sizeof(rules));
    char cmd[8];
    while (std::fscanf(fh, "%7s", cmd) == 1) {
        if (cmd[0] == 'B') {
            int n = 0;
            if (std::fscanf(fh, "%d", &n) != 1 || n < 0 || n > fr::kMaxClasses) return 3;
            rules.frame.n_background = n;
            for (int k = 0; k < n; ++k)
                if (std::fscanf(fh, "%d", &rules.frame.background[k]) != 1) return 3;
        } else if (cmd[0] == 'M') {
            int inside = 0, valid = 0, ratio_q = 0;
            if (std::fscanf(fh, "%d %d %d", &inside, &valid, &ratio_q) != 3) return 3;
            std::printf("%d\n", tr::matches(inside, valid, ratio_q) ? 1 : 0);
        } else if (cmd[0] == 'R') {
            int d = 0, cls = 0, n = 0;
            tr::Stats s;
            if (std::fscanf(fh, "%d %d %d %d %d %d %d %d %d %d", &d, &cls, &rules.frame.min_pixels, &rules.frame.min_points, &rules.ratio_q,
                            &s.pixels, &s.valid, &s.eroded, &s.eroded_valid, &n) != 10 || n < 0 || n > tr::kMaxPairs)
                return 3;
            std::vector<int> inside((size_t)n);               // exactly n: a read past the candidates is the sanitizer's to find
            for (int k = 0; k < n; ++k)
                if (std::fscanf(fh, "%d", &inside[(size_t)k]) != 1) return 3;
            int match = -2;
            const int st = tr::decide(rules, d, cls, s, inside.data(), n, &match);
            std::printf("%d %d\n", st, match);
        } else if (cmd[0] == 'L') {
            int id = 0, status = 0, valid = 0, inside = 0;
            if (std::fscanf(fh, "%d %d %d %d", &id, &status, &valid, &inside) != 4) return 3;
            std::printf("%d\n", tr::label_of(id, status, valid != 0, inside != 0));
        } else if (cmd[0] == 'E') {
            int status = 0, flags = 0;
            if (std::fscanf(fh, "%d %d", &status, &flags) != 2) return 3;
            std::printf("%d\n", tr::emits(status, flags) ? 1 : 0);
        } else {
            return 3;
        }
    }
    std::fclose(fh);
    return 0;
}
