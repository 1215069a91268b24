// The library's choice for hmmr_conv_desc_t.tile = 0, table-driven (csrc/conv_tiles.h), against the four hand-written rules it replaced,
// which are kept here verbatim as the thing to compare against.  Host code only: no HIP, no GPU.
//
//     g++ -std=c++17 -O1 -I include -I human_dynamics_amd/csrc tools/tile_choice_check.cpp -o /tmp/tile_choice_check && /tmp/tile_choice_check
//     (once more with -fsanitize=address,undefined)
//
// Sweep: M = 1 .. 257 x 56 x 56 -- every value up to 4096, then 32 k and 32 k + 1, which is every value of (M + 31) / 32 and so every
// change of (rbs + rb - 1) / rb for every candidate --, cout in {64, 128, 256, 512, 1024, 2048}, K steps in {4, 6, 8, 16, 32, 64, 128},
// the conv3 form on and off, split and bf16 operands, 1 / 2 / 5 / 8 K slices of the generic kernel.  Prints the number of points; exit
// status 1 at the first difference.
#include <stdio.h>

#include <vector>

#include "conv_tiles.h"

namespace old_rules {

int generic(int M, int cout, int slices) {
    int tile;
    const long long t128 = (long long)((M + 127) / 128) * ((cout + 127) / 128);
    const long long t12864 = (long long)((M + 127) / 128) * ((cout + 63) / 64);
    if (cout >= 128 && cout % 128 == 0 && t128 * slices >= 192) tile = 5;
    else if (t12864 * slices >= 192) tile = 6;
    else tile = 3;
    return tile;
}

int patch() { return 9; }

int s3(int M, int cout, bool split) {
    int tile = 0;
    const bool narrow = cout == 64;
    static const int cand[9][3] = {{12, 14, 0}, {13, 8, 0}, {15, 12, 0}, {16, 10, 0}, {21, 7, 0}, {27, 4, 0}, {28, 6, 0}, {19, 20, 1}, {20, 16, 1}};
    const long long rbs = (M + 31) / 32, nts = narrow ? 1 : cout / 128;
    double best = 0;
    for (const auto& cd : cand) {
        if ((cd[2] != 0) != narrow || ((cd[0] == 21 || cd[0] == 27 || cd[0] == 28) && !split)) continue;
        const long long tiles = ((rbs + cd[1] - 1) / cd[1]) * nts;
        const double cost = (double)((tiles + 255) / 256) * (cd[1] + 1.5);
        if (!tile || cost < best) { tile = cd[0]; best = cost; }
    }
    return tile;
}

int s1(long long M, int cout, int nk, bool c3) {
    int tile = 0;
    const int tiles_n = cout / 128;
    static const int cand[6][3] = {{25, 8, 6}, {24, 14, 4}, {26, 8, 3}, {22, 7, 6}, {23, 8, 6}, {29, 4, 6}};      // tile, row blocks, ring depth
    const long long rbs = (M + 31) / 32;
    double best = 0;
    for (const auto& cd : cand) {
        if (nk < cd[2] || (c3 && cd[0] != 24 && cd[0] != 25 && cd[0] != 26)) continue;
        const long long tiles = ((rbs + cd[1] - 1) / cd[1]) * tiles_n;
        double cost = (double)((tiles + 255) / 256) * (cd[1] + 1.5) * (cd[0] == 22 || cd[0] == 23 ? 1.15 : 1.0);
        if (cd[0] == 26) cost = (double)((tiles + 511) / 512) * 2.0 * (cd[1] + 1.5) * (c3 ? 0.8 : nk <= 32 ? 0.88 : 1.05);
        if (!tile || cost < best) { tile = cd[0]; best = cost; }
    }
    return tile;
}

}  // namespace old_rules

int main() {
    std::vector<int> ms;
    const int m_max = 257 * 56 * 56;
    for (int m = 1; m <= 4096; ++m) ms.push_back(m);
    for (int m = 4128; m <= m_max; m += 32) { ms.push_back(m); if (m + 1 <= m_max) ms.push_back(m + 1); }
    ms.push_back(m_max);
    const int couts[] = {64, 128, 256, 512, 1024, 2048}, ksteps[] = {4, 6, 8, 16, 32, 64, 128}, slices[] = {1, 2, 5, 8};
    long long points = 0;
    const auto differ = [](const char* what, int m, int cout, int x, int y, int was, int is) {
        printf("%s: M %d, cout %d, (%d, %d): was tile %d, is tile %d\n", what, m, cout, x, y, was, is);
        return 1;
    };
    if (old_rules::patch() != conv_tiles::choose_patch()) return differ("patch", 0, 0, 0, 0, old_rules::patch(), conv_tiles::choose_patch());
    ++points;
    for (int m : ms)
        for (int cout : couts) {
            for (int s : slices) {
                const int was = old_rules::generic(m, cout, s), is = conv_tiles::choose_generic(m, cout, s);
                if (was != is) return differ("generic", m, cout, s, 0, was, is);
                ++points;
            }
            for (int split = 0; split < 2; ++split) {
                const int was = old_rules::s3(m, cout, split), is = conv_tiles::choose_s3(m, cout, split);
                if (was != is) return differ("3x3 stream", m, cout, split, 0, was, is);
                ++points;
            }
            if (cout % 128) continue;
            for (int nk : ksteps)
                for (int c3 = 0; c3 < 2; ++c3) {
                    const int was = old_rules::s1(m, cout, nk, c3), is = conv_tiles::choose_s1(m, cout, nk, c3);
                    if (was != is) return differ("1x1 stream", m, cout, nk, c3, was, is);
                    ++points;
                }
        }
    printf("tile = 0: %lld points (%zu values of M), the table-driven choice equals the four former rules everywhere\n", points, ms.size());
    return 0;
}
