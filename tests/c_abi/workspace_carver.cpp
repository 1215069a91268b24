// csrc/workspace.h alone, with a main of its own (no HIP, no library): the bump carver over the grids the stages' layouts span --
// runs of 256-byte takes, the track front end's packed 8 / 4-byte planes, mixed alignments in any order, zero-byte takes, a carver
// inside a region of another.  Every offset must be a multiple of its alignment, at or past the end of the take before it (no
// overlap, monotone), and total() must be the rounded end of the last take.  Meant to be built with -fsanitize=address,undefined:
//     c++ -std=c++17 -fsanitize=address,undefined -I human_dynamics_amd/csrc tests/c_abi/workspace_carver.cpp -o carver && ./carver
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "workspace.h"

static long long failures = 0, takes = 0, layouts = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { if (++failures <= 10) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Take { size_t bytes, align; };

// one layout: the takes in order, checked one by one, then written into a real allocation of total() bytes (the sanitizer
// watches the writes: a take that reached past total() or into its neighbour's bytes would show here)
static size_t run(const std::vector<Take>& seq, bool touch) {
    WsCarver c;
    std::vector<size_t> off;
    size_t end = 0;
    for (const Take& t : seq) {
        const size_t before = c.total(), o = c.take(t.bytes, t.align);
        ++takes;
        EXPECT(o % t.align == 0, "offset %zu, align %zu", o, t.align);
        EXPECT(o >= end && o >= before, "offset %zu before the end %zu of the take in front", o, end);
        EXPECT(o - before < t.align, "offset %zu skips %zu bytes, align %zu", o, o - before, t.align);
        end = o + t.bytes;
        EXPECT(c.total() >= end && c.total() - end < t.align && c.total() % t.align == 0, "total %zu after a take ending at %zu, align %zu", c.total(),
               end, t.align);
        off.push_back(o);
    }
    ++layouts;
    if (touch && c.total() <= ((size_t)64 << 20)) {
        unsigned char* buf = (unsigned char*)malloc(c.total() ? c.total() : 1);
        for (size_t i = 0; i < c.total(); ++i) buf[i] = 0;
        for (size_t k = 0; k < seq.size(); ++k)
            for (size_t i = 0; i < seq[k].bytes; ++i) {
                EXPECT(buf[off[k] + i] == 0, "take %zu overlaps an earlier one at byte %zu", k, off[k] + i);
                buf[off[k] + i] = (unsigned char)(k + 1);
            }
        free(buf);
    }
    return c.total();
}

int main() {
    EXPECT(align_up(0, 256) == 0 && align_up(1, 256) == 256 && align_up(256, 256) == 256 && align_up(257, 256) == 512 && align_up(13, 4) == 16 &&
           align_up(80, 8) == 80, "align_up");
    EXPECT(run({}, true) == 0, "an empty layout");
    const int sizes[] = {1, 2, 3, 5, 7, 20, 31, 32, 33, 63, 64, 65, 100, 160, 255, 256, 257, 300, 4096, 100000};
    for (int n : sizes) {
        const size_t m = (size_t)n;
        const bool touch = n <= 300;
        // the f_movie stages (three operand widths), IEF's grouped sets, the ResNet's eight maps, SMPL's groups of 32, a rasteriser slab
        for (size_t e : {(size_t)2, (size_t)4}) {
            run({{m * 2048 * e, 256}, {m * 2048 * 4, 256}, {m * 2048 * 4, 256}, {m * 2048 * 4, 256}, {5 * m * 2048 * 4, 256}}, touch && n <= 64);
            run({{m * 2048 * e, 256}, {m * 2048 * e, 256}, {m * 2048 * e, 256}, {5 * m * 2048 * 4, 256}}, touch && n <= 64);
            for (size_t g = 1; g <= 7; ++g)
                run({{m * 2048 * e, 256}, {g * align_up(m * 1024 * e, 256), 256}, {g * align_up(m * 1024 * e, 256), 256}, {g * align_up(m * 1024 * e, 256), 256},
                     {g * align_up(m * 128 * 4, 256), 256}, {g * align_up(m * 128 * 4, 256), 256}, {g * 4 * m * 1024 * 4, 256}}, touch && n <= 33);
            run({{m * 230 * 232 * 4 * e, 256}, {m * 112 * 112 * 64 * e, 256}, {m * 56 * 56 * 256 * e, 256}, {m * 56 * 56 * 256 * e, 256},
                 {m * 56 * 56 * 256 * e, 256}, {m * 56 * 56 * 256 * e, 256}, {m * 56 * 56 * 64 * e, 256}, {m * 56 * 56 * 64 * e, 256}}, n <= 2);
        }
        const size_t mp = (m + 31) / 32 * 32;
        EXPECT(run({{mp * 224 * 4, 256}, {mp * 288 * 4, 256}}, touch) == align_up(mp * 224 * 4, 256) + align_up(mp * 288 * 4, 256), "SMPL, m = %d", n);
        const size_t ch = m < 64 ? m : 64, nv = 10, nf = 8;
        run({{ch * nv * 16, 256}, {ch * 16, 256}, {ch * nf * 8, 256}, {ch * nf * 48, 256}, {ch * nf * 16, 256}}, true);
        // the track front end: packed double and int planes -- 80 bytes per row, nothing rounded away
        EXPECT(run({{24 * m, 8}, {24 * m, 8}, {24 * m, 8}, {4 * m, 4}, {4 * m, 4}}, touch) == 80 * m, "track planes, n = %d", n);
        // a region carved by a second carver inside the first (the whole-video call): the union of two uses
        WsCarver outer, tail;
        const size_t phi = outer.take((m + 1) * 2048 * 4);
        tail.take(m * 20 * 2048 * 4); tail.take(m * 20 * 2048 * 4); tail.take(m * 2048 * 4); tail.take(3 * m * 85 * 4);
        const size_t resnet = m * 1000 + 17, region = outer.take(tail.total() > resnet ? tail.total() : resnet);
        EXPECT(phi == 0 && region == align_up((m + 1) * 2048 * 4, 256) && region % 256 == 0 && outer.total() >= region + tail.total() &&
               outer.total() >= region + resnet && outer.total() % 256 == 0, "nested carvers, n = %d", n);
    }
    // mixed alignments in every order, zero-byte takes among them
    const size_t aligns[] = {1, 4, 8, 16, 256, 4096}, bytes[] = {0, 1, 3, 4, 7, 8, 9, 255, 256, 257, 1000};
    for (size_t a0 : aligns) for (size_t a1 : aligns) for (size_t a2 : aligns)
        for (size_t b0 : bytes) for (size_t b1 : bytes) for (size_t b2 : bytes)
            run({{b0, a0}, {b1, a1}, {b2, a2}, {0, a0}, {b0, a2}}, b0 + b1 + b2 < 600);
    WsCarver z;
    EXPECT(z.take(0) == 0 && z.total() == 0 && z.take(0, 8) == 0 && z.take(1) == 0 && z.take(0) == 256 && z.take(0) == 256 && z.total() == 256,
           "zero-byte takes neither move the carver nor share bytes with a real take");
    printf("workspace carver: %lld layouts, %lld takes, %lld failures\n", layouts, takes, failures);
    return failures ? 1 : 0;
}
