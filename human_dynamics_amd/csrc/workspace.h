// The one bump carver for caller-owned workspaces.  Every stage states its layout ONCE, as a host function
// `X_layout(args)` that takes its buffers from a WsCarver in order and returns their offsets and the total; the size query
// returns `layout.total` and the entry point forms every pointer as `base + offset` from the same value, so the bytes
// reported and the bytes used cannot drift apart.  Plain C++: no HIP, no allocation.
#pragma once
#include <stddef.h>

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct WsCarver {
    size_t off = 0;
    // offset of the next `bytes`, a multiple of `align`; the end is rounded up to `align` as well, so a run of takes with one
    // alignment is the sum of the rounded sizes
    size_t take(size_t bytes, size_t align = 256) {
        const size_t o = align_up(off, align);
        off = align_up(o + bytes, align);
        return o;
    }
    size_t total() const { return off; }
};
