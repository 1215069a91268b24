// The vocabulary the hand-scheduled split-operand kernels share (conv3x3_stream, conv1x1_stream, b1_unit, unit_pair, bottleneck_split;
// stem, bottleneck and gemm_conv use the waits, the LDS read and the host part): each idiom ONCE.  Free functions and one struct (xfrag); a helper
// moves here when a SECOND kernel needs it.  Schedules -- which wait goes where, with what count -- stay in the kernels.
#pragma once
#include <type_traits>
#include <utility>

#include "common.h"
#include "hmmr_hip.h"

// ---- host: a launch with dynamic LDS.  `once`: the caller's static DeviceOnce of this kernel instantiation; lds_attr: the
// MaxDynamicSharedMemorySize asked for once per device (gemm_conv.hip asks for all 160 KB and launches with less), lds: this launch's
// (static: no instantiation becomes an exported symbol of the library)
template <class K, class... Args>
static int launch_with_lds(K kern, DeviceOnce& once, dim3 grid, dim3 block, int lds_attr, int lds, hipStream_t stream, Args... args) {
    if (const unsigned long long bit = once.due()) {
        HMMR_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, lds_attr));
        once.mark(bit);
    }
    hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
    HMMR_CHECK_HIP(hipGetLastError());
    return 0;
}
// development builds: the stamp buffer's address travels in the reserved debug words
static inline unsigned long long* probe_stamp_buffer() {
    const hmmr_debug_t* d = hmmr_debug_state();
    return (unsigned long long*)(((unsigned long long)(unsigned)d->reserved[1] << 32) | (unsigned)d->reserved[0]);
}

// ---- small types
struct xfrag { shalf8 hi, lo; };            // MFMA B-operand fragment: 32 pixels x 16 channels
template <int V> using ic = std::integral_constant<int, V>;
// f(ic<I0>{}), f(ic<I1>{}), ... in order
template <class F, int... I> __device__ __forceinline__ void static_for(F&& f, std::integer_sequence<int, I...>) { (f(ic<I>{}), ...); }

// ---- address-space pointers (global_load_lds takes them) and the LDS byte address of a __shared__ pointer
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
__device__ __forceinline__ unsigned lds_addr(void* p) { return (unsigned)(unsigned long long)(lptr_t)p; }

// ---- counted waits.  The gfx9 s_waitcnt immediate: vmcnt[3:0] | expcnt[6:4] | lgkmcnt[11:8] | vmcnt_hi[15:14]; 63 / 15 = "do not
// wait" for vmcnt / lgkmcnt, expcnt is never waited for (7)
constexpr unsigned waitcnt_imm(int vm, int lgkm) { return (vm & 15) | (7 << 4) | (lgkm << 8) | ((vm >> 4) << 14); }
static_assert(waitcnt_imm(63, 0) == (63 | (7 << 4) | (0 << 8) | (3 << 14)) && waitcnt_imm(63, 0) == 0xC07F, "lgkmcnt(0) alone: the literal five files spelled out");
static_assert(waitcnt_imm(0, 0) == 0x0070 && waitcnt_imm(63, 15) == 0xCF7F, "everything; nothing");
static_assert(waitcnt_imm(63, 5) == 0xC57F && waitcnt_imm(37, 0) == 0x8075 && waitcnt_imm(37, 15) == 0x8F75, "lgkmcnt(5) alone; vmcnt(37) lgkmcnt(0); vmcnt(37) alone");
template <int N> __device__ __forceinline__ void wait_vm_lgkm0() {            // s_waitcnt vmcnt(N) lgkmcnt(0)
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(N, 0));
}
template <int N> __device__ __forceinline__ void wait_vm() {                  // s_waitcnt vmcnt(N) alone
    static_assert(N >= 0 && N < 64, "vmcnt is a 6-bit counter");
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(N, 15));
}
template <int N> __device__ __forceinline__ void wait_lgkm() {                // s_waitcnt lgkmcnt(N) alone
    static_assert(N >= 0 && N <= 15, "lgkmcnt is a 4-bit counter");
    __builtin_amdgcn_s_waitcnt(waitcnt_imm(63, N));
}

// ---- LDS accesses as inline assembly.  hipcc waits lgkmcnt(0) wherever LDS data is first used -- never a counted wait -- which drains a
// loop's fragment requests whenever an older value is touched (~100 cycles with the matrix pipe idle: profiles/r04a).  These the compiler
// does not track: the caller places its own waits (LDS operations of a wave complete in order)
template <class T, int OFF> __device__ __forceinline__ T lds_rd128(unsigned addr) {
    static_assert(sizeof(T) == 16, "a ds_read_b128");
    T v; asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF)); return v;
}
template <int OFF> __device__ __forceinline__ unsigned long long lds_rd64(unsigned addr) {
    unsigned long long v; asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(v) : "v"(addr), "n"(OFF)); return v;
}
template <int OFF> __device__ __forceinline__ void lds_wr64(unsigned addr, unsigned long long v) {
    asm volatile("ds_write_b64 %0, %1 offset:%2" : : "v"(addr), "v"(v), "n"(OFF) : "memory");
}

// ---- the dump page: where the row stores of pixels beyond M go, so that every wave issues the same vector-memory instructions (the
// counted waits rely on it).  A lane's 16 bytes (g_dump_page + 16 lane), up to 4 row blocks of 128 B further: 96 x 16 B.  One per
// translation unit, declared as g_split_flags is.  The kernels name it directly, not through an accessor: where a kernel names the
// page inside a lambda (host + device to hipcc: conv1x1_stream, unit_pair) hipcc makes it a global symbol read through the GOT; behind
// a __device__ accessor it turns local and pc-relative, another instruction stream (profiles/stream_kit.log)
static __device__ u32x4 g_dump_page[64 + 32] __attribute__((unused));

// ---- dead trunk rows.  Ahead of a stride-2 unit with an identity shortcut the raw trunk has ONE reader, x[:, ::s, ::s] (resnet.hip:
// plan_unit), so the producing launch is told the stride (hmmr_tail_desc_t.trunk_keep_stride) and row m = (img, y, x) of [.][H][W] is
// LIVE iff y % s == 0 and x % s == 0.  A dead row in range takes the dump path for its TRUNK pointer only (same instructions, same
// counted waits; its h1' row is stored as ever), but not to the page above: with 3 rows of 4 aimed at it every CU of an XCD would write
// the same dozen L2 lines.  The region: one 128-byte line per wave -- line (workgroup % TRUNK_DEAD_WGS) * 4 + wave (the 32-pixel block
// of the workgroup), a lane's 16 bytes at 16 * (lane & 7): the 8 lanes of a row piece that hold the same slot of different rows land
// on each other, nobody reads it.  Workgroups are numbered in dispatch order and the chip holds at most 512 of these kernels' at once
// (two per CU), so waves resident together -- on one CU or not -- never share a line.  512 KB: it stays in L2.  Rows beyond M keep
// the page.  Declared and named like the page, for the same reason.
#ifndef TRUNK_DEAD_SHARED_PAGE
#define TRUNK_DEAD_SHARED_PAGE 0    /* A/B: 1 aims the dead rows at the dump page as well (measured: DESIGN.md section 5) */
#endif
constexpr int TRUNK_DEAD_WGS = 1024;
static __device__ u32x4 g_dead_rows[TRUNK_DEAD_WGS * 4 * 8] __attribute__((unused));
static_assert(sizeof(u32x4) * TRUNK_DEAD_WGS * 4 * 8 <= 512 * 1024, "the dead-row region lives in L2");
// where a dead row's 16 bytes go: `wave` = the 32-pixel block of the workgroup, `dlane` = 4 * (lane & 7) (a macro: the kernels name the arrays)
#define TRUNK_DEAD_ROW(wave, dlane) (TRUNK_DEAD_SHARED_PAGE ? (bsplit_t*)g_dump_page + lane * 4 \
                                     : (bsplit_t*)g_dead_rows + (((int)blockIdx.x & (TRUNK_DEAD_WGS - 1)) * 4 + (wave)) * 32 + (dlane))
// host: the keep stride a launch runs with -- the descriptor's (hmmr_bottleneck_tail has checked it), none under hmmr_debug_t.keep_dead_rows;
// counted for hmmr_trunk_keep_launches.  Called once per launch, behind the entry's refusals
static inline int trunk_keep_of(const hmmr_tail_desc_t* d) {
    const int s = hmmr_debug_state()->keep_dead_rows ? 0 : d->trunk_keep_stride;
    if (s > 1) hmmr_count_launch(HMMR_COUNT_TRUNK_KEEP);
    return s;
}
// bit r: row mbase + r of a wave's 32 is live under keep stride s (every bit with s <= 1).  Lane L answers for row L & 31 -- one
// pair of divisions per lane -- and a ballot collects the answers.  Once per tile, where the row pointers are set up: never in a chunk loop
__device__ __forceinline__ unsigned trunk_live_mask(int mbase, int lane, int H, int W, int s) {
    if (s <= 1) return ~0u;
    asm volatile("" : "+s"(H), "+s"(W), "+s"(s));       // (made HERE, per tile: hoisted out of a persistent kernel's tile loop the divisors' reciprocals would sit in vector registers across its chunk loop)
    const unsigned m = (unsigned)(mbase + (lane & 31)), rem = m % (unsigned)(H * W), y = rem / (unsigned)W, x = rem - y * (unsigned)W;
    return (unsigned)__ballot(y % (unsigned)s == 0 && x % (unsigned)s == 0);
}

// ---- the staging tile: a 32 x 32 block of split values on its way from the MFMA's D layout (lane (lr, lh) = pixel lr, channels
// 8 g + 4 lh .. + 3 of register group g) to 16-byte row stores.  32 rows (pixels) of 128 B = 8 slots of 16 B: slot 2 g = the hi halves of
// group g's 8 channels, 2 g + 1 the lo halves, XOR-swizzled by sw = (lr >> 1) & 7.  Row piece q covers rows 8 q .. 8 q + 7: lane L holds
// the 16 bytes of row 8 q + (L >> 3) in physical slot L & 7.  Shared: the slot address and one group's two stores.  Reading the row pieces back
// through a helper, and the BN / clamp / split / stage sequence of a block as one function, kept the parent's instructions in b1_unit only
// and reordered kernels of conv3x3_stream and unit_pair (profiles/stream_kit.log): those stay written out in the kernels
// this lane's 8 bytes of group g, hi (pl 0) or lo (pl 1) halves, in the tile at `tile` (a pointer, or an LDS byte address)
template <class B> __device__ __forceinline__ B stage_slot(B tile, int lr, int lh, int g, int sw, int pl) {
    return tile + lr * 128 + (((2 * g + pl) ^ sw) << 4) + 8 * lh;
}
// one group's split halves (four hi halves, four lo halves, packed): two 8-byte stores
__device__ __forceinline__ void stage_store_group(char* tile, int lr, int lh, int g, int sw, unsigned long long hi, unsigned long long lo) {
    *(unsigned long long*)stage_slot(tile, lr, lh, g, sw, 0) = hi;
    *(unsigned long long*)stage_slot(tile, lr, lh, g, sw, 1) = lo;
}
__device__ __forceinline__ void stage_store_group(char* tile, int lr, int lh, int g, int sw, const unsigned (&h)[2], const unsigned (&l)[2]) {
    *(unsigned long long*)stage_slot(tile, lr, lh, g, sw, 0) = (unsigned long long)h[0] | ((unsigned long long)h[1] << 32);
    *(unsigned long long*)stage_slot(tile, lr, lh, g, sw, 1) = (unsigned long long)l[0] | ((unsigned long long)l[1] << 32);
}
