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
