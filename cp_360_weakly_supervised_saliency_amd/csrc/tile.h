// Tile primitives shared by every MFMA kernel file (conv_igemm, conv_small, wino, clstm_train and the fused stem / band3x3 /
// l1block / lfirst / l2block kernels): the 16-byte vector types, the MFMA wrappers, the LDS-DMA instruction and its counted
// waits, the LDS swizzles, the packed-row channel order, the 16-byte pack / unpack helpers and the zero block.  One definition
// of each; a new kernel file includes this header (conv_common.h includes it too) instead of pasting them.
#pragma once
#include "common.h"

typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(4))) unsigned int u32x4;   // native vector: stays in VGPRs (HIP's uint4 struct
                                                                   // kept one staging set in scratch memory)

// bytes per element of a CP360_* dtype code (0: not a floating-point activation type)
static inline int elem_bytes(int dtype) { return dtype == CP360_F32 ? 4 : ((dtype == CP360_BF16 || dtype == CP360_F16) ? 2 : 0); }
// dtype code -> element type: calls f with a value of the element type as a tag (a generic lambda: `using T = decltype(tag)`) and
// returns what it returns.  The caller has checked the code (elem_bytes(dtype) != 0).  A kernel that exists for the 16-bit types
// only stays uninstantiated for f32 behind `if constexpr (sizeof(T) == 2)`.
template <typename F> static inline auto with_elem(int dtype, F&& f) {
    if (dtype == CP360_F32) return f(float());
    if (dtype == CP360_F16) return f(f16_raw());
    return f(bf16_raw());
}

// 16 zero bytes in device memory: invalid tile rows (m >= M) and the K tail (c >= c_in)
// load from here, so the select happens on the ADDRESS before the load and nothing has
// to wait for the loaded data until the ds_write that consumes it.  (static: one per translation unit)
static __device__ __attribute__((aligned(16))) unsigned int g_zero16[4] = {0u, 0u, 0u, 0u};

// ------------------------------------------------------------------ MFMA: one 16-byte chunk of K
template <typename T>
__device__ __forceinline__ void mma_chunk(f32x4& acc, const u32x4& a, const u32x4& b);

template <>
__device__ __forceinline__ void mma_chunk<float>(f32x4& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma_chunk<bf16_raw>(f32x4& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc,
                                                  0, 0, 0);
}

template <>
__device__ __forceinline__ void mma_chunk<f16_raw>(f32x4& acc, const u32x4& a, const u32x4& b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0,
                                                 0, 0);
}

// ------------------------------------------------------------------ LDS-DMA
// global_load_lds_dwordx4: global -> LDS with no VGPR staging.  A DMA wave-instruction
// writes 1 KiB linearly (LDS address = M0 + lane*16), so the XOR swizzle of
// the LDS image is applied on the SOURCE side: lane l, which lands in physical chunk c
// of row r, fetches the logical chunk that the ds_read side's swizzle (an involution) maps
// there.  The per-lane source address also carries the CubePad / im2col gather.
// Pipeline (one barrier per K step): at step `it` a wave waits (counted vmcnt) for its own
// DMA of step `it`, meets the barrier (everyone's step-`it` data has landed and everyone has
// finished reading the buffer of step it-1), issues the DMA of step it+2 into that freed
// buffer and computes step `it`: every HBM/L2 load has two full MFMA phases to arrive.
// The DMA is issued from inline asm (the compiler would otherwise drain vmcnt(0) before
// every ds_read); its completion is counted by hand (wait_vmcnt below): a kernel knows how
// many DMA instructions each thread issues per step.  M0 is saved and restored around it.
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst /* wave-uniform */) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_dst)
        : "memory");
}

// the same with the non-temporal hint: a weight stream much larger than the 256 MB Infinity Cache, past the head of a workgroup's
// share (ConvK::w_pin) - it then no longer sweeps the cache of the split-K slabs / activations the next launches read, and the heads
// of the streams, which every workgroup asks for at once when the launch starts, are still there from the previous step (measured on
// the Winograd GEMM first: csrc/wino.hip fill_one)
__device__ __forceinline__ void glds16_nt(const void* gsrc, unsigned lds_dst /* wave-uniform */) {
    unsigned keep;
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %2\n\t"
        "s_nop 0\n\t"
        "global_load_lds_dwordx4 %1, off nt\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "v"(gsrc), "s"(lds_dst)
        : "memory");
}

template <int N> __device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

template <int N> __device__ __forceinline__ void wait_vmcnt_upto(int n);   // s_waitcnt vmcnt(min(n, N)), n wave-uniform
template <> __device__ __forceinline__ void wait_vmcnt_upto<0>(int) { wait_vmcnt<0>(); }
template <int N> __device__ __forceinline__ void wait_vmcnt_upto(int n) {
    if (n >= N) wait_vmcnt<N>();
    else wait_vmcnt_upto<N - 1>(n);
}

// ------------------------------------------------------------------ XCD-aware work index
// Workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MiB L2): workgroup blockIdx.x takes work item w such
// that every XCD gets a CONTIGUOUS range of the nwg items - neighbours in w share an operand panel through that XCD's L2.
// reverse: items in descending order (cp360_set_launch_order).  Bijective on [0, nwg): placement affects speed, never results.
// How w splits into (channel tile, pixel tile, split) is the kernel's business.
__device__ __forceinline__ int xcd_work_index(int nwg, int reverse) {
    const int L = blockIdx.x, xcd = L & 7, q = nwg >> 3, r = nwg & 7;
    int w = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (L >> 3);
    if (reverse) w = nwg - 1 - w;
    return w;
}

// ------------------------------------------------------------------ LDS swizzles (byte offset of a 16-byte chunk)
// 128-byte tile rows (8 chunks): chunk c of row r at chunk c ^ ((r >> 1) & 7)
__device__ __forceinline__ int lds_swz(int row, int chunk) {
    return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4);
}
// 64-byte tile rows (4 chunks, one MFMA k-block): chunk c of row r at chunk c ^ ((-(r >> 2)) & 3), which keeps every
// 16-lane ds_read_b128 group on 16 distinct 16-byte slots of the 256-byte bank row (4 rows per bank row)
__device__ __forceinline__ int lds_swz64(int row, int chunk) {
    return row * 64 + ((chunk ^ ((0 - (row >> 2)) & 3)) << 4);
}
// resident patches of 128-byte pixels (band3x3.hip, l1block.hip): chunk c of patch pixel p sits at chunk c ^ px_swz(p), so 16
// consecutive pixels starting ANYWHERE land on 16 distinct 16-byte bank slots
__device__ __forceinline__ int px_swz(int p) { return ((p >> 1) & 3) << 1; }

// ------------------------------------------------------------------ packed row order
// Channel order inside a 32-row group of the packed weights.  MFMA row block i gives a lane the
// four consecutive rows 4*(lane>>4) .. +3; the pack kernel permutes the rows so that blocks 2p
// and 2p+1 TOGETHER give it EIGHT consecutive channels:  packed row 32q + 16*b + 4*g + e  holds
// channel 32q + 8*g + 4*b + e.  A lane then owns a 16-byte (bf16) / 32-byte (f32) piece of a pixel
// and the four lane groups of a pixel 64 / 128 contiguous bytes: outputs, residuals and split-K
// slabs are moved with 16-byte accesses straight from / to global memory.
__device__ __forceinline__ int acc_chan(int i, int lane) { return (i >> 1) * 32 + (lane >> 4) * 8 + (i & 1) * 4; }
// the inverse, for the pack kernels: packed row R <- channel
__host__ __device__ __forceinline__ int row_chan(int R) { return (R & ~31) + ((R >> 2) & 3) * 8 + ((R >> 4) & 1) * 4 + (R & 3); }
// Split-K slabs (cp360_conv_desc.slab_rows) keep the PACKED row order inside each 32-channel group, so the
// four lane groups of a pixel store 64 contiguous bytes per MFMA block (in true channel order a store
// instruction would write 16-byte pieces 32 bytes apart: +37 % HBM write traffic measured).  Column of the
// 4-channel group that starts at channel n (n % 4 == 0):
__host__ __device__ __forceinline__ int slab_col(int n) { return (n & ~31) + ((n >> 3) & 3) * 4 + ((n >> 2) & 1) * 16; }

// ------------------------------------------------------------------ element access
template <typename T> __device__ __forceinline__ float load_as_f32(const T* p);
template <> __device__ __forceinline__ float load_as_f32<float>(const float* p) { return *p; }
template <> __device__ __forceinline__ float load_as_f32<bf16_raw>(const bf16_raw* p) { return bf16_to_f32(*p); }

// store 4 consecutive channels
__device__ __forceinline__ void store4(float* p, const float v[4]) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ void store4(bf16_raw* p, const float v[4]) {
    uint2 o;
    o.x = (unsigned)f32_to_bf16(v[0]) | ((unsigned)f32_to_bf16(v[1]) << 16);
    o.y = (unsigned)f32_to_bf16(v[2]) | ((unsigned)f32_to_bf16(v[3]) << 16);
    *reinterpret_cast<uint2*>(p) = o;
}
__device__ __forceinline__ void store4(f16_raw* p, const float v[4]) {
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
    const f16x4 o = {(f16_raw)v[0], (f16_raw)v[1], (f16_raw)v[2], (f16_raw)v[3]};
    *reinterpret_cast<f16x4*>(p) = o;
}
__device__ __forceinline__ void load4(const f16_raw* p, float v[4]) {
    typedef __attribute__((ext_vector_type(4))) _Float16 f16x4;
    const f16x4 t = *reinterpret_cast<const f16x4*>(p);
    v[0] = (float)t[0]; v[1] = (float)t[1]; v[2] = (float)t[2]; v[3] = (float)t[3];
}
__device__ __forceinline__ void load4(const float* p, float v[4]) {
    float4 t = *reinterpret_cast<const float4*>(p);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}
__device__ __forceinline__ void load4(const bf16_raw* p, float v[4]) {
    uint2 t = *reinterpret_cast<const uint2*>(p);
    v[0] = __uint_as_float(t.x << 16); v[1] = __uint_as_float(t.x & 0xffff0000u);
    v[2] = __uint_as_float(t.y << 16); v[3] = __uint_as_float(t.y & 0xffff0000u);
}

// ------------------------------------------------------------------ direct epilogue (16-byte pieces)
// With the acc_chan row order a lane owns 8 consecutive channels of a pixel per block pair: bias,
// residual, ReLU, ONE rounding and the store happen on 16-byte pieces straight against global memory
// (a pixel's four lane groups cover 64 bytes (16-bit types) / 128 bytes (f32) contiguously) - no LDS
// round trip, no barriers, and the residual loads of JB pixel blocks are in flight together.
__device__ __forceinline__ u32x4 pack8(const float v[8], bf16_raw) {
    u32x4 o;
    o.x = (unsigned)f32_to_bf16(v[0]) | ((unsigned)f32_to_bf16(v[1]) << 16);
    o.y = (unsigned)f32_to_bf16(v[2]) | ((unsigned)f32_to_bf16(v[3]) << 16);
    o.z = (unsigned)f32_to_bf16(v[4]) | ((unsigned)f32_to_bf16(v[5]) << 16);
    o.w = (unsigned)f32_to_bf16(v[6]) | ((unsigned)f32_to_bf16(v[7]) << 16);
    return o;
}
__device__ __forceinline__ u32x4 pack8(const float v[8], f16_raw) {
    const f16x8 h = {(f16_raw)v[0], (f16_raw)v[1], (f16_raw)v[2], (f16_raw)v[3],
                     (f16_raw)v[4], (f16_raw)v[5], (f16_raw)v[6], (f16_raw)v[7]};
    return __builtin_bit_cast(u32x4, h);
}
__device__ __forceinline__ void unpack8(const u32x4& r, float v[8], bf16_raw) {
    v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
    v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
    v[4] = __uint_as_float(r.z << 16); v[5] = __uint_as_float(r.z & 0xffff0000u);
    v[6] = __uint_as_float(r.w << 16); v[7] = __uint_as_float(r.w & 0xffff0000u);
}
__device__ __forceinline__ void unpack8(const u32x4& r, float v[8], f16_raw) {
    const f16x8 h = __builtin_bit_cast(f16x8, r);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)h[e];
}

__device__ __forceinline__ float fast_sigmoid(float x) { return 1.f / (1.f + __expf(-x)); }
