// Definitions shared by the convolution kernels of conv_igemm.hip and conv_small.hip: the kernel argument block, the
// elements-per-chunk trait, the small-tile launcher and the device pieces every kernel body would otherwise paste - the
// work-item decode (conv_tile_of) and the half-sub-step stagger of the 8-wave kernels (CP360_STAGGER_STEP).  The tile
// primitives (vector types, MFMA wrappers, LDS-DMA, swizzles, packed-row order, pack / unpack helpers) live in tile.h.
#pragma once
#include "tile.h"

struct ConvK {
    const unsigned char* in;
    const unsigned char* w;
    unsigned char* out;
    const float* bias;
    const unsigned char* res;
    float* partial;
    int n_img, h_in, w_in, c_in, pix_stride, kh, kw, sy, sx, h_out, w_out, c_out;
    int pad_mode, pad, ld_out, out_coff, ld_res, relu, splits;
    int M, c_pad, steps_per_tap, nsteps, steps_per_split, k_total, hw_out;
    int nt, mt, m_fast;
    int clip_rows, nsub, sub_per_split;   // clip-resident kernel: pixels per clip, 64-byte sub-steps in all / per split
    int w_pin;                            // clip-resident kernel: sub-steps at the head of a workgroup's weight stream loaded with the
                                          // default cache policy, the rest non-temporal (conv_igemm.hip, clip_body)
    int reverse;                          // 1: work items in descending order (cp360_set_launch_order)
    int epi_direct;                       // 1: direct 16-byte epilogue, 0: LDS-staged epilogue
    int slab_rows;                        // 1: split-K slabs in packed-row column order (slab_col)
    // second source (cp360_conv_desc.c_in2 > 0): one extra 1x1 "tap" (index kh*kw, packed behind the others)
    // gathered from in2 [n_img, h_in2, w_in2, pix_stride2] at (oy * sy2, ox * sx2) - the Bottleneck's downsample
    // branch accumulated into the conv3 tile (ring kernels only)
    const unsigned char* in2;
    int c_in2, c_pad2, pix_stride2, h_in2, w_in2, sy2, sx2, ntap;
};

template <typename T> struct Elem;
template <> struct Elem<float> { static constexpr int EPC = 4; };      // elements per 16-byte chunk
template <> struct Elem<bf16_raw> { static constexpr int EPC = 8; };
template <> struct Elem<f16_raw> { static constexpr int EPC = 8; };

// The padding of the packed forward weights [rows][tap][c_pad], ONE rule for the packers (conv_igemm.hip) and for every other
// writer of those layouts (adam.hip): rows to 256; the channels of a tap to a 128-byte step in the tap-major layout and to a
// 64-byte sub-step in the channel-major one (cp360_conv_desc.clip_resident).
static inline int conv_c_pad(int c_in, int dtype, int chan_major) {
    const int unit = (chan_major ? 64 : 128) / elem_bytes(dtype);
    return (c_in + unit - 1) / unit * unit;
}
static inline int conv_rows_pad(int c_out) { return (c_out + 255) / 256 * 256; }

// conv_small.hip keeps a [tap][tile row] source-offset table in LDS: kh * kw (+ 1 for a second source) must fit
#define CP360_SMALL_MAX_TAPS 16

// conv_small.hip: the 64 x 64-tile kernel for launches whose pixel count cannot fill the chip with the big tiles
// (k.nt / k.mt / k.m_fast: 64 x 64 tiles, from resolve_launch of conv_igemm.hip).  dtype: CP360_F32 / CP360_BF16 / CP360_F16.
void cp360_launch_conv_small(const ConvK& k, int dtype, hipStream_t st);

// ------------------------------------------------------------------ work item -> (channel tile, pixel tile, split)
// XCD-aware work mapping.  Workgroups are dealt round-robin over the 8 XCDs (each with a private 4 MiB L2): xcd_work_index
// gives every XCD a CONTIGUOUS range of work items, and the items are ordered so that neighbours share an operand panel.
// m_fast: the m-tiles of one (n-tile, split) are adjacent -> the weight panel is fetched from HBM once per XCD and re-read
// from L2 (ConvLSTM: weights >> activations); otherwise n-tiles are adjacent -> the activation panel is shared (ResNet).
// M_FAST: the kernel is only ever launched pixel tiles fastest (the clip-resident kernel, whose workgroups of one
// (channel tile, split) share the weight stream).  Placement only affects speed, never results (bijective map).
// bn x bm: the kernel's tile; n0 / m0: first output channel / first pixel of this workgroup's tile.
template <bool M_FAST = false>
__device__ __forceinline__ void conv_tile_of(const ConvK& p, int bn, int bm, int* n0, int* m0, int* split) {
    const int w = xcd_work_index(p.nt * p.mt * p.splits, p.reverse);
    int nt_i, mt_i;
    if (M_FAST || p.m_fast) {
        mt_i = w % p.mt;
        const int rest = w / p.mt;
        nt_i = rest % p.nt;
        *split = rest / p.nt;
    } else {
        nt_i = w % p.nt;
        const int rest = w / p.nt;
        mt_i = rest % p.mt;
        *split = rest / p.mt;
    }
    *n0 = nt_i * bn;
    *m0 = mt_i * bm;
}

// ------------------------------------------------------------------ half-sub-step stagger of the 8-wave kernels
// One sub-step of the K loop of an 8-wave kernel, its two halves HEAD and TAIL (statements) given by the kernel body.
// A sub-step is two PHASES separated by a second barrier, and the two waves that share a SIMD (w and w+4) run half a
// sub-step apart (MI355X_MICROARCH.md, "Two waves per SIMD", item 9).  HEAD = the fragment reads of the sub-step's stage,
// the refill DMA and whatever MFMAs the kernel puts under them; TAIL = the remaining MFMAs, all operands in registers.
//   waves 0-3 (LAG = false):  B1  HEAD(s)    B2  TAIL(s)
//   waves 4-7 (LAG = true ):  B1  TAIL(s-1)  B2  HEAD(s)
// so while one wave of a SIMD waits for its LDS reads the other feeds the matrix pipe from registers.  Stage s is read
// between B1(s) and B1(s+1) by both groups and refilled after B1(s+1), exactly as without the stagger; a lagging wave
// drains its LDS reads (lgkmcnt) before B1 because the tail operands it read last are first used after it - and runs one
// more TAIL behind its last sub-step.  The DMA completion count in front of B1 (hand-counted vmcnt) is the kernel's.
// (A macro, not a template over two lambdas: that form did not compile to the same code - up to 9 more VGPRs.)
#define CP360_STAGGER_STEP(LAG, HEAD, TAIL)                                                                \
        {                                                                                                  \
            if (LAG) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                    \
            __builtin_amdgcn_s_barrier();                                                                  \
            __builtin_amdgcn_sched_barrier(0);                                                             \
            if (!LAG) HEAD else TAIL                                                                       \
            __builtin_amdgcn_sched_barrier(0);                                                             \
            __builtin_amdgcn_s_barrier();                                                                  \
            __builtin_amdgcn_sched_barrier(0);                                                             \
            if (!LAG) TAIL else HEAD                                                                       \
        }
