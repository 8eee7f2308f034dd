// Definitions shared by the convolution kernels of conv_igemm.hip and conv_small.hip: the kernel argument block, the
// elements-per-chunk trait and the small-tile launcher.  The tile primitives (vector types, MFMA wrappers, LDS-DMA, swizzles,
// packed-row order, pack / unpack helpers) live in tile.h.
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
