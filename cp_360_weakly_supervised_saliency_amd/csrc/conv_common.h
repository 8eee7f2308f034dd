// Definitions shared by the convolution kernels of conv_igemm.hip and conv_small.hip: the kernel argument block, the
// elements-per-chunk trait, the small-tile launcher and the device pieces every kernel body would otherwise paste - the
// work-item decode (conv_tile_of), the source-pixel map (CP360_SRC_PIXEL_OFF) and the small tile's table of it
// (CP360_BUILD_OFFTAB), where a split's K range starts and how it advances (CP360_SPLIT_START, CP360_K_ADVANCE), the
// element-wise epilogue nest and the predicate in front of it (CP360_EPILOGUE_SCALAR, CP360_VECTOR_EPILOGUE_OK), the small
// tile's eight-channel epilogue (CP360_EPILOGUE_SMALL8) and the half-sub-step stagger of the 8-wave kernels
// (CP360_STAGGER_STEP).  Three sites keep their own text because no shared form compiled to their code - ring_body's map, the
// small tile's split start, epilogue_direct.  The tile primitives (vector types, MFMA wrappers, LDS-DMA,
// swizzles, packed-row order, pack / unpack helpers) live in tile.h.
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

// The shared pieces below are statement macros under band.h's conventions (own locals end in an underscore, arguments are
// parenthesised, the protocol comment sits on the macro): a kernel that uses one compiles to the instructions of the written-out
// form it replaced, which the force-inlined function forms did not.  All need the ConvK `p` in scope.
// ------------------------------------------------------------------ output pixel, tap -> input pixel
// THE address arithmetic of every generic convolution: OFF <- the element offset (inside p.in) of the input pixel that tap (KY, KX)
// of output pixel PIX = (image, oy, ox) reads, through cubepad_src() with GEOM when the convolution sits behind a CubePad
// (pad_mode); -1 when there is no output pixel PIX.  SECOND_TAP: this is the second source's one 1x1 tap (index p.ntap), which
// reads p.in2 at (oy * sy2, ox * sx2) - the offset is then inside p.in2, KY and KX are not evaluated.  Kernels without a second
// source pass `false` and carry no branch for it.  Which tile row a thread owns, the decode of the tap (once per tap where a
// thread has several rows), a guard of its own and where the offset goes are the caller's.
// (ring_body of conv_igemm.hip keeps this map written out - the macro did not compile to its code; a change here goes there too.)
#define CP360_SRC_PIXEL_OFF(OFF, SECOND_TAP, PIX, KY, KX, GEOM)                                                       \
    {                                                                                                                 \
        const int m_ = (PIX);                                                                                         \
        int off_ = -1;                                                                                                \
        if (m_ < p.M) {                                                                                               \
            const int img_ = m_ / p.hw_out, rem_ = m_ - img_ * p.hw_out;                                              \
            const int oy_ = rem_ / p.w_out, ox_ = rem_ - oy_ * p.w_out;                                               \
            if (SECOND_TAP) {                                                                                         \
                off_ = ((img_ * p.h_in2 + oy_ * p.sy2) * p.w_in2 + ox_ * p.sx2) * p.pix_stride2;                      \
            } else {                                                                                                  \
                const int ky_ = (KY), kx_ = (KX);                                                                     \
                const int py_ = oy_ * p.sy + ky_, px_ = ox_ * p.sx + kx_;                                             \
                int pix_;                                                                                             \
                if (p.pad_mode) {                                                                                     \
                    const int grp_ = img_ / 6, f_ = img_ - grp_ * 6;                                                  \
                    pix_ = grp_ * 6 * p.h_in * p.w_in + cubepad_src(f_, py_, px_, (GEOM));                            \
                } else {                                                                                              \
                    pix_ = (img_ * p.h_in + py_) * p.w_in + px_;                                                      \
                }                                                                                                     \
                off_ = pix_ * p.pix_stride;                                                                           \
            }                                                                                                         \
        }                                                                                                             \
        (OFF) = off_;                                                                                                 \
    }

// conv_small.hip's [tap][tile row] table of those offsets, OFFTAB[tap * 64 + r] for the 64 pixels from M0, built by NT threads (TID).
// All divisions and the branchy cubepad_src() run here, once per (tap, row); inside the K loop a tap change is one LDS read per
// thread.  (Computed in the loop - as the big tiles do - the divergent code and the waits the compiler merges at its join points
// cost more than the MFMAs of a 64 x 64 tile.)
#define CP360_BUILD_OFFTAB(OFFTAB, M0, TID, NT)                                                                       \
    {                                                                                                                 \
        const int ntap_all_ = p.ntap + (p.c_in2 > 0 ? 1 : 0);                                                         \
        const CubePadGeom geom_{p.h_in, p.pad, p.pad, p.pad, p.pad};                                                  \
        for (int t_ = (TID); t_ < ntap_all_ * 64; t_ += (NT)) {                                                       \
            const int tp_ = t_ >> 6, r_ = t_ & 63;                                                                    \
            int o_;                                                                                                   \
            CP360_SRC_PIXEL_OFF(o_, tp_ >= p.ntap, (M0) + r_, tp_ / p.kw, tp_ - tp_ / p.kw * p.kw, geom_)             \
            (OFFTAB)[t_] = o_;                                                                                        \
        }                                                                                                             \
    }

// ------------------------------------------------------------------ K range of a split: where it starts, how it advances
// (TAP, C0) <- the first tap and channel of the K range that starts at unit U_BEGIN: a unit is UNIT channels (a 128-byte step, or a
// 64-byte sub-step in the ring kernels), UNITS_PER_TAP of them per tap.  SECOND (compile-time): everything past the first ntap
// taps is the second source's one tap, however long.
// (conv_small.hip keeps its branch form of this written out: the same function, other code.)
#define CP360_SPLIT_START(TAP, C0, SECOND, U_BEGIN, UNITS_PER_TAP, UNIT)                                              \
    {                                                                                                                 \
        (TAP) = (U_BEGIN) / (UNITS_PER_TAP);                                                                          \
        if (SECOND) (TAP) = min((TAP), p.ntap);                                                                       \
        (C0) = ((U_BEGIN) - (TAP) * (UNITS_PER_TAP)) * (UNIT);                                                        \
    }
// One unit further: C0 += UNIT and, at the tap's padded length CPAD, on to the next tap, which SET_TAP(TAP) makes current - while
// MORE_TAPS (`true`, but for the ring kernels: their last tap, the second source's, may be longer than the others' c_pad).
#define CP360_K_ADVANCE(TAP, C0, UNIT, CPAD, MORE_TAPS, SET_TAP)                                                      \
    {                                                                                                                 \
        (C0) += (UNIT);                                                                                               \
        if ((C0) >= (CPAD) && (MORE_TAPS)) {                                                                          \
            (C0) = 0;                                                                                                 \
            ++(TAP);                                                                                                  \
            SET_TAP(TAP);                                                                                             \
        }                                                                                                             \
    }

// ------------------------------------------------------------------ element-wise epilogue
// The vector epilogues (epilogue_lds of conv_igemm.hip) move 16-byte pieces of EPC elements: not for a split-K slab, and only when
// every row of the output and of the residual starts on one.
#define CP360_VECTOR_EPILOGUE_OK(EPC)                                                                                 \
    (!p.partial && (p.c_out % (EPC) == 0) && (p.ld_out % (EPC) == 0) && (p.out_coff % (EPC) == 0) && (p.ld_res % (EPC) == 0))
// The nest that ends every MFMA body when they may not run: a lane holds channels n .. n+3 (acc_chan order) of one pixel for each
// (i, j) sub-tile of ACC[4][MJ] and stores them itself - into the split's f32 slab (true channel order, or slab_col under
// slab_rows), or bias + residual + ReLU, one rounding, store4.  CH0 = n0 + the wave's first tile channel.  The lane's pixel of
// block j is row ROW0 + 16 j + ml counted from pixel BASE, an output pixel iff that row < NROWS: the generic kernels
// count from pixel 0 (BASE 0, ROW0 = m0 + the wave's first tile row, NROWS = p.M), the clip-resident body inside its clip
// (BASE = m0, ROW0 = the wave's first tile row, NROWS = rows_valid).  Needs T, lane, ml = lane & 15 and split in scope.
#define CP360_EPILOGUE_SCALAR(ACC, MJ, CH0, BASE, ROW0, NROWS)                                                        \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_) {                                                                \
        const int n_ = (CH0) + acc_chan(i_, lane);                                                                    \
        if (n_ >= p.c_out) continue;                                                                                  \
        _Pragma("unroll") for (int j_ = 0; j_ < (MJ); ++j_) {                                                         \
            const int row_ = (ROW0) + j_ * 16 + ml;                                                                   \
            if (row_ >= (NROWS)) continue;                                                                            \
            const int m_ = (BASE) + row_;                                                                             \
            float v_[4] = {(ACC)[i_][j_][0], (ACC)[i_][j_][1], (ACC)[i_][j_][2], (ACC)[i_][j_][3]};                   \
            if (p.partial) {                                                                                          \
                store4(p.partial + ((size_t)split * p.M + m_) * p.c_out + (p.slab_rows ? slab_col(n_) : n_), v_);     \
            } else {                                                                                                  \
                if (p.bias) {                                                                                         \
                    const float4 bb_ = *reinterpret_cast<const float4*>(p.bias + n_);                                 \
                    v_[0] += bb_.x; v_[1] += bb_.y; v_[2] += bb_.z; v_[3] += bb_.w;                                   \
                }                                                                                                     \
                if (p.res) {                                                                                          \
                    float r_[4];                                                                                      \
                    load4(reinterpret_cast<const T*>(p.res) + (size_t)m_ * p.ld_res + n_, r_);                        \
                    v_[0] += r_[0]; v_[1] += r_[1]; v_[2] += r_[2]; v_[3] += r_[3];                                   \
                }                                                                                                     \
                if (p.relu) {                                                                                         \
                    v_[0] = fmaxf(v_[0], 0.f); v_[1] = fmaxf(v_[1], 0.f);                                             \
                    v_[2] = fmaxf(v_[2], 0.f); v_[3] = fmaxf(v_[3], 0.f);                                             \
                }                                                                                                     \
                store4(reinterpret_cast<T*>(p.out) + (size_t)m_ * p.ld_out + p.out_coff + n_, v_);                    \
            }                                                                                                         \
        }                                                                                                             \
    }

// Eight consecutive channels of a pixel against global memory, ONE form for both element sizes: they are one 16-byte piece of
// 16-bit elements or two of f32.  add_res8: v += the residual pieces rr; store8: v rounded once (pack8) and stored at dst.
#define CP360_ADD_RES8_16BIT(V, RR)                                                                                   \
    {                                                                                                                 \
        float r_[8];                                                                                                  \
        unpack8((RR)[0], r_, T());                                                                                    \
        _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) (V)[e_] += r_[e_];                                           \
    }
#define CP360_ADD_RES8_F32(V, RR)                                                                                     \
    _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) {                                                                \
        (V)[e_] += __uint_as_float((RR)[0][e_]);                                                                      \
        (V)[4 + e_] += __uint_as_float((RR)[1][e_]);                                                                  \
    }
template <typename T> __device__ __forceinline__ void store8(T* dst, const float (&v)[8]) {
    if constexpr (sizeof(T) == 4) {
        *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<float4*>(dst + 4) = make_float4(v[4], v[5], v[6], v[7]);
    } else {
        *reinterpret_cast<u32x4*>(dst) = pack8(v, T());
    }
}

// The small tile's epilogue (both kernels of conv_small.hip): after the K loop a lane owns EIGHT consecutive channels N .. N+7 of
// pixel m for each of its two pixel blocks (ACC[0][j], ACC[1][j]: the acc_chan row order; MW0 = the wave's first pixel) - the split's
// slab, or bias + residual + ReLU + one rounding, in 16-byte pieces straight against global memory (two per eight f32 channels).
// c_out % 8 == 0 on this path.  Ends the kernel for the lane.  Needs T, lane and split in scope.
#define CP360_EPILOGUE_SMALL8(ACC, N, MW0, ADD_RES)                                                                   \
    {                                                                                                                 \
        const int ml_ = lane & 15;                                                                                    \
        const int n_ = (N);                                                                                           \
        if (n_ >= p.c_out) return;                                                                                    \
        float bb_[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};                                                      \
        if (!p.partial && p.bias) {                                                                                   \
            const float4 t0_ = *reinterpret_cast<const float4*>(p.bias + n_);                                         \
            const float4 t1_ = *reinterpret_cast<const float4*>(p.bias + n_ + 4);                                     \
            bb_[0] = t0_.x; bb_[1] = t0_.y; bb_[2] = t0_.z; bb_[3] = t0_.w;                                           \
            bb_[4] = t1_.x; bb_[5] = t1_.y; bb_[6] = t1_.z; bb_[7] = t1_.w;                                           \
        }                                                                                                             \
        const T* res_ = reinterpret_cast<const T*>(p.res);                                                            \
        T* outp_ = reinterpret_cast<T*>(p.out);                                                                       \
        u32x4 rr_[2][sizeof(T) == 4 ? 2 : 1];                                                                         \
        if (!p.partial && res_) {                          /* both pixel blocks' residual pieces in flight together */\
            _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_) {                                                        \
                const int m_ = (MW0) + j_ * 16 + ml_;                                                                 \
                const T* s_ = m_ < p.M ? res_ + (size_t)m_ * p.ld_res + n_ : reinterpret_cast<const T*>(g_zero16);    \
                rr_[j_][0] = *reinterpret_cast<const u32x4*>(s_);                                                     \
                if (sizeof(T) == 4) rr_[j_][sizeof(T) == 4 ? 1 : 0] = *reinterpret_cast<const u32x4*>(m_ < p.M ? s_ + 4 : s_);   \
            }                                                                                                         \
        }                                                                                                             \
        _Pragma("unroll") for (int j_ = 0; j_ < 2; ++j_) {                                                            \
            const int m_ = (MW0) + j_ * 16 + ml_;                                                                     \
            if (m_ >= p.M) continue;                                                                                  \
            float v_[8];                                                                                              \
            _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) {                                                        \
                v_[e_] = (ACC)[0][j_][e_];                                                                            \
                v_[4 + e_] = (ACC)[1][j_][e_];                                                                        \
            }                                                                                                         \
            if (p.partial) {                                                                                          \
                float* dst_ = p.partial + ((size_t)split * p.M + m_) * p.c_out;                                       \
                store4(dst_ + (p.slab_rows ? slab_col(n_) : n_), v_);                                                 \
                store4(dst_ + (p.slab_rows ? slab_col(n_ + 4) : n_ + 4), v_ + 4);                                     \
                continue;                                                                                             \
            }                                                                                                         \
            _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) v_[e_] += bb_[e_];                                       \
            if (res_) ADD_RES(v_, rr_[j_])                                                                            \
            if (p.relu) {                                                                                             \
                _Pragma("unroll") for (int e_ = 0; e_ < 8; ++e_) v_[e_] = fmaxf(v_[e_], 0.f);                         \
            }                                                                                                         \
            store8(outp_ + (size_t)m_ * p.ld_out + p.out_coff + n_, v_);                                              \
        }                                                                                                             \
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
