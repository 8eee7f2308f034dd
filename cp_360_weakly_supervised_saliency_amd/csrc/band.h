// The pieces the fused static-stage kernels share (band3x3.hip, l1block.hip, l2block.hip, lfirst.hip, stem.hip - and these five
// files only; what EVERY MFMA kernel file uses stays in tile.h): the epilogue piece of an accumulator pair, the A-fragment fetch,
// the cube-padded band gather, the MFMAs over an LDS tile in groups of four pixel blocks, the phase stamp of the diagnostic builds
// and, host side, the 16-bit dtype dispatch, the shared argument checks and the packers' final conversion.  One definition of each.
// A kernel that uses a piece compiles to the instructions of the written-out form it replaced.  The device pieces are therefore
// macros, in the style of CP360_STAGGER_STEP: as force-inlined functions - also with the very text of the written-out form - the
// gather, the epilogue piece and row_chan() compiled to different code in the kernels that used them.
#pragma once
#include "tile.h"

// ------------------------------------------------------------------ epilogue piece of an accumulator pair
// Two 16-row accumulator blocks LO, HI of one pixel block (acc_chan order: together a lane's EIGHT consecutive channels of a pixel) +
// their biases BLO, BHI (expressions in the piece's own counter e_ = 0 .. 3; a residual term is appended there: `b0[e_] + rv[e_]` - NOT parenthesised, the sum
// runs left to right: accumulator + bias + residual) through ACT (CP360_RELU | CP360_NOACT) -> V[8], which the caller rounds once
// with pack8() and stores where it goes (global memory, the t tile, a slice, a B fragment).
#define CP360_RELU(x) fmaxf((x), 0.f)
#define CP360_NOACT(x) (x)
#define CP360_BIAS_ACT8(V, LO, HI, BLO, BHI, ACT)                                                                   \
    _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) {                                                            \
        V[e_] = ACT((LO)[e_] + BLO);                                                                              \
        V[4 + e_] = ACT((HI)[e_] + BHI);                                                                          \
    }

// ------------------------------------------------------------------ A fragments
// Fragment i of a fragment-ordered filter (cp360_frag_pack_1x1 and the conv2 packers) is 1 KiB at BASE + i * 1024, lane l's 16 bytes at
// + l * 16; BASE (const unsigned char*) in global memory (L2 -> registers) or in LDS.  DST[fr_][fk_] <- fragment INDEX, an expression in
// the fetch's own counters fr_ < R and fk_ < K (CP360_LOAD_FRAGS1: DST[fr_], fr_ < R).  Needs lane in scope.
#define CP360_LOAD_FRAGS(DST, R, K, BASE, INDEX)                                                                   \
    _Pragma("unroll") for (int fr_ = 0; fr_ < (R); ++fr_)                                                         \
        _Pragma("unroll") for (int fk_ = 0; fk_ < (K); ++fk_)                                                     \
            DST[fr_][fk_] = *reinterpret_cast<const u32x4*>((BASE) + ((INDEX) * 64 + lane) * 16);
#define CP360_LOAD_FRAGS1(DST, R, BASE, INDEX)                                                                     \
    _Pragma("unroll") for (int fr_ = 0; fr_ < (R); ++fr_) DST[fr_] = *reinterpret_cast<const u32x4*>((BASE) + ((INDEX) * 64 + lane) * 16);
// load_a3(u, a): conv3's fragments of the layer2 / layer3 tails (W3F: order 0 of cp360_frag_pack_1x1, KB3 k-blocks) for unit
// u = pass * H3 + half: the 32-row pair w4 + 4 * pass, k-blocks 4 half .. + 3.  Needs KB3, H3, w4 and lane in scope.
#define CP360_DEF_LOAD_A3(W3F)                                                                                     \
    auto load_a3 = [&](int u, u32x4 (&a)[2][4]) __attribute__((always_inline)) {                                  \
        const int p = w4 + 4 * (u / H3), h = u % H3;                                                              \
        CP360_LOAD_FRAGS(a, 2, 4, reinterpret_cast<const unsigned char*>(W3F), (size_t)((p * 2 + fr_) * KB3 + h * 4 + fk_)) \
    }
// load_a1(q, a): the chained conv1's fragments (W1F: w1 [128, 512], order 0): this wave's 32 rows, K slice q = k-blocks 4 q .. + 3
#define CP360_DEF_LOAD_A1(W1F)                                                                                     \
    auto load_a1 = [&](int q, u32x4 (&a)[2][4]) __attribute__((always_inline)) {                                  \
        CP360_LOAD_FRAGS(a, 2, 4, reinterpret_cast<const unsigned char*>(W1F), (size_t)((w4 * 2 + fr_) * 16 + 4 * q + fk_)) \
    }

// ------------------------------------------------------------------ the cube-padded band gather
// ROWS x NP cube-padded pixels (PATCH_PX in all) of C channels, from padded row ROW0 of face F of the cube XG, to LDS at LDS_DST by
// LDS-DMA: instruction i = patch pixels PPI i .. PPI i + PPI - 1 (1 KiB, CH16 = 64 / PPI 16-byte chunks per pixel), wave WAVE of four
// issues i = WAVE, WAVE + 4, ...; each lane fetches through cubepad_src() (the halo comes from the neighbouring faces), a ragged last
// instruction fills up from the zero block.  Chunk c of patch pixel q_ = (pr_, pc_) lands at chunk c ^ KEY, KEY an expression in the
// gather's own q_, pr_, pc_: px_swz(q_) for 128-byte pixels, the position keys of l2block.hip / lfirst.hip for wider ones (the B reads
// there say why).  Needs the element type T in scope (XG is a const T*); every other name comes in as an argument.
#define CP360_GATHER_BAND_PATCH(XG, C, F, ROW0, NP, GEOM, PATCH_PX, PATCH_INST, PPI, KEY, LDS_DST, WAVE, LANE)      \
    {                                                                                                             \
        const T* xg_ = (XG);                                                                                      \
        _Pragma("unroll 1") for (int inst_ = (WAVE); inst_ < (PATCH_INST); inst_ += 4) {                          \
            const int q_ = inst_ * (PPI) + (LANE) / (64 / (PPI));                                                 \
            const void* src_ = g_zero16;                                                                          \
            if ((PATCH_PX) % (PPI) == 0 || q_ < (PATCH_PX)) {                                                     \
                const int pr_ = q_ / (NP), pc_ = q_ - pr_ * (NP);                                                 \
                const int sp_ = cubepad_src((F), (ROW0) + pr_, pc_, (GEOM));    /* pixel index inside the cube */  \
                src_ = xg_ + (size_t)sp_ * (C) + ((((LANE) & (64 / (PPI) - 1)) ^ (KEY)) << 3);                    \
            }                                                                                                     \
            glds16(src_, __builtin_amdgcn_readfirstlane((LDS_DST) + inst_ * 1024));                               \
        }                                                                                                         \
    }

// ------------------------------------------------------------------ MFMAs over an LDS tile
// ACC[rb][j] += A[rb][kb] . k-block KBASE + kb of pixel block j of TILE ([pixel][16-bit channels], STRIDE bytes per pixel), kb = 0 .. 3,
// the PB pixel blocks in groups of four (fewer live B fragments); the sched_barrier keeps the next group's fragment reads from
// being hoisted (spills).  Needs T, lrow and lchunk in scope.
#define CP360_MMA_OVER_TILE(ACC, A, TILE, STRIDE, KBASE, PB)                                                       \
    _Pragma("unroll") for (int kb = 0; kb < 4; ++kb) {                                                            \
        _Pragma("unroll") for (int j0 = 0; j0 < (PB); j0 += 4) {                                                  \
            u32x4 b[4];                                                                                           \
            _Pragma("unroll") for (int u = 0; u < 4; ++u)                                                         \
                if (j0 + u < (PB))                                                                                \
                    b[u] = *reinterpret_cast<const u32x4*>((TILE) + ((j0 + u) * 16 + lrow) * (STRIDE) + (((KBASE) + kb) * 4 + lchunk) * 16); \
            _Pragma("unroll") for (int rb = 0; rb < 2; ++rb)                                                      \
                _Pragma("unroll") for (int u = 0; u < 4; ++u)                                                     \
                    if (j0 + u < (PB)) mma_chunk<T>((ACC)[rb][j0 + u], (A)[rb][kb], b[u]);                        \
            __builtin_amdgcn_sched_barrier(0);                                                                    \
        }                                                                                                         \
    }

// ------------------------------------------------------------------ phase stamps (diagnostic builds only)
// s_memtime of wave 0 of every workgroup at phase boundary k into buffer[blockIdx.x * 16 + k] (-DL1_STAMPS / -DL2_STAMPS,
// tools/l1_stamps.sh / tools/l2_stamps.sh); needs `wave` and `lane` in scope.  The product build executes no stamp.
#define CP360_PHASE_STAMP(buffer, k)                                                                        \
    { __builtin_amdgcn_sched_barrier(0);                                                                    \
      if (wave == 0 && lane == 0 && blockIdx.x < 8192) buffer[blockIdx.x * 16 + (k)] = __builtin_amdgcn_s_memtime(); \
      __builtin_amdgcn_sched_barrier(0); }

// ------------------------------------------------------------------ host side
// dtype code -> 16-bit element type, for the launches of an entry point: calls launch with a value of the element type as a tag
// (`using T = decltype(tag)`), then returns the status of the launch.  Anything else (F32 included) is refused with
// CP360_ERR_BAD_DTYPE and instantiates nothing - these kernels exist for the 16-bit types only.
template <typename F> static inline int with_elem16(int dtype, F&& launch) {
    if (dtype == CP360_BF16) launch(bf16_raw());
    else if (dtype == CP360_F16) launch(f16_raw());
    else return CP360_ERR_BAD_DTYPE;
    CP360_CHECK_HIP();
    return CP360_OK;
}
// the argument checks of the per-face launches, in the order the ABI tests pin: batch, whole cubes, the supported faces, 32-bit pixel
// offsets (n_img x face x face x channels elements)
static inline int check_faces(int n_img, bool supported, int face, int channels) {
    if (n_img <= 0) return CP360_ERR_BAD_SHAPE;
    if (n_img % 6 != 0) return CP360_ERR_BATCH_NOT_6N;
    if (!supported) return CP360_ERR_UNSUPPORTED;
    if ((long long)n_img * face * face * channels >= (1LL << 31)) return CP360_ERR_BAD_SHAPE;
    return CP360_OK;
}
// a packer's final conversion of the folded weight (the product with the BN scale is the packer's own: see frag_pack_kernel)
template <typename T> __device__ __forceinline__ void store_folded(T* __restrict__ packed, int idx, float v) {
    if constexpr (__is_same(T, f16_raw)) packed[idx] = (f16_raw)v;
    else packed[idx] = f32_to_bf16(v);
}
