/* libcp360 - C ABI of the MI355X (gfx950) 360-saliency hot path.
 *
 * The reference (hsientzucheng/CP-360-Weakly-Supervised-Saliency) has no FFI layer:
 * its "operator API" is the Python call surface of model/cube_pad.py,
 * model/resnet_cubic.py, model/clstm.py, utils/equi_to_cube.py,
 * utils/cube_to_equi.py and static_model/class_activation_model.py.  The Python
 * shims in cp_360_weakly_supervised_saliency_amd/ keep those names and bind the
 * entry points below through ctypes.  Each entry point cites
 * the reference code whose arithmetic it replaces.
 *
 * Conventions
 *  - plain pointers and sizes only; every buffer is caller-allocated DEVICE memory
 *    unless the parameter name ends in _host;
 *  - every function is asynchronous on the hipStream_t passed as `void* stream`
 *    (0 = the null stream) and never allocates, frees or synchronises;
 *  - return value: 0 = ok, negative = cp360_status; no exceptions, no exit()
 *    (the reference print+exit()s on batch % 6 != 0, cube_pad.py:33-35);
 *  - face order along the batch dimension is [back, down, front, left, right, top]
 *    (cube_pad.py:49), batches are frame-major / face-minor ([6N, ...]);
 *  - "NCHW" is the reference's tensor layout; "NHWC" (channels innermost) is the
 *    layout the fused pipeline keeps in HBM between kernels.
 */
#ifndef CP360_H
#define CP360_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    CP360_OK = 0,
    CP360_ERR_BAD_SHAPE = -1,      /* negative / zero / inconsistent sizes        */
    CP360_ERR_BATCH_NOT_6N = -2,   /* cube_pad.py:33-35                           */
    CP360_ERR_NOT_SQUARE = -3,     /* CubePad transposes strips: faces must be n x n */
    CP360_ERR_BAD_DTYPE = -4,
    CP360_ERR_NULL = -5,
    CP360_ERR_ALIGN = -6,          /* channel counts / strides not 16-byte friendly */
    CP360_ERR_HIP = -7,            /* a HIP runtime call failed                   */
    CP360_ERR_UNSUPPORTED = -8
} cp360_status;

typedef enum {
    CP360_F32 = 0,
    CP360_BF16 = 1,
    CP360_F16 = 2,
    CP360_U8 = 3
} cp360_dtype;

const char* cp360_strerror(int status);
/* library / ABI version: major*10000 + minor*100 + patch.  Bumped on EVERY change of a struct, a
 * signature or a packed-weight layout: the binding (_lib.py: ABI_VERSION) refuses a library whose
 * version or sizeof(cp360_conv_desc) differs, so a stale out-of-band .so fails at load time. */
#define CP360_VERSION 306
int cp360_version(void);
/* sizeof(cp360_conv_desc) as the library was compiled. */
size_t cp360_conv_desc_bytes(void);

/* ------------------------------------------------------------------ K2: CubePad
 * Replaces CubePad.forward / CubePadding.forward, model/cube_pad.py:28-42,95-216
 * (33 torch.cat + 8 index_select per call).  Pure permutation-with-replication of
 * input elements -> results are bit-exact for every dtype.
 */

/* Host helper: the (face, i, j) -> flat source index table the kernels implement
 * (f'*n*n + i'*n + j'), int32 [6, n+pt+pd, n+pl+pr] written to host memory.  Same
 * inline function as the device code; used by tests and by callers that want to
 * gather on their own. */
int cp360_cubepad_table_host(int n, int pl, int pr, int pt, int pd, int32_t* table_host);

/* x [n6, C, n, n] -> y [n6, C, n+pt+pd, n+pl+pr], elem_size in {1, 2, 4, 8} bytes. */
int cp360_cubepad_nchw(const void* x, void* y, int n6, int C, int n,
                       int pl, int pr, int pt, int pd, int elem_size, void* stream);

/* x [n6, n, n, C] -> y [n6, n+pt+pd, n+pl+pr, Cy] with Cy >= C (extra channels are
 * written as zero); C*elem_size and Cy*elem_size must be multiples of 4 bytes. */
int cp360_cubepad_nhwc(const void* x, void* y, int n6, int C, int Cy, int n,
                       int pl, int pr, int pt, int pd, int elem_size, void* stream);

/* ------------------------------------------------------------------ layout glue */
/* [N, C, H, W] <-> [N, H, W, C]; dtype CP360_F32 or CP360_BF16 on either side (the
 * fused pipeline's bf16 mode converts here).  The NHWC side may be a channel slice of
 * a wider pixel: ld = elements per NHWC pixel (0 = C, dense), coff = first channel -
 * this is how clstm.py:55's torch.cat((input_, prev_hidden), 1) is laid out. */
int cp360_nchw_to_nhwc(const void* x, void* y, int N, int C, int H, int W,
                       int in_dtype, int out_dtype, int ld_y, int y_coff, void* stream);
int cp360_nhwc_to_nchw(const void* x, void* y, int N, int C, int H, int W,
                       int in_dtype, int out_dtype, int ld_x, int x_coff, void* stream);

/* ------------------------------------------------------------------ K1: equi -> cube
 * Replaces Equi2Cube.to_cube (utils/equi_to_cube.py:112-129, 18 cv2.remap calls per
 * frame) fused with the x/255 of dataset_feat_extractor.py:142, im_norm
 * (utils/utils.py:28-33), the float32 cast and the HWC->CHW permute of
 * class_activation_model.py:55.
 *   equi   [F, H, W, 3]   u8 or f32 (HWC, as decoded frames arrive)
 *   grid   [6, cd, cd, 2] f32 (x, y) - the float32 maps to_cube hands to cv2.remap
 *   out    F frames x 6 faces:
 *            out_layout 0: [6F, 3, cd, cd]           (NCHW, the reference's batch)
 *            out_layout 1: [6F, cd, cd, 4]           (NHWC, 4th channel = 0)
 *   value  = (bilinear(equi * scale) - mean[c]) * istd[c]
 *   cv_fixed_point != 0: OpenCV INTER_LINEAR coordinate quantisation (1/32 px,
 *   round-half-even), taps outside the image contribute 0 (BORDER_CONSTANT).
 */
int cp360_equi2cube(const void* equi, const float* grid, void* out,
                    int F, int H, int W, int cd,
                    const float* mean3_host, const float* istd3_host, float scale,
                    int in_dtype, int out_dtype, int out_layout, int cv_fixed_point,
                    void* stream);

/* ------------------------------------------------------------------ K6: cube -> equi
 * Replaces Cube2Equi.to_equi_nn (utils/cube_to_equi.py:37-66: six full-size
 * grid_samples + masked scatter) and, when out_max != NULL, the channel max of
 * temporal_model/test_temporal.py:83-84.
 *   x        [6B, C, w, w] (layout 0, NCHW) or [6B, w, w, C] (layout 1, NHWC), f32
 *   face_map [2w, 4w] int8, coord [2w, 4w, 2] f32 = pixel-space sampling position
 *            (x, y) already un-normalised on the host (align_corners folded in)
 *   out_full [B, C, 2w, 4w] f32 or NULL;  out_max [B, 2w, 4w] f32 or NULL
 */
int cp360_cube2equi(const float* x, const int8_t* face_map, const float* coord,
                    float* out_full, float* out_max, int B, int C, int w,
                    int layout, void* stream);

/* ------------------------------------------------------------------ K0: PIL-exact Lanczos resize
 * Replaces Image.fromarray(frame).convert('RGB').resize((w, h), resample=Image.LANCZOS) of
 * static_model/dataset_feat_extractor.py:119-142 (the frame resize in front of the cube
 * projection) for uint8 HWC frames, bit-exact with Pillow's 8-bit resampler.
 */
/* Taps per output index for a resize in_size -> out_size (Pillow's ksize); < 0: error. */
int cp360_resize_ksize(int in_size, int out_size);
/* HOST: Pillow's coefficient tables for one axis.  bounds int32 [out_size][2] = (first input
 * index, tap count), kk int32 [out_size][ksize] 22-bit fixed point.  Returns ksize. */
int cp360_resize_coeffs_host(int in_size, int out_size, int* bounds, int* kk);
/* The same for Pillow's other filters: filter 0 = LANCZOS (support 3), 1 = BICUBIC (a = -0.5, support 2 -
 * utils/utils.py:21, the overlay's heatmap.resize(..., resample=Image.CUBIC)). */
int cp360_resize_ksize2(int in_size, int out_size, int filter);
int cp360_resize_coeffs_host2(int in_size, int out_size, int filter, int* bounds, int* kk);
/* in u8 [F, h_in, w_in, 3] -> out u8 [F, h_out, w_out, 3] (device); the filter is whatever the tables hold.  Tables are DEVICE copies of
 * cp360_resize_coeffs_host(w_in, w_out) / (h_in, h_out); tmp u8 [F, h_in, w_out, 3] is needed
 * when both axes change (horizontal pass first, as Pillow). */
int cp360_resize_lanczos_u8(const void* in, void* out, void* tmp, int F, int h_in, int w_in,
                            int h_out, int w_out, const int* hbounds, const int* hkk, int hksize,
                            const int* vbounds, const int* vkk, int vksize, void* stream);
/* Which kernels that call runs, as text, without launching: "horizontal <none | LDS window | bytewise>, vertical <none | dword |
 * bytewise>", or "copy" when neither axis changes.  The choice depends on the geometry, F and the alignment of the three
 * pointers (never dereferenced here; tmp as for the call).  The call launches from the same record.  Returns the length
 * written (without the terminating 0; truncated to cap - 1) or a negative status.  HOST: needs no GPU. */
int cp360_resize_plan_describe(const void* in, const void* out, const void* tmp, int F, int h_in, int w_in,
                               int h_out, int w_out, int hksize, int vksize, char* buf, size_t cap);

/* ------------------------------------------------------------------ K3/K4/K5: convolution
 * Implicit-GEMM convolution on MFMA.  Replaces nn.Conv2d(+BatchNorm2d eval)(+ReLU)
 * (+residual add) of model/resnet_cubic.py:85-106,163-175, the per-face CAM GEMM of
 * static_model/class_activation_model.py:70-83 (as a 1x1 convolution) and the three
 * 3x3 convolutions of model/clstm.py:56-64.  Zero padding never occurs on this path
 * (every reference conv has padding=0); the CubePad(p) that precedes a 3x3 / 7x7 conv
 * is fused into the tile loader (pad_mode 1) instead of being materialised.
 */
typedef struct {
    int dtype;        /* CP360_F32 (mfma_f32_16x16x4_f32, exact f32), CP360_BF16
                         (mfma_f32_16x16x32_bf16) or CP360_F16 (mfma_f32_16x16x32_f16),
                         f32 accumulate - activations, packed weights and outputs
                         all have this type                                       */
    int n_img;        /* images (6 * frames)                                      */
    int h_in, w_in;   /* spatial size of the (unpadded) input tensor              */
    int c_in;         /* K elements taken per tap (normally = channels)           */
    int pix_stride;   /* elements between neighbouring input pixels (>= c_in for a
                         normal conv; 4 for the stem's 8-pixel x 4-channel trick) */
    int kh, kw;       /* taps                                                     */
    int sy, sx;       /* stride in input pixels                                   */
    int h_out, w_out;
    int c_out;
    int pad_mode;     /* 0: no padding; 1: fused CubePad(pad) - needs h_in == w_in */
    int pad;
    int ld_out;       /* elements between output pixels (>= c_out)                */
    int out_coff;     /* first output channel inside an ld_out-wide pixel         */
    int ld_res;       /* residual pixel stride (0 when residual == NULL)          */
    int relu;
    int splits;       /* split-K factor (>= 1); > 1 needs `partial`               */
    int tile_px;      /* 0: the library's launch planner picks the tile; for c_out >=
                         256 (tuning, tests): 128 / 160 / 256 / 304 force the pixel tile
                         of the 8-wave 256-channel kernels (160: 16-bit types only - the
                         tile the planner takes when the larger ones leave CUs without
                         a workgroup; 129 = the 256x128 short-K
                         kernel that runs two workgroups per CU), 64 forces the
                         4-wave 128x128 kernel; any c_out % 8 == 0: 6464 forces the
                         64 x 64-tile small-M kernel (csrc/conv_small.hip), which the
                         planner picks by itself for f32 launches that cannot fill the
                         chip with the big tiles (one frame = 6 faces: BASELINE C2)  */
    int clip_resident;/* 1: CubePad(1) + 3x3 stride-1 convolution on cube faces small
                         enough that a whole cube (6 n^2 <= 304 pixels, n <= 7: the
                         ConvLSTM of model/clstm.py at cube size 224) is one tile:
                         the packed weights are channel- and tile-major
                         ([n / 256][c / 64 B][tap][n % 256][64 B]) and
                         every tap reads the clip's activations from an LDS-resident
                         tile (cubepad halo never leaves the cube).  Also 16x16 faces
                         (cube size 512): one face per tile, resident with its CubePad
                         ring (18 x 18 rows); and 8x8 faces (cube size 256): half a
                         cube (three faces) per tile with the whole cube resident.
                         Must be the same at pack and forward time; other
                         geometries: UNSUPPORTED                                     */
    int slab_rows;    /* 1: the f32 `partial` sums keep the packed row order inside each
                         32-channel group (the 4-channel group of channel n sits at
                         column (n & ~31) + ((n >> 3) & 3) * 4 + ((n >> 2) & 1) * 16), so
                         a pixel's lanes store 64 contiguous bytes; cp360_conv_finish
                         (same desc) and cp360_lstm_gates(slab_rows = 1) read that order.
                         Needs c_out % 32 == 0.  0: true channel order (raw CAM scores) */
    /* --- second source (0 = none): one more 1x1 filter accumulated into the same output tile, gathered
       from a second tensor in2 [n_img, h_in2, w_in2, pix_stride2] at pixel (oy * sy2, ox * sx2):
       out = act(conv(in) + W2 . in2 + bias (+ residual)).  This is the Bottleneck's downsample branch
       (model/resnet_cubic.py:99-104: conv1x1(stride) + BatchNorm on the block input, added to bn3's output
       before the ReLU) computed inside conv3's tile, so its [M, c_out] result never goes through HBM.
       Needs c_out >= 256, no clip_resident; pack with cp360_conv_pack_weights2, run with
       cp360_conv_forward2. */
    int c_in2, pix_stride2, h_in2, w_in2, sy2, sx2;
} cp360_conv_desc;

/* Bytes of packed weights for a desc (rows padded to the tile, K padded per tap). */
size_t cp360_conv_packed_bytes(const cp360_conv_desc* d);
/* Split-K factor (>= 1) that fills the 256 CUs for this geometry (d->splits ignored). */
int cp360_conv_suggest_splits(const cp360_conv_desc* d);
/* Which kernel and split count the planner picks for this descriptor, as text (e.g. "conv_small 64x64, 228 workgroups, splits 3").
 * Returns the length written (without the terminating 0; truncated to cap - 1) or a negative status. */
int cp360_conv_plan_describe(const cp360_conv_desc* d, char* buf, size_t cap);
/* With BOTH weight layouts at hand (tap-major and clip-resident): 1 = launch this descriptor's geometry on the
 * clip-resident kernel, 0 = on the tap-major path (whose planner then picks the 64 x 64-tile kernel: few cubes and few
 * output channels, e.g. layer4's conv2 of ONE frame in f32, give the clip kernel 2 tiles for 256 CUs).  d->clip_resident
 * and d->splits are ignored. */
int cp360_conv_prefer_clip(const cp360_conv_desc* d);
/* The tile_px value that names the kernel the planner launches this descriptor on (0: the kernel follows from the
 * descriptor without the image count - clip-resident, fewer than 256 output channels - or the descriptor is refused).
 * Written into a descriptor of the same convolution on MORE images it keeps that launch on the same kernel, where the
 * cost model would choose again by rounds of the chip (the joint back half of cp360_resnet_forward_multi). */
int cp360_conv_plan_tile(const cp360_conv_desc* d);
/* Bytes of split-K workspace (0 when splits == 1). */
size_t cp360_conv_partial_bytes(const cp360_conv_desc* d);
/* Pack OIHW f32 weights [c_out, c_in_w, kh_w, kw_w] times scale[c_out] (BatchNorm
 * folding; NULL = 1) into the kernel's [c_out_pad][tap][c_pad] layout and dtype.
 * stem_mode != 0 packs a [c_out, 3, 7, 7] filter for the kh=7, kw=1, c_in=32 form
 * (k index = kx*4 + c). */
int cp360_conv_pack_weights(const cp360_conv_desc* d, const float* w_oihw, const float* scale,
                            void* packed, int stem_mode, void* stream);
/* Same with a second source (d->c_in2 > 0): w2_oi f32 [c_out, c_in2] times scale2[c_out] is packed behind
 * the taps of the first filter. */
int cp360_conv_pack_weights2(const cp360_conv_desc* d, const float* w_oihw, const float* scale,
                             const float* w2_oi, const float* scale2, void* packed, void* stream);
/* out = act(conv(in) + bias (+ residual)).  bias f32 [c_out] or NULL.
 * d->splits > 1, or out == NULL: the raw f32 sums go to `partial`
 * ([splits, M, c_out], M = n_img*h_out*w_out; bias / residual / relu NOT applied)
 * and cp360_conv_finish or cp360_lstm_gates must follow. */
int cp360_conv_forward(const cp360_conv_desc* d, const void* in, const void* packed_w,
                       const float* bias, const void* residual, void* out,
                       float* partial, void* stream);
/* cp360_conv_forward with the second source in2 (NULL iff d->c_in2 == 0). */
int cp360_conv_forward2(const cp360_conv_desc* d, const void* in, const void* in2, const void* packed_w,
                        const float* bias, const void* residual, void* out,
                        float* partial, void* stream);
/* out = act(sum_s partial[s] + bias (+ residual)) in d->dtype at the desc's ld_out/out_coff. */
int cp360_conv_finish(const cp360_conv_desc* d, const float* partial, const float* bias,
                      const void* residual, void* out, void* stream);
/* The same with one more f32 addend `extra` [M, c_out] in the slabs' column order (d->slab_rows). */
int cp360_conv_finish_add(const cp360_conv_desc* d, const float* partial, const float* extra, const float* bias,
                          const void* residual, void* out, void* stream);

/* The shape-specific fused kernels (resident-patch stem, stem + max-pool, layer1 / layer2 / layer3 Bottleneck tails, layer2's
 * first block, the launch-order hint) are INTERNAL building blocks of cp360_resnet_forward: include/cp360_internal.h.  A binder
 * of the reference needs the stage contexts (bottom of this file), the per-operator calls K0 / K1 / K2 / K6 / K7 / K8 / K9 and,
 * for its own networks, the generic convolution above. */

/* ------------------------------------------------------------------ K3b: max-pool
 * CubePad(1) + MaxPool2d(3, stride 2, padding 0) (resnet_cubic.py:128,169-170),
 * NHWC, pad fused: x [n6, n, n, C] -> y [n6, (n-1)/2+... , .., C] with
 * h_out = (n + 2 - 3)/2 + 1. */
int cp360_cubepad_maxpool3s2(const void* x, void* y, int n6, int n, int C, int dtype, void* stream);

/* ------------------------------------------------------------------ K5: ConvLSTM gates
 * model/clstm.py:68-80.  gates_partial: f32 [splits, M, 4*Hc] pre-activation sums
 * (split-K slabs of the Gates convolution, channel order in|remember|out|cell),
 * bias f32 [4*Hc]; c_prev/c_next f32 [M, Hc]; h_out (dtype h_dtype) is written at
 * h_out[m*ld_h + h_coff + j]; h_f32 (optional) receives an f32 copy [M, Hc]. */
int cp360_lstm_gates(const float* gates_partial, int splits, const float* bias,
                     const float* c_prev, float* c_next, void* h_out, int h_dtype,
                     int ld_h, int h_coff, float* h_f32, int M, int Hc, int slab_rows, void* stream);
/* The same plus the NEXT step's input: x_next f32 (frame t+1 of clip 0; clip b at + b*clip_stride elements,
 * pixel-major [P, Hc]) is window-normalised with minmax [M/P, 2] (test_temporal.py:77) and written to
 * h_out[m*ld_h + x_coff + j] - the x half of the ConvLSTM's concatenated input - in the same pass (one launch per
 * step less).  Needs input_size == Hc.  x_next == NULL: plain cp360_lstm_gates. */
int cp360_lstm_gates_next(const float* gates_partial, int splits, const float* bias,
                          const float* c_prev, float* c_next, void* h_out, int h_dtype,
                          int ld_h, int h_coff, float* h_f32, int M, int Hc, int slab_rows,
                          const float* x_next, const float* minmax, int x_coff, int P, size_t clip_stride,
                          void* stream);
/* The same when the clips sit in n_groups separately allocated buffers of group_clips clips each (cp360_clstm_window_multi):
 * clip b's frame is at x_groups[b / group_clips] + (b % group_clips) * clip_stride; x_groups is a HOST array of
 * 1 .. CP360_MAX_CLIP_GROUPS device pointers, minmax [M/P, 2] covers all clips.  One group = cp360_lstm_gates_next. */
#define CP360_MAX_CLIP_GROUPS 4
int cp360_lstm_gates_next_groups(const float* gates_partial, int splits, const float* bias,
                                 const float* c_prev, float* c_next, void* h_out, int h_dtype,
                                 int ld_h, int h_coff, float* h_f32, int M, int Hc, int slab_rows,
                                 const float* const* x_groups, int n_groups, int group_clips, const float* minmax,
                                 int x_coff, int P, size_t clip_stride, void* stream);

/* ------------------------------------------------------------------ K5t: ConvLSTM training
 * The backward pass of one cell update (model/clstm.py:54-80) and of the saliency map (to_equi_nn + channel max), for
 * temporal_model/train_temporal.py.  Operand dtypes: CP360_F32 or CP360_BF16 (GEMM operands / activations); accumulation,
 * cell state, gate activations and every gradient of a parameter are f32.  Each gradient element is written by one thread
 * in a fixed order: results are bit-reproducible.  M = pixels = n_img * face^2, n_img = 6 * clips, Hc = hidden channels.
 *
 * Forward gate epilogue: cp360_lstm_gates (plain slabs, slab_rows 0) that also keeps acts f32 [M, 4 Hc]: the activated gates
 * in|remember|out|cell (clstm.py:68-76) for the backward pass. */
int cp360_train_gates(const float* gates_partial, int splits, const float* bias, const float* c_prev, float* c_next,
                      void* h_out, int h_dtype, int ld_h, int h_coff, float* h_f32, float* acts, int M, int Hc, void* stream);
/* dh f32 [M, Hc] (d hidden_t), dc f32 [M, Hc] (in: d cell_t from step t+1, out: d cell_{t-1}), acts / c_prev / c_next as saved
 * by cp360_train_gates  ->  dgates [M, 4 Hc] (dtype dg_dtype): the gradient of the Gates convolution's output. */
int cp360_train_gates_backward(const float* dh, float* dc, const float* acts, const float* c_prev, const float* c_next,
                               void* dgates, int dg_dtype, int M, int Hc, void* stream);
/* Data gradient ("dgrad") of CubePad(1) + 3x3 convolution, in two launches.  The filter f32 OIHW [c_out, c_in, 3, 3] is packed
 * once per weight version for input channels [ci0, ci0 + n): packed [n][9 c_out] (k = tap * c_out + co).
 * cp360_train_dgrad: dy [n_img, face, face, c_out] -> dxpad f32 [n_img, face+2, face+2, n], the "full" correlation onto the
 * zero-padded grid.  cp360_train_cubepad_adjoint then sums each padded position onto its CubePad source (a gather over the
 * inverse table of cp360_train_cubepad_inverse_host: offsets [6 face^2 + 1], entries [6 (face+2)^2] = padded positions of
 * one cube, ascending), masks with (act > 0) when act (dtype act_dtype: F32 or dx_dtype, [.., act_ld], channels from
 * act_coff) is given, and writes (accumulate 0) or adds onto (1) dx [n_img, face, face, n] of dtype dx_dtype. */
size_t cp360_train_dgrad_packed_bytes(int dtype, int c_out, int n);
int cp360_train_dgrad_pack(int dtype, const float* w, int c_out, int c_in, int ci0, int n, void* packed, void* stream);
int cp360_train_dgrad(int dtype, const void* dy, int n_img, int face, int c_out, const void* packed, int n, float* dxpad,
                      void* stream);
int cp360_train_cubepad_inverse_host(int face, int32_t* offsets, int32_t* entries);
int cp360_train_cubepad_adjoint(const float* dxpad, const int32_t* offsets, const int32_t* entries, int n_img, int face, int n,
                                const void* act, int act_dtype, int act_ld, int act_coff, void* dx, int dx_dtype,
                                int accumulate, void* stream);
/* Weight gradient ("wgrad"), ONE launch for all steps: dy [n_img, face, face, c_out] and x [n_img, face, face, ldx] (channels
 * [0, c_in) are the convolution's input) of the same dtype, n_img = steps * 6 * clips; pad_table int32 [6, face+2, face+2]
 * = cp360_cubepad_table_host(face, 1, 1, 1, 1) on the device.  dw f32 OIHW [c_out, c_in, 3, 3] = sum dy * CubePad(x), db f32
 * [c_out] = sum dy (NULL: not computed); written (accumulate 0) or added onto (1). */
int cp360_train_wgrad(int dtype, const void* dy, const void* x, int ldx, const int32_t* pad_table, int n_img, int face,
                      int c_out, int c_in, float* dw, float* db, int accumulate, void* stream);
/* Saliency map of the hidden state h f32 [6B, w, w, C] (NHWC) as cp360_cube2equi(want_max) plus the argmax channel per output
 * pixel (int32 [B, 2w, 4w]; ties: the lowest channel, as torch.max on the CPU), and its backward: dmap f32 [B, 2w, 4w] is
 * ADDED onto dh f32 [6B, w, w, C] through the argmax channel and the bilinear taps (zero padding), a gather over the inverse
 * table of cp360_train_c2e_inverse_host (offsets [6 w^2 + 1], entries [32 w^2] = output pixel << 2 | tap; returns the number
 * of entries or a negative status). */
int cp360_train_saliency_forward(const float* h, const int8_t* face_map, const float* coord, float* out_max, int32_t* argmax,
                                 int B, int C, int w, void* stream);
int cp360_train_c2e_inverse_host(const int8_t* face_map, const float* coord, int w, int32_t* offsets, int32_t* entries);
int cp360_train_saliency_backward(const float* dmap, const int32_t* argmax, const float* coord, const int32_t* offsets,
                                  const int32_t* entries, float* dh, int B, int C, int w, void* stream);

/* ------------------------------------------------------------------ K5w: CubePad(1) + 3x3 convolution in the Winograd domain
 * The three ConvLSTM convolutions of model/clstm.py:56-64 as F(2x2, 3x3) for the 16-bit types: a w x w face is cut into
 * th x th tiles of 2 x 2 outputs (th = ceil(w / 2)); U = G g G^T is packed once per filter (16 matrices [c_out, c_in]), the
 * input transform V = B^T d B reads the cube-padded 4 x 4 window behind every tile, sixteen f32-accumulated MFMA GEMMs
 * M_p = V_p U_p^T (256 channels x 384 tiles per workgroup, both operands streamed) replace the 9-tap implicit GEMM, and
 * Y = A^T M A (+ bias, ReLU - or the LSTM gate update) writes the activations: 16 / 36 of the direct form's multiplies at even
 * face sizes, 256 / 441 at 7x7.  U and V are rounded once to the 16-bit type, every sum is f32.  f32 convolutions stay on
 * cp360_conv_forward (exact f32 MFMA, the 1e-3 parity path).
 *   in   [n_img, w, w, pix_stride] (the first c_in channels of a pixel), n_img = 6 * cubes
 *   v    workspace of cp360_wino_v_bytes: [16][ceil(c_in / 32)][m_pad][32] (m_pad = tiles rounded up to 384)
 *   m    workspace of cp360_wino_m_bytes: f32 [16][m_pad][c_out].  Odd faces (w = 2 th - 1): a tile of a face's last tile row /
 *        column keeps only the first row / column of its 2 x 2 outputs, which A^T M A computes without transform-domain row 3 /
 *        column 3 - cp360_wino_gemm does NOT write those rows of m (31 of a 7x7 face's 256 (tile, position) pairs), no
 *        cp360_wino_output* reads them, and cp360_wino_input / _output_input write zeros to the matching rows of v.
 *   out  [n_img, w, w, ld_out] at channel out_coff (ld_out 0 = c_out) */
typedef struct {
    int dtype;        /* CP360_BF16 or CP360_F16                                   */
    int n_img;        /* faces (6 * cubes)                                         */
    int face;         /* w: faces are w x w                                        */
    int c_in;         /* % 8 == 0                                                  */
    int pix_stride;   /* elements between neighbouring input pixels (>= c_in)      */
    int c_out;        /* % 8 == 0 (% 16 for the gate epilogue)                     */
    int ld_out, out_coff, relu;
} cp360_wino_desc;
size_t cp360_wino_packed_bytes(const cp360_wino_desc* d);
size_t cp360_wino_v_bytes(const cp360_wino_desc* d);
size_t cp360_wino_m_bytes(const cp360_wino_desc* d);
/* 1: the library's planner runs this geometry in the Winograd domain (16-bit type and at most 0.8 of the direct form's MFMAs
 * after padding the tile count to 384: 4 clips of 7x7 faces, one clip of 16x16 faces, ...), 0: on the direct kernels. */
int cp360_wino_preferred(const cp360_wino_desc* d);
int cp360_wino_pack_weights(const cp360_wino_desc* d, const float* w_oihw /* f32 [c_out, c_in, 3, 3] */, void* packed, void* stream);
int cp360_wino_input(const cp360_wino_desc* d, const void* in, void* v, void* stream);
int cp360_wino_gemm(const cp360_wino_desc* d, const void* v, const void* packed, float* m, void* stream);
int cp360_wino_output(const cp360_wino_desc* d, const float* m, const float* bias, void* out, void* stream);
/* Output transform of the Gates convolution + cp360_lstm_gates_next's update in one pass (gate g of hidden channel j is
 * convolution channel g * Hc + j, Hc = c_out / 4; bias f32 [c_out]); arguments as cp360_lstm_gates_next, h_out in d->dtype. */
int cp360_wino_output_gates(const cp360_wino_desc* d, const float* m, const float* bias, const float* c_prev, float* c_next,
                            void* h_out, int ld_h, int h_coff, float* h_f32, const float* x_next, const float* minmax,
                            int x_coff, size_t clip_stride, void* stream);
/* x_next in n_groups buffers of group_clips clips each: as cp360_lstm_gates_next_groups. */
int cp360_wino_output_gates_groups(const cp360_wino_desc* d, const float* m, const float* bias, const float* c_prev, float* c_next,
                                   void* h_out, int ld_h, int h_coff, float* h_f32, const float* const* x_groups, int n_groups,
                                   int group_clips, const float* minmax, int x_coff, size_t clip_stride, void* stream);
/* cp360_wino_output of THIS convolution fused with cp360_wino_input of the NEXT one (same faces, next c_in = this c_out, dense
 * pixels): v_next = what cp360_wino_input would make of this convolution's output, bit for bit, in one launch and without the
 * activation tensor.  Faces up to 9 x 9 (a cube's 32-channel image in LDS); larger: CP360_ERR_UNSUPPORTED, run the two calls. */
int cp360_wino_output_input(const cp360_wino_desc* d, const float* m, const float* bias, void* v_next, void* stream);
/* cp360_wino_input + cp360_wino_gemm + cp360_wino_output. */
int cp360_wino_forward(const cp360_wino_desc* d, const void* in, const void* packed, const float* bias, void* out, void* v,
                       float* m, void* stream);

/* ------------------------------------------------------------------ K5o: fused Adam for ConvLSTM training
 * torch.optim.Adam with amsgrad False and maximize False, one pass over p, g, m (exp_avg), v (exp_avg_sq), all f32, in place:
 *   g' = g + weight_decay p;  m += (1 - beta1)(g' - m);  v = beta2 v + (1 - beta2) g'^2;
 *   p -= (lr / bias_corr1) m / (sqrt(v) / bias_corr2_sqrt + eps)
 * f32 arithmetic with IEEE division and square root; the hyper-parameters and the bias corrections 1 - beta1^step and
 * sqrt(1 - beta2^step) come from the host in double.  No atomics: a step is bit-reproducible.  Pointers 16-byte aligned.
 * cp360_train_adam: any tensor of n elements.
 * cp360_train_adam_conv: a filter OIHW [c_out, c_in, 3, 3] (c_in % 4 == 0); the same update, and in the same pass the new p
 * rounded to dtype (CP360_F32 / CP360_BF16) is written into every pack pointer that is not NULL, in the layouts of
 * cp360_conv_pack_weights without a scale (fwd_tap_major: clip_resident 0, fwd_chan_major: clip_resident 1) and of
 * cp360_train_dgrad_pack, for input channels [ci0, ci0 + n_dgrad).  Padding rows and columns of the packs are not touched: the
 * packs must have been made by those functions once.  With packs c_out % 4 == 0. */
int cp360_train_adam(float* p, const float* g, float* m, float* v, long long n, double lr, double beta1, double beta2,
                     double eps, double weight_decay, double bias_corr1, double bias_corr2_sqrt, void* stream);
int cp360_train_adam_conv(float* p, const float* g, float* m, float* v, int c_out, int c_in, double lr, double beta1,
                          double beta2, double eps, double weight_decay, double bias_corr1, double bias_corr2_sqrt, int dtype,
                          void* fwd_tap_major, void* fwd_chan_major, void* dgrad_packed, int ci0, int n_dgrad, void* stream);

/* ------------------------------------------------------------------ K5f: flow resize and flow loss
 * The part of a training iteration that grows with the flow's resolution (temporal_model/train_temporal.py:110-167), for
 * temporal_model/train_temporal.py.  f32 only (dtype CP360_F32); no atomics, fixed-order sums: results are bit-reproducible.
 *
 * Flow resize: cv2.resize(flow, (w_out, h_out), INTER_CUBIC) * fscale, OpenCV's generic float path (taps s-1 .. s+2 of
 * s = floor((d + 0.5) * in / out - 0.5), Keys coefficients with A = -0.75 in float, replicated borders, horizontal pass first,
 * f32 accumulation).  cp360_flow_resize_coeffs_host builds one axis: ofs int32 [out_size] (= s), coef f32 [out_size, 4].
 * cp360_flow_resize: flow f32 [F, h_in, w_in, 2] -> out f32 [F, h_out, w_out, 2]; the tables of both axes on the device
 * (16-byte aligned coef).  Equal sizes: a copy times fscale (cv2 copies), the tables may be NULL. */
int cp360_flow_resize_coeffs_host(int in_size, int out_size, int32_t* ofs, float* coef);
int cp360_flow_resize(int dtype, const float* flow, int F, int h_in, int w_in, float* out, int h_out, int w_out,
                      const int32_t* yofs, const float* ycoef, const int32_t* xofs, const float* xcoef, float fscale,
                      void* stream);
/* Flow loss of B clips x L pairs: maps f32 [B, L + 1, 2w, 4w] (the saliency maps of steps seq_len - L - 1 ..), flow f32
 * [B, L, h, w_loss, 2] (resized and scaled; pair (b, l) warps map l towards map l + 1).  Forward: loss f32 [3] = the sum-MSE
 * terms (smooth, temporal, motion mask) over all pairs.  Backward: grad_loss f32 [3] (device: d loss / d term) -> dmaps f32
 * [B, L + 1, 2w, 4w] (written; map 0 of each clip gets zero).  work: cp360_flow_loss_work_bytes (0: unsupported geometry),
 * shared by both directions.  Faces w <= 16, h and w_loss >= 2. */
size_t cp360_flow_loss_work_bytes(int B, int L, int w, int h, int w_loss);
int cp360_flow_loss_forward(int dtype, const float* maps, const float* flow, int B, int L, int w, int h, int w_loss, float mm_th,
                            float* loss, float* work, void* stream);
int cp360_flow_loss_backward(int dtype, const float* maps, const float* flow, const float* grad_loss, int B, int L, int w, int h,
                             int w_loss, float mm_th, float* dmaps, float* work, void* stream);

/* ------------------------------------------------------------------ K7: window normalise
 * temporal_model/test_temporal.py:66-67,70-73,77: per clip min / max over the whole
 * window, then (x - mn) / (mx - mn).
 *   x: B windows of T frames, frame = [P, C] f32 (P = 6*w*w pixels, NHWC); window b starts
 *   at x + b*clip_stride elements (0 = T*P*C, dense clips; P*C = the reference's stride-1
 *   sliding window over one feature sequence, zero-copy) ; minmax [B, 2] f32 (out) */
int cp360_window_minmax(const float* x, float* minmax, float* scratch /* [B*256*2] */,
                        int B, size_t per_clip, size_t clip_stride, void* stream);
/* y[b, p, y_coff + c] = (x[b, t, p, c] - mn_b) / (mx_b - mn_b); y has pixel stride ld_y
 * and dtype y_dtype; optional second destination y2 (f32, [B, P, C]) for the cell. */
int cp360_window_normalize(const float* x, const float* minmax, void* y, int y_dtype,
                           int ld_y, int y_coff, float* y2, int B, int T, int t,
                           int P, int C, size_t clip_stride, void* stream);

/* All T frames of every window in one launch: y [T, B, P, C] (dense, y_dtype) = (x[b, t] - mn_b) / (mx_b - mn_b). */
int cp360_window_normalize_frames(const float* x, const float* minmax, void* y, int y_dtype, int B, int T, int P, int C,
                                  size_t clip_stride, void* stream);

/* ------------------------------------------------------------------ K9: overlay renderer
 * utils/utils.py:9-25 as used by temporal_model/test_temporal.py:90-97.
 * cp360_overlay_colorize: heat f32 [h, w] (optionally squared first, test_temporal.py:94) -> min-max
 * normalised in float32 as numpy does -> 256-entry colormap lookup as matplotlib's Colormap.__call__(bytes=True)
 * -> rgb u8 [h, w, 3].  lut768: device u8 [256, 3] (the shim builds 'jet' on the host).  The bicubic upsample
 * is cp360_resize_lanczos_u8 with cp360_resize_coeffs_host2(filter = 1) tables.
 * cp360_overlay_blend_u8: PIL.Image.blend: out = (u8)(img + alpha * (heat - img)), float arithmetic, 0 <= alpha <= 1. */
int cp360_overlay_colorize(const float* heat, int h, int w, int square, const uint8_t* lut768, uint8_t* rgb,
                           void* stream);
int cp360_overlay_blend_u8(const uint8_t* img, const uint8_t* heat_rgb, uint8_t* out, long long n_bytes,
                           float alpha, void* stream);

/* ------------------------------------------------------------------ K10: Farneback optical flow
 * cv2.calcOpticalFlowFarneback(prev, next, None, pyr_scale, levels, winsize, iterations, poly_n, poly_sigma, 0), the
 * alternative the reference carries beneath its DeepFlow call (utils/optical_flow.py:32), batched over the F + 1 frames of a
 * video: every frame's pyramid level and polynomial expansion is computed once, pair p uses frames p and p + 1.  The
 * specification is DESIGN.md "K10"; tests/farneback_restate.py restates it in float64.  f32, no atomics, fixed-order sums:
 * bit-reproducible and independent of the batch size.  Sign: prev(y, x) ~ next(y + flow[y, x, 1], x + flow[y, x, 0]).
 *
 * Layouts: images f32 [N, h, w]; R f32 [N, 5, h, w] and M f32 [P, 5, h, w] planar; flow f32 [P, h, w, 2] = (dx, dy).
 *
 * Host routines (no GPU):
 *   levels_host        the pyramid of an H x W image: returns L (the number of coarser levels) or a negative status and fills
 *                      h, w, ksz, sigma of levels k = 0 (full size) .. L where the pointers are not NULL (cap entries each;
 *                      all four NULL: the count alone).  cvRound = round half to even.
 *   gauss_host         the ksz taps (f32, normalised in double) of a level's Gaussian; sigma 0: ksz 3, {0.25, 0.5, 0.25}.
 *   poly_tables_host   g, xg, xxg f32 [2n + 1] and ig = {ig11, ig03, ig33, ig55} of the polynomial expansion (n <= 7). */
int cp360_optflow_levels_host(int H, int W, double pyr_scale, int levels, int cap, int* hs, int* ws, int* ksz, double* sigma);
int cp360_optflow_gauss_host(int ksz, double sigma, float* taps);
int cp360_optflow_poly_tables_host(int n, double sigma, float* g, float* xg, float* xxg, float* ig);
/* The stages, one entry point each (device pointers):
 *   gray           rgb u8 [n_pixels, 3] (a frame already resized, channels as the video reader delivers them) -> gray f32
 *                  [n_pixels] = (c0 1868 + c1 9617 + c2 4899 + 8192) >> 14 on the REVERSED channels (c0 = rgb[2])
 *   pyr_level      gray f32 [N, H, W] -> out f32 [N, lh, lw]: ksz x ksz Gaussian (reflect-101, folded as often as it takes),
 *                  then the bilinear resize with the arithmetic of cp360_resize_linear_f32; tmp f32 [N, H, W] scratch; ksz <= 255
 *   poly_exp       img f32 [N, h, w] -> R [N, 5, h, w] = the local coefficients of [y, x, y^2, x^2, xy]; replicate-clamped
 *   matrices       pair p: R0 + p r_stride (prev), R1 + p r_stride (next), flow [P, h, w, 2] -> M [P, 5, h, w]
 *   blur_solve     M [P, 5, h, w] -> flow [P, h, w, 2]: winsize^2 box mean (odd, <= 33; replicate-clamped) and the 2 x 2 solve
 *   flow_upsample  flow [P, h, w, 2] -> out [P, h_out, w_out, 2] = bilinear resize times mul */
int cp360_optflow_gray(const uint8_t* rgb, float* gray, long long n_pixels, void* stream);
int cp360_optflow_pyr_level(const float* gray, int N, int H, int W, int ksz, double sigma, float* out, int lh, int lw, float* tmp,
                            void* stream);
int cp360_optflow_poly_exp(const float* img, int N, int h, int w, int poly_n, double poly_sigma, float* R, void* stream);
int cp360_optflow_matrices(const float* R0, const float* R1, size_t r_stride, const float* flow, float* M, int P, int h, int w,
                           void* stream);
int cp360_optflow_blur_solve(const float* M, float* flow, int P, int h, int w, int winsize, void* stream);
int cp360_optflow_flow_upsample(const float* flow, int P, int h, int w, float* out, int h_out, int w_out, float mul, void* stream);
/* gray f32 [F + 1, H, W] (0 .. 255) -> flow f32 [F, H, W, 2] on the stream; work: 16-byte aligned device memory of at least
 * the queried size (0: unsupported geometry), owned by the caller.  flags other than 0 (Gaussian window, initial flow):
 * CP360_ERR_UNSUPPORTED; an even winsize: CP360_ERR_BAD_SHAPE. */
size_t cp360_optflow_work_bytes(int F, int H, int W, double pyr_scale, int levels);
int cp360_optflow_farneback(const float* gray, int F, int H, int W, double pyr_scale, int levels, int winsize, int iterations,
                            int poly_n, double poly_sigma, int flags, float* flow, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K11: 360-degree stabilisation
 * The camera rotation between the frames of an equirectangular video, fitted to the flow K10 computes, and the frames re-rendered
 * without it.  The reference has no counterpart (its README leaves moving cameras to the user): the specification is the
 * package's own, DESIGN.md "K11", restated in float64 in tests/stabilize_restate.py.  Pixel (x, y) of an H x W image looks along
 * dir(x, y) = (cos phi cos theta, sin phi, cos phi sin theta), theta = (2 (x + 1/2) / W - 1) pi, phi = (1 - 2 (y + 1/2) / H) pi / 2
 * (utils/sph_utils.py); pix() is its inverse.  Rotations are f32 [.., 3, 3], row-major.
 *
 *   fit      flow f32 [F, H, W, 2] (K10's convention) -> R f32 [F, 3, 3]: a scene direction p of frame t's camera is seen at
 *            R_t p in frame t + 1; diag f64 [F, 4] = {the scale c after the last update, in pixels; sum of weights, weighted RMS
 *            residual in pixels and |delta| of the last iteration}.  Gauss-Newton on the robust Wahba problem: iteration 0 is
 *            plain least squares with the solid-angle weight cos phi, later ones weigh by cos phi / (1 + r^2 / c^2)^2 with c
 *            halved per iteration down to c_min_px pixels.  Per-pixel terms f32, sums f64 in a fixed order, no atomics: bit-
 *            reproducible and independent of F.  Non-finite flow values weigh 0; a singular system (all weights 0, fewer than 3
 *            independent directions) leaves R = I with the diagnostics' sum of weights 0.  2 + 2 iters launches, no
 *            host synchronisation.
 *   flow     R [F, 3, 3] -> G f32 [F, H, W, 2] = pix(R dir(x, y)) - (x, y), x wrapped into [-W / 2, W / 2): what fit inverts
 *   rotate   out[n](x, y) = bilinear(frames[n], pix(R[n] dir(x, y))), columns wrap modulo W, rows clamp to 0 .. H - 1;
 *            frames u8 [N, H, W, 3] (rintf, half to even) or f32 [N, H, W, C], C <= 4 (CP360_ERR_UNSUPPORTED above); not in place
 * work: 16-byte aligned device memory of cp360_stab_work_bytes(F, H, W) bytes for fit, of cp360_stab_work_bytes(0, H, W) bytes
 * for flow and rotate (the per-row and per-column sin / cos tables every call rebuilds); 0 = bad or unsupported sizes.  A
 * workspace that is too small: CP360_ERR_BAD_SHAPE.  flow and G are read and written as pairs of floats: 8-byte aligned, else
 * CP360_ERR_ALIGN, before any launch. */
size_t cp360_stab_work_bytes(int F, int H, int W);
int cp360_stab_fit(const float* flow, int F, int H, int W, int iters, double c_min_px, float* R, double* diag, void* work,
                   size_t work_bytes, void* stream);
int cp360_stab_flow(const float* R, int F, int H, int W, float* G, void* work, size_t work_bytes, void* stream);
int cp360_stab_rotate(int dtype, const void* frames, const float* R, int N, int H, int W, int C, void* out, void* work,
                      size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K12: the viewport pilot
 * What a 360-degree saliency map is used for: choosing where to look and rendering that view (the purpose of the reference's
 * utils/fov_visual.py - box_proh, fov_module, draw_cube_fov_box - which does not compile).  The specification is the package's
 * own, DESIGN.md "K12", restated in float64 in tests/viewport_restate.py; geometry, tables and the bilinear sample are K11's
 * (csrc/sphere.h).  A camera is R f32 [3, 3] row-major, camera-to-world, with the columns (forward, up, right) of the view:
 * R = I looks along dir of the panorama's centre, (1, 0, 0), with up +y and right +z.  tx = tan(hfov / 2), ty = tx h / w.
 *
 *   render   out[n](i, j) = bilinear(frames[n], pix(R[n] d)), d = (1, v, u) / sqrt(1 + v^2 + u^2), u = ((2 i + 1) / w - 1) tx,
 *            v = (1 - (2 j + 1) / h) ty: the gnomonic view of h x w pixels; columns wrap, rows clamp, no anti-aliasing.  frames
 *            u8 [N, H, W, 3] (rintf, half to even) or f32 [N, H, W, C], C <= 4 (CP360_ERR_UNSUPPORTED above) -> out [N, h, w, C]
 *            of the same type; not in place; no workspace.  0 < hfov_rad < pi, else CP360_ERR_BAD_SHAPE.
 *   outline  the view's frame drawn on the panorama, u8 [N, H, W, 3]; out may be frames.  Pixel (x, y): d = R[n]^T dir(x, y) =
 *            (d_f, d_u, d_r), u = d_r / d_f, v = d_u / d_f, b = border_px 2 tx / w (border_px > 0).  The pixel takes rgb[0..2]
 *            (three bytes of HOST memory, read during the call) where d_f > 0, |u| <= tx, |v| <= ty and not (|u| <= tx - b and
 *            |v| <= ty - b); every other pixel is copied.  A non-finite R draws nothing.
 *   smooth   maps f32 [F, hm, wm] -> out f32 [F, hm, wm]: out_i = sum_j a_j s_j e_ij / sum_j a_j e_ij, the von Mises-Fisher
 *            kernel e_ij = expf(kappa (p_i . p_j - 1)), kappa = 1 / sigma_rad^2 (double, rounded once), a_j = cos phi_j, p = dir of
 *            the map's pixel centres.  Terms f32, the two sums f64 in ascending j; non-finite s_j count as 0; a constant map
 *            comes back constant.  All pairs: hm wm <= 16384 (CP360_ERR_UNSUPPORTED above).  Not in place.
 *   peak     smooth, maps [F, hm, wm] -> idx i32 [F] = argmax of the finite values of smooth (lowest index on ties), val f32 [F]
 *            = smooth there, dir f32 [F, 3] = c / |c| with c = sum_j a_j s_j e(p*, p_j) p_j on the raw map, p* = dir(idx): one
 *            mean-shift step, the sub-pixel position (terms f32, sums f64 in a fixed order).  |c| = 0: dir = p*.  A frame with no
 *            finite value: idx = -1, dir = (1, 0, 0), val = NaN.
 * work (outline, smooth, peak): 16-byte aligned device memory of cp360_stab_work_bytes(0, H, W) bytes - of (0, hm, wm) for the
 * maps - for K11's tables, which every call rebuilds; too small: CP360_ERR_BAD_SHAPE.  Asynchronous on the stream, no atomics,
 * bit-reproducible, independent of N / F. */
int cp360_view_render(int dtype, const void* frames, const float* R, int N, int H, int W, int C, double hfov_rad, void* out, int h,
                      int w, void* stream);
int cp360_view_outline(const uint8_t* frames, const float* R, int N, int H, int W, double hfov_rad, int h, int w, double border_px,
                       const uint8_t* rgb, uint8_t* out, void* work, size_t work_bytes, void* stream);
int cp360_view_smooth(const float* maps, int F, int hm, int wm, double sigma_rad, float* out, void* work, size_t work_bytes,
                      void* stream);
int cp360_view_peak(const float* smooth, const float* maps, int F, int hm, int wm, double sigma_rad, float* dir_out, int* idx_out,
                    float* val_out, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K16: the camera path by dynamic programming
 * Which target to follow over time: the path over the map's pixels that collects the most saliency while the camera turns at
 * most step degrees a frame and pays turn_cost per degree (the dynamic programme of Pano2Vid / AutoCam and Deep 360 Pilot).  The
 * definition is the package's own and exact in integers, DESIGN.md "K16", restated in tests/campath_restate.py.  A state is a pixel
 * of the hm x wm map, P = hm wm <= 16384, p_j its centre's direction.
 *
 *   table_host  out int32 (HOST memory, cp360_path_table_bytes(hm, wm) bytes): cost [hm][hm][wm / 2 + 1] by (row of i, row of j,
 *               column difference folded to 0 .. wm / 2) = rint(turn_cost * the angle of p_i and p_j in degrees) where the angle
 *               (atan2(|p x q|, p . q), double) is at most step_rad, else -1; behind it span [hm][hm], the largest allowed column
 *               difference of the row pair, -1 for none.  Symmetric in the rows.  0 <= turn_cost <= 4096, 0 < step_rad <= pi.
 *   path        smooth f32 [F, hm, wm], gain f32 [F], table_dev = the table in DEVICE memory, starts_dev int32 [S + 1] in device
 *               memory: ascending, starts[0] = 0, starts[S] = F, sequence s = frames starts[s] .. starts[s + 1] - 1 (values are
 *               clamped into 0 .. F; an empty sequence writes nothing).  Vote q[t][j] = (int)rintf(min(max(smooth[t][j] gain[t], 0),
 *               4096)), one f32 product, 0 where it is not finite.  Per sequence [lo, hi): acc[lo] = q[lo], acc[t][j] = q[t][j] +
 *               max_i (acc[t-1][i] - cost(i, j)) over the allowed i, back[t][j] = the lowest maximising i; idx[hi-1] = the lowest
 *               argmax of acc[hi-1], idx[t-1] = back[t][idx[t]].  -> idx_out int32 [F], dir_out f32 [F, 3] = the pixel centres'
 *               directions, score_out int32 [S] = acc[hi-1][idx[hi-1]] (< 2^28).  Integers: bit-identical between runs, and a
 *               sequence's result does not depend on the others.  One workgroup per sequence, then one thread per sequence.
 *   refine      K12's mean-shift step on the raw maps about p* = dir(idx[t]) for GIVEN indices (int32 [F], device): with peak's idx
 *               it is peak's dir bit for bit; an index outside 0 .. P - 1 gives (1, 0, 0).
 * work: 16-byte aligned device memory; path: cp360_path_work_bytes(F, hm, wm) bytes (K11's tables, then the back-pointers u16
 * [F][P]); refine: as K12's.  The _bytes functions return 0 for bad or unsupported sizes.  NULL: CP360_ERR_NULL; F, hm, wm < 1,
 * S < 1, S > F or a parameter out of range: CP360_ERR_BAD_SHAPE; P > 16384 or F > 65535: CP360_ERR_UNSUPPORTED.  Asynchronous on
 * the stream, no atomics, no host synchronisation. */
size_t cp360_path_table_bytes(int hm, int wm);
int cp360_path_table_host(int hm, int wm, double turn_cost, double step_rad, int32_t* out);
size_t cp360_path_work_bytes(int F, int hm, int wm);
int cp360_view_path(const float* smooth, const float* gain, int F, int hm, int wm, const int32_t* table_dev,
                    const int32_t* starts_dev, int S, int32_t* idx_out, float* dir_out, int32_t* score_out, void* work,
                    size_t work_bytes, void* stream);
int cp360_view_refine(const float* maps, const int32_t* idx, int F, int hm, int wm, double sigma_rad, float* dir_out, void* work,
                      size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K20: several cameras at once
 * Two people talking are two targets: camera k >= 1 plans K16's path on the maps with the caps about the cameras before it taken
 * out (exclude), and the views of all cameras are rendered side by side on one canvas (render_multi).  The definition is the
 * package's own, DESIGN.md "K20", restated in tests/director_restate.py.
 *
 *   exclude       maps f32 [F, hm, wm], dirs f32 [F, Kx, 3] (device), 1 <= Kx <= 7, c = (float)cos(radius_rad), 0 < radius_rad
 *                 <= pi: out[t][j] = +0 where ((p_x d_x + p_y d_y) + p_z d_z) >= c in f32 for any direction d of frame t, p the
 *                 pixel centre's direction from K11's tables; else the input's bits, a NaN included.  A direction with a
 *                 non-finite component excludes nothing.  Element-wise: out may be maps.  work: as cp360_view_smooth's.
 *   render_multi  frames as cp360_view_render's, R f32 [N, K, 3, 3], 1 <= K <= 8 -> out [N, hc, wc, C] of the frames' type.
 *                 tiles int32 [K][4] = (x0, y0, w, h) and hfov_rad double [K] in HOST memory: canvas pixel (x0 + i, y0 + j) is
 *                 pixel (i, j) of cp360_view_render's view of h x w pixels and hfov_rad[k] under R[n][k], bit for bit.  A pixel in
 *                 no tile, or in the tile of a camera with a non-finite entry, takes fill: C values of the frames' type in HOST
 *                 memory, read during the call.  One launch; not in place.
 * In this order, before any launch: a NULL pointer: CP360_ERR_NULL; a size < 1, Kx outside 1 .. 7, K outside 1 .. 8, a radius or a
 * field of view out of range, a tile that is empty, leaves the canvas or overlaps another: CP360_ERR_BAD_SHAPE; a dtype that is
 * neither CP360_F32 nor CP360_U8: CP360_ERR_BAD_DTYPE; hm wm > 16384, F > 65535, C > 4, u8 with C != 3, an image beyond
 * cp360_view_render's limits or frames == out: CP360_ERR_UNSUPPORTED; a misaligned workspace: CP360_ERR_ALIGN; one that is too
 * small: CP360_ERR_BAD_SHAPE.  Asynchronous on the stream, no atomics, no host synchronisation, independent of F / N. */
int cp360_view_exclude(const float* maps, const float* dirs, int F, int hm, int wm, int Kx, double radius_rad, float* out, void* work,
                       size_t work_bytes, void* stream);
int cp360_view_render_multi(int dtype, const void* frames, const float* R, int N, int H, int W, int C, int K, const int32_t* tiles,
                            const double* hfov_rad, const void* fill, void* out, int hc, int wc, void* stream);

/* ------------------------------------------------------------------ K21: anti-aliased views by supersampling
 * A view coarser than its source aliases: rho = tan(hfov / 2) max(W, 2 H) / (pi w) source pixels per view pixel at the view's
 * centre passes 1 for 2048 x 4096 frames in 1280 columns.  The definition is the package's own, DESIGN.md "K21", restated in
 * float64 in tests/viewport_aa_restate.py.  For a factor ss = 1 .. 4:
 *
 *   render_aa        out[n](i, j) = the mean of the ss x ss samples (ss i + a, ss j + b), a, b = 0 .. ss - 1, of cp360_view_render's
 *                    view of ss h x ss w pixels and the same hfov_rad under R[n], each sample in f32 and NOT rounded for u8
 *                    frames: added in f32 with b outer and a inner, starting from the first sample, divided by (float)(ss ss), then
 *                    stored as render stores (u8: rintf, clamp).  So out is an ordered f32 sum of cp360_view_render's own output
 *                    for f32 frames of the fine view, bit for bit, and ss = 1 is cp360_view_render itself.  A box filter over the
 *                    pixel in the view plane; no pyramid, no workspace, one launch.  Arguments otherwise as cp360_view_render's.
 *   render_multi_aa  cp360_view_render_multi with a factor per tile, ss int32 [K] in HOST memory: tile k is render_aa's view with
 *                    ss[k], bit for bit; a list of ones is cp360_view_render_multi itself.
 * The status codes are their counterparts', in the same order; in addition ss == NULL: CP360_ERR_NULL; a factor outside 1 .. 4:
 * CP360_ERR_BAD_SHAPE (last of its group); a fine view ss h x ss w beyond cp360_view_render's limits: CP360_ERR_UNSUPPORTED
 * (before frames == out).  Asynchronous on the stream, no atomics, no host synchronisation, independent of N. */
int cp360_view_render_aa(int dtype, const void* frames, const float* R, int N, int H, int W, int C, double hfov_rad, int ss,
                         void* out, int h, int w, void* stream);
int cp360_view_render_multi_aa(int dtype, const void* frames, const float* R, int N, int H, int W, int C, int K, const int32_t* tiles,
                               const double* hfov_rad, const int32_t* ss, const void* fill, void* out, int hc, int wc, void* stream);

/* ------------------------------------------------------------------ K22: zoom, a field of view per frame
 * One lens per frame instead of one per call, and a measure of how wide the target is, from which the host chooses the lens.  The
 * definition is the package's own, DESIGN.md "K22", restated in float64 in tests/zoom_restate.py.  Every launch has an earlier call
 * as its bit-exact oracle.
 *
 *   lens          lens f32 [N, 4] = (tx, ty, b, 0) per frame, 16-byte aligned, on the device for the three launches below.
 *                 lens_host fills it in HOST memory without a GPU call, with the arithmetic of cp360_view_render and
 *                 cp360_view_outline: t = tan(hfov / 2) in double, tx = (float)t, ty = (float)(t h / w), b = (float)(border_px 2 t /
 *                 w), 0.f for border_px == 0.
 *   render_zoom   frame n of out = cp360_view_render's (ss == NULL) or cp360_view_render_aa's (ss int32 [N] on the DEVICE, 4-byte
 *                 aligned; a value outside 2 .. 4 renders as the factor 1) frame under the lens (tx, ty) of frame n, bit for bit.
 *                 No value of a lens decides an address: a tangent that is not finite or not positive ends in the sampler's guard.
 *   outline_zoom  frame n of out = cp360_view_outline's frame with (tx, ty, b) of frame n, bit for bit; a frame whose b is not
 *                 greater than 0 draws nothing.  out may be frames.
 *   spread        maps f32 [F, hm, wm], dirs f32 [F, 3] (cp360_view_peak's or cp360_view_refine's) -> q f32 [F]: with d = dirs[f], the
 *                 cap in_j = ((p_x d_x + p_y d_y) + p_z d_z) >= (float)cos(window_rad), top = the largest finite s_j in the cap, m_j
 *                 = a_j fmaxf(s_j - (float)level top, 0) for the finite s_j in the cap (else 0), g_j = ((p_x - d_x)^2 + (p_y - d_y)^2
 *                 + (p_z - d_z)^2) / 2: q[f] = (float)(sum m_j g_j / sum m_j), the two sums in f64 in K12d's order - the mean of 1 -
 *                 cos(angle) over the part of the target above level times its peak.  NaN for a non-finite d, a cap without a finite
 *                 pixel, top <= 0 or a sum of m that is not positive and finite.  One workgroup per frame; workspace: the tables.
 * cp360_head_agreement_zoom (below, K17) is cp360_head_agreement with the camera's tangents from cam_lens[f].
 * Status codes, in this order and before any launch.  lens_host: NULL: CP360_ERR_NULL; N, h, w < 1, border_px negative or not
 * finite, a field of view outside (0, pi): CP360_ERR_BAD_SHAPE.  render_zoom: cp360_view_render's (lens NULL: CP360_ERR_NULL; ss
 * given and a view 4 h x 4 w beyond the limits: CP360_ERR_UNSUPPORTED), then lens not 16-byte or ss not 4-byte aligned:
 * CP360_ERR_ALIGN.  outline_zoom: NULL; N, H, W < 1: CP360_ERR_BAD_SHAPE; an image beyond the limits: CP360_ERR_UNSUPPORTED; lens or
 * workspace misaligned: CP360_ERR_ALIGN; workspace too small: CP360_ERR_BAD_SHAPE.  spread: NULL; F, hm, wm < 1, window_rad outside
 * (0, pi], level outside (0, 1): CP360_ERR_BAD_SHAPE; hm wm > 16384 or F > 65535: CP360_ERR_UNSUPPORTED; the workspace as above.
 * Asynchronous on the stream, no atomics, no host synchronisation, independent of N / F. */
int cp360_view_lens_host(const double* hfov_rad, int N, int h, int w, double border_px, float* lens);
int cp360_view_render_zoom(int dtype, const void* frames, const float* R, const float* lens, const int32_t* ss, int N, int H, int W,
                           int C, void* out, int h, int w, void* stream);
int cp360_view_outline_zoom(const uint8_t* frames, const float* R, const float* lens, int N, int H, int W, const uint8_t* rgb,
                            uint8_t* out, void* work, size_t work_bytes, void* stream);
int cp360_view_spread(const float* maps, const float* dirs, int F, int hm, int wm, double window_rad, double level, float* q,
                      void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K13: shot detection
 * Where the hard cuts of an equirectangular video are: K10 - K12 assume one continuous take.  The signature of a frame is the
 * colour histogram of the whole sphere, every pixel weighted by the solid angle of its row: a camera rotation leaves it nearly
 * unchanged, a cut does not.  The reference has no counterpart: the specification is the package's own, DESIGN.md "K13", restated
 * in integers in tests/shots_restate.py.
 *
 *   weights_host  a int32 [H] (HOST memory): a_y = floor(cos(phi_y) 1024 + 1/2), phi_y = (1 - (2 y + 1) / H) pi / 2, the latitude of
 *                 row y's pixel centres, in double from the exact fraction (rows y and H - 1 - y get the same weight);
 *                 *total_per_width (optional) = sum_y a_y, so that T = W * total_per_width
 *   signatures    frames u8 [F, H, W, 3], contiguous, at ANY byte address; weights = the table above in DEVICE memory ->
 *                 sig int64 [F, 3, 64], sig[f, c, b] = sum of a_y over the pixels with frames[f, y, x, c] >> 2 == b.  Every
 *                 sig[f, c, :] sums to T.  Integers only: bit-identical between runs, launch geometries and batch sizes.  Every byte
 *                 is read once; two launches, no global atomics, no trigonometry, no host synchronisation.
 * work: 16-byte aligned device memory of cp360_shot_work_bytes(F, H, W) bytes (the workgroups' u32 partial sums); 0 = bad or
 * unsupported sizes; too small: CP360_ERR_BAD_SHAPE.  F, H or W < 1: CP360_ERR_BAD_SHAPE; F or H > 65535, H W > 2^28,
 * W > 2^21 or T >= 2^62: CP360_ERR_UNSUPPORTED. */
int cp360_shot_weights_host(int H, int32_t* a, long long* total_per_width);
size_t cp360_shot_work_bytes(int F, int H, int W);
int cp360_shot_signatures(const uint8_t* frames, int F, int H, int W, const int32_t* weights, long long* sig, void* work,
                          size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K14: saliency metrics on the sphere, a video per call
 * AUC-Judd, NSS, CC, SIM and KL of F saliency maps against F ground-truth maps on an h x w equirectangular grid, every pixel
 * weighted by the solid angle of its row.  K8 below keeps the reference's flat, one-frame functions; the specification of these
 * is the package's own, DESIGN.md "K14", restated in float64 and exact integers in tests/sphere_eval_restate.py.
 *
 *   resample  src f32 [F, hs, ws] -> dst f32 [F, h, w]: grid pixel (x, y) samples the source at sx = (float)((double)((2 x + 1)
 *             ws) / (double)(2 w) - 0.5), sy alike, bilinear with K11's sample (columns wrap, rows clamp, no contraction, no
 *             anti-aliasing); a source that is already h x w is copied bit for bit.  hs, ws as for K11's images.
 *   scores    S, G f32 [F, h, w]; fixations u8 [F, h, w] (non-zero = fixated) or NULL: the rule G_i > mu_G + 2 sigma_G with the
 *             weighted mean and deviation, compared in double; weights int32 [h] (DEVICE memory; cp360_shot_weights_host's table
 *             for the solid angle, 1024 everywhere for a flat grid; values are clamped to 0 .. 1024) -> scores f64 [F, 5] = (auc,
 *             nss, cc, sim, kl) and n_fix int32 [F].  With a_i the weight of pixel i's row and sums in double: CC the weighted
 *             Pearson coefficient from centred sums; P_i = a_i (S_i - min S) / sum_j a_j (S_j - min S), Q_i alike from G, SIM =
 *             sum_i min(P_i, Q_i), KL = sum_i Q_i log(eps + Q_i / (P_i + eps)), eps = 2^-52; NSS = the mean over the fixated pixels
 *             of (S_i - mu_S) / sigma_S; AUC = the trapezoid sum over (0, 0), (A_i / A_neg, c_i / n_fix) by descending S_i, (1, 1),
 *             c_i = #{fixated j: S_j >= S_i}, A_i = the weight of the pixels that are not fixated with S_j >= S_i, A_neg that of all
 *             of them: an integer over 2 A_neg n_fix, rounded once, no jitter.  n_fix = 0 or h w: AUC and NSS are NaN; no variance:
 *             CC and NSS are NaN; no mass above the minimum: SIM and KL are NaN; a non-finite value in a frame's S or G: all five
 *             of that frame are NaN.  Three launches, no host synchronisation, no global atomics; a frame's numbers are
 *             bit-identical between runs, batch sizes and places in the batch.
 * work: 16-byte aligned device memory of cp360_seval_work_bytes(F, h, w) bytes (20 bytes per pixel); 0 = bad or unsupported sizes;
 * too small: CP360_ERR_BAD_SHAPE.  F, h or w < 1: CP360_ERR_BAD_SHAPE; F > 65535 or h w > 2^21: CP360_ERR_UNSUPPORTED. */
size_t cp360_seval_work_bytes(int F, int h, int w);
int cp360_seval_resample(const float* src, int F, int hs, int ws, float* dst, int h, int w, void* stream);
int cp360_seval_scores(const float* S, const float* G, const uint8_t* fixations, const int32_t* weights, int F, int h, int w,
                       double* scores, int32_t* n_fix, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K15: fixations from scan-paths, shuffled AUC on the sphere
 * A video's fixations are N points in CSR form: lonlat f64 [N, 2] in radians (longitude = theta, latitude = phi of K11's
 * geometry, north up; may be NULL when N = 0), offsets int32 [F + 1] ascending from 0 to N (DEVICE memory: an offset outside
 * 0 .. N is clamped into it); the points of frame f are offsets[f] .. offsets[f + 1] - 1.  A point with a non-finite coordinate
 * contributes nothing anywhere.  The specification is the package's own, DESIGN.md "K15", restated in tests/fixations_restate.py.
 *
 *   counts   counts int32 [F, h, w] = the number of frame f's points in each pixel, n_points int32 [F] = the number of its finite
 *            points.  The pixel, in float64 with one operation per step: u = (lon / pi + 1) (w / 2), x = floor(u) mod w in 0 ..
 *            w - 1 (longitudes wrap; a u that overflows: column 0); v = (1 - lat / (pi / 2)) (h / 2), y = clamp(floor(v), 0, h - 1)
 *            (latitudes beyond the poles clamp).  No trigonometry: numpy gives the same integers.
 *   density  out f32 [F, h, w]: G[f, i] = sum_k expf(kappa (p_i . q_k - 1)) over the frame's finite points in ascending k, kappa =
 *            (float)(1 / sigma_rad^2) (cp360_view_smooth's kernel), p_i from K11's tables, q_k = dir(lon_k, lat_k) computed in double
 *            and rounded to f32, the sum in f32 in that order: un-normalised, bit-identical whatever the batch and the frame's
 *            place in it; a frame without points is zero.  sigma_rad finite and > 0, else CP360_ERR_BAD_SHAPE.
 *   sauc     shuffled AUC: S f32 [F, h, w], pos int32 [F, h, w] (clamped to 0 .. 1023), neg int32 [Fn, h, w], Fn = 1 (one map for
 *            every frame) or F (clamped to 0 .. 2^20; every pixel counts, fixated ones included) -> auc f64 [F], c_tot int64 [F] =
 *            sum pos, a_neg int64 [F] = sum neg.  For a pixel with pos_i > 0: C_i = sum of pos_j over pos_j > 0, S_j >= S_i, A_i =
 *            sum of neg_j over S_j >= S_i; AUC = the trapezoid sum over (0, 0), the distinct (A_i / A_neg, C_i / C_tot) by
 *            descending S_i, (1, 1) = an integer over 2 A_neg C_tot, rounded once; no jitter, no random draw.  C_tot = 0, A_neg =
 *            0, a non-finite value in the frame's S, or 2 A_neg C_tot >= 2^53: NaN for that frame.
 * work: 16-byte aligned device memory of cp360_fix_work_bytes(F, h, w) bytes for sauc, of cp360_fix_work_bytes(0, h, w) bytes for
 * density (K11's tables, which every call rebuilds); counts needs none; 0 = bad or unsupported sizes; too small:
 * CP360_ERR_BAD_SHAPE.  F, h or w < 1, N < 0, Fn not 1 or F: CP360_ERR_BAD_SHAPE; F > 65535, h w > 2^21 or N >= 2^31:
 * CP360_ERR_UNSUPPORTED.  Asynchronous on the stream; the only atomics add integers. */
size_t cp360_fix_work_bytes(int F, int h, int w);
int cp360_fix_counts(const double* lonlat, const int32_t* offsets, long long N, int F, int h, int w, int32_t* counts,
                     int32_t* n_points, void* stream);
int cp360_fix_density(const double* lonlat, const int32_t* offsets, long long N, int F, int h, int w, double sigma_rad, float* out,
                      void* work, size_t work_bytes, void* stream);
int cp360_fix_sauc(const float* S, const int32_t* pos, const int32_t* neg, int Fn, int F, int h, int w, double* auc,
                   long long* c_tot, long long* a_neg, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K19: the human ceiling and the prior baselines, per point
 * One score pair per fixation point of K15's CSR points (lonlat, offsets as above; the points of one frame are taken as different
 * viewers'): scores f64 [N, 2] = (auc, nss) of point k against a map l_k f64 [h w], weights int32 [h] as for cp360_seval_scores
 * (DEVICE memory, clamped to 0 .. 1024), A = the sum of the weights a_j over all pixels, i_k = the pixel of point k by the binning
 * of counts.  The specification is the package's own, DESIGN.md "K19", restated in tests/ceiling_restate.py.
 *
 *   leave-one-out  S = NULL (Fs is ignored): e_k(j) = density's f32 term expf(kappa (p_j . q_k - 1)) with its kappa =
 *                  (float)(1 / sigma_rad^2), its rounding of q_k and its order in the dot product; T_f[j] = sum_k (double)e_k(j)
 *                  over the frame's finite points in ascending k; l_k[j] = max(T_f[j] - (double)e_k(j), 0) - the sum over the other
 *                  viewers, at N h w terms a video and not N n h w.  sigma_rad finite and > 0, else CP360_ERR_BAD_SHAPE.
 *   map            S f32 [Fs, h, w], Fs = 1 (one map for every frame) or F: l_k[j] = (double)S[f or 0][j] for every point of
 *                  frame f; sigma_rad is ignored.
 *   scores         mu = sum_a l_k / A, sigma = sqrt(sum_a (l_k - mu)^2 / A), nss = (l_k[i_k] - mu) / sigma.  A_k = the sum of a_j
 *                  over j != i_k with l_k[j] >= l_k[i_k] (int64), A_neg = A - a_{i_k}, auc = (double)(2 A_neg - A_k) / (2.0
 *                  (double)A_neg), rounded once: cp360_seval_scores' AUC-Judd with the one fixated pixel i_k, bit for bit in map
 *                  mode.  A point with a non-finite coordinate, or one outside every frame's (clamped) range: NaN, NaN.  A frame
 *                  with one finite point in leave-one-out mode has l = 0 everywhere: auc = 1/2 exactly, nss = NaN.  A_neg = 0: auc
 *                  = NaN.  A non-finite value in a frame's S: NaN, NaN for that frame's points alone.  A constant S: auc = 1/2.
 * A point's two numbers are bit-identical between runs and whatever F, N and the point's place in the batch: a wave per point,
 * sums in one fixed order, no atomics.
 * work: 16-byte aligned device memory of cp360_fix_point_work_bytes(F, h, w) bytes (K11's tables, which every call rebuilds, and
 * 8 F h w bytes for T; 0 = bad or unsupported sizes); too small: CP360_ERR_BAD_SHAPE.  In this order, before any launch: a NULL
 * pointer (S may be NULL; lonlat and scores when N = 0): CP360_ERR_NULL; F, h or w < 1, N < 0, Fs not 1 or F (map), sigma_rad
 * (leave-one-out): CP360_ERR_BAD_SHAPE; F > 65535, h w > 2^21 or N >= 2^31: CP360_ERR_UNSUPPORTED; alignment (lonlat, scores 8
 * bytes, the others 4, work 16): CP360_ERR_ALIGN; the workspace.  N = 0 is valid.  Asynchronous on the stream. */
size_t cp360_fix_point_work_bytes(int F, int h, int w);
int cp360_fix_point_scores(const float* S, int Fs, const double* lonlat, const int32_t* offsets, long long N, int F, int h, int w,
                           double sigma_rad, const int32_t* weights, double* scores, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K17: ground truth from head tracking
 * A headset logs the head's orientation: what a viewer saw is the headset's window, the view of a camera in K12's convention
 * (R f32 [3, 3] camera-to-world, columns forward / up / right).  A video's viewers are N cameras in CSR form: R f32 [N, 3, 3] (may
 * be NULL when N = 0), offsets int32 [F + 1] ascending from 0 to N as for K15 (DEVICE memory; whatever it holds, every access
 * stays inside R).  A view is (hfov_rad, aspect = h_v / w_v): tx = tan(hfov_rad / 2), ty = tx aspect in double, each rounded to
 * f32 once.  The direction p = dir(x, y) of a grid pixel is inside the view of R <=> d_f > 0, |d_r / d_f| <= tx and |d_u / d_f| <= ty
 * with (d_f, d_u, d_r) = R^T p in f32, term by term as cp360_view_outline decides it (the pixels its frame encloses); a camera with
 * a non-finite entry has an empty view.  The specification is the package's own, DESIGN.md "K17", restated in
 * tests/headtrack_restate.py.
 *
 *   footprints  counts int32 [F, h, w] = the number of frame f's cameras whose view holds the pixel, n_views int32 [F] = the number
 *               of its finite cameras: counts / n_views is the share of the viewers who had the pixel in view.
 *   agreement   Rc f32 [F, 3, 3], the camera that is judged, one per frame, with its own view (cam_hfov_rad, cam_aspect); weights
 *               int32 [h] as for cp360_seval_scores (DEVICE memory, clamped to 0 .. 1024) -> inter, uni int64 [N]: for viewer k of
 *               frame f, inter[k] = sum of a_y over the pixels inside both views, uni[k] = over the pixels inside either;
 *               inter / uni is the intersection over union of the two windows on the sphere.  A non-finite viewer: inter = 0, uni
 *               = the area of Rc[f]'s view; a non-finite Rc[f] is an empty view.
 * Both decide with the one function, so inter, uni and counts agree pixel for pixel.  Exact integers, no atomics: a frame's
 * counts and a pair's sums are bit-identical between runs and whatever F, N and their place in the batch.
 * work: 16-byte aligned device memory of cp360_fix_work_bytes(0, h, w) bytes (K11's tables, which every call rebuilds); too small:
 * CP360_ERR_BAD_SHAPE.  F, h or w < 1, N < 0, hfov_rad outside (0, pi), aspect <= 0 or a tangent that is not finite in f32:
 * CP360_ERR_BAD_SHAPE; F > 65535, h w > 2^21 or N >= 2^31: CP360_ERR_UNSUPPORTED.  N = 0 is valid.  Asynchronous on the stream. */
int cp360_head_footprints(const float* R, const int32_t* offsets, long long N, int F, int h, int w, double hfov_rad, double aspect,
                          int32_t* counts, int32_t* n_views, void* work, size_t work_bytes, void* stream);
int cp360_head_agreement(const float* Rc, double cam_hfov_rad, double cam_aspect, const float* R, const int32_t* offsets,
                         long long N, int F, int h, int w, double hfov_rad, double aspect, const int32_t* weights, long long* inter,
                         long long* uni, void* work, size_t work_bytes, void* stream);
/* K22c: agreement with a lens per frame for the camera that is judged: cam_lens f32 [F, 4] = K22's (tx, ty, b, 0) per frame (DEVICE
 * memory, 16-byte aligned; cp360_view_lens_host's table), of which (tx, ty) of frame f take the place of the tangents of
 * (cam_hfov_rad, cam_aspect); everything else, the viewers' window and the status codes are agreement's (cam_lens NULL:
 * CP360_ERR_NULL, misaligned: CP360_ERR_ALIGN).  The lens rounds ty as (float)(t h / w), agreement as (float)(t aspect): the same
 * value where h / w is exact in double and the product rounds alike, as for a power of two. */
int cp360_head_agreement_zoom(const float* Rc, const float* cam_lens, const float* R, const int32_t* offsets, long long N, int F,
                              int h, int w, double hfov_rad, double aspect, const int32_t* weights, long long* inter,
                              long long* uni, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K18: the supervised loss - K14's KL, CC and NSS with a gradient
 * N maps f32 [N, mh, mw] (a training window's maps, flattened over clips and steps) against ground truth G f32 [N, h, w] on the
 * loss grid; fix u8 [N, h, w] (non-zero = fixated) or NULL = K14's derived mask; weights int32 [h] as for cp360_seval_scores
 * (DEVICE memory, clamped to 0 .. 1024); kl_eps finite and > 0 (K14's is 2^-52).  The specification is the package's own,
 * DESIGN.md "K18", restated in tests/suploss_restate.py.
 *
 *   forward   S = cp360_seval_resample(maps) on the h x w grid (mh > h is valid: no anti-aliasing), then K14's sums in K14's
 *             order -> terms f64 [N, 3] = (kl, cc, nss), valid u8 [N, 3], stats f64 [N, CP360_SUP_LOSS_STATS] = (mu_S, mu_G, Vs,
 *             Vg, min S, min G, Z, Z_G, K1, K2, mm, n_fix, A, the mask's threshold, cc, nss).  A term K14 defines as NaN (a
 *             non-finite value in the map's S or G, no variance, no mass above the minimum, n_fix = 0 or h w) is K14's NaN with
 *             valid = 0; valid is also 0 where the term or a scalar of its gradient is not finite.  A map's numbers do not depend
 *             on N or on its place in the batch.
 *   backward  stats and valid from forward, gterms f64 [N, 3] -> dmaps f32 [N, mh, mw] = sum_t gterms[n, t] valid[n, t]
 *             dterm_t/dmaps[n]: the gradient with respect to S (the header of csrc/suploss.hip) through the adjoint of the
 *             resampler, tap weights formed in double from the sampler's f32 fractions, f64 sums in a fixed order rounded to f32
 *             once.  An invalid term, or one whose gterms entry is 0, contributes exactly +0.  Bit-reproducible; a map alone gives
 *             the bits it gives inside a batch.  dmaps must not share memory with the inputs.
 * work: 16-byte aligned device memory of cp360_sup_loss_work_bytes(N, mh, mw, h, w) bytes (12 bytes per grid pixel: S in f32 and dS
 * in f64; both entry points rebuild what they read); 0 = bad or unsupported sizes.  Status, decided before any HIP call: NULL:
 * CP360_ERR_NULL; N, mh, mw, h or w < 1, or kl_eps not finite or <= 0: CP360_ERR_BAD_SHAPE; N > 65535, h w > 2^21, mh mw > 2^21 or
 * mh > 65535: CP360_ERR_UNSUPPORTED; a misaligned pointer: CP360_ERR_ALIGN; a workspace that is too small: CP360_ERR_BAD_SHAPE.
 * Asynchronous on the stream, no host synchronisation, no atomics. */
#define CP360_SUP_LOSS_STATS 16
size_t cp360_sup_loss_work_bytes(int N, int mh, int mw, int h, int w);
int cp360_sup_loss_forward(const float* maps, const float* G, const uint8_t* fix, const int32_t* weights, int N, int mh, int mw,
                           int h, int w, double kl_eps, double* terms, uint8_t* valid, double* stats, void* work, size_t work_bytes,
                           void* stream);
int cp360_sup_loss_backward(const float* maps, const float* G, const uint8_t* fix, const int32_t* weights, const double* stats,
                            const uint8_t* valid, const double* gterms, int N, int mh, int mw, int h, int w, double kl_eps,
                            float* dmaps, void* work, size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K8: saliency metrics
 * utils/eval_saliency.py on the device: AUC_Judd (:90-146), AUC_Borji (:14-87), CorrCoeff (:149-176),
 * similarity (:179-190).  Every reference metric first resizes both maps with
 * cv2.resize(x, (240, 120), cv2.INTER_LANCZOS4) - the flag lands in the `dst` slot, so OpenCV's default
 * INTER_LINEAR runs: cp360_resize_linear_f32.  The AUCs share cp360_metric_auc_prepare (normalised
 * saliency + the values at fixated pixels, F > mean(F) + 2 std(F)) and a workspace of
 * cp360_metric_work_bytes(n) bytes; all pointers are device memory.
 */
/* cv2.resize(src [h, w] f32, (dw, dh)) with INTER_LINEAR (half-pixel centres, edge clamp) -> dst [dh, dw]. */
int cp360_resize_linear_f32(const float* src, int h, int w, float* dst, int dh, int dw, void* stream);
size_t cp360_metric_work_bytes(int n);
/* sal, fix: resized maps, n pixels each.  mode 0 (AUC_Judd): S = sal + jitter (f64 [n] or NULL, the
 * reference's randn / 1e7), min-max normalised in f64.  mode 1 (AUC_Borji): S[S > mean + 2 std] = 1, then
 * min-max normalised in f32.  work[0] (as double) = number of fixated pixels afterwards. */
int cp360_metric_auc_prepare(const float* sal, const float* fix, const double* jitter, int n, int mode,
                             void* work, void* stream);
/* out2[0] = AUC-Judd, out2[1] = number of fixated pixels (doubles). */
int cp360_metric_auc_judd(int n, void* work, double* out2, void* stream);
/* rr int32 [n_fix, n_splits]: the reference's np.random.randint(0, n, (n_fix, n_splits)); aucs f64 [n_splits]
 * (their mean is the score); step = the threshold spacing (0.01). */
int cp360_metric_auc_borji(int n, int n_splits, const int* rr, double step, void* work, double* aucs,
                           void* stream);
/* out2[0] = CorrCoeff(a, b), out2[1] = similarity(a, b) of two resized maps (doubles). */
int cp360_metric_cc_sim(const float* a, const float* b, int n, double* out2, void* stream);

/* ------------------------------------------------------------------ stage contexts: ONE entry point per network stage
 * (csrc/ctx.hip).  A cp360_ctx owns the packed / BatchNorm-folded weights of the two networks and the kernel choice for
 * every layer (fused tail kernels, tile shapes, split-K: everything the per-kernel entry points above leave to the
 * caller), so a binder needs three calls per stage - load, workspace_bytes, forward - instead of re-implementing the
 * launch planning.  The Python shims of this package call these (pipeline.py, static_model/class_activation_model.py:
 * cam_device, temporal_model/test_temporal.py: ClipRunner); the per-kernel entry points stay for tests and tuning.
 *  - a context is bound to one device; one context per GPU; not thread-safe within a context;
 *  - weights are DEVICE f32 tensors in the reference's state-dict layout, read during *_load only (packed copies are
 *    owned by the context, hipMalloc / hipFree inside load / destroy - the only allocations this library makes);
 *  - activations, workspace and outputs are caller-allocated; `workspace` must be 256-byte aligned and at least
 *    *_workspace_bytes(...) for the same shape; forward calls are asynchronous on `stream` and never allocate.
 */
/* Eval-mode BatchNorm2d as y = x * scale + bias (model/resnet_cubic.py:66-70 with eps 1e-5): scale = g / sqrt(var + eps),
 * bias = b - mean * scale, each operation rounded once in f32 (IEEE divide / sqrt, no FMA contraction), all pointers
 * device f32 [n].  The folding cp360_resnet_load applies; public so that a caller planning its own launches folds
 * identically. */
int cp360_fold_bn(const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                  float* scale, float* bias, int n, void* stream);

typedef struct cp360_ctx cp360_ctx;
int cp360_create(int device, cp360_ctx** out);
void cp360_destroy(cp360_ctx* ctx);

/* One convolution + its BatchNorm (model/resnet_cubic.py:65-83,115-128): OIHW weight and the four BatchNorm vectors. */
typedef struct {
    const float* weight;
    const float* bn_weight;
    const float* bn_bias;
    const float* bn_mean;
    const float* bn_var;
} cp360_conv_bn;

/* ResNet-50-cubic + CAM.  convs[53] in torchvision's key order: conv1/bn1, then for layerL.B: conv1/bn1, conv2/bn2,
 * conv3/bn3 and, for block 0 of a layer, downsample.0/downsample.1.  fc_weight [num_classes, 2048]; fc_shift = min(fc_weight)
 * when that is negative, else 0 (class_activation_model.py:51-52: the global scalar shift, computed by the caller).
 * dtype: CP360_F32 (exact-f32 MFMA path), CP360_BF16 or CP360_F16. */
int cp360_resnet_load(cp360_ctx* ctx, int dtype, const cp360_conv_bn* convs, int n_convs, const float* fc_weight,
                      int num_classes, float fc_shift, float bn_eps, void* stream);
size_t cp360_resnet_workspace_bytes(cp360_ctx* ctx, int n_img, int cube_dim);
/* faces_p3 [n_img, cube_dim+6, cube_dim+6, 4]: normalised cube faces WITH their CubePad(3) ring, NHWC4, in the loaded
 * dtype (what cp360_equi2cube writes with the CubePad(3)-gathered grid) -> cam_out f32 [n_img, cd/32, cd/32, num_classes]
 * (the per-face CAM scores of class_activation_model.py:70-83, NHWC) and, if feat_out != NULL, the layer4 features
 * [n_img, cd/32, cd/32, 2048] in the loaded dtype.  resnet_cubic.py:163-175 + class_activation_model.py:46-83. */
int cp360_resnet_forward(cp360_ctx* ctx, const void* faces_p3, int n_img, int cube_dim, float* cam_out, void* feat_out,
                         void* workspace, size_t workspace_bytes, void* stream);

/* ConvLSTM cell (model/clstm.py:19-82).  w1 [4H, Cin+H, 3, 3], w2 / wg [4H, 4H, 3, 3], biases [4H]; `face` = the cube
 * face size the cell will run at (7 at cube 224, 16 at cube 512): it selects the weight layout of the kernel for that size. */
int cp360_clstm_load(cp360_ctx* ctx, int dtype, const float* w1, const float* b1, const float* w2, const float* b2,
                     const float* wg, const float* bg, int input_size, int hidden_size, int face, void* stream);
/* The 16-bit cell in the Winograd domain ("K5w" above): when a launch shape has enough tiles (cp360_wino_preferred on Conv2's
 * shape - e.g. 4 cubes of 7x7 faces, one cube of 16x16 faces) cp360_clstm_step / cp360_clstm_window run the three convolutions
 * as F(2x2, 3x3).  Its filters (16 / 9 of the direct packing's bytes) are packed on request:
 *   cp360_clstm_wino_state  0: (n_clips, face) runs on the direct kernels; 1: in the Winograd domain; 2: it would, but
 *                           cp360_clstm_load_wino has not been called - the direct kernels run until it has
 *   cp360_clstm_load_wino   the same f32 filters as cp360_clstm_load (call it after that; workspace sizes change with it). */
int cp360_clstm_wino_state(cp360_ctx* ctx, int n_clips, int face);
int cp360_clstm_load_wino(cp360_ctx* ctx, const float* w1, const float* w2, const float* wg, void* stream);
size_t cp360_clstm_workspace_bytes(cp360_ctx* ctx, int n_clips, int face);
/* One cell update for n_clips cubes in lock step on the fused layout: xh [6 n_clips, face, face, Cin + H] (loaded dtype):
 * channels [0, Cin) = the input frame, [Cin, Cin + H) = the previous hidden state - the NEW hidden state is written
 * back there; c_prev / c_next f32 [6 n_clips, face, face, H]; h_f32 (optional) an f32 copy of the new hidden state.
 * x_next != NULL (needs Cin == H): frame t+1 of clip 0 (f32, pixel-major [6 face^2, H]; clip b at + b * clip_stride
 * elements) is window-normalised with minmax [n_clips, 2] (temporal_model/test_temporal.py:77) into the x half of xh in
 * the same pass.  model/clstm.py:42-82. */
int cp360_clstm_step(cp360_ctx* ctx, void* xh, const float* c_prev, float* c_next, float* h_f32, int n_clips, int face,
                     const float* x_next, const float* minmax, size_t clip_stride, void* workspace,
                     size_t workspace_bytes, void* stream);

/* One WINDOW of the temporal stage in one call (temporal_model/test_temporal.py:63-80 for n_clips windows in lock step):
 * min / max over each window, hidden = cell = normalised frame 0, T cell updates (frame 0 fed again first).
 *   cam       f32: window b = T frames of [6 face^2, Cin] (pixel-major) starting at cam + b * clip_stride elements
 *             (clip_stride 0 = dense T * P * Cin; P * Cin = the reference's stride-1 sliding window over one sequence)
 *   xh        [6 n_clips, face, face, Cin + H] scratch in the loaded dtype (the fused [x | h] buffer of cp360_clstm_step)
 *   cell0/1   f32 [6 n_clips, face, face, H] scratch (ping-pong cell state)
 *   h_out     f32 [6 n_clips, face, face, H]: the final hidden state (:80);  h_all (optional) f32 [T, 6 n_clips, face, face, H]:
 *             the hidden state after EVERY step (return_all_steps)
 *   minmax    f32 [n_clips, 2] (out), mm_scratch f32 [n_clips * 512]
 * Needs Cin == H (:70-73).  The window issues exactly the launches of T cp360_clstm_step calls (same bits).
 * workspace: cp360_clstm_window_workspace_bytes. */
size_t cp360_clstm_window_workspace_bytes(cp360_ctx* ctx, int n_clips, int T, int face);
int cp360_clstm_window(cp360_ctx* ctx, const float* cam, size_t clip_stride, int n_clips, int T, int face, void* xh,
                       float* cell0, float* cell1, float* h_out, float* h_all, float* minmax, float* mm_scratch,
                       void* workspace, size_t workspace_bytes, void* stream);
/* The windows of n_groups independent batches of n_clips clips each in ONE run of the T cell updates, at n_groups * n_clips
 * clips: the batches' CAM buffers stay where they are (cams: a HOST array of n_groups device pointers, each as
 * cp360_clstm_window's cam with the same clip_stride), the fused [x | h] buffer and the cell state for all clips are built in
 * the workspace.  With the Winograd plan at both clip counts every row of every GEMM is computed as in n_groups
 * cp360_clstm_window calls (rows are independent, no split-K): the same bits, and each launch streams the filters once for all
 * groups.  (On the direct kernels the split counts depend on the clip count: right, not bit-equal.)
 *   h_out     HOST array of n_groups device pointers, each f32 [6 n_clips, face, face, H]
 *   h_all     NULL, or a HOST array of n_groups device pointers, each f32 [T, 6 n_clips, face, face, H]
 *   minmax    f32 [n_groups * n_clips, 2] (out): group g's rows start at row g * n_clips
 * 1 <= n_groups <= CP360_MAX_CLIP_GROUPS.  workspace: cp360_clstm_window_multi_workspace_bytes (256-byte aligned). */
size_t cp360_clstm_window_multi_workspace_bytes(cp360_ctx* ctx, int n_groups, int n_clips, int T, int face);
int cp360_clstm_window_multi(cp360_ctx* ctx, const float* const* cams, size_t clip_stride, int n_groups, int n_clips, int T,
                             int face, float* const* h_out, float* const* h_all, float* minmax, void* workspace,
                             size_t workspace_bytes, void* stream);

/* The launch plan cp360_resnet_forward would follow for n_img faces of cube_dim^2, one line per layer: which fused kernel or
 * generic path runs (the fused Bottleneck kernels are specialised to 16-bit types and the face sizes of cube 224 / 512; any
 * other geometry - and f32 - takes the per-convolution path, whose tile / split-K choice per launch is listed).  Returns the
 * length written (truncated to cap - 1) or a negative status.  Costs no GPU work. */
int cp360_resnet_plan_describe(cp360_ctx* ctx, int n_img, int cube_dim, char* buf, size_t cap);

/* The static stages of n_groups in-flight batches of n_img faces each, the 14x14 and 7x7 layers as ONE pass (16-bit types,
 * cube 224).  FRONT: stem .. layer3.0 runs per group at n_img faces, as in cp360_resnet_forward; each group's layer3.0
 * output is written into its rows of a hand-over buffer in the workspace.  BACK: layer3.1 .. layer4 and the CAM run once at
 * n_groups * n_img faces - the 7x7 launches of layer4, 0.6 - 0.9 of a round of the chip per batch of 384 faces, fill it at
 * 768, and the layer3 tails lose their half-empty last round.  Every back launch keeps the kernel family, the split-K count, the K ranges, the finish order and the
 * epilogue of the plan at n_img faces (GEMM rows are independent, CubePad stays inside a cube): each group's CAM is
 * cp360_resnet_forward's bit for bit.
 *   faces_p3  HOST array of n_groups device pointers, each as cp360_resnet_forward's faces_p3
 *   cam_out   HOST array of n_groups device pointers with cam_out[g] == cam_out[0] + g * n_img * (cd/32)^2 * num_classes:
 *             the CAM launch writes all groups at once (anything else: CP360_ERR_BAD_SHAPE, before any launch)
 * n_groups == 1 is cp360_resnet_forward (any type, any cube size).  n_groups >= 2 where cp360_resnet_can_pair_static
 * answers 0 (f32, other cube sizes): CP360_ERR_UNSUPPORTED - call cp360_resnet_forward per batch there.
 * workspace: cp360_resnet_forward_multi_workspace_bytes (256-byte aligned).  cp360_resnet_plan_describe_multi: the plan as
 * text, naming the front, the cut and the back. */
int cp360_resnet_can_pair_static(cp360_ctx* ctx, int n_groups, int n_img, int cube_dim);
size_t cp360_resnet_forward_multi_workspace_bytes(cp360_ctx* ctx, int n_groups, int n_img, int cube_dim);
int cp360_resnet_forward_multi(cp360_ctx* ctx, const void* const* faces_p3, int n_groups, int n_img, int cube_dim,
                               float* const* cam_out, void* workspace, size_t workspace_bytes, void* stream);
int cp360_resnet_plan_describe_multi(cp360_ctx* ctx, int n_groups, int n_img, int cube_dim, char* buf, size_t cap);

/* ------------------------------------------------------------------ K23: ego-motion from flow, the independent-motion flow
 * A travelling 360-degree camera: the rotation R and the unit direction of translation e of every frame pair fitted to the flow
 * K10 computes, and the part of the flow that this camera motion and a static scene cannot explain at any depth.  The
 * specification is the package's own, DESIGN.md "K23" (7o), restated in float64 in tests/egomotion_restate.py; geometry and
 * conventions are K11's (R: a scene direction p of frame t's camera is seen at R p in frame t + 1; flow f32 [F, H, W, 2]).
 * Per pixel p = dir(x, y), g = R^T dir(x + dx, y + dy); a static point at depth d has g = normalize(p - (|T| / d) e).
 *   fit       R0 f32 [F, 3, 3] (the start, K11's fit) -> R f32 [F, 3, 3], e f32 [F, 3], diag f64 [F, 8] = (share of the sphere
 *             that moves by more than t_min_px at R0, sum of weights, weighted RMS of the epipolar residual in px, lambda_0 /
 *             lambda_2 and lambda_1 / lambda_2 of the last scatter matrix, |delta| of the last rotation step, the scale c in
 *             px, flag: 0 fitted, 1 gated, 2 singular).  share < min_share (no translation), no finite pixel or a scatter
 *             matrix of rank <= 1: e = (0, 0, 0) and R = R0 bit for bit.  Non-finite flow values weigh 0.  iters >= 1,
 *             c_min_px > 0, t_min_px >= 0, min_share >= 0 (else CP360_ERR_BAD_SHAPE).
 *   residual  res f32 [F, H, W, 2] = pix(g) - pix(g*), x wrapped into [-W / 2, W / 2), g* the point of the legal arc from p to -e
 *             nearest to g (e = 0: g* = p, the de-rotated flow; p an epipole: g* = g); mag f32 [F, H, W] = angle(g, g*) W / 2 pi,
 *             or NULL when not wanted.  e is a unit vector or exactly 0.  A non-finite flow value: NaN in that pixel.
 * work: 16-byte aligned device memory of cp360_ego_work_bytes(F, H, W) bytes for fit (never less than cp360_stab_work_bytes(F, H,
 * W)), of (0, H, W) for residual (K11's tables); 0 = bad or unsupported sizes; too small: CP360_ERR_BAD_SHAPE.  flow and res are
 * read and written as pairs of floats: 8-byte aligned, else CP360_ERR_ALIGN, before any launch.  Asynchronous on the stream, no
 * atomics, bit-reproducible, a pair's result independent of F and of its place in the batch. */
size_t cp360_ego_work_bytes(int F, int H, int W);
int cp360_ego_fit(const float* flow, const float* R0, int F, int H, int W, int iters, double c_min_px, double t_min_px,
                  double min_share, float* R, float* e, double* diag, void* work, size_t work_bytes, void* stream);
int cp360_ego_residual(const float* flow, const float* R, const float* e, int F, int H, int W, float* res, float* mag, void* work,
                       size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K24: viewport-adaptive streaming
 * From a saliency map to "how likely is this pixel, or this tile, to be in somebody's window", and the quality that a tile plan
 * delivers to the viewers who watched.  The specification is the package's own, DESIGN.md "K24" (7p), restated in
 * tests/streaming_restate.py.  Source pixel j of an hs x ws map (S = hs ws <= 4096) stands for a viewer whose camera is cams[j]
 * (f32 [S, 9], K12's convention, built on the host: utils/streaming.py); the window is K17's (hfov_rad, aspect), its tangents
 * rounded as K17's; the grid has h x w pixels (P = h w <= 2^21) in rows x cols tiles (T = rows cols <= 4096, rows <= h, cols <= w),
 * pixel (x, y) in tile ((y rows) / h) cols + (x cols) / w.  All DEVICE memory.
 *
 *   view_incidence  inc u32 [S, ceil(P / 32)]: bit i % 32 of word i / 32 of row j = whether dir(i) is inside the view of cams[j],
 *                   cp360_head_footprints' decision bit for bit (a non-finite camera: an empty row); the bits past P are 0.
 *                   work: cp360_fix_work_bytes(0, h, w) bytes, K11's tables.
 *   tile_incidence  tinc u32 [S, ceil(T / 32)]: bit t of row j = the OR of inc[j, i] over the pixels of tile t.
 *   view_expect     sal f32 [F, S], weights int32 [hs] as for cp360_seval_scores (clamped to 0 .. 1024), bits u32 [S, ceil(P / 32)]
 *                   (inc, or tinc with P = T) -> out f32 [F, P], total f32 [F].  m[f, j] = sal[f, j] (float)a_y(j / ws) where
 *                   sal[f, j] > 0 and finite, else 0; acc = 0, then for j = 0 .. S - 1 ascending, acc = acc + m[f, j] where bit
 *                   (j, i) is set, in f32; total[f] the same sum over every j; out[f, i] = total > 0 ? acc / total : 0.  The order
 *                   is the definition: a frame's numbers are bit-identical between runs, whatever F and its place in the batch.
 *   view_quality    R, offsets, N: K17's viewers in CSR form; levels u8 [F, T], 1 <= L <= 8 (a value >= L counts as L - 1) ->
 *                   qarea int64 [N, L]: for viewer k of frame f, qarea[k, l] = the sum of a_y over the pixels inside its view
 *                   whose tile has level l in frame f.  Exact integers; sum_l qarea[k, l] is cp360_head_agreement's uni of the
 *                   viewer against itself.  A non-finite viewer: zeros.  work: cp360_view_quality_work_bytes(h, w) bytes (K11's
 *                   tables and the tile of every column and row; 0 = bad or unsupported sizes).
 * Status codes, in this order and before any launch: a NULL pointer (sal, out, total when F = 0 and R, levels, qarea when N = 0 may
 * be NULL): CP360_ERR_NULL; a size < 1 (F = 0 is valid for view_expect, F = 0 with N = 0 for view_quality), N < 0, rows > h,
 * cols > w, L outside 1 .. 8 or a window that cp360_head_footprints refuses: CP360_ERR_BAD_SHAPE; S > 4096, T > 4096, P > 2^21,
 * F > 65535 or N >= 2^31: CP360_ERR_UNSUPPORTED; a pointer not 4-byte (qarea 8-byte, work 16-byte) aligned: CP360_ERR_ALIGN; a
 * workspace that is too small: CP360_ERR_BAD_SHAPE.  N = 0 and F = 0 launch nothing.  Asynchronous on the stream, no atomics, no
 * host synchronisation. */
int cp360_view_incidence(const float* cams, int S, int h, int w, double hfov_rad, double aspect, uint32_t* inc, void* work,
                         size_t work_bytes, void* stream);
int cp360_tile_incidence(const uint32_t* inc, int S, int h, int w, int rows, int cols, uint32_t* tinc, void* stream);
int cp360_view_expect(const float* sal, int F, int hs, int ws, const int32_t* weights, const uint32_t* bits, int P, float* out,
                      float* total, void* stream);
size_t cp360_view_quality_work_bytes(int h, int w);
int cp360_view_quality(const float* R, const int32_t* offsets, long long N, int F, int h, int w, double hfov_rad, double aspect,
                       const int32_t* weights, const uint8_t* levels, int rows, int cols, int L, long long* qarea, void* work,
                       size_t work_bytes, void* stream);

/* ------------------------------------------------------------------ K25: the conservative remap on the sphere, with its adjoint
 * The resampler for maps finer than the grid: a grid pixel is the solid-angle-weighted mean of the source pixels it overlaps, so
 * a constant stays a constant, the integral over the sphere is kept and every source pixel is read.  cp360_seval_resample (four
 * bilinear taps, no pre-filter) stays the default of every consumer.  The specification is the package's own, DESIGN.md "K25"
 * (7q), restated in tests/resample_restate.py.  Source hs x ws, grid h x w, same seam and poles; per axis:
 *   n_src > n_dst   conservative: the run of grid index d is floor(d n_src / n_dst) .. ceil((d + 1) n_src / n_dst) - 1; column
 *                   weight (float)((double)ov / ws) with the integer overlap ov, row weight the overlap in z = cos(pi t) over the
 *                   band's own z range, formed in float64 and rounded once
 *   otherwise       sphere_sample's two taps: the run (i0, i1) with the weights (1 - t, t), t in f32 as cp360_seval_resample forms
 *                   it; columns wrap, rows clamp
 *   forward   dst f32 [F, h, w]: col[j] = sum over the run of y, ascending, of wy src[r, j]; out = sum over the run of x, in run
 *             order, of wx col[j]; f32, every product and sum rounded on its own, the order fixed by the two shapes alone.  Where
 *             neither axis is finer the call is cp360_seval_resample's, bit for bit.  Non-finite values are not hidden.
 *   adjoint   d_src f32 [F, hs, ws] = the transpose applied to d_dst f32 [F, h, w], gathered per source pixel, both sums in f64
 *             and rounded once.
 *   run_cap   R of one axis: ceil(n_src / n_dst) + 1 where conservative, else 2; 0 for a size < 1.  R > 256 on either axis:
 *             CP360_ERR_UNSUPPORTED.
 *   axis_host HOST only, no GPU: axis 0 = rows, 1 = columns -> start int32 [n_dst], count int32 [n_dst], weights f32 [n_dst, R]
 *             zero-padded (tapped: start = i0, count = 2, the second index is start + 1, wrapped or clamped).
 *   plan      plan_host fills plan_bytes bytes of HOST memory (16-byte aligned) with both axes' tables; the caller uploads them
 *             once per (hs, ws, h, w) and hands the DEVICE copy to forward and adjoint, which clamp whatever they read from it.
 * Limits are cp360_seval_resample's (F <= 65535, h w <= 2^21, hs <= 65535, hs ws <= 2^28); F = 0 is valid and launches nothing.
 * Status codes, in this order and before any launch: a NULL pointer (src, dst may be NULL when F = 0): CP360_ERR_NULL; a size < 1 or
 * F < 0: CP360_ERR_BAD_SHAPE; a limit or the run cap: CP360_ERR_UNSUPPORTED; a pointer not 4-byte (plan 16-byte) aligned:
 * CP360_ERR_ALIGN; a plan below plan_bytes: CP360_ERR_BAD_SHAPE.  Asynchronous on the stream, no atomics, no host synchronisation;
 * a frame's numbers depend neither on F nor on its place in the batch. */
int cp360_sresample_run_cap(int n_src, int n_dst);
int cp360_sresample_axis_host(int n_src, int n_dst, int axis, int32_t* start, int32_t* count, float* weights);
size_t cp360_sresample_plan_bytes(int hs, int ws, int h, int w);
int cp360_sresample_plan_host(int hs, int ws, int h, int w, void* plan, size_t plan_bytes);
int cp360_sresample_forward(const float* src, int F, int hs, int ws, float* dst, int h, int w, const void* plan, size_t plan_bytes,
                            void* stream);
int cp360_sresample_adjoint(const float* d_dst, int F, int h, int w, float* d_src, int hs, int ws, const void* plan,
                            size_t plan_bytes, void* stream);

/* ------------------------------------------------------------------ K26: video quality on the sphere, per cell
 * The weighted squared error behind WS-PSNR and a windowed structural similarity on integer luma behind WS-SSIM, of a decoded
 * video against its source.  The specification is the package's own, DESIGN.md "K26" (7r), restated in tests/quality_restate.py.
 * ref, dist u8 [F, H, W, 3], contiguous, each from any byte address; rows x cols cells (1 <= rows <= H, 1 <= cols <= W), pixel
 * (y, x) in cell ((y rows) / H) cols + (x cols) / W (K24's tile rule), T = rows cols; weights int32 [H] as for
 * cp360_shot_signatures (clamped to 0 .. 1024).  All DEVICE memory.
 *   sse     int64 [F, T, 3]: sse[f, t, c] = the sum over the pixels of cell t of a_y (ref - dist)^2.  Exact.
 *   ssim_q  int64 [F, T] or NULL (not computed; needs H % 4 == 0, W % 4 == 0, H >= 8, W >= 8).  Y = (4899 R + 9617 G + 1868 B +
 *           8192) >> 14; a 4 x 4 block has s1 = sum Yr, s2 = sum Yd, ss = sum (Yr^2 + Yd^2), s12 = sum Yr Yd; window (i, j), i = 0
 *           .. H / 4 - 2, j = 0 .. W / 4 - 1, is the blocks (i, j), (i, j + 1), (i + 1, j), (i + 1, j + 1), column j + 1 modulo
 *           W / 4.  With the window's sums in int64: vars = 64 ss - s1^2 - s2^2, covar = 64 s12 - s1 s2, A = (2 s1 s2 + 416)
 *           (2 covar + 235963), B = (s1^2 + s2^2 + 416)(vars + 235963), q = (int64)rint((double)A / (double)B 2^24).
 *           ssim_q[f, t] = the sum over the windows whose pixel (4 i + 4, (4 j + 4) % W) lies in cell t of ww_i q, ww_i = a_4i + ..
 *           + a_4i+7.  Exact up to the one correctly rounded f64 quotient per window.
 *   work    cp360_sphere_quality_work_bytes(F, H, W, rows, cols) bytes (the cell of every column and row, the weights; 0 = bad
 *           or unsupported sizes).
 * No result depends on the order of accumulation, the launch geometry, F or the frames' addresses.
 * Status codes, in this order and before any launch: a NULL pointer (ssim_q may be NULL): CP360_ERR_NULL; a size < 1, rows > H,
 * cols > W, or ssim_q with H % 4, W % 4 != 0 or H, W < 8: CP360_ERR_BAD_SHAPE; H W 65025 1024 >= 2^62, F or H > 65535, H W > 2^28,
 * W > 2^21, or ssim_q with H W >= 2^29: CP360_ERR_UNSUPPORTED; sse, ssim_q not 8-byte, weights not 4-byte, work not 16-byte
 * aligned: CP360_ERR_ALIGN; a workspace that is too small: CP360_ERR_BAD_SHAPE.  Asynchronous on the stream, no host
 * synchronisation; the results are zeroed on the stream and added to with 64-bit integer atomics. */
size_t cp360_sphere_quality_work_bytes(int F, int H, int W, int rows, int cols);
int cp360_sphere_quality(const uint8_t* ref, const uint8_t* dist, int F, int H, int W, int rows, int cols, const int32_t* weights,
                         long long* sse, long long* ssim_q, void* work, size_t work_bytes, void* stream);

/* Diagnostic only (bench.py `held_clock_ghz`): a bare bf16 MFMA loop on pseudo-random operands, n_workgroups x 4 waves, each
 * wave stamped once around `iters` x 16 MFMAs.  stamps: device u64 [n_workgroups * 4][2] = {d s_memtime (shader cycles),
 * d s_memrealtime (100 MHz ticks)} per wave; held clock of a wave = 0.1 GHz * [0] / [1].  A buffer of its own: no output of
 * the library depends on it. */
int cp360_clock_probe(unsigned long long* stamps, int n_workgroups, int iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CP360_H */
