// One C entry point per network stage (include/cp360.h, "stage contexts"): cp360_ctx owns the packed / BN-folded
// weights of a stage and the kernel choice for every layer - which fused kernel runs where, tile shapes, split-K -
// that the Python shims used to plan (ops.Conv.__call__, model/resnet_cubic.py: layer1_nhwc .. layer4).  A binder of
// another language gets the whole static stage / one ConvLSTM step from ONE call:
//
//   cp360_resnet_forward  = ResNet.forward to layer4 (model/resnet_cubic.py:163-175: CubePad(3) input -> conv7x7 s2 +
//                           bn + relu -> CubePad(1) + maxpool -> 16 Bottlenecks :85-106) + the CAM GEMM of
//                           static_model/class_activation_model.py:46-52,70-83
//   cp360_clstm_step      = ConvLSTMCell.forward (model/clstm.py:42-82) on the fused [x | h] layout
//
// Host-side C++ only: every launch goes through the per-kernel entry points of this library, in exactly the order and
// with exactly the descriptors the Python planning produces, so both paths give the same bits (tests/test_ctx.py).
#include "common.h"
#include <algorithm>
#include <new>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

namespace {

// ---------------------------------------------------------------- small device helpers
__global__ void fold_bn_kernel(const float* __restrict__ g, const float* __restrict__ b, const float* __restrict__ mu,
                               const float* __restrict__ var, float eps, float* __restrict__ scale,
                               float* __restrict__ bias, int n) {
    // eval-mode BatchNorm as y = x * scale + bias, every operation rounded once like torch's g / sqrt(var + eps),
    // b - mu * scale: IEEE divide / sqrt (hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt; the __f*_rn
    // intrinsics map to the approximate native forms here) and no contraction into an FMA - the same bits as the
    // host-side folding of model/resnet_cubic.py
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = var[i] + eps;
    const float s = g[i] / sqrtf(v);
    scale[i] = s;
    const float t = mu[i] * s;
    bias[i] = b[i] - t;
}
__global__ void add_vec_kernel(float* __restrict__ a, const float* __restrict__ b, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) a[i] = a[i] + b[i];
}
__global__ void sub_scalar_kernel(const float* __restrict__ x, float s, float* __restrict__ y, long long n) {
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < n; i += (long long)gridDim.x * 256) y[i] = x[i] - s;
}
void launch_fold_bn(const float* g, const float* b, const float* mu, const float* var, float eps, float* scale, float* bias, int n,
                    hipStream_t st) {
    hipLaunchKernelGGL(fold_bn_kernel, dim3((n + 255) / 256), dim3(256), 0, st, g, b, mu, var, eps, scale, bias, n);
}

int es_of(int dtype) { return dtype == CP360_F32 ? 4 : 2; }
size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// The context's allocations and launches belong to ITS device, whatever device the calling thread has current
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) { ok = false; return; }
        if (prev != dev && hipSetDevice(dev) != hipSuccess) ok = false;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

struct Owned {                                   // device allocations a context owns
    std::vector<void*> ptrs;
    void* take(size_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) return nullptr;
        ptrs.push_back(p);
        return p;
    }
    void release() {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

// One convolution with resident packed weights (the C++ counterpart of ops.Conv)
struct CConv {
    int c_out = 0, c_in_w = 0, kh_w = 0, kw_w = 0, stride = 1, pad = 0, relu = 0;
    bool stem = false, clip_ok = false;
    int c_in = 0, kh = 0, kw = 0, pix_stride = 0;
    int c_in2 = 0, stride2 = 0;                  // second source (the downsample branch inside conv3)
    void* packed = nullptr;                      // tap-major layout
    void* packed_clip = nullptr;                 // channel-major layout of the clip-resident kernel
    float* bias = nullptr;
};

// The descriptor of `c` on n_img inputs of h_in x w_in with dense output, no residual and one split; a second source (the
// downsample branch) with the geometry its stride implies.  Plan::conv adjusts what a call site states otherwise.
void fill_desc(const CConv& c, int dtype, int n_img, int h_in, int w_in, int clip_resident, cp360_conv_desc* d) {
    *d = cp360_conv_desc{};
    d->dtype = dtype;
    d->n_img = n_img; d->h_in = h_in; d->w_in = w_in;
    d->c_in = c.c_in; d->pix_stride = c.pix_stride;
    d->kh = c.kh; d->kw = c.kw; d->sy = c.stride; d->sx = c.stride;
    const int p2 = 2 * c.pad;
    d->h_out = (h_in + p2 - c.kh) / c.stride + 1;
    d->w_out = c.stem ? (w_in + p2 - c.kw_w) / c.stride + 1 : (w_in + p2 - c.kw) / c.stride + 1;
    d->c_out = c.c_out;
    d->pad_mode = c.pad > 0 ? 1 : 0; d->pad = c.pad;
    d->ld_out = c.c_out;
    d->relu = c.relu; d->splits = 1;
    d->clip_resident = clip_resident;
    if (c.c_in2 > 0) {
        d->c_in2 = c.c_in2; d->sy2 = d->sx2 = c.stride2;
        d->h_in2 = (d->h_out - 1) * c.stride2 + 1; d->w_in2 = (d->w_out - 1) * c.stride2 + 1; d->pix_stride2 = c.c_in2;
    }
}

// pack `c` (weights w_oihw f32 on the device, times scale) in the layout(s) its call sites need
int pack_conv(Owned& own, CConv& c, int dtype, const float* w, const float* scale, const float* w2, const float* scale2,
              bool want_plain, bool want_clip, hipStream_t st) {
    cp360_conv_desc d;
    if (want_plain) {
        fill_desc(c, dtype, 6, c.kh > 8 ? c.kh : 8, c.stem ? 16 : (c.kw > 8 ? c.kw : 8), 0, &d);
        const size_t nb = cp360_conv_packed_bytes(&d);
        if (!nb) return CP360_ERR_UNSUPPORTED;
        if (!(c.packed = own.take(nb))) return CP360_ERR_HIP;
        const int rc = c.c_in2 > 0 ? cp360_conv_pack_weights2(&d, w, scale, w2, scale2, c.packed, st)
                                   : cp360_conv_pack_weights(&d, w, scale, c.packed, c.stem ? 1 : 0, st);
        if (rc) return rc;
    }
    if (want_clip) {
        fill_desc(c, dtype, 6, 7, 7, 1, &d);
        const size_t nb = cp360_conv_packed_bytes(&d);
        if (!nb) return CP360_ERR_UNSUPPORTED;
        if (!(c.packed_clip = own.take(nb))) return CP360_ERR_HIP;
        const int rc = cp360_conv_pack_weights(&d, w, scale, c.packed_clip, 0, st);
        if (rc) return rc;
    }
    return CP360_OK;
}

bool clip_geometry(const CConv& c, int n_img, int h, int w) {
    return c.clip_ok && h == w && (6 * h * w <= 304 || h == 8 || h == 16) && n_img % 6 == 0;
}

// clip-resident kernel or tap-major path?  With one packing there is no choice; with both (layer4's conv2) the library's cost
// model decides (cp360_conv_prefer_clip: one frame in f32 runs better on the 64 x 64 tiles of conv_small.hip)
bool use_clip(const CConv& c, int dtype, int n_img, int h, int w) {
    if (!clip_geometry(c, n_img, h, w) || !c.packed_clip) return false;
    if (!c.packed) return true;
    cp360_conv_desc d;
    fill_desc(c, dtype, n_img, h, w, 1, &d);
    return cp360_conv_prefer_clip(&d) != 0;
}

// ---------------------------------------------------------------- ResNet-50-cubic + CAM
struct CBlock {
    CConv c1, c2, c3;
    bool has_ds = false;
    int planes = 0, stride = 1;
    // fused-tail packings (16-bit types): layer1 K3d, layer2 / layer3 K3e
    void *w2 = nullptr, *w3f = nullptr, *wdf = nullptr, *w1f = nullptr;   // w1f: the chained NEXT conv1's fragments
    float *b2 = nullptr, *b3 = nullptr, *b1n = nullptr;
    void* w0f = nullptr;                          // layer1.0: its OWN conv1's fragments (run inside the tail kernel at 56x56 faces)
    float* b0 = nullptr;
    int next_c = 0;
};

struct CResnet {
    bool loaded = false;
    int dtype = 0, num_classes = 0;
    CConv stem, cam;
    void* stem_packed = nullptr;                 // resident-patch stem kernel (16-bit)
    std::vector<CBlock> layer[4];
};

struct CClstm {
    bool loaded = false;
    int dtype = 0, cin = 0, ch = 0;
    CConv c1, c2, g;
    float* gbias = nullptr;
    // Winograd-domain filters U = G g G^T of the three convolutions (cp360_clstm_load_wino; csrc/wino.hip), 16-bit types
    void *u1 = nullptr, *u2 = nullptr, *ug = nullptr;
    bool wino_loaded = false;
};

// the Winograd descriptors of a cell update on n6 faces of face x face
void wino_descs(const CClstm& Cl, int n6, int face, cp360_wino_desc* d1, cp360_wino_desc* d2, cp360_wino_desc* dg) {
    const int c4 = 4 * Cl.ch, cx = Cl.cin + Cl.ch;
    *d1 = cp360_wino_desc{Cl.dtype, n6, face, cx, cx, c4, c4, 0, 1};
    *d2 = cp360_wino_desc{Cl.dtype, n6, face, c4, c4, c4, c4, 0, 1};
    *dg = cp360_wino_desc{Cl.dtype, n6, face, c4, c4, c4, c4, 0, 0};
}
// the library's rule, on Conv2's shape (the same test as ConvLSTMCell.uses_winograd of the CP360_CTX=0 path)
bool wino_wanted(const CClstm& Cl, int n_clips, int face) {
    if (Cl.dtype == CP360_F32) return false;
    cp360_wino_desc d1, d2, dg;
    wino_descs(Cl, 6 * n_clips, face, &d1, &d2, &dg);
    // every one of the three convolutions has to be a shape the Winograd kernels take (Conv1's K = input + hidden channels is
    // not Conv2's): a cell whose Conv1 fails the check stays on the direct kernels instead of failing in cp360_clstm_step
    if (!cp360_wino_v_bytes(&d1) || !cp360_wino_v_bytes(&d2) || !cp360_wino_v_bytes(&dg)) return false;
    return cp360_wino_preferred(&d2) == 1;
}

}  // namespace

struct cp360_ctx {
    int device = 0;
    Owned own_resnet, own_clstm;
    CResnet rn;
    CClstm cl;
};

extern "C" int cp360_fold_bn(const float* bn_weight, const float* bn_bias, const float* bn_mean, const float* bn_var, float eps,
                             float* scale, float* bias, int n, void* stream) {
    if (!bn_weight || !bn_bias || !bn_mean || !bn_var || !scale || !bias) return CP360_ERR_NULL;
    if (n <= 0) return CP360_ERR_BAD_SHAPE;
    launch_fold_bn(bn_weight, bn_bias, bn_mean, bn_var, eps, scale, bias, n, (hipStream_t)stream);
    CP360_CHECK_HIP();
    return CP360_OK;
}

extern "C" int cp360_create(int device, cp360_ctx** out) {
    if (!out) return CP360_ERR_NULL;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count) return CP360_ERR_HIP;
    cp360_ctx* c = new (std::nothrow) cp360_ctx();
    if (!c) return CP360_ERR_HIP;
    c->device = device;
    *out = c;
    return CP360_OK;
}

extern "C" void cp360_destroy(cp360_ctx* ctx) {
    if (!ctx) return;
    DeviceGuard guard(ctx->device);
    ctx->own_resnet.release();
    ctx->own_clstm.release();
    delete ctx;
}

namespace {

struct Folded { float* scale; float* bias; };

int fold(Owned& own, const cp360_conv_bn& p, int n, float eps, hipStream_t st, Folded* f) {
    if (!p.weight || !p.bn_weight || !p.bn_bias || !p.bn_mean || !p.bn_var) return CP360_ERR_NULL;
    f->scale = (float*)own.take((size_t)n * 4);
    f->bias = (float*)own.take((size_t)n * 4);
    if (!f->scale || !f->bias) return CP360_ERR_HIP;
    launch_fold_bn(p.bn_weight, p.bn_bias, p.bn_mean, p.bn_var, eps, f->scale, f->bias, n, st);
    return CP360_OK;
}

void set_geom(CConv& c, int c_out, int c_in, int k, int stride, int pad, int relu) {
    c.c_out = c_out; c.c_in_w = c_in; c.kh_w = c.kw_w = k; c.stride = stride; c.pad = pad; c.relu = relu;
    c.c_in = c_in; c.kh = c.kw = k; c.pix_stride = c_in;
    c.clip_ok = pad == 1 && stride == 1 && k == 3 && c_out >= 256;
}

}  // namespace

// convs: torchvision order - [0] conv1 / bn1 (stem), then per layer L = 1..4 and block B: conv1, conv2, conv3 and, for
// block 0, the downsample pair behind conv3: 1 + 16 * 3 + 4 = 53 entries.
extern "C" int cp360_resnet_load(cp360_ctx* ctx, int dtype, const cp360_conv_bn* convs, int n_convs,
                                 const float* fc_weight, int num_classes, float fc_shift, float bn_eps, void* stream) {
    if (!ctx || !convs || !fc_weight) return CP360_ERR_NULL;
    if (dtype != CP360_F32 && dtype != CP360_BF16 && dtype != CP360_F16) return CP360_ERR_BAD_DTYPE;
    if (n_convs != 53 || num_classes <= 0 || num_classes % 4 != 0) return CP360_ERR_BAD_SHAPE;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return CP360_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    ctx->own_resnet.release();
    ctx->rn = CResnet();
    CResnet& R = ctx->rn;
    Owned& own = ctx->own_resnet;
    R.dtype = dtype;
    R.num_classes = num_classes;
    const bool h16 = dtype != CP360_F32;
    int rc;
    // ---- stem: conv 7x7 s2 (3 -> 64) in its "7 taps of 8 pixels x 4 channels" form + the resident-patch kernel's packing
    {
        Folded f;
        if ((rc = fold(own, convs[0], 64, bn_eps, st, &f))) return rc;
        CConv& c = R.stem;
        c.c_out = 64; c.c_in_w = 3; c.kh_w = c.kw_w = 7; c.stride = 2; c.pad = 0; c.relu = 1; c.stem = true;
        c.c_in = 32; c.kh = 7; c.kw = 1; c.pix_stride = 4;
        c.bias = f.bias;
        if ((rc = pack_conv(own, c, dtype, convs[0].weight, f.scale, nullptr, nullptr, true, false, st))) return rc;
        if (h16) {
            if (!(R.stem_packed = own.take(cp360_stem_packed_bytes(dtype)))) return CP360_ERR_HIP;
            if ((rc = cp360_stem_pack_weights(dtype, convs[0].weight, f.scale, R.stem_packed, st))) return rc;
        }
    }
    // ---- Bottlenecks
    static const int nblk[4] = {3, 4, 6, 3};
    int idx = 1, inplanes = 64;
    for (int L = 0; L < 4; ++L) {
        const int planes = 64 << L, lstride = L == 0 ? 1 : 2;
        R.layer[L].resize(nblk[L]);
        for (int b = 0; b < nblk[L]; ++b) {
            CBlock& B = R.layer[L][b];
            B.planes = planes;
            B.stride = b == 0 ? lstride : 1;
            B.has_ds = b == 0;
            const cp360_conv_bn &p1 = convs[idx], &p2 = convs[idx + 1], &p3 = convs[idx + 2];
            Folded f1, f2, f3, fd{nullptr, nullptr};
            if ((rc = fold(own, p1, planes, bn_eps, st, &f1))) return rc;
            if ((rc = fold(own, p2, planes, bn_eps, st, &f2))) return rc;
            if ((rc = fold(own, p3, planes * 4, bn_eps, st, &f3))) return rc;
            const cp360_conv_bn* pd = B.has_ds ? &convs[idx + 3] : nullptr;
            if (pd && (rc = fold(own, *pd, planes * 4, bn_eps, st, &fd))) return rc;
            idx += B.has_ds ? 4 : 3;
            set_geom(B.c1, planes, inplanes, 1, 1, 0, 1);
            set_geom(B.c2, planes, planes, 3, B.stride, 1, 1);
            set_geom(B.c3, planes * 4, planes, 1, 1, 0, 1);
            B.c1.bias = f1.bias;
            B.c2.bias = f2.bias;
            B.c3.bias = f3.bias;
            if ((rc = pack_conv(own, B.c1, dtype, p1.weight, f1.scale, nullptr, nullptr, true, false, st))) return rc;
            // conv2: layer4's (7x7 faces at cube 224 / 16x16 at cube 512) may run clip-resident: both layouts
            if ((rc = pack_conv(own, B.c2, dtype, p2.weight, f2.scale, nullptr, nullptr, true, B.c2.clip_ok, st))) return rc;
            if (B.has_ds) {                       // downsample branch as conv3's second source: bias = b3 + bd
                B.c3.c_in2 = inplanes;
                B.c3.stride2 = B.stride;
                B.c3.clip_ok = false;
                hipLaunchKernelGGL(add_vec_kernel, dim3((planes * 4 + 255) / 256), dim3(256), 0, st, f3.bias, fd.bias, planes * 4);
                if ((rc = pack_conv(own, B.c3, dtype, p3.weight, f3.scale, pd->weight, fd.scale, true, false, st))) return rc;
            } else if ((rc = pack_conv(own, B.c3, dtype, p3.weight, f3.scale, nullptr, nullptr, true, false, st))) {
                return rc;
            }
            // fused-tail packings (16-bit)
            if (h16 && L == 0) {
                if (!(B.w2 = own.take(cp360_l1block_conv2_bytes(dtype)))) return CP360_ERR_HIP;
                if ((rc = cp360_l1block_pack_conv2(dtype, p2.weight, f2.scale, B.w2, st))) return rc;
                B.b2 = f2.bias;
                if (!(B.w3f = own.take(cp360_frag_packed_bytes(dtype, 256, 64)))) return CP360_ERR_HIP;
                if ((rc = cp360_frag_pack_1x1(dtype, p3.weight, f3.scale, B.w3f, 256, 64, 0, st))) return rc;
                B.b3 = f3.bias;               // (with the downsample branch: already b3 + bd)
                if (B.has_ds) {
                    if (!(B.wdf = own.take(cp360_frag_packed_bytes(dtype, 256, 64)))) return CP360_ERR_HIP;
                    if ((rc = cp360_frag_pack_1x1(dtype, pd->weight, fd.scale, B.wdf, 256, 64, 0, st))) return rc;
                    if (b == 0 && inplanes == 64 && planes == 64) {       // the block's own conv1 (64 -> 64) for the in-patch form
                        if (!(B.w0f = own.take(cp360_frag_packed_bytes(dtype, 64, 64)))) return CP360_ERR_HIP;
                        if ((rc = cp360_frag_pack_1x1(dtype, p1.weight, f1.scale, B.w0f, 64, 64, 0, st))) return rc;
                        B.b0 = f1.bias;
                    }
                }
            } else if (h16 && L == 1 && B.has_ds) {          // layer2.0 after its conv1 as one launch (K3f, 56x56 -> 28x28 faces)
                if (!(B.w2 = own.take(cp360_l2block_packed_bytes(dtype)))) return CP360_ERR_HIP;
                if ((rc = cp360_l2block_pack_weights(dtype, p2.weight, f2.scale, B.w2, st))) return rc;
                B.b2 = f2.bias;
                if (!(B.w3f = own.take(cp360_l2first_w3d_bytes(dtype)))) return CP360_ERR_HIP;
                if ((rc = cp360_l2first_pack_w3d(dtype, p3.weight, f3.scale, pd->weight, fd.scale, B.w3f, st))) return rc;
                B.b3 = f3.bias;               // b3 + bd
            } else if (h16 && (L == 1 || L == 2) && !B.has_ds) {
                const size_t nb = L == 1 ? cp360_l2block_packed_bytes(dtype) : cp360_l3block_packed_bytes(dtype);
                if (!(B.w2 = own.take(nb))) return CP360_ERR_HIP;
                rc = L == 1 ? cp360_l2block_pack_weights(dtype, p2.weight, f2.scale, B.w2, st)
                            : cp360_l3block_pack_weights(dtype, p2.weight, f2.scale, B.w2, st);
                if (rc) return rc;
                B.b2 = f2.bias;
                if (!(B.w3f = own.take(cp360_frag_packed_bytes(dtype, planes * 4, planes)))) return CP360_ERR_HIP;
                if ((rc = cp360_frag_pack_1x1(dtype, p3.weight, f3.scale, B.w3f, planes * 4, planes, 0, st))) return rc;
                B.b3 = f3.bias;
            }
            // the NEXT conv1 chained onto the PREVIOUS tail kernel: layer1 blocks (256 -> 64, k-major fragments), layer1's
            // last block (layer2.0's conv1, 256 -> 128, k-major), layer2's identity blocks 2.. (512 -> 128, row-major)
            if (h16) {
                CBlock* prev = nullptr;
                int order = 1;
                if (L == 0 && b > 0) prev = &R.layer[0][b - 1];
                else if (L == 1 && b == 0) prev = &R.layer[0][nblk[0] - 1];
                else if (L == 1 && b >= 1) { prev = &R.layer[1][b - 1]; order = 0; }   // (b == 1: onto layer2.0's fused kernel)
                if (prev) {
                    if (!(prev->w1f = own.take(cp360_frag_packed_bytes(dtype, planes, inplanes)))) return CP360_ERR_HIP;
                    if ((rc = cp360_frag_pack_1x1(dtype, p1.weight, f1.scale, prev->w1f, planes, inplanes, order, st))) return rc;
                    prev->b1n = f1.bias;
                    prev->next_c = planes;
                }
            }
            inplanes = planes * 4;
        }
    }
    if (idx != 53) return CP360_ERR_BAD_SHAPE;
    // ---- CAM: 1x1 convolution with the shifted classifier weight (class_activation_model.py:46-52), raw f32 scores
    {
        const long long n = (long long)num_classes * 2048;
        float* w = (float*)own.take((size_t)n * 4);
        if (!w) return CP360_ERR_HIP;
        hipLaunchKernelGGL(sub_scalar_kernel, dim3(1024), dim3(256), 0, st, fc_weight, fc_shift, w, n);
        set_geom(R.cam, num_classes, 2048, 1, 1, 0, 0);
        if ((rc = pack_conv(own, R.cam, dtype, w, nullptr, nullptr, nullptr, true, false, st))) return rc;
    }
    CP360_CHECK_HIP();
    R.loaded = true;
    return CP360_OK;
}

namespace {

// ---------------------------------------------------------------- the stage planner: plan once, then run / size / describe
// A plan is a list of steps over SYMBOLIC operands.  plan_resnet() / plan_clstm() are the only functions that decide anything
// (which kernel, tiles, split-K, which slot a tensor lives in, the workspace, the describing text); run_step() resolves the slots
// to pointers and launches.  A new fused kernel is one StepKind, one rule in the planner and one `case` in run_step().
enum Slot {
    SLOT_NONE = -1,
    SLOT_ACT0, SLOT_ACT1, SLOT_ACT2, SLOT_ACT3,  // activation quarters of the workspace (at most x, mid, out and the next mid live)
    SLOT_INPUT, SLOT_CAM,                        // the caller's input (the stage's faces, the cell's [x | h]) and CAM buffer
    SLOT_PARTIAL, SLOT_BORDER,                   // split-K partial slabs; the fused stem + max-pool kernel's border scratch
    SLOT_HAND,                                   // the hand-over buffer between the per-group front and the joint back (JointPlan)
    SLOT_COUNT
};

enum StepKind {
    STEP_CONV,                                   // generic convolution (+ its split-K finish)
    STEP_F32_FINISH,                             // split-K slabs -> raw f32 sums in a caller-owned buffer (the CAM at one frame)
    STEP_STEM_POOL, STEP_STEM_RESIDENT, STEP_MAXPOOL,
    STEP_L1_FIRST, STEP_L1, STEP_L1_WIDE,
    STEP_L2_FIRST, STEP_L2_TAIL, STEP_L2_TAIL_NEXT, STEP_L3_TAIL
};

struct Step {
    StepKind kind = STEP_CONV;
    const CConv* conv = nullptr;                 // whose packs / bias the step reads (convolutions, the stem)
    const CBlock* block = nullptr;               // ... or whose fused-tail packs
    const void* stem_packed = nullptr;           // ... or the stem kernels' resident-patch packing
    cp360_conv_desc d{};                         // STEP_CONV / STEP_F32_FINISH: fully resolved (splits, slab_rows, clip_resident)
    int size = 0;                                // fused kernels: the face (stem: cube, max-pool: input) size they are told
    // in: the input (a tail kernel's conv1 output `mid`); in2: the second source; res: the residual (tail kernels: the block
    // input x); out; out2: the chained next conv1's output / the border scratch; sums: where raw f32 sums go (SLOT_NONE: none)
    int in = SLOT_NONE, in2 = SLOT_NONE, res = SLOT_NONE, out = SLOT_NONE, out2 = SLOT_NONE, sums = SLOT_NONE;
};

// What a generic convolution call states beyond the convolution and its input geometry; a call site sets what it uses
struct ConvArgs {
    int in, out;
    int ld_out = 0, out_coff = 0;
    int residual = SLOT_NONE, ld_res = 0;
    int x2 = SLOT_NONE, h2 = 0, w2 = 0, ps2 = 0;  // second source and its geometry
    bool raw = false;                            // leave the f32 sums ([splits, M, c_out]) for the caller's epilogue ...
    bool raw_slab_rows = false;                  // ... in packed-row order
    int raw_dst = SLOT_NONE;                     // ... in this caller-owned buffer (reduced there when the planner splits)
    int force_splits = 0;
    explicit ConvArgs(int in_, int out_ = SLOT_NONE) : in(in_), out(out_) {}
};

// What both stages plan: the steps and the split-K workspace they need
struct Plan {
    int dtype = 0, n_img = 0;
    std::vector<Step> steps;
    size_t partial_need = 0;                     // bytes of split-K workspace: the maximum over the steps
    Step& add(StepKind kind) {
        steps.emplace_back();
        steps.back().kind = kind;
        return steps.back();
    }

    // One generic convolution on n_img faces of h x w (ops.Conv.__call__): appends its step (and, for raw sums that the planner
    // splits on their way to a caller-owned buffer, the f32 finish behind it) and returns a copy of the convolution's
    Step conv(const CConv& c, int h, int w, const ConvArgs& a) {
        Step s;
        s.conv = &c;
        cp360_conv_desc& d = s.d;
        fill_desc(c, dtype, n_img, h, w, use_clip(c, dtype, n_img, h, w) ? 1 : 0, &d);
        if (a.ld_out > 0) d.ld_out = a.ld_out;
        d.out_coff = a.out_coff;
        d.ld_res = a.ld_res;
        if (c.c_in2 > 0 && a.h2 > 0) { d.h_in2 = a.h2; d.w_in2 = a.w2; d.pix_stride2 = a.ps2; }
        const int splits = a.force_splits > 0 ? a.force_splits : cp360_conv_suggest_splits(&d);
        d.splits = splits;
        d.slab_rows = (c.c_out % 32 == 0 && ((splits > 1 && !a.raw) || (a.raw && a.raw_slab_rows))) ? 1 : 0;
        s.in = a.in;
        s.in2 = a.x2;
        if (!a.raw) { s.res = a.residual; s.out = a.out; }
        // raw sums with a caller-owned destination AND split-K (the CAM scores at one frame): slabs in the workspace,
        // reduced into raw_dst by an f32 finish
        const bool raw_reduce = a.raw && a.raw_dst != SLOT_NONE && splits > 1;
        if (a.raw || splits > 1) s.sums = a.raw_dst != SLOT_NONE && !raw_reduce ? a.raw_dst : SLOT_PARTIAL;
        if (s.sums == SLOT_PARTIAL)
            partial_need = std::max(partial_need, (size_t)splits * n_img * d.h_out * d.w_out * c.c_out * sizeof(float));
        steps.push_back(s);
        if (raw_reduce) {
            Step f;
            f.kind = STEP_F32_FINISH;
            f.d = d;
            f.d.dtype = CP360_F32;
            f.d.relu = 0;
            f.in = SLOT_PARTIAL;
            f.out = a.raw_dst;
            steps.push_back(f);
        }
        return s;
    }
};

// the pointers behind the slots of one call
struct Bufs {
    void* p[SLOT_COUNT] = {};
    void* operator[](int slot) const { return slot < 0 ? nullptr : p[slot]; }
};

int run_step(const Step& s, const Plan& P, const Bufs& at, hipStream_t st) {
    const int dtype = P.dtype, n = P.n_img;
    const CBlock* B = s.block;
    switch (s.kind) {
    case STEP_CONV: {
        const CConv& c = *s.conv;
        const void* pk = s.d.clip_resident ? c.packed_clip : c.packed;
        if (!pk) return CP360_ERR_UNSUPPORTED;
        if (s.sums == SLOT_NONE) return cp360_conv_forward2(&s.d, at[s.in], at[s.in2], pk, c.bias, at[s.res], at[s.out], nullptr, st);
        float* sums = (float*)at[s.sums];
        const int rc = cp360_conv_forward2(&s.d, at[s.in], at[s.in2], pk, nullptr, nullptr, nullptr, sums, st);
        if (rc || s.out == SLOT_NONE) return rc;
        return cp360_conv_finish(&s.d, sums, c.bias, at[s.res], at[s.out], st);
    }
    case STEP_F32_FINISH:
        return cp360_conv_finish_add(&s.d, (const float*)at[s.in], nullptr, nullptr, nullptr, at[s.out], st);
    case STEP_STEM_POOL:
        return cp360_stem_pool_forward(dtype, at[s.in], s.stem_packed, s.conv->bias, at[s.out], at[s.out2], n, s.size, st);
    case STEP_STEM_RESIDENT:
        return cp360_stem_forward(dtype, at[s.in], s.stem_packed, s.conv->bias, at[s.out], n, s.size, 1, st);
    case STEP_MAXPOOL:
        return cp360_cubepad_maxpool3s2(at[s.in], at[s.out], n, s.size, 64, dtype, st);
    case STEP_L1_FIRST:                                  // in: the block input x (conv1 runs inside the kernel)
        return cp360_l1block_forward_first(dtype, at[s.in], B->w0f, B->b0, B->w2, B->b2, B->w3f, B->b3, B->wdf, at[s.out], B->w1f,
                                           B->b1n, at[s.out2], n, s.size, st);
    case STEP_L1:                                        // block 0: x feeds the downsample branch; later blocks: x is the residual
        return cp360_l1block_forward(dtype, at[s.in], B->w2, B->b2, B->w3f, B->b3, B->has_ds ? nullptr : at[s.res],
                                     B->has_ds ? at[s.res] : nullptr, B->wdf, at[s.out], B->w1f, B->b1n, at[s.out2], n, s.size, st);
    case STEP_L1_WIDE:
        return cp360_l1block_forward_wide(dtype, at[s.in], B->w2, B->b2, B->w3f, B->b3, at[s.res], at[s.out], B->w1f, B->b1n,
                                          at[s.out2], n, s.size, st);
    case STEP_L2_FIRST: {
        const bool next = s.out2 != SLOT_NONE;
        return cp360_l2first_forward(dtype, at[s.in], B->w2, B->b2, B->w3f, B->b3, at[s.res], at[s.out], next ? B->w1f : nullptr,
                                     next ? B->b1n : nullptr, at[s.out2], n, s.size, st);
    }
    case STEP_L2_TAIL:
        return cp360_l2block_forward(dtype, at[s.in], B->w2, B->b2, B->w3f, B->b3, at[s.res], at[s.out], n, s.size, st);
    case STEP_L2_TAIL_NEXT:
        return cp360_l2block_forward_next(dtype, at[s.in], B->w2, B->b2, B->w3f, B->b3, at[s.res], at[s.out], B->w1f, B->b1n,
                                          at[s.out2], n, s.size, st);
    case STEP_L3_TAIL:
        return cp360_l3block_forward(dtype, at[s.in], B->w2, B->b2, B->w3f, B->b3, at[s.res], at[s.out], n, s.size, st);
    }
    return CP360_ERR_UNSUPPORTED;
}

// an activation slot that holds none of the (up to three) live tensors
int free_slot(int a, int b = SLOT_NONE, int c = SLOT_NONE) {
    int s = SLOT_ACT0;
    while (s == a || s == b || s == c) ++s;
    return s;
}

struct ResnetWs {
    size_t act = 0, partial = 0, border = 0;
    size_t total() const { return 4 * act + partial + border; }
};

struct StagePlan : Plan {
    bool describe = false;                       // also write `text`: one line per note / planned generic launch
    std::string text;
    char where[32] = "";
    void note(const char* line) {
        if (describe) { text += line; text += "\n"; }
    }
    void at(int layer, int block) { snprintf(where, sizeof(where), "layer%d.%d", layer, block); }
    void conv(const CConv& c, int h, int w, const ConvArgs& a) {
        const Step s = Plan::conv(c, h, w, a);
        if (!describe) return;
        char plan[200], line[320];
        cp360_conv_desc dd = s.d;
        dd.splits = 1;
        if (cp360_conv_plan_describe(&dd, plan, sizeof(plan)) < 0) plan[0] = 0;
        snprintf(line, sizeof(line), "  %s conv %dx%d %d -> %d @ %dx%d%s: %s%s", where, c.kh_w, c.kw_w, c.c_in_w, c.c_out, h, w,
                 c.stride > 1 ? " stride 2" : "", plan, a.force_splits > 0 ? " (split count fixed by the caller)" : "");
        note(line);
    }
    size_t n_ordered = 0;                        // steps [0, n_ordered) run under launch order 2, the CAM after the restore
    // The cut of cp360_resnet_forward_multi (0: this plan has none): steps [0, cut) are the front, run per group; the running
    // activation there (layer3.0's output, in slot cut_x, cut_bytes of it) is handed over; steps [cut, end) are the back
    size_t cut = 0, cut_bytes = 0, text_cut = 0;
    int cut_x = SLOT_NONE;
    int feat = SLOT_NONE;                        // where layer4's output ends up, and its size
    size_t feat_bytes = 0;
    ResnetWs ws;
};

// The static stage on n_img faces of cd x cd (input [n_img, cd+6, cd+6, 4] NHWC4): its launch sequence, workspace and text
int plan_resnet(const CResnet& R, int n_img, int cd, StagePlan* P) {
    if (!R.loaded) return CP360_ERR_NULL;
    if (n_img <= 0 || cd < 32 || cd % 32 != 0) return CP360_ERR_BAD_SHAPE;
    if (n_img % 6 != 0) return CP360_ERR_BATCH_NOT_6N;
    const int dtype = R.dtype, es = es_of(dtype);
    const bool h16 = dtype != CP360_F32;
    P->dtype = dtype;
    P->n_img = n_img;
    P->steps.reserve(64);
    P->ws.act = align_up((size_t)n_img * (cd / 2) * (cd / 2) * 64 * es);   // the largest activation: stem output = layer1 output
    P->ws.border = align_up(cp360_stem_pool_border_bytes(n_img));
    if (P->describe) {
        char head[160];
        snprintf(head, sizeof(head), "static stage, %d faces of %d^2, %s:", n_img, cd,
                 dtype == CP360_F32 ? "f32" : (dtype == CP360_F16 ? "f16" : "bf16"));
        P->note(head);
    }
    int x = SLOT_ACT0;                                   // the running activation
    int mid = SLOT_NONE;                                 // the next block's conv1 output, where a fused kernel already computed it
    int face = cd / 4;
    // ---- stem + CubePad(1) + max-pool
    if (h16 && cd == 224) {
        P->note("stem: FUSED stem + CubePad(1) + max-pool, one launch (K3a+K3b, cube 224, 16-bit)");
        Step& s = P->add(STEP_STEM_POOL);
        s.conv = &R.stem; s.stem_packed = R.stem_packed; s.in = SLOT_INPUT; s.out = x; s.out2 = SLOT_BORDER; s.size = cd;
    } else {
        const int full = free_slot(x);                   // the stem's output in front of the max-pool
        if (h16 && cd == 512) {
            P->note("stem: resident-patch stem kernel (K3a, cube 512, 16-bit) + cubepad_maxpool kernel");
            Step& s = P->add(STEP_STEM_RESIDENT);
            s.conv = &R.stem; s.stem_packed = R.stem_packed; s.in = SLOT_INPUT; s.out = full; s.size = cd;
        } else {
            P->note("stem: generic convolution (7 taps of 8 pixels x 4 channels) + cubepad_maxpool kernel");
            snprintf(P->where, sizeof(P->where), "stem");
            P->conv(R.stem, cd + 6, cd + 6, ConvArgs(SLOT_INPUT, full));
        }
        Step& s = P->add(STEP_MAXPOOL);
        s.in = full; s.out = x; s.size = cd / 2;
    }
    // per-convolution Bottleneck (Bottleneck.forward_nhwc): x -> a free slot; conv1 is skipped where `mid` already holds it
    auto bottleneck = [&](const CBlock& B, int hin) {
        const int hout = (hin + 2 - 3) / B.stride + 1;
        if (mid == SLOT_NONE) {
            mid = free_slot(x);
            P->conv(B.c1, hin, hin, ConvArgs(x, mid));
        }
        const int mid2 = free_slot(x, mid), out = free_slot(x, mid, mid2);
        P->conv(B.c2, hin, hin, ConvArgs(mid, mid2));
        ConvArgs a(mid2, out);
        if (B.has_ds) { a.x2 = x; a.h2 = a.w2 = hin; a.ps2 = B.c3.c_in2; }
        else { a.residual = x; a.ld_res = B.c3.c_out; }
        P->conv(B.c3, hout, hout, a);
        x = out;
        mid = SLOT_NONE;
    };
    // a fused tail kernel: mid (+ x as residual / second source) -> out (+ the next block's conv1 output when `chained`)
    auto tail = [&](StepKind kind, const CBlock& B, int size, bool chained) {
        Step& s = P->add(kind);
        s.block = &B;
        s.size = size;
        s.in = kind == STEP_L1_FIRST ? x : mid;
        s.res = x;
        s.out = free_slot(x, mid);
        s.out2 = chained ? free_slot(x, mid, s.out) : SLOT_NONE;
        x = s.out;
        mid = s.out2;
    };
    auto conv1 = [&](const CBlock& B) {                  // a fused tail's conv1 as its own launch, unless `mid` holds it
        if (mid != SLOT_NONE) return;
        mid = free_slot(x);
        P->conv(B.c1, face, face, ConvArgs(x, mid));
    };
    // ---- layer1
    {
        const std::vector<CBlock>& Lr = R.layer[0];
        if (h16 && (face == 56 || face == 128)) {
            // conv1 of block 0 inside the block's tail kernel at face 56; at face 128 (or without its packed filter) its own launch
            const bool first_in = face == 56 && Lr[0].w0f != nullptr;
            P->note(first_in ? "layer1: ONE fused launch per Bottleneck (K3d: [block 0: its conv1 on the resident patch +] conv2 + conv3 + residual / downsample + the next conv1)"
                             : "layer1: conv1 of block 0, then ONE fused launch per Bottleneck (K3d: conv2 + conv3 + residual / downsample + the next conv1)");
            P->at(1, 0);
            if (!first_in) conv1(Lr[0]);
            // every block's kernel also computes the next conv1 - the last one layer2.0's (256 -> 128: the wide form)
            for (size_t b = 0; b < Lr.size(); ++b)
                tail(b == 0 && first_in ? STEP_L1_FIRST : (b > 0 && Lr[b].next_c == 128 ? STEP_L1_WIDE : STEP_L1), Lr[b], face,
                     Lr[b].w1f != nullptr);
            if (Lr.back().next_c != 128) mid = SLOT_NONE;      // `mid` carries over only as layer2.0's conv1 (256 -> 128)
        } else {
            P->note("layer1: GENERIC path, one launch per convolution (the fused tail kernels need a 16-bit type and 56x56 / 128x128 faces)");
            for (size_t b = 0; b < Lr.size(); ++b) { P->at(1, (int)b); bottleneck(Lr[b], face); }
        }
    }
    // ---- layer2 / layer3: first block per convolution, identity blocks as fused tails where the kernels exist
    for (int L = 1; L <= 2; ++L) {
        const std::vector<CBlock>& Lr = R.layer[L];
        if (L == 2) mid = SLOT_NONE;                     // no kernel of layer2 computes layer3.0's conv1
        P->at(L + 1, 0);
        if (L == 1 && h16 && face == 56) {
            // layer2.0: conv1 (unless layer1's last tail kernel computed it), then ONE launch (K3f), which also computes
            // layer2.1's conv1
            P->note("layer2.0: ONE fused launch after its conv1 (K3f: stride-2 conv2 + conv3 + downsample + layer2.1's conv1)");
            conv1(Lr[0]);
            tail(STEP_L2_FIRST, Lr[0], face / 2, Lr[0].w1f != nullptr);
        } else {
            P->note(L == 1 ? "layer2.0: generic path, one launch per convolution (downsample branch inside conv3)"
                           : "layer3.0: generic path, one launch per convolution (downsample branch inside conv3)");
            bottleneck(Lr[0], face);
        }
        face /= 2;
        const bool fused = h16 && (L == 1 ? (face == 28 || face == 64) : (face == 14 || face == 32));
        if (!fused) {
            P->note(L == 1 ? "layer2.1-3: GENERIC path, one launch per convolution (the fused tail kernel needs a 16-bit type and 28x28 / 64x64 faces)"
                           : "layer3.1-5: GENERIC path, one launch per convolution (the fused tail kernel needs a 16-bit type and 14x14 / 32x32 faces)");
            for (size_t b = 1; b < Lr.size(); ++b) { P->at(L + 1, (int)b); bottleneck(Lr[b], face); }
            continue;
        }
        P->note(L == 1 ? "layer2.1-3: conv1 + ONE fused tail launch per Bottleneck (K3e; at 28x28 faces the next block's conv1 rides on the tail)"
                       : "layer3.1-5: conv1 + ONE fused tail launch per Bottleneck (K3e, C = 256)");
        const bool chain = L == 1 && face == 28;          // the next block's conv1 rides on the tail kernel
        if (L == 2 && cd == 224) {
            // the 14x14 and 7x7 layers of several batches may run as ONE pass from here (layer3.1's conv1): measured at 64 against
            // 128 frames, the layer3 tails cost 0.96 and layer4's 7x7 launches 0.70 - 0.76 of twice the single pass (148 tiles of
            // 256 pixels per batch fill the chip badly); the 56x56 / 28x28 launches are 5 - 10 rounds of the chip either way
            P->cut = P->steps.size();
            P->cut_x = x;
            P->cut_bytes = (size_t)n_img * face * face * Lr[0].c3.c_out * es;
            P->text_cut = P->text.size();
        }
        for (size_t b = 1; b < Lr.size(); ++b) {
            const CBlock& B = Lr[b];
            P->at(L + 1, (int)b);
            conv1(B);
            if (chain && B.w1f) tail(STEP_L2_TAIL_NEXT, B, face, true);
            else tail(L == 1 ? STEP_L2_TAIL : STEP_L3_TAIL, B, face, false);
        }
    }
    // ---- layer4: per convolution (conv2 on the clip-resident kernel at 7x7 / 16x16 faces)
    P->note("layer4: one launch per convolution (conv2 clip-resident or on small tiles by cp360_conv_prefer_clip; downsample inside conv3)");
    for (size_t b = 0; b < R.layer[3].size(); ++b) {
        P->at(4, (int)b);
        bottleneck(R.layer[3][b], face);
        if (b == 0) face /= 2;
    }
    // ---- CAM: raw f32 scores [n_img, face, face, num_classes] straight into the caller's buffer (no bias / activation)
    P->note("CAM: 1x1 convolution with the shifted fc.weight, raw f32 scores (split-K reduced by an f32 finish when the planner splits)");
    snprintf(P->where, sizeof(P->where), "CAM");
    P->n_ordered = P->steps.size();
    ConvArgs a(x);
    a.raw = true;
    a.raw_dst = SLOT_CAM;
    P->conv(R.cam, face, face, a);
    P->feat = x;
    P->feat_bytes = (size_t)n_img * face * face * 2048 * es;
    P->ws.partial = align_up(P->partial_need);
    return CP360_OK;
}

// the launch-order hint for the span of an object, restored on every exit
struct LaunchOrder {
    int old;
    bool held = true;
    explicit LaunchOrder(int mode) : old(cp360_set_launch_order(mode)) {}
    void restore() { if (held) cp360_set_launch_order(old); held = false; }
    ~LaunchOrder() { restore(); }
};

int run_plan(const StagePlan& P, const void* faces_p3, float* cam_out, void* feat_out, unsigned char* ws, hipStream_t st) {
    Bufs at;
    for (int i = 0; i < 4; ++i) at.p[SLOT_ACT0 + i] = ws + i * P.ws.act;
    at.p[SLOT_INPUT] = const_cast<void*>(faces_p3);
    at.p[SLOT_CAM] = cam_out;
    at.p[SLOT_PARTIAL] = ws + 4 * P.ws.act;
    at.p[SLOT_BORDER] = ws + 4 * P.ws.act + P.ws.partial;
    LaunchOrder order(2);
    for (size_t i = 0; i < P.steps.size(); ++i) {
        if (i == P.n_ordered) order.restore();
        const int rc = run_step(P.steps[i], P, at, st);
        if (rc) return rc;
    }
    if (feat_out && hipMemcpyAsync(feat_out, at[P.feat], P.feat_bytes, hipMemcpyDeviceToDevice, st) != hipSuccess) return CP360_ERR_HIP;
    return CP360_OK;
}

}  // namespace

// ---------------------------------------------------------------- the static stages of several batches, back half as one pass
// The front (stem .. layer3.0) runs per group at n_img faces; each group's layer3.0 output goes straight into its rows of a
// hand-over buffer; the back (layer3.1 .. layer4, CAM) runs ONCE at n_groups * n_img faces.  The back's steps are the steps
// of the plan at n_img faces with the image count replaced: split-K count, K ranges, finish order and epilogue are the
// descriptor's, the kernel is pinned through tile_px - every output row is summed exactly as in the plan at n_img faces.
namespace {
struct JointPlan {
    StagePlan one;                               // the plan of one group; its steps [0, cut) are the front
    Plan back;
    size_t back_ordered = 0;                     // back steps [0, back_ordered) run under launch order 2
    size_t partial = 0, hand = 0;                // hand: the hand-over buffer of all groups
    int n_groups = 0;
    size_t total() const { return 4 * one.ws.act + partial + one.ws.border + hand; }
};

// CP360_OK: the joint plan; CP360_ERR_UNSUPPORTED: this geometry / type has no cut (run cp360_resnet_forward per group)
int plan_joint(const CResnet& R, int n_groups, int n_img, int cd, JointPlan* J) {
    if (n_groups <= 0 || n_groups > CP360_MAX_CLIP_GROUPS) return CP360_ERR_BAD_SHAPE;
    const int rc = plan_resnet(R, n_img, cd, &J->one);
    if (rc) return rc;
    J->n_groups = n_groups;
    const StagePlan& S = J->one;
    J->partial = S.ws.partial;
    if (n_groups == 1) return CP360_OK;                   // the plain plan
    // the producer of the handed-over activation must be the front's last step, and the back must fit the front's slots
    if (S.cut == 0 || S.cut >= S.n_ordered || S.steps[S.cut - 1].out != S.cut_x) return CP360_ERR_UNSUPPORTED;
    if ((size_t)n_groups * S.cut_bytes > S.ws.act) return CP360_ERR_UNSUPPORTED;
    if ((long long)n_groups * n_img > 0x7fffffff / (14 * 14 * 1024)) return CP360_ERR_BAD_SHAPE;   // the kernels' 32-bit offsets
    Plan& B = J->back;
    B.dtype = S.dtype;
    B.n_img = n_groups * n_img;
    bool handed = true;                                   // until a back step reuses slot cut_x, reads of it mean the hand-over buffer
    for (size_t i = S.cut; i < S.steps.size(); ++i) {
        Step s = S.steps[i];
        if (handed) {
            if (s.in == S.cut_x) s.in = SLOT_HAND;
            if (s.in2 == S.cut_x) s.in2 = SLOT_HAND;
            if (s.res == S.cut_x) s.res = SLOT_HAND;
            if (s.out == S.cut_x || s.out2 == S.cut_x) handed = false;
        }
        const int tile = s.kind == STEP_CONV ? cp360_conv_plan_tile(&s.d) : 0;
        if (s.kind == STEP_CONV || s.kind == STEP_F32_FINISH) {
            s.d.n_img = B.n_img;
            if (tile == 160 || tile == 256 || tile == 304) {
                // the three pixel tiles of conv_igemm_ring_kernel share one K loop (ring_body: the same steps in the same order for
                // every output element), so among them the cost model may choose again for the joint pixel count; any other
                // kernel stays the one of the plan at n_img faces
                const int joint = cp360_conv_plan_tile(&s.d);
                s.d.tile_px = (joint == 160 || joint == 256 || joint == 304) ? joint : tile;
            } else {
                s.d.tile_px = tile;
            }
            if (s.kind == STEP_CONV && cp360_conv_packed_bytes(&s.d) == 0) return CP360_ERR_UNSUPPORTED;   // (a bound of the kernels at this count)
            if (s.sums == SLOT_PARTIAL || (s.kind == STEP_F32_FINISH && s.in == SLOT_PARTIAL))
                B.partial_need = std::max(B.partial_need, (size_t)s.d.splits * B.n_img * s.d.h_out * s.d.w_out * s.d.c_out * sizeof(float));
        }
        B.steps.push_back(s);
    }
    J->back_ordered = S.n_ordered - S.cut;
    J->partial = std::max(S.ws.partial, align_up(B.partial_need));
    J->hand = align_up((size_t)n_groups * S.cut_bytes);
    return CP360_OK;
}

int run_joint(const JointPlan& J, const void* const* faces_p3, float* cam_out, unsigned char* ws, hipStream_t st) {
    const StagePlan& S = J.one;
    Bufs at;
    for (int i = 0; i < 4; ++i) at.p[SLOT_ACT0 + i] = ws + i * S.ws.act;
    at.p[SLOT_CAM] = cam_out;
    at.p[SLOT_PARTIAL] = ws + 4 * S.ws.act;
    at.p[SLOT_BORDER] = ws + 4 * S.ws.act + J.partial;
    unsigned char* hand = ws + 4 * S.ws.act + J.partial + S.ws.border;
    LaunchOrder order(2);
    for (int g = 0; g < J.n_groups; ++g) {
        cp360_set_launch_order(2);                        // every front starts the alternation where the plain pass does;
        at.p[SLOT_INPUT] = const_cast<void*>(faces_p3[g]);            // the back goes on from the last front's phase at the cut
        at.p[SLOT_HAND] = hand + (size_t)g * S.cut_bytes;
        for (size_t i = 0; i < S.cut; ++i) {
            Step s = S.steps[i];
            if (i == S.cut - 1) s.out = SLOT_HAND;
            const int rc = run_step(s, S, at, st);
            if (rc) return rc;
        }
    }
    at.p[SLOT_INPUT] = nullptr;
    at.p[SLOT_HAND] = hand;
    for (size_t i = 0; i < J.back.steps.size(); ++i) {
        if (i == J.back_ordered) order.restore();
        const int rc = run_step(J.back.steps[i], J.back, at, st);
        if (rc) return rc;
    }
    return CP360_OK;
}

}  // namespace

// 1: cp360_resnet_forward_multi runs the back half of n_groups batches of n_img faces as one pass (16-bit types, cube 224,
// 2 .. CP360_MAX_CLIP_GROUPS groups); 0: it does not (f32, other cube sizes, one group, nothing loaded): one
// cp360_resnet_forward per batch is the way there.
extern "C" int cp360_resnet_can_pair_static(cp360_ctx* ctx, int n_groups, int n_img, int cube_dim) {
    if (!ctx || n_groups < 2) return 0;
    JointPlan J;
    return plan_joint(ctx->rn, n_groups, n_img, cube_dim, &J) == CP360_OK ? 1 : 0;
}

extern "C" size_t cp360_resnet_forward_multi_workspace_bytes(cp360_ctx* ctx, int n_groups, int n_img, int cube_dim) {
    if (!ctx) return 0;
    JointPlan J;
    return plan_joint(ctx->rn, n_groups, n_img, cube_dim, &J) ? 0 : J.total();
}

extern "C" int cp360_resnet_forward_multi(cp360_ctx* ctx, const void* const* faces_p3, int n_groups, int n_img, int cube_dim,
                                          float* const* cam_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx || !faces_p3 || !cam_out) return CP360_ERR_NULL;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return CP360_ERR_HIP;
    JointPlan J;
    const int rc = plan_joint(ctx->rn, n_groups, n_img, cube_dim, &J);
    if (rc) return rc;
    if (!workspace) return CP360_ERR_NULL;
    const size_t per_group = (size_t)n_img * (cube_dim / 32) * (cube_dim / 32) * ctx->rn.num_classes;
    for (int g = 0; g < n_groups; ++g) {
        if (!faces_p3[g] || !cam_out[g]) return CP360_ERR_NULL;
        if (cam_out[g] != cam_out[0] + (size_t)g * per_group) return CP360_ERR_BAD_SHAPE;   // ONE CAM launch writes all groups
    }
    if (((size_t)workspace & 255) != 0) return CP360_ERR_ALIGN;
    if (workspace_bytes < J.total()) return CP360_ERR_BAD_SHAPE;
    if (n_groups == 1) return run_plan(J.one, faces_p3[0], cam_out[0], nullptr, (unsigned char*)workspace, (hipStream_t)stream);
    return run_joint(J, faces_p3, cam_out[0], (unsigned char*)workspace, (hipStream_t)stream);
}

extern "C" int cp360_resnet_plan_describe_multi(cp360_ctx* ctx, int n_groups, int n_img, int cube_dim, char* buf, size_t cap) {
    if (!ctx || !buf || cap == 0) return CP360_ERR_NULL;
    JointPlan J;
    J.one.describe = true;
    const int rc = plan_joint(ctx->rn, n_groups, n_img, cube_dim, &J);
    if (rc) return rc;
    std::string text;
    if (n_groups == 1) {
        text = J.one.text;
    } else {
        char line[320];
        const std::string& t = J.one.text;
        const size_t head = t.find('\n') + 1;
        snprintf(line, sizeof(line), "static stages of %d groups, back half as one pass; per group: %s", n_groups, t.substr(0, head).c_str());
        text = line;
        snprintf(line, sizeof(line), "FRONT: %zu launch steps, once per group at %d faces (stem .. layer3.0)\n", J.one.cut, n_img);
        text += line;
        text += t.substr(head, J.one.text_cut - head);
        snprintf(line, sizeof(line), "CUT: in front of layer3.1's conv1; layer3.0's output [%d, 14, 14, 1024] of every group is written into its "
                 "rows of the hand-over buffer (%zu bytes)\n", n_img, J.hand);
        text += line;
        snprintf(line, sizeof(line), "BACK: %zu launch steps, ONCE at %d x %d = %d faces; kernel, split-K count and K ranges of every launch "
                 "are those of the plan at %d faces listed here (workgroups: x %d)\n", J.back.steps.size(), n_groups, n_img, n_groups * n_img,
                 n_img, n_groups);
        text += line;
        text += t.substr(J.one.text_cut);
    }
    const size_t n = text.size() < cap - 1 ? text.size() : cap - 1;
    memcpy(buf, text.data(), n);
    buf[n] = 0;
    return (int)n;
}

extern "C" int cp360_resnet_plan_describe(cp360_ctx* ctx, int n_img, int cube_dim, char* buf, size_t cap) {
    if (!ctx || !buf || cap == 0) return CP360_ERR_NULL;
    StagePlan plan;
    plan.describe = true;
    const int rc = plan_resnet(ctx->rn, n_img, cube_dim, &plan);
    if (rc) return rc;
    const size_t n = plan.text.size() < cap - 1 ? plan.text.size() : cap - 1;
    memcpy(buf, plan.text.data(), n);
    buf[n] = 0;
    return (int)n;
}

extern "C" size_t cp360_resnet_workspace_bytes(cp360_ctx* ctx, int n_img, int cube_dim) {
    if (!ctx) return 0;
    StagePlan plan;
    return plan_resnet(ctx->rn, n_img, cube_dim, &plan) ? 0 : plan.ws.total();
}

extern "C" int cp360_resnet_forward(cp360_ctx* ctx, const void* faces_p3, int n_img, int cube_dim, float* cam_out,
                                    void* feat_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx) return CP360_ERR_NULL;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return CP360_ERR_HIP;
    StagePlan plan;
    const int rc = plan_resnet(ctx->rn, n_img, cube_dim, &plan);
    if (rc) return rc;
    if (!faces_p3 || !cam_out || !workspace) return CP360_ERR_NULL;
    if (((size_t)workspace & 255) != 0) return CP360_ERR_ALIGN;
    if (workspace_bytes < plan.ws.total()) return CP360_ERR_BAD_SHAPE;
    return run_plan(plan, faces_p3, cam_out, feat_out, (unsigned char*)workspace, (hipStream_t)stream);
}

// ---------------------------------------------------------------- ConvLSTM cell
extern "C" int cp360_clstm_load(cp360_ctx* ctx, int dtype, const float* w1, const float* b1, const float* w2, const float* b2,
                                const float* wg, const float* bg, int input_size, int hidden_size, int face, void* stream) {
    if (!ctx || !w1 || !b1 || !w2 || !b2 || !wg || !bg) return CP360_ERR_NULL;
    if (dtype != CP360_F32 && dtype != CP360_BF16 && dtype != CP360_F16) return CP360_ERR_BAD_DTYPE;
    if (input_size <= 0 || hidden_size <= 0 || face <= 0 || hidden_size % 4 != 0) return CP360_ERR_BAD_SHAPE;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return CP360_ERR_HIP;
    hipStream_t st = (hipStream_t)stream;
    ctx->own_clstm.release();
    ctx->cl = CClstm();
    CClstm& Cl = ctx->cl;
    Owned& own = ctx->own_clstm;
    Cl.dtype = dtype; Cl.cin = input_size; Cl.ch = hidden_size;
    const int c4 = 4 * hidden_size;
    set_geom(Cl.c1, c4, input_size + hidden_size, 3, 1, 1, 1);
    set_geom(Cl.c2, c4, c4, 3, 1, 1, 1);
    set_geom(Cl.g, c4, c4, 3, 1, 1, 0);
    auto own_copy = [&](const float* src, int n) -> float* {
        float* d = (float*)own.take((size_t)n * 4);
        if (d && hipMemcpyAsync(d, src, (size_t)n * 4, hipMemcpyDeviceToDevice, st) != hipSuccess) return nullptr;
        return d;
    };
    if (!(Cl.c1.bias = own_copy(b1, c4)) || !(Cl.c2.bias = own_copy(b2, c4)) || !(Cl.gbias = own_copy(bg, c4))) return CP360_ERR_HIP;
    // one packing per convolution: the layout the kernel chosen for THIS face size reads (0.72 GB in 16-bit types)
    const bool clip = clip_geometry(Cl.c1, 6, face, face);
    int rc;
    if ((rc = pack_conv(own, Cl.c1, dtype, w1, nullptr, nullptr, nullptr, !clip, clip, st))) return rc;
    if ((rc = pack_conv(own, Cl.c2, dtype, w2, nullptr, nullptr, nullptr, !clip, clip, st))) return rc;
    if ((rc = pack_conv(own, Cl.g, dtype, wg, nullptr, nullptr, nullptr, !clip, clip, st))) return rc;
    CP360_CHECK_HIP();
    Cl.loaded = true;
    return CP360_OK;
}

// 0: a cell update on n_clips cubes of face x face runs on the direct kernels; 1: in the Winograd domain (filters loaded); 2: it
// would, once cp360_clstm_load_wino has been called - until then cp360_clstm_step / cp360_clstm_window take the direct kernels
extern "C" int cp360_clstm_wino_state(cp360_ctx* ctx, int n_clips, int face) {
    if (!ctx || !ctx->cl.loaded || n_clips <= 0 || face <= 0) return 0;
    if (!wino_wanted(ctx->cl, n_clips, face)) return 0;
    return ctx->cl.wino_loaded ? 1 : 2;
}

// Pack U = G g G^T of the three filters (f32 OIHW on the device, as cp360_clstm_load's) for the Winograd path: 16 / 9 of the
// direct packing's bytes (1.28 GB at 1000 hidden channels), so it is made only when a launch shape asks for it.
extern "C" int cp360_clstm_load_wino(cp360_ctx* ctx, const float* w1, const float* w2, const float* wg, void* stream) {
    if (!ctx || !w1 || !w2 || !wg) return CP360_ERR_NULL;
    CClstm& Cl = ctx->cl;
    if (!Cl.loaded) return CP360_ERR_NULL;
    if (Cl.dtype == CP360_F32) return CP360_ERR_BAD_DTYPE;
    if (Cl.wino_loaded) return CP360_OK;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return CP360_ERR_HIP;
    cp360_wino_desc d1, d2, dg;
    wino_descs(Cl, 6, 8, &d1, &d2, &dg);
    const cp360_wino_desc* ds[3] = {&d1, &d2, &dg};
    const float* ws[3] = {w1, w2, wg};
    void** us[3] = {&Cl.u1, &Cl.u2, &Cl.ug};
    for (int k = 0; k < 3; ++k) {
        const size_t nb = cp360_wino_packed_bytes(ds[k]);
        if (!nb) return CP360_ERR_UNSUPPORTED;
        if (!(*us[k] = ctx->own_clstm.take(nb))) return CP360_ERR_HIP;
        const int rc = cp360_wino_pack_weights(ds[k], ws[k], *us[k], stream);
        if (rc) return rc;
    }
    Cl.wino_loaded = true;
    return CP360_OK;
}

namespace {
struct ClstmWs {
    size_t act = 0, partial = 0;
    size_t wv = 0, wm = 0;                         // Winograd path: V (transformed input) and M (f32 position sums) instead of slabs
    size_t total() const { return 2 * act + partial + wv + wm; }
};

struct ClstmPlan : Plan {
    bool wino = false;                             // the cell update in the Winograd domain (csrc/wino.hip) ...
    cp360_wino_desc d1{}, d2{}, dg{};
    int face = 0, M = 0, splits = 1, slab_rows = 0;          // ... or on the direct kernels: `steps` = Conv1, Conv2, Gates (raw slabs)
    ClstmWs ws;
};

// One cell update on n_clips cubes of face x face
int plan_clstm(const CClstm& Cl, int n_clips, int face, ClstmPlan* P) {
    if (!Cl.loaded) return CP360_ERR_NULL;
    if (n_clips <= 0 || face <= 0) return CP360_ERR_BAD_SHAPE;
    const int n6 = 6 * n_clips, c4 = 4 * Cl.ch;
    P->dtype = Cl.dtype;
    P->n_img = n6;
    P->face = face;
    P->M = n6 * face * face;
    P->ws.act = align_up((size_t)P->M * c4 * es_of(Cl.dtype));
    P->wino = Cl.wino_loaded && wino_wanted(Cl, n_clips, face);
    if (P->wino) {
        wino_descs(Cl, n6, face, &P->d1, &P->d2, &P->dg);
        // V / M are shared by the three convolutions: sized for the largest (Conv1's K = input + hidden channels exceeds Conv2's
        // 4 * hidden when input > 3 * hidden)
        P->ws.wv = align_up(std::max(cp360_wino_v_bytes(&P->d1), std::max(cp360_wino_v_bytes(&P->d2), cp360_wino_v_bytes(&P->dg))));
        P->ws.wm = align_up(std::max(cp360_wino_m_bytes(&P->d1), std::max(cp360_wino_m_bytes(&P->d2), cp360_wino_m_bytes(&P->dg))));
        return CP360_OK;
    }
    // clstm.py:55-64: cat(x, h) -> [CubePad(1) + conv3x3 + bias + relu] x 2 -> CubePad(1) + conv3x3 (Gates, bias in the gate kernel)
    ConvArgs a(SLOT_INPUT, SLOT_ACT0);
    a.ld_out = c4;
    P->conv(Cl.c1, face, face, a);
    a.in = SLOT_ACT0;
    a.out = SLOT_ACT1;
    P->conv(Cl.c2, face, face, a);
    ConvArgs g(SLOT_ACT1);
    g.raw = true;
    g.raw_slab_rows = c4 % 32 == 0;                // gate slabs in packed-row order (64-byte stores)
    P->splits = P->conv(Cl.g, face, face, g).d.splits;
    P->slab_rows = g.raw_slab_rows ? 1 : 0;
    P->ws.partial = align_up(P->partial_need);
    return CP360_OK;
}

// The pointers of cp360_clstm_step that the gate kernels take
struct CellIo {
    void* xh;
    const float* c_prev;
    float *c_next, *h_f32;
    const float* const* x_groups;                  // NULL, or frame t+1 of the first clip of every group (host array)
    int n_groups, group_clips;
    const float* minmax;
    size_t clip_stride;
};

int run_clstm(const ClstmPlan& P, const CClstm& Cl, const CellIo& c, unsigned char* ws, hipStream_t st) {
    unsigned char *a1 = ws, *a2 = ws + P.ws.act;
    int rc;
    if (P.wino) {
        // per convolution input transform -> 16 GEMMs -> output transform (+ bias + ReLU); the Gates convolution's output
        // transform is the gate kernel
        unsigned char* v = ws + 2 * P.ws.act;
        float* m = (float*)(ws + 2 * P.ws.act + P.ws.wv);
        // between two convolutions the output transform of one and the input transform of the next are ONE launch (faces up to
        // 9 x 9: cp360_wino_output_input; larger faces: the two launches through the activation buffers a1 / a2)
        if ((rc = cp360_wino_input(&P.d1, c.xh, v, st))) return rc;
        if ((rc = cp360_wino_gemm(&P.d1, v, Cl.u1, m, st))) return rc;
        rc = cp360_wino_output_input(&P.d1, m, Cl.c1.bias, v, st);
        if (rc == CP360_ERR_UNSUPPORTED) {
            if ((rc = cp360_wino_output(&P.d1, m, Cl.c1.bias, a1, st))) return rc;
            rc = cp360_wino_input(&P.d2, a1, v, st);
        }
        if (rc) return rc;
        if ((rc = cp360_wino_gemm(&P.d2, v, Cl.u2, m, st))) return rc;
        rc = cp360_wino_output_input(&P.d2, m, Cl.c2.bias, v, st);
        if (rc == CP360_ERR_UNSUPPORTED) {
            if ((rc = cp360_wino_output(&P.d2, m, Cl.c2.bias, a2, st))) return rc;
            rc = cp360_wino_input(&P.dg, a2, v, st);
        }
        if (rc) return rc;
        if ((rc = cp360_wino_gemm(&P.dg, v, Cl.ug, m, st))) return rc;
        return cp360_wino_output_gates_groups(&P.dg, m, Cl.gbias, c.c_prev, c.c_next, c.xh, Cl.cin + Cl.ch, Cl.cin, c.h_f32,
                                              c.x_groups, c.n_groups, c.group_clips, c.minmax, 0, c.clip_stride, st);
    }
    Bufs at;
    at.p[SLOT_INPUT] = c.xh;
    at.p[SLOT_ACT0] = a1;
    at.p[SLOT_ACT1] = a2;
    at.p[SLOT_PARTIAL] = ws + 2 * P.ws.act;
    for (const Step& s : P.steps)
        if ((rc = run_step(s, P, at, st))) return rc;
    // clstm.py:68-80: gates, cell / hidden update; the new hidden goes into the h half of xh; with x_next the next
    // frame's window normalisation (test_temporal.py:77) is written into the x half in the same pass
    return cp360_lstm_gates_next_groups((const float*)at[SLOT_PARTIAL], P.splits, Cl.gbias, c.c_prev, c.c_next, c.xh, Cl.dtype,
                                        Cl.cin + Cl.ch, Cl.cin, c.h_f32, P.M, Cl.ch, P.slab_rows, c.x_groups, c.n_groups,
                                        c.group_clips, c.minmax, 0, 6 * P.face * P.face, c.clip_stride, st);
}
}  // namespace

extern "C" size_t cp360_clstm_workspace_bytes(cp360_ctx* ctx, int n_clips, int face) {
    if (!ctx) return 0;
    ClstmPlan plan;
    return plan_clstm(ctx->cl, n_clips, face, &plan) ? 0 : plan.ws.total();
}

extern "C" int cp360_clstm_step(cp360_ctx* ctx, void* xh, const float* c_prev, float* c_next, float* h_f32, int n_clips,
                                int face, const float* x_next, const float* minmax, size_t clip_stride, void* workspace,
                                size_t workspace_bytes, void* stream) {
    if (!ctx) return CP360_ERR_NULL;
    if (x_next && (!minmax || ctx->cl.cin != ctx->cl.ch)) return CP360_ERR_BAD_SHAPE;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return CP360_ERR_HIP;
    ClstmPlan plan;
    const int rc = plan_clstm(ctx->cl, n_clips, face, &plan);
    if (rc) return rc;
    if (!xh || !c_prev || !c_next || !workspace) return CP360_ERR_NULL;
    if (((size_t)workspace & 255) != 0) return CP360_ERR_ALIGN;
    if (workspace_bytes < plan.ws.total()) return CP360_ERR_BAD_SHAPE;
    const CellIo cell{xh, c_prev, c_next, h_f32, x_next ? &x_next : nullptr, 1, n_clips, minmax, clip_stride};
    return run_clstm(plan, ctx->cl, cell, (unsigned char*)workspace, (hipStream_t)stream);
}

// ---------------------------------------------------------------- one window of the temporal stage
// The window issues exactly the launches of T cp360_clstm_step calls (the same bits); its workspace is one cell update's.
namespace {
int window_plan(cp360_ctx* ctx, int n_clips, int T, int face, size_t* ws_bytes) {
    CClstm& Cl = ctx->cl;
    if (!Cl.loaded) return CP360_ERR_NULL;
    if (n_clips <= 0 || T <= 0 || face <= 0 || Cl.cin != Cl.ch) return CP360_ERR_BAD_SHAPE;
    ClstmPlan plan;
    const int rc = plan_clstm(Cl, n_clips, face, &plan);
    if (rc) return rc;
    *ws_bytes = plan.ws.total();
    return CP360_OK;
}
}  // namespace

extern "C" size_t cp360_clstm_window_workspace_bytes(cp360_ctx* ctx, int n_clips, int T, int face) {
    if (!ctx) return 0;
    size_t bytes = 0;
    return window_plan(ctx, n_clips, T, face, &bytes) ? 0 : bytes;
}

extern "C" int cp360_clstm_window(cp360_ctx* ctx, const float* cam, size_t clip_stride, int n_clips, int T, int face, void* xh,
                                  float* cell0, float* cell1, float* h_out, float* h_all, float* minmax, float* mm_scratch,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    if (!ctx || !cam || !xh || !cell0 || !cell1 || !h_out || !minmax || !mm_scratch || !workspace) return CP360_ERR_NULL;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return CP360_ERR_HIP;
    CClstm& Cl = ctx->cl;
    size_t ws_bytes = 0;
    int rc = window_plan(ctx, n_clips, T, face, &ws_bytes);
    if (rc) return rc;
    if (((size_t)workspace & 255) != 0) return CP360_ERR_ALIGN;
    if (workspace_bytes < ws_bytes) return CP360_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int P = 6 * face * face, C = Cl.cin, H = Cl.ch;
    const size_t M = (size_t)n_clips * P;
    const size_t per_clip = (size_t)T * P * C, stride = clip_stride ? clip_stride : per_clip;
    // test_temporal.py:66-67: min / max over the whole window;  :70-73: hidden = cell = normalised frame 0
    if ((rc = cp360_window_minmax(cam, minmax, mm_scratch, n_clips, per_clip, stride, st))) return rc;
    if ((rc = cp360_window_normalize(cam, minmax, xh, Cl.dtype, C + H, C, cell0, n_clips, T, 0, P, C, stride, st))) return rc;
    // frame 0 is fed again first (:76-79)
    if ((rc = cp360_window_normalize(cam, minmax, xh, Cl.dtype, C + H, 0, nullptr, n_clips, T, 0, P, C, stride, st))) return rc;
    float* c[2] = {cell0, cell1};
    for (int t = 0; t < T; ++t) {
        float* hf = h_all ? h_all + (size_t)t * M * H : (t == T - 1 ? h_out : nullptr);
        const float* xnext = t + 1 < T ? cam + (size_t)(t + 1) * P * C : nullptr;   // frame t+1's normalisation rides on the gates
        if ((rc = cp360_clstm_step(ctx, xh, c[t & 1], c[(t + 1) & 1], hf, n_clips, face, xnext, minmax, stride, workspace, ws_bytes, st)))
            return rc;
    }
    if (h_all && hipMemcpyAsync(h_out, h_all + (size_t)(T - 1) * M * H, M * H * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
        return CP360_ERR_HIP;
    return CP360_OK;
}

// ---------------------------------------------------------------- the windows of several batches in one run
// The cell updates run ONCE at n_groups * n_clips clips: a Winograd GEMM launch then has n_groups tile blocks per (position,
// channel tile) and reads that pair's filters from HBM once for all of them (csrc/wino.hip) instead of once per batch.
namespace {
struct MultiWs {
    size_t xh = 0, cell = 0, h = 0, scratch = 0, step = 0;
    size_t total() const { return xh + 2 * cell + h + scratch + step; }
};

int multi_plan(cp360_ctx* ctx, int n_groups, int n_clips, int T, int face, ClstmPlan* plan, MultiWs* ws) {
    CClstm& Cl = ctx->cl;
    if (!Cl.loaded) return CP360_ERR_NULL;
    if (n_groups <= 0 || n_groups > CP360_MAX_CLIP_GROUPS || n_clips <= 0 || T <= 0 || face <= 0 || Cl.cin != Cl.ch) return CP360_ERR_BAD_SHAPE;
    if ((long long)n_groups * n_clips > 65535) return CP360_ERR_BAD_SHAPE;
    const int rc = plan_clstm(Cl, n_groups * n_clips, face, plan);
    if (rc) return rc;
    const size_t M = (size_t)plan->M;
    ws->xh = align_up(M * (Cl.cin + Cl.ch) * es_of(Cl.dtype));
    ws->cell = ws->h = align_up(M * Cl.ch * sizeof(float));
    ws->scratch = align_up((size_t)n_groups * n_clips * 512 * sizeof(float));
    ws->step = plan->ws.total();
    return CP360_OK;
}
}  // namespace

extern "C" size_t cp360_clstm_window_multi_workspace_bytes(cp360_ctx* ctx, int n_groups, int n_clips, int T, int face) {
    if (!ctx) return 0;
    ClstmPlan plan;
    MultiWs ws;
    return multi_plan(ctx, n_groups, n_clips, T, face, &plan, &ws) ? 0 : ws.total();
}

extern "C" int cp360_clstm_window_multi(cp360_ctx* ctx, const float* const* cams, size_t clip_stride, int n_groups, int n_clips,
                                        int T, int face, float* const* h_out, float* const* h_all, float* minmax, void* workspace,
                                        size_t workspace_bytes, void* stream) {
    if (!ctx || !cams || !h_out || !minmax || !workspace) return CP360_ERR_NULL;
    DeviceGuard guard(ctx->device);
    if (!guard.ok) return CP360_ERR_HIP;
    CClstm& Cl = ctx->cl;
    ClstmPlan plan;
    MultiWs mw;
    int rc = multi_plan(ctx, n_groups, n_clips, T, face, &plan, &mw);
    if (rc) return rc;
    for (int g = 0; g < n_groups; ++g)
        if (!cams[g] || !h_out[g] || (h_all && !h_all[g])) return CP360_ERR_NULL;
    if (((size_t)workspace & 255) != 0) return CP360_ERR_ALIGN;
    if (workspace_bytes < mw.total()) return CP360_ERR_BAD_SHAPE;
    hipStream_t st = (hipStream_t)stream;
    const int P = 6 * face * face, C = Cl.cin, H = Cl.ch;
    const size_t Mg = (size_t)n_clips * P;                                 // pixels of one group
    const size_t per_clip = (size_t)T * P * C, stride = clip_stride ? clip_stride : per_clip;
    unsigned char* w = (unsigned char*)workspace;
    unsigned char* xh = w;
    float* c[2] = {(float*)(w + mw.xh), (float*)(w + mw.xh + mw.cell)};
    float* hj = (float*)(w + mw.xh + 2 * mw.cell);                         // the hidden state of all groups after a step
    float* scratch = (float*)(w + mw.xh + 2 * mw.cell + mw.h);
    unsigned char* step_ws = w + mw.xh + 2 * mw.cell + mw.h + mw.scratch;
    // per group what cp360_clstm_window does up front, on that group's rows of the joint buffers
    for (int g = 0; g < n_groups; ++g) {
        float* mm = minmax + (size_t)g * n_clips * 2;
        unsigned char* xg = xh + (size_t)g * Mg * (C + H) * es_of(Cl.dtype);
        if ((rc = cp360_window_minmax(cams[g], mm, scratch + (size_t)g * n_clips * 512, n_clips, per_clip, stride, st))) return rc;
        if ((rc = cp360_window_normalize(cams[g], mm, xg, Cl.dtype, C + H, C, c[0] + (size_t)g * Mg * H, n_clips, T, 0, P, C, stride, st))) return rc;
        if ((rc = cp360_window_normalize(cams[g], mm, xg, Cl.dtype, C + H, 0, nullptr, n_clips, T, 0, P, C, stride, st))) return rc;
    }
    const float* xn[CP360_MAX_CLIP_GROUPS];
    for (int t = 0; t < T; ++t) {
        const bool keep = h_all || t == T - 1;
        for (int g = 0; g < n_groups; ++g) xn[g] = cams[g] + (size_t)(t + 1) * P * C;   // frame t+1's normalisation rides on the gates
        const CellIo cell{xh, c[t & 1], c[(t + 1) & 1], keep ? hj : nullptr, t + 1 < T ? xn : nullptr, n_groups, n_clips, minmax, stride};
        if ((rc = run_clstm(plan, Cl, cell, step_ws, st))) return rc;
        for (int g = 0; keep && g < n_groups; ++g) {
            const float* src = hj + (size_t)g * Mg * H;
            if (h_all && hipMemcpyAsync(h_all[g] + (size_t)t * Mg * H, src, Mg * H * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
                return CP360_ERR_HIP;
            if (t == T - 1 && hipMemcpyAsync(h_out[g], src, Mg * H * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
                return CP360_ERR_HIP;
        }
    }
    return CP360_OK;
}
