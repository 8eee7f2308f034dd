"""Functional layer over the C ABI (include/cp360.h).  Tensors named *_nhwc are plain
contiguous torch tensors of shape [N, H, W, C] - the layout the fused pipeline keeps in
HBM.  torch is used for allocation and stream ownership only; all arithmetic happens in
libcp360.so.  Every function here fails (RuntimeError / ImportError) without a GPU or
without the built library - there is no CPU fallback.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, check, dtype_code, lib, ptr, require_gpu, stream

IMAGENET_MEAN = (0.485, 0.456, 0.406)      # dataset_feat_extractor.py:150-151
IMAGENET_STD = (0.229, 0.224, 0.225)


# ----------------------------------------------------------------------------- CubePad
def pads_of(lrtd_pad):
    """model/cube_pad.py:12-20,60-70: an int pads all four sides, else [l, r, t, d]."""
    if isinstance(lrtd_pad, (int, np.integer)):
        return (int(lrtd_pad),) * 4
    p_l, p_r, p_t, p_d = lrtd_pad
    return int(p_l), int(p_r), int(p_t), int(p_d)


def cubepad_table(n, lrtd_pad):
    """Host int32 [6, Hp, Wp] source-index table of the kernels (no GPU needed)."""
    pl, pr, pt, pd = pads_of(lrtd_pad)
    tab = np.empty((6, n + pt + pd, n + pl + pr), dtype=np.int32)
    check(lib().cp360_cubepad_table_host(n, pl, pr, pt, pd, tab.ctypes.data_as(C.c_void_p)))
    return tab


def cubepad_nchw(x, lrtd_pad):
    """x [6N, C, n, n] contiguous -> [6N, C, n+pt+pd, n+pl+pr] (cube_pad.py:28-42)."""
    require_gpu(x)
    if x.dim() != 4:
        raise ValueError("CubePad expects a 4-D tensor")
    if x.shape[2] != x.shape[3]:
        raise ValueError("CubePad needs square faces (cube_pad.py transposes strips)")
    pl, pr, pt, pd = pads_of(lrtd_pad)
    x = x.contiguous()
    n6, Cc, n, _ = x.shape
    y = torch.empty((n6, Cc, n + pt + pd, n + pl + pr), dtype=x.dtype, device=x.device)
    check(lib().cp360_cubepad_nchw(ptr(x), ptr(y), n6, Cc, n, pl, pr, pt, pd, x.element_size(), stream()))
    return y


def cubepad_nhwc(x, lrtd_pad, c_out=None):
    """x [6N, n, n, C] -> [6N, n+pt+pd, n+pl+pr, c_out or C] (extra channels zero)."""
    require_gpu(x)
    pl, pr, pt, pd = pads_of(lrtd_pad)
    n6, n, n2, Cc = x.shape
    if n != n2:
        raise ValueError("CubePad needs square faces")
    cy = Cc if c_out is None else int(c_out)
    y = torch.empty((n6, n + pt + pd, n + pl + pr, cy), dtype=x.dtype, device=x.device)
    check(lib().cp360_cubepad_nhwc(ptr(x), ptr(y), n6, Cc, cy, n, pl, pr, pt, pd, x.element_size(), stream()))
    return y


# ----------------------------------------------------------------------------- layout
def nchw_to_nhwc(x, out_dtype=None, out=None, coff=0):
    """[N, C, H, W] contiguous -> [N, H, W, C] (or channels [coff, coff+C) of ``out``)."""
    require_gpu(x, out)
    x = x.contiguous()
    N, Cc, H, W = x.shape
    if out is None:
        out = torch.empty((N, H, W, Cc), dtype=out_dtype or x.dtype, device=x.device)
    ld = out.shape[3]
    check(lib().cp360_nchw_to_nhwc(ptr(x), ptr(out), N, Cc, H, W, dtype_code(x.dtype), dtype_code(out.dtype),
                                   ld, coff, stream()))
    return out


def nhwc_to_nchw(x, out_dtype=None, channels=None, coff=0):
    """[N, H, W, ld] (channels [coff, coff+channels)) -> [N, channels, H, W]."""
    require_gpu(x)
    N, H, W, ld = x.shape
    Cc = ld if channels is None else channels
    y = torch.empty((N, Cc, H, W), dtype=out_dtype or x.dtype, device=x.device)
    check(lib().cp360_nhwc_to_nchw(ptr(x), ptr(y), N, Cc, H, W, dtype_code(x.dtype), dtype_code(y.dtype),
                                   ld, coff, stream()))
    return y


def as_nhwc(x, dtype=None):
    """Accept the reference's [N, C, H, W] tensor in either memory format and return
    an [N, H, W, C] contiguous tensor of ``dtype`` (zero-copy when already so)."""
    require_gpu(x)
    v = x.permute(0, 2, 3, 1)
    if v.is_contiguous() and (dtype is None or dtype == x.dtype):
        return v
    if v.is_contiguous():
        x = x.contiguous()        # rare: physical NHWC but a dtype change is wanted
    return nchw_to_nhwc(x.contiguous(), out_dtype=dtype or x.dtype)


def nchw_view(x_nhwc):
    """Logical [N, C, H, W] view (torch channels_last strides) of an NHWC tensor."""
    return x_nhwc.permute(0, 3, 1, 2)


# ----------------------------------------------------------------------------- K1 / K6
def equi2cube(frames, grid, cube_dim, out_dtype=torch.float32, layout='nhwc4', scale=None,
              mean=IMAGENET_MEAN, std=IMAGENET_STD, cv_fixed_point=True):
    """frames [F, H, W, 3] u8 / f32 (device), grid [6, cd, cd, 2] f32 (device).
    Returns [6F, 3, cd, cd] (layout 'nchw') or [6F, cd, cd, 4] (layout 'nhwc4').  ``grid`` may be any
    [6, n, n, 2] table of sampling points with n = cube_dim: passing the CubePad(3)-gathered grid
    ([6, cd+6, cd+6, 2], ``Equi2Cube.grid_p3``) with cube_dim = cd+6 yields the padded faces directly."""
    require_gpu(frames, grid)
    F, H, W, three = frames.shape
    if three != 3:
        raise ValueError("frames must be [F, H, W, 3]")
    frames = frames.contiguous()
    if scale is None:
        scale = 1.0 / 255.0 if frames.dtype == torch.uint8 else 1.0
    code = {'nchw': 0, 'nhwc4': 1}[layout]
    shape = (6 * F, 3, cube_dim, cube_dim) if code == 0 else (6 * F, cube_dim, cube_dim, 4)
    out = torch.empty(shape, dtype=out_dtype, device=frames.device)
    m = (C.c_float * 3)(*[float(v) for v in mean])
    s = (C.c_float * 3)(*[float(np.float32(1.0) / np.float32(v)) for v in std])
    check(lib().cp360_equi2cube(ptr(frames), ptr(grid), ptr(out), F, H, W, cube_dim, m, s, float(scale),
                                dtype_code(frames.dtype), dtype_code(out_dtype), code,
                                1 if cv_fixed_point else 0, stream()))
    return out


def cube2equi(x, face_map, coord, layout='nchw', want_full=True, want_max=False):
    """x f32 [6B, C, w, w] ('nchw') or [6B, w, w, C] ('nhwc'); face_map int8 [2w,4w];
    coord f32 [2w,4w,2] pixel-space sampling positions.  Returns (full, max)."""
    require_gpu(x, face_map, coord)
    # the C ABI reads raw pointers as f32 / int8 / f32: anything else would be silently reinterpreted
    if x.dtype != torch.float32:
        raise ValueError("cube2equi samples f32 features (got %s): pass the f32 hidden state" % x.dtype)
    if face_map.dtype != torch.int8 or coord.dtype != torch.float32:
        raise ValueError("face_map must be int8 and coord f32 (got %s, %s)" % (face_map.dtype, coord.dtype))
    x = x.contiguous()
    face_map, coord = face_map.contiguous(), coord.contiguous()
    if layout == 'nchw':
        n6, Cc, w, _ = x.shape
    else:
        n6, w, _, Cc = x.shape
    if n6 % 6:
        raise ValueError("batch must be a multiple of 6 faces")
    B = n6 // 6
    full = torch.empty((B, Cc, 2 * w, 4 * w), dtype=torch.float32, device=x.device) if want_full else None
    mx = torch.empty((B, 2 * w, 4 * w), dtype=torch.float32, device=x.device) if want_max else None
    check(lib().cp360_cube2equi(ptr(x), ptr(face_map), ptr(coord), ptr(full), ptr(mx), B, Cc, w,
                                0 if layout == 'nchw' else 1, stream()))
    return full, mx


# ----------------------------------------------------------------------------- convolution
def _check_buf(name, t, dtype, min_shape=None, numel=None):
    """A caller-provided destination / operand handed to the library as a raw pointer: wrong dtype,
    strides or size would be an out-of-bounds device access, so fail in Python first."""
    if t is None:
        return
    if t.dtype != dtype:
        raise ValueError("%s must be %s, got %s" % (name, dtype, t.dtype))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % name)
    if min_shape is not None:
        if t.dim() != len(min_shape) or any(a != b for a, b in zip(t.shape[:-1], min_shape[:-1])) \
                or t.shape[-1] < min_shape[-1]:
            raise ValueError("%s has shape %s, needs %s (last dimension at least)" % (name, tuple(t.shape), tuple(min_shape)))
    if numel is not None and t.numel() < numel:
        raise ValueError("%s holds %d elements, needs %d" % (name, t.numel(), numel))


def _shares_bytes(a, b):
    """Whether the storage byte ranges data_ptr() .. + numel * element_size of two contiguous tensors intersect: a destination
    that starts elsewhere in its operand's buffer (two overlapping views) is an alias that comparing data_ptr() misses."""
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + b.numel() * b.element_size() and b0 < a0 + a.numel() * a.element_size()


def _out_for(out, shape, dtype, device, src, same_ok=False):
    """The destination of a kernel that reads `src`: a new tensor, or the caller's `out` when it has this shape and dtype on this
    device and shares no byte with src (same_ok: or is src itself, for an element-wise kernel)."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if out.shape != shape or out.device != device:                     # torch.Size is a tuple
        raise ValueError("out must be another tensor of shape %s on the frames' device" % (tuple(shape),))
    _check_buf('out', out, dtype)
    if _shares_bytes(out, src) and not (same_ok and out.data_ptr() == src.data_ptr()):
        raise ValueError("out must be frames themselves or share no memory with them (pixels are copied in no order across frames)"
                         if same_ok else "out must not share memory with frames (a gather: not in place)")
    return out


def _frames_nhwc(frames, u8_only, n='N'):
    """The frame checks of K11c, K12a, K12b and K13 -> (N, H, W, C): a non-empty contiguous [N, H, W, C], uint8 with 3 channels
    or (unless u8_only) float32 with at most 4."""
    if u8_only:
        if frames.dim() != 4 or frames.numel() == 0 or frames.dtype != torch.uint8 or frames.shape[3] != 3:
            raise ValueError("frames must be a non-empty uint8 [%s, H, W, 3], got %s %s" % (n, frames.dtype, tuple(frames.shape)))
    else:
        if frames.dim() != 4 or frames.numel() == 0 or frames.dtype not in (torch.uint8, torch.float32):
            raise ValueError("frames must be a non-empty uint8 [N, H, W, 3] or float32 [N, H, W, C], got %s %s"
                             % (frames.dtype, tuple(frames.shape)))
        if frames.shape[3] > 4 or (frames.dtype == torch.uint8 and frames.shape[3] != 3):
            raise ValueError("frames must have 3 channels (uint8) or at most 4 (float32), got %d" % frames.shape[3])
    _check_buf('frames', frames, frames.dtype)
    return tuple(int(s) for s in frames.shape)


def _map_shape(maps, why=''):
    """The map checks of K12c, K12d, K16c, K20a and K22d -> (F, hm, wm): a non-empty contiguous float32 [F, hm, wm] of at most
    16384 pixels."""
    if maps.dim() != 3 or maps.numel() == 0:
        raise ValueError("maps must be a non-empty float32 [F, hm, wm], got %s" % (tuple(maps.shape),))
    _check_buf('maps', maps, torch.float32)
    F, hm, wm = (int(s) for s in maps.shape)
    if hm * wm > 16384:
        raise ValueError("maps of more than 16384 pixels are not supported%s, got %d x %d" % (why, hm, wm))
    return F, hm, wm


def _render_args(frames, R, h, w, out, *more):
    """What K12a / K21 and K22a check alike (``viewport_render``, ``viewport_render_zoom``): the frames, a camera each and the
    destination of h x w views -> (N, H, W, C, out).  `more`: the call's other tensors, which must be on the GPU too."""
    require_gpu(frames, R, out, *more)
    N, H, W, C_ = _frames_nhwc(frames, u8_only=False)
    _stab_rotations(R, N)
    return N, H, W, C_, _out_for(out, (N, h, w, C_), frames.dtype, frames.device, frames)


def _outline_args(frames, R, rgb, out, work, *more):
    """What K12b and K22b check alike (``viewport_outline``, ``viewport_outline_zoom``): the frames, a camera each, the colour,
    the destination, which may be the frames, and the workspace -> (N, H, W, out, work, the colour as the library takes it)."""
    require_gpu(frames, R, out, *more)
    N, H, W, _ = _frames_nhwc(frames, u8_only=True)
    _stab_rotations(R, N)
    rgb = tuple(int(v) for v in rgb)
    if len(rgb) != 3 or min(rgb) < 0 or max(rgb) > 255:
        raise ValueError("rgb must be three values of 0 .. 255, got %r" % (rgb,))
    out = _out_for(out, (N, H, W, 3), torch.uint8, frames.device, frames, same_ok=True)
    return N, H, W, out, _stab_work(0, H, W, frames.device, work), C.cast((C.c_ubyte * 3)(*rgb), C.c_void_p)


def _work(bytes_fn, what, F, h, w, device, work, limits=''):
    """The workspace of one call of the library, bytes_fn(F, h, w) bytes: `work` when it is a contiguous float64 tensor on
    `device` that holds as many, else a new one.  The callers hand the library work.numel() * 8 as the byte count, so a tensor
    of another element size must not pass."""
    nbytes = bytes_fn(int(F), int(h), int(w))
    if nbytes == 0:
        raise ValueError("%s: unsupported geometry: %d x %d x %d%s" % (what, F, h, w, limits))
    if work is None or work.device != device or work.dtype != torch.float64 or not work.is_contiguous() \
            or work.numel() * 8 < nbytes:
        work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
    return work


# Optional launch timer (bench.py installs one): an object with
# ``wrap(tag, flops, fn)`` that brackets the conv_forward launch with HIP events on the
# current stream.  None = no instrumentation (default).
LAUNCH_TIMER = None


class Conv:
    """One convolution of the path with its packed weights resident on the device.

    weight: f32 [c_out, c_in, kh, kw] (torch, any device); ``scale`` / ``bias``: per
    output channel f32 (BatchNorm folding happens in the pack kernel: w * scale[n]).
    pad > 0 means "preceded by CubePad(pad)" (fused into the tile loader).
    """

    def __init__(self, weight, scale=None, bias=None, stride=1, pad=0, relu=False, dtype=torch.float32,
                 device='cuda', stem=False, clip_resident=None, second=None):
        self.dtype = dtype
        self.device = torch.device(device)
        self.stride = int(stride)
        self.pad = int(pad)
        self.relu = bool(relu)
        self.stem = bool(stem)
        self.tag = 'conv'
        self._w_src = weight.detach()          # packed lazily per layout (no copy kept: the module owns it)
        self.c_out, self.c_in_w, self.kh_w, self.kw_w = weight.shape
        if stem:
            assert (self.c_in_w, self.kh_w, self.kw_w) == (3, 7, 7)
            self.c_in, self.kh, self.kw, self.pix_stride = 32, 7, 1, 4
        else:
            self.c_in, self.kh, self.kw, self.pix_stride = self.c_in_w, self.kh_w, self.kw_w, self.c_in_w
        self.bias = None if bias is None else bias.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self._scale = None if scale is None else scale.detach().to(device=self.device, dtype=torch.float32).contiguous()
        # cp360_conv_desc.clip_resident: CubePad(1) + 3x3 stride 1 with c_out >= 256 may run on the
        # clip-resident kernel when the faces turn out to be <= 7x7 at call time (ConvLSTM at cube 224,
        # layer4 conv2); it reads a channel-major packing, made on first use
        if clip_resident is None:
            clip_resident = (not stem and self.pad == 1 and self.stride == 1 and self.kh == 3 and self.kw == 3
                             and self.c_out >= 256)
        self.clip_resident_ok = bool(clip_resident)
        self.clip_only = False                  # True: never ask cp360_conv_prefer_clip (only the channel-major packing exists)
        # second source (cp360_conv_desc.c_in2): (weight2 [c_out, c_in2, 1, 1], scale2, bias2, stride2) - a 1x1
        # convolution of a SECOND tensor accumulated into the same tile (the Bottleneck's downsample branch
        # inside conv3); its bias is folded into this conv's bias
        self.second = None
        if second is not None:
            w2, s2, b2, st2 = second
            if stem or self.c_out < 256 or w2.shape[0] != self.c_out or tuple(w2.shape[2:]) != (1, 1):
                raise ValueError("a second source needs c_out >= 256 and a [c_out, c_in2, 1, 1] filter")
            self.second = (w2.detach(), None if s2 is None else s2.detach().to(device=self.device, dtype=torch.float32).contiguous(),
                           int(st2))
            self.c_in2 = int(w2.shape[1])
            if b2 is not None:
                b2 = b2.detach().to(device=self.device, dtype=torch.float32)
                self.bias = b2.contiguous() if self.bias is None else (self.bias + b2).contiguous()
            clip_resident = False
            self.clip_resident_ok = False
        self._packed = {}
        self._stem_packed = None                # resident-patch stem kernel (16-bit types, cube 224), on first use
        self._band_packed = None                # resident-band 3x3 kernel (64 -> 64 on 56x56 faces), on first use
        self._partial = None
        self._splits_cache = {}

    def packed_for(self, clip_resident):
        """Packed weights in the layout of cp360_conv_desc.clip_resident (0 / 1), built on first use."""
        t = self._packed.get(clip_resident)
        if t is None:
            d = self._desc(6, 7, 7, 1, clip_resident=clip_resident) if clip_resident else \
                self._desc(6, max(self.kh, 8), max(self.kw, 8) if not self.stem else 16, 1)
            nbytes = lib().cp360_conv_packed_bytes(C.byref(d))
            if nbytes == 0:
                raise ValueError("unsupported convolution geometry for libcp360")
            w = self._w_src.to(device=self.device, dtype=torch.float32).contiguous()
            t = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            if self.second is not None:
                w2 = self.second[0].to(device=self.device, dtype=torch.float32).reshape(self.c_out, self.c_in2).contiguous()
                check(lib().cp360_conv_pack_weights2(C.byref(d), ptr(w), ptr(self._scale), ptr(w2), ptr(self.second[1]),
                                                     ptr(t), stream()))
            else:
                check(lib().cp360_conv_pack_weights(C.byref(d), ptr(w), ptr(self._scale), ptr(t), 1 if self.stem else 0,
                                                    stream()))
            self._packed[clip_resident] = t
        return t

    @property
    def packed(self):
        return self.packed_for(0)               # the tap-major packing every kernel but the clip-resident one reads

    def out_hw(self, h_in, w_in):
        p2 = 2 * self.pad
        return (h_in + p2 - self.kh) // self.stride + 1, \
               ((w_in + p2 - self.kw_w) // self.stride + 1 if self.stem else (w_in + p2 - self.kw) // self.stride + 1)

    def _desc(self, n_img, h_in, w_in, splits, ld_out=None, out_coff=0, ld_res=0, relu=None, tile_px=0,
              clip_resident=0, slab_rows=0, x2_shape=None):
        d = ConvDesc()
        d.dtype = dtype_code(self.dtype)
        d.n_img, d.h_in, d.w_in = n_img, h_in, w_in
        d.c_in, d.pix_stride = self.c_in, self.pix_stride
        d.kh, d.kw, d.sy, d.sx = self.kh, self.kw, self.stride, self.stride
        d.h_out, d.w_out = self.out_hw(h_in, w_in)
        d.c_out = self.c_out
        d.pad_mode, d.pad = (1 if self.pad > 0 else 0), self.pad
        d.ld_out = self.c_out if ld_out is None else ld_out
        d.out_coff, d.ld_res = out_coff, ld_res
        d.relu = int(self.relu if relu is None else relu)
        d.splits = splits
        d.tile_px = tile_px
        d.clip_resident = clip_resident
        d.slab_rows = slab_rows
        if self.second is not None:
            st2 = self.second[2]
            d.c_in2 = self.c_in2
            d.sy2 = d.sx2 = st2
            if x2_shape is None:                     # packing: any consistent geometry (the layout does not depend on it)
                d.h_in2, d.w_in2, d.pix_stride2 = (d.h_out - 1) * st2 + 1, (d.w_out - 1) * st2 + 1, self.c_in2
            else:
                d.h_in2, d.w_in2, d.pix_stride2 = x2_shape[1], x2_shape[2], x2_shape[3]
        return d

    def _stem_resident(self, xp):
        """cp360_stem_forward: the padded faces' rows of an 8-row output band stay in LDS (K3a)."""
        L = lib()
        code = dtype_code(self.dtype)
        if self._stem_packed is None:
            w = self._w_src.to(device=self.device, dtype=torch.float32).contiguous()
            t = torch.empty(L.cp360_stem_packed_bytes(code), dtype=torch.uint8, device=self.device)
            check(L.cp360_stem_pack_weights(code, ptr(w), ptr(self._scale), ptr(t), stream()))
            self._stem_packed = t
        n_img, cd = xp.shape[0], xp.shape[1] - 6
        out = torch.empty((n_img, cd // 2, cd // 2, 64), dtype=self.dtype, device=xp.device)
        check(L.cp360_stem_forward(code, ptr(xp.contiguous()), ptr(self._stem_packed), ptr(self.bias), ptr(out), n_img,
                                   cd, int(self.relu), stream()))
        return out

    def stem_pool(self, xp):
        """cp360_stem_pool_forward: stem + CubePad(1) + max-pool 3x3 s2 in one kernel (cube 224, 16-bit types, ReLU):
        xp [n_img, 230, 230, 4] -> [n_img, 56, 56, 64]; None when this convolution / input is not that case."""
        if not (self.stem and self.relu and self.dtype in (torch.bfloat16, torch.float16) and xp.dtype == self.dtype
                and tuple(xp.shape[1:]) == (230, 230, 4) and xp.shape[0] % 6 == 0):
            return None
        require_gpu(xp)
        L = lib()
        code = dtype_code(self.dtype)
        if self._stem_packed is None:
            w = self._w_src.to(device=self.device, dtype=torch.float32).contiguous()
            t = torch.empty(L.cp360_stem_packed_bytes(code), dtype=torch.uint8, device=self.device)
            check(L.cp360_stem_pack_weights(code, ptr(w), ptr(self._scale), ptr(t), stream()))
            self._stem_packed = t
        n_img = xp.shape[0]
        y = torch.empty((n_img, 56, 56, 64), dtype=self.dtype, device=xp.device)
        border = torch.empty(L.cp360_stem_pool_border_bytes(n_img), dtype=torch.uint8, device=xp.device)
        check(L.cp360_stem_pool_forward(code, ptr(xp.contiguous()), ptr(self._stem_packed), ptr(self.bias), ptr(y),
                                        ptr(border), n_img, 224, stream()))
        return y

    def _band_resident(self, x):
        """cp360_band3x3_forward: layer1 conv2 with the band's padded pixels resident in LDS (K3c)."""
        L = lib()
        code = dtype_code(self.dtype)
        if self._band_packed is None:
            w = self._w_src.to(device=self.device, dtype=torch.float32).contiguous()
            t = torch.empty(L.cp360_band3x3_packed_bytes(code), dtype=torch.uint8, device=self.device)
            check(L.cp360_band3x3_pack_weights(code, ptr(w), ptr(self._scale), ptr(t), stream()))
            self._band_packed = t
        out = torch.empty_like(x)
        check(L.cp360_band3x3_forward(code, ptr(x.contiguous()), ptr(self._band_packed), ptr(self.bias), ptr(out),
                                      x.shape[0], 56, 64, int(self.relu), stream()))
        return out

    def nsteps(self):
        bk = 32 if self.dtype == torch.float32 else 64
        return self.kh * self.kw * ((self.c_in + bk - 1) // bk)

    def raw_sum_f32(self, x, out=None):
        """The convolution's raw f32 sums [n_img, h_out, w_out, c_out] (no bias / activation, true channel order) - how the
        CAM scores leave (class_activation_model.py:77-83).  The library's planner may split K (one frame = 6 faces gives a
        CAM GEMM of M = 294 rows: 80 small tiles for 256 CUs); the slabs are then reduced by cp360_conv_finish with an f32
        descriptor.  ``out``: f32 buffer of >= M * c_out elements (flat), else a fresh tensor."""
        n_img, h_in, w_in, _ = x.shape
        h_out, w_out = self.out_hw(h_in, w_in)
        M = n_img * h_out * w_out
        key = (n_img, h_in, w_in, 0)
        splits = self._splits_cache.get(key)
        if splits is None:
            splits = lib().cp360_conv_suggest_splits(C.byref(self._desc(n_img, h_in, w_in, 1)))
            self._splits_cache[key] = splits
        if splits == 1:
            part, _ = self(x, raw_f32=True, splits=1, partial_buf=out, clip_resident=False)
            return part[: M * self.c_out].view(n_img, h_out, w_out, self.c_out)
        part, _ = self(x, raw_f32=True, splits=splits, clip_resident=False)
        if out is None:
            out = torch.empty(M * self.c_out, dtype=torch.float32, device=x.device)
        else:
            require_gpu(out)
            _check_buf('out', out, torch.float32, numel=M * self.c_out)
        d = self._desc(n_img, h_in, w_in, splits, relu=False)
        d.dtype = dtype_code(torch.float32)                     # the finish writes f32 whatever the convolution's type
        check(lib().cp360_conv_finish(C.byref(d), ptr(part), None, None, ptr(out), stream()))
        return out.view(-1)[: M * self.c_out].view(n_img, h_out, w_out, self.c_out)

    def __call__(self, x, residual=None, out=None, out_coff=0, raw_f32=False, splits=None, partial_buf=None,
                 tile_px=0, clip_resident=None, slab_rows=False, x2=None):
        """x [n_img, h, w, c] NHWC (for the stem: the materialised CubePad(3) output
        [n_img, h+6, w+6, 4]).  Returns [n_img, h_out, w_out, c_out] in self.dtype, or
        with raw_f32=True the (partial [splits, M, c_out] f32, splits) pair whose
        reduction / bias / activation the caller finishes (cp360_lstm_gates, CAM)."""
        require_gpu(x, residual, out, x2)
        n_img, h_in, w_in, cx = x.shape
        if (x2 is not None) != (self.second is not None):
            raise ValueError("x2 goes with a conv built with second=...")
        if (self.stem and h_in == w_in and h_in in (230, 518) and cx == 4 and residual is None and out is None and not raw_f32
                and splits is None and tile_px == 0 and self.dtype in (torch.bfloat16, torch.float16)
                and x.dtype == self.dtype):
            return self._stem_resident(x)
        if (not self.stem and self.c_in == 64 and self.c_out == 64 and self.kh == 3 and self.kw == 3 and self.pad == 1
                and self.stride == 1 and h_in == 56 and w_in == 56 and n_img % 6 == 0 and residual is None and out is None
                and not raw_f32 and splits is None and tile_px == 0 and self.dtype in (torch.bfloat16, torch.float16)
                and x.dtype == self.dtype):
            return self._band_resident(x)
        if x.dtype != self.dtype:
            raise ValueError("activation dtype %s != conv dtype %s" % (x.dtype, self.dtype))
        if not self.stem and cx != self.c_in:
            raise ValueError("input has %d channels, conv expects %d" % (cx, self.c_in))
        if self.stem and cx != 4:
            raise ValueError("stem expects an NHWC4 input")
        h_out, w_out = self.out_hw(h_in, w_in)
        M = n_img * h_out * w_out
        x = x.contiguous()
        x2s = None
        if x2 is not None:
            st2 = self.second[2]
            if x2.dtype != self.dtype or not x2.is_contiguous() or x2.dim() != 4 or x2.shape[0] != n_img \
                    or x2.shape[3] < self.c_in2 or (h_out - 1) * st2 >= x2.shape[1] or (w_out - 1) * st2 >= x2.shape[2]:
                raise ValueError("x2 must be a contiguous %s [n_img, >=%d, >=%d, >=%d] tensor"
                                 % (self.dtype, (h_out - 1) * st2 + 1, (w_out - 1) * st2 + 1, self.c_in2))
            x2s = tuple(x2.shape)
        _check_buf('out', out, self.dtype, (n_img, h_out, w_out, self.c_out + out_coff))
        _check_buf('residual', residual, self.dtype, (n_img, h_out, w_out, self.c_out))
        ld_out = self.c_out if out is None else out.shape[3]
        ld_res = 0 if residual is None else residual.shape[3]
        L = lib()
        # clip-resident kernel: whole cubes of <= 304 pixels (faces <= 7x7), half a cube of 8x8 faces, or one 16x16 face + ring per tile
        cr = self.clip_resident_ok if clip_resident is None else bool(clip_resident)
        cr = int(cr and h_in == w_in and (6 * h_in * w_in <= 304 or h_in in (8, 16)) and n_img % 6 == 0 and tile_px == 0)
        if clip_resident and not cr:
            raise ValueError("clip_resident needs CubePad(1)+3x3 stride 1 on faces of at most 7x7, 8x8 or 16x16")
        if cr and clip_resident is None and not self.clip_only:
            # both layouts can be packed: few cubes x few channels (layer4's conv2 of one frame) run better on the small
            # tap-major tiles (cp360_conv_prefer_clip; same rule in csrc/ctx.hip)
            key = ('clip', n_img, h_in, w_in)
            pref = self._splits_cache.get(key)
            if pref is None:
                pref = L.cp360_conv_prefer_clip(C.byref(self._desc(n_img, h_in, w_in, 1, clip_resident=1)))
                self._splits_cache[key] = pref
            cr = int(bool(pref))
        if splits is None:
            key = (n_img, h_in, w_in, cr)
            splits = self._splits_cache.get(key)
            if splits is None:
                splits = L.cp360_conv_suggest_splits(C.byref(self._desc(n_img, h_in, w_in, 1, clip_resident=cr, x2_shape=x2s)))
                self._splits_cache[key] = splits
        # split-K slabs read back by cp360_conv_finish (or, on request, by cp360_lstm_gates) keep the packed
        # row order: contiguous 64-byte stores (cp360_conv_desc.slab_rows)
        sr = int(self.c_out % 32 == 0 and ((splits > 1 and not raw_f32) or (raw_f32 and slab_rows)))
        if raw_f32 and slab_rows and not sr:
            raise ValueError("slab_rows needs c_out % 32 == 0")
        d = self._desc(n_img, h_in, w_in, splits, ld_out, out_coff, ld_res, tile_px=tile_px, clip_resident=cr,
                       slab_rows=sr, x2_shape=x2s)
        packed = self.packed_for(cr)
        def forward(*a):
            if x2 is not None:                       # (desc, in, in2, packed, ...)
                return L.cp360_conv_forward2(a[0], a[1], ptr(x2), *a[2:])
            if LAUNCH_TIMER is None:
                return L.cp360_conv_forward(*a)
            flops = 2.0 * M * self.c_out * self.c_in_w * self.kh_w * self.kw_w
            return LAUNCH_TIMER.wrap(self.tag, flops, lambda: L.cp360_conv_forward(*a))

        if raw_f32 or splits > 1:
            need = splits * M * self.c_out
            if partial_buf is not None:          # caller-owned destination for the raw sums
                require_gpu(partial_buf)
                _check_buf('partial_buf', partial_buf, torch.float32, numel=need)
                check(forward(C.byref(d), ptr(x), ptr(packed), None, None, None,
                                           ptr(partial_buf), stream()))
                return partial_buf, splits
            if self._partial is None or self._partial.numel() < need:
                self._partial = torch.empty(need, dtype=torch.float32, device=x.device)
            check(forward(C.byref(d), ptr(x), ptr(packed), None, None, None,
                                       ptr(self._partial), stream()))
            if raw_f32:
                return self._partial, splits
            if out is None:
                out = torch.empty((n_img, h_out, w_out, self.c_out), dtype=self.dtype, device=x.device)
            check(L.cp360_conv_finish(C.byref(d), ptr(self._partial), ptr(self.bias), ptr(residual), ptr(out),
                                      stream()))
            return out
        if out is None:
            out = torch.empty((n_img, h_out, w_out, self.c_out), dtype=self.dtype, device=x.device)
        check(forward(C.byref(d), ptr(x), ptr(packed), ptr(self.bias), ptr(residual), ptr(out),
                                   None, stream()))
        return out


def frag_pack_1x1(weight, scale, dtype, order, device):
    """1x1 filter [n_out, k(, 1, 1)] (f32) times scale[n_out] -> MFMA A fragments (cp360_frag_pack_1x1)."""
    n_out, k = int(weight.shape[0]), int(weight.shape[1])
    code = dtype_code(dtype)
    nbytes = lib().cp360_frag_packed_bytes(code, n_out, k)
    if nbytes == 0:
        raise ValueError("fragment packing needs a 16-bit type and n_out, k multiples of 32")
    w = weight.detach().to(device=device, dtype=torch.float32).reshape(n_out, k).contiguous()
    sc = None if scale is None else scale.detach().to(device=device, dtype=torch.float32).contiguous()
    t = torch.empty(nbytes, dtype=torch.uint8, device=device)
    check(lib().cp360_frag_pack_1x1(code, ptr(w), ptr(sc), ptr(t), n_out, k, int(order), stream()))
    return t


class L1Block:
    """K3d (csrc/l1block.hip): one layer1 Bottleneck after its conv1 as ONE launch - conv2 + bn2 + relu ->
    conv3 + bn3 + (residual | downsample(x)) + relu -> optionally the next block's conv1 + bn1 + relu.
    16-bit types, 56x56 faces.  Arguments: (weight, bn scale, bn bias) triples of the convolutions."""

    def __init__(self, conv2, conv3, downsample=None, next_conv1=None, dtype=torch.float16, device='cuda', own_conv1=None):
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("L1Block runs in fp16 / bf16")
        self.dtype, self.device = dtype, torch.device(device)
        L, code = lib(), dtype_code(dtype)
        f32 = lambda t: None if t is None else t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        w2, s2, b2 = conv2
        if tuple(w2.shape) != (64, 64, 3, 3) or tuple(conv3[0].shape[:2]) != (256, 64):
            raise ValueError("L1Block is layer1's geometry: conv2 64->64 3x3, conv3 64->256 1x1")
        self.w2 = torch.empty(L.cp360_l1block_conv2_bytes(code), dtype=torch.uint8, device=self.device)
        check(L.cp360_l1block_pack_conv2(code, ptr(f32(w2)), ptr(f32(s2)), ptr(self.w2), stream()))
        self.b2 = f32(b2)
        w3, s3, b3 = conv3
        self.w3 = frag_pack_1x1(w3, s3, dtype, 0, self.device)
        self.b3 = f32(b3)
        self.wd = None
        if downsample is not None:
            wd, sd, bd = downsample
            if tuple(wd.shape[:2]) != (256, 64):
                raise ValueError("layer1's downsample is 64->256, stride 1")
            self.wd = frag_pack_1x1(wd, sd, dtype, 0, self.device)
            self.b3 = (self.b3 + f32(bd)).contiguous()
        # own_conv1 (the first block): the block's OWN conv1 (64 -> 64) for first(): it then runs inside the kernel, on the resident patch
        self.w0 = self.b0 = None
        if own_conv1 is not None:
            w0, s0, b0 = own_conv1
            if tuple(w0.shape[:2]) != (64, 64) or downsample is None:
                raise ValueError("own_conv1 is layer1.0's conv1 (64 -> 64) and goes with the downsample form")
            self.w0 = frag_pack_1x1(w0, s0, dtype, 0, self.device)
            self.b0 = f32(b0)
        self.w1 = self.b1 = None
        self.next_c = 0
        if next_conv1 is not None:
            w1, s1, b1 = next_conv1
            # 256 -> 64: the next layer1 block's conv1; 256 -> 128: layer2.0's conv1 behind the LAST (identity) block
            if tuple(w1.shape[:2]) not in ((64, 256), (128, 256)) or (w1.shape[0] == 128 and downsample is not None):
                raise ValueError("the chained conv1 is 256->64, or 256->128 behind an identity block")
            self.w1 = frag_pack_1x1(w1, s1, dtype, 1, self.device)
            self.b1 = f32(b1)
            self.next_c = int(w1.shape[0])

    def __call__(self, mid, residual=None, x_ds=None):
        """mid [n_img, n, n, 64] with n = 56 (cube 224) or 128 (cube 512); residual [n_img, n, n, 256] (identity blocks)
        or x_ds [n_img, n, n, 64] (the first block).  Returns (out [n_img, n, n, 256], next conv1's output
        [n_img, n, n, 64] or None)."""
        require_gpu(mid, residual, x_ds)
        if (self.wd is None) != (x_ds is None) or (residual is None) == (x_ds is None):
            raise ValueError("identity blocks take residual=, the downsample block takes x_ds=")
        n_img, n = mid.shape[0], mid.shape[1]
        if n not in (56, 128):
            raise ValueError("L1Block handles 56x56 and 128x128 faces")
        _check_buf('mid', mid, self.dtype, (n_img, n, n, 64))
        _check_buf('residual', residual, self.dtype, (n_img, n, n, 256))
        _check_buf('x_ds', x_ds, self.dtype, (n_img, n, n, 64))
        for t in (mid, residual, x_ds):
            if t is not None and t.shape[3] not in (64, 256):
                raise ValueError("dense NHWC tensors only")
        out = torch.empty((n_img, n, n, 256), dtype=self.dtype, device=mid.device)
        nxt = None if self.w1 is None else torch.empty((n_img, n, n, self.next_c), dtype=self.dtype, device=mid.device)
        if self.next_c == 128:
            check(lib().cp360_l1block_forward_wide(dtype_code(self.dtype), ptr(mid), ptr(self.w2), ptr(self.b2), ptr(self.w3),
                                                   ptr(self.b3), ptr(residual), ptr(out), ptr(self.w1), ptr(self.b1),
                                                   ptr(nxt), n_img, n, stream()))
            return out, nxt
        check(lib().cp360_l1block_forward(dtype_code(self.dtype), ptr(mid), ptr(self.w2), ptr(self.b2), ptr(self.w3),
                                          ptr(self.b3), ptr(residual), ptr(x_ds), ptr(self.wd), ptr(out), ptr(self.w1),
                                          ptr(self.b1), ptr(nxt), n_img, n, stream()))
        return out, nxt

    def first(self, x):
        """layer1.0 with its own conv1 inside the kernel (cp360_l1block_forward_first): x [n_img, 56, 56, 64] = the block input (conv1's
        input and the downsample source).  Returns (out, next conv1's output or None); same bits as conv1 as a launch + __call__."""
        require_gpu(x)
        if self.w0 is None or self.wd is None:
            raise ValueError("first() needs own_conv1= and downsample=")
        n_img, n = x.shape[0], x.shape[1]
        if n != 56:
            raise ValueError("the in-kernel conv1 exists for 56x56 faces")
        _check_buf('x', x, self.dtype, (n_img, n, n, 64))
        out = torch.empty((n_img, n, n, 256), dtype=self.dtype, device=x.device)
        nxt = None if self.w1 is None else torch.empty((n_img, n, n, self.next_c), dtype=self.dtype, device=x.device)
        check(lib().cp360_l1block_forward_first(dtype_code(self.dtype), ptr(x), ptr(self.w0), ptr(self.b0), ptr(self.w2), ptr(self.b2),
                                                ptr(self.w3), ptr(self.b3), ptr(self.wd), ptr(out), ptr(self.w1), ptr(self.b1),
                                                ptr(nxt), n_img, n, stream()))
        return out, nxt


class L2Block:
    """K3e (csrc/l2block.hip): the tail of a layer2 identity Bottleneck as ONE launch - conv2 + bn2 + relu ->
    conv3 + bn3 + residual + relu (-> the next identity block's conv1 + bn1 + relu when `next_conv1` is given, 28x28
    faces).  16-bit types, 28x28 / 64x64 faces.  (weight, bn scale, bn bias) triples."""

    def __init__(self, conv2, conv3, dtype=torch.float16, device='cuda', next_conv1=None):
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("L2Block runs in fp16 / bf16")
        self.dtype, self.device = dtype, torch.device(device)
        L, code = lib(), dtype_code(dtype)
        f32 = lambda t: None if t is None else t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        w2, s2, b2 = conv2
        w3, s3, b3 = conv3
        if tuple(w2.shape) != (128, 128, 3, 3) or tuple(w3.shape[:2]) != (512, 128):
            raise ValueError("L2Block is layer2's geometry: conv2 128->128 3x3, conv3 128->512 1x1")
        self.w2 = torch.empty(L.cp360_l2block_packed_bytes(code), dtype=torch.uint8, device=self.device)
        check(L.cp360_l2block_pack_weights(code, ptr(f32(w2)), ptr(f32(s2)), ptr(self.w2), stream()))
        self.b2 = f32(b2)
        self.w3 = frag_pack_1x1(w3, s3, dtype, 0, self.device)
        self.b3 = f32(b3)
        self.w1 = self.b1 = None
        if next_conv1 is not None:
            w1, s1, b1 = next_conv1
            if tuple(w1.shape[:2]) != (128, 512):
                raise ValueError("the chained conv1 is 512->128")
            self.w1 = frag_pack_1x1(w1, s1, dtype, 0, self.device)
            self.b1 = f32(b1)

    def __call__(self, mid, residual, chain=True):
        """mid [n_img, n, n, 128], residual [n_img, n, n, 512] -> out [n_img, n, n, 512]; n = 28 (cube 224) or 64 (cube 512).
        With `next_conv1` (and 28x28 faces, chain=True): returns (out, next conv1's output [n_img, 28, 28, 128])."""
        require_gpu(mid, residual)
        n_img, n = mid.shape[0], mid.shape[1]
        if n not in (28, 64):
            raise ValueError("L2Block handles 28x28 and 64x64 faces")
        _check_buf('mid', mid, self.dtype, (n_img, n, n, 128))
        _check_buf('residual', residual, self.dtype, (n_img, n, n, 512))
        if mid.shape[3] != 128 or residual.shape[3] != 512:
            raise ValueError("dense NHWC tensors only")
        out = torch.empty((n_img, n, n, 512), dtype=self.dtype, device=mid.device)
        if self.w1 is not None and chain:
            if n != 28:
                raise ValueError("the chained conv1 exists for 28x28 faces")
            nxt = torch.empty((n_img, n, n, 128), dtype=self.dtype, device=mid.device)
            check(lib().cp360_l2block_forward_next(dtype_code(self.dtype), ptr(mid), ptr(self.w2), ptr(self.b2), ptr(self.w3),
                                                   ptr(self.b3), ptr(residual), ptr(out), ptr(self.w1), ptr(self.b1), ptr(nxt),
                                                   n_img, n, stream()))
            return out, nxt
        check(lib().cp360_l2block_forward(dtype_code(self.dtype), ptr(mid), ptr(self.w2), ptr(self.b2), ptr(self.w3),
                                          ptr(self.b3), ptr(residual), ptr(out), n_img, n, stream()))
        return out


class L2First:
    """K3f (csrc/lfirst.hip): layer2's first Bottleneck after its conv1 as ONE launch - conv2 (CubePad(1) + 3x3 stride 2) +
    bn2 + relu -> conv3 + bn3 + downsample(x) + relu.  16-bit types, 56x56 -> 28x28 faces.  (weight, bn scale, bn bias) triples."""

    def __init__(self, conv2, conv3, downsample, dtype=torch.float16, device='cuda', next_conv1=None):
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("L2First runs in fp16 / bf16")
        self.dtype, self.device = dtype, torch.device(device)
        L, code = lib(), dtype_code(dtype)
        f32 = lambda t: None if t is None else t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        (w2, s2, b2), (w3, s3, b3), (wd, sd, bd) = conv2, conv3, downsample
        if tuple(w2.shape) != (128, 128, 3, 3) or tuple(w3.shape[:2]) != (512, 128) or tuple(wd.shape[:2]) != (512, 256):
            raise ValueError("L2First is layer2.0's geometry: conv2 128->128 3x3 s2, conv3 128->512, downsample 256->512 s2")
        self.w2 = torch.empty(L.cp360_l2block_packed_bytes(code), dtype=torch.uint8, device=self.device)
        check(L.cp360_l2block_pack_weights(code, ptr(f32(w2)), ptr(f32(s2)), ptr(self.w2), stream()))
        self.b2 = f32(b2)
        self.w3d = torch.empty(L.cp360_l2first_w3d_bytes(code), dtype=torch.uint8, device=self.device)
        check(L.cp360_l2first_pack_w3d(code, ptr(f32(w3).reshape(512, 128)), ptr(f32(s3)), ptr(f32(wd).reshape(512, 256)),
                                       ptr(f32(sd)), ptr(self.w3d), stream()))
        self.b3d = (f32(b3) + f32(bd)).contiguous()
        self.w1 = self.b1 = None
        if next_conv1 is not None:                       # layer2.1's conv1 (512 -> 128) chained onto this launch
            w1, s1, b1 = next_conv1
            if tuple(w1.shape[:2]) != (128, 512):
                raise ValueError("the chained conv1 is 512->128")
            self.w1 = frag_pack_1x1(w1, s1, dtype, 0, self.device)
            self.b1 = f32(b1)

    def __call__(self, mid, x, chain=True):
        """mid [n_img, 56, 56, 128] (conv1 output), x [n_img, 56, 56, 256] (block input) -> out [n_img, 28, 28, 512]
        (with ``next_conv1`` and chain=True: (out, the next block's conv1 output [n_img, 28, 28, 128]))."""
        require_gpu(mid, x)
        n_img = mid.shape[0]
        _check_buf('mid', mid, self.dtype, (n_img, 56, 56, 128))
        _check_buf('x', x, self.dtype, (n_img, 56, 56, 256))
        if mid.shape[3] != 128 or x.shape[3] != 256:
            raise ValueError("dense NHWC tensors only")
        out = torch.empty((n_img, 28, 28, 512), dtype=self.dtype, device=mid.device)
        nxt = torch.empty((n_img, 28, 28, 128), dtype=self.dtype, device=mid.device) if (self.w1 is not None and chain) else None
        check(lib().cp360_l2first_forward(dtype_code(self.dtype), ptr(mid), ptr(self.w2), ptr(self.b2), ptr(self.w3d),
                                          ptr(self.b3d), ptr(x), ptr(out), ptr(self.w1) if nxt is not None else None,
                                          ptr(self.b1) if nxt is not None else None, ptr(nxt), n_img, 28, stream()))
        return out if nxt is None else (out, nxt)


class L3Block:
    """K3e at layer3's geometry (csrc/l2block.hip, C = 256): the tail of a layer3 identity Bottleneck as ONE launch -
    conv2 + bn2 + relu -> conv3 + bn3 + residual + relu.  16-bit types, 14x14 faces.  (weight, bn scale, bn bias) triples."""

    def __init__(self, conv2, conv3, dtype=torch.float16, device='cuda'):
        if dtype not in (torch.float16, torch.bfloat16):
            raise ValueError("L3Block runs in fp16 / bf16")
        self.dtype, self.device = dtype, torch.device(device)
        L, code = lib(), dtype_code(dtype)
        f32 = lambda t: None if t is None else t.detach().to(device=self.device, dtype=torch.float32).contiguous()
        w2, s2, b2 = conv2
        w3, s3, b3 = conv3
        if tuple(w2.shape) != (256, 256, 3, 3) or tuple(w3.shape[:2]) != (1024, 256):
            raise ValueError("L3Block is layer3's geometry: conv2 256->256 3x3, conv3 256->1024 1x1")
        self.w2 = torch.empty(L.cp360_l3block_packed_bytes(code), dtype=torch.uint8, device=self.device)
        check(L.cp360_l3block_pack_weights(code, ptr(f32(w2)), ptr(f32(s2)), ptr(self.w2), stream()))
        self.b2 = f32(b2)
        self.w3 = frag_pack_1x1(w3, s3, dtype, 0, self.device)
        self.b3 = f32(b3)

    def __call__(self, mid, residual):
        """mid [n_img, n, n, 256], residual [n_img, n, n, 1024] -> out [n_img, n, n, 1024]; n = 14 (cube 224) or 32 (cube 512)."""
        require_gpu(mid, residual)
        n_img, n = mid.shape[0], mid.shape[1]
        if n not in (14, 32):
            raise ValueError("L3Block handles 14x14 and 32x32 faces")
        _check_buf('mid', mid, self.dtype, (n_img, n, n, 256))
        _check_buf('residual', residual, self.dtype, (n_img, n, n, 1024))
        if mid.shape[3] != 256 or residual.shape[3] != 1024:
            raise ValueError("dense NHWC tensors only")
        out = torch.empty((n_img, n, n, 1024), dtype=self.dtype, device=mid.device)
        check(lib().cp360_l3block_forward(dtype_code(self.dtype), ptr(mid), ptr(self.w2), ptr(self.b2), ptr(self.w3),
                                          ptr(self.b3), ptr(residual), ptr(out), n_img, n, stream()))
        return out


class launch_order:
    """``with ops.launch_order(2): ...`` - work-item order of the launches issued inside (cp360_set_launch_order: 0
    ascending, 1 descending, 2 alternating).  A performance hint: a consumer that walks its input against the order its
    producer wrote it in starts with the lines still resident in the 256 MB Infinity Cache."""

    def __init__(self, mode):
        self.mode = int(mode)

    def __enter__(self):
        self.old = lib().cp360_set_launch_order(self.mode)
        return self

    def __exit__(self, *exc):
        lib().cp360_set_launch_order(self.old)
        return False


def cubepad_maxpool3s2(x):
    """CubePad(1) + MaxPool2d(3, 2, 0) on NHWC (resnet_cubic.py:169-170)."""
    require_gpu(x)
    n6, n, _, Cc = x.shape
    ho = (n + 2 - 3) // 2 + 1
    y = torch.empty((n6, ho, ho, Cc), dtype=x.dtype, device=x.device)
    check(lib().cp360_cubepad_maxpool3s2(ptr(x), ptr(y), n6, n, Cc, dtype_code(x.dtype), stream()))
    return y


def lstm_gates(partial, splits, bias, c_prev, c_next, h_out, h_coff, h_f32, M, Hc, slab_rows=False, x_next=None):
    """model/clstm.py:68-80.  ``x_next`` = (cam, minmax, x_coff, P, clip_stride, t_next): also write the window-
    normalised frame t_next of every clip into channels [x_coff, x_coff + Hc) of ``h_out`` (the next step's input)."""
    require_gpu(partial, bias, c_prev, c_next, h_out, h_f32)
    _check_buf('gates partial', partial, torch.float32, numel=splits * M * 4 * Hc)
    _check_buf('gates bias', bias, torch.float32, numel=4 * Hc)
    _check_buf('c_prev', c_prev, torch.float32, numel=M * Hc)
    _check_buf('c_next', c_next, torch.float32, numel=M * Hc)
    _check_buf('h_f32', h_f32, torch.float32, numel=M * Hc)
    if not h_out.is_contiguous() or h_out.numel() < M * h_out.shape[-1] or h_coff + Hc > h_out.shape[-1]:
        raise ValueError("h_out must be contiguous [.., ld] with M pixels and h_coff + Hc <= ld")
    if x_next is not None:
        cam, minmax, x_coff, P, clip_stride, t_next = x_next
        require_gpu(cam, minmax)
        _check_buf('cam', cam, torch.float32, numel=(M // P - 1) * clip_stride + (t_next + 1) * P * Hc)
        _check_buf('minmax', minmax, torch.float32, numel=2 * (M // P))
        xp = C.c_void_p(cam.data_ptr() + 4 * t_next * P * Hc)
        check(lib().cp360_lstm_gates_next(ptr(partial), splits, ptr(bias), ptr(c_prev), ptr(c_next), ptr(h_out),
                                          dtype_code(h_out.dtype), h_out.shape[-1], h_coff, ptr(h_f32), M, Hc,
                                          int(slab_rows), xp, ptr(minmax), x_coff, P, clip_stride, stream()))
        return
    check(lib().cp360_lstm_gates(ptr(partial), splits, ptr(bias), ptr(c_prev), ptr(c_next), ptr(h_out),
                                 dtype_code(h_out.dtype), h_out.shape[-1], h_coff, ptr(h_f32), M, Hc,
                                 int(slab_rows), stream()))


class WinoConv:
    """CubePad(1) + 3x3 convolution in the Winograd F(2x2, 3x3) domain (csrc/wino.hip, include/cp360.h "K5w"): the 16-bit
    form of the ConvLSTM convolutions (model/clstm.py:56-64) when the launch has enough tiles to fill 384-row GEMM tiles.
    weight f32 [c_out, c_in, 3, 3], bias f32 [c_out] or None.  ``preferred(n_img, face)`` = the library's planner."""

    # one V / M workspace pair per (device, dtype, HIP stream), shared by every convolution launched on that stream: V is dead
    # once the GEMM has run and M once its output transform has (stream order - which only holds within ONE stream, hence the key)
    _ws = {}

    def __init__(self, weight, bias=None, relu=False, dtype=torch.bfloat16, device='cuda'):
        if dtype not in (torch.bfloat16, torch.float16):
            raise ValueError("the Winograd path runs in bf16 / fp16 (f32 stays on the direct kernels)")
        if tuple(weight.shape[2:]) != (3, 3):
            raise ValueError("a [c_out, c_in, 3, 3] filter")
        self.dtype, self.device, self.relu = dtype, torch.device(device), bool(relu)
        self.c_out, self.c_in = int(weight.shape[0]), int(weight.shape[1])
        self._w_src = weight.detach()
        self.bias = None if bias is None else bias.detach().to(device=self.device, dtype=torch.float32).contiguous()
        self._packed = None
        self.tag = 'wino'

    def desc(self, n_img, face, pix_stride=None, ld_out=0, out_coff=0, relu=None):
        d = _lib.WinoDesc()
        d.dtype = dtype_code(self.dtype)
        d.n_img, d.face, d.c_in, d.c_out = n_img, face, self.c_in, self.c_out
        d.pix_stride = self.c_in if pix_stride is None else pix_stride
        d.ld_out, d.out_coff = ld_out, out_coff
        d.relu = int(self.relu if relu is None else relu)
        return d

    def preferred(self, n_img, face):
        return bool(lib().cp360_wino_preferred(C.byref(self.desc(n_img, face))))

    @property
    def packed(self):
        if self._packed is None:
            d = self.desc(6, 8)
            w = self._w_src.to(device=self.device, dtype=torch.float32).contiguous()
            t = torch.empty(lib().cp360_wino_packed_bytes(C.byref(d)), dtype=torch.uint8, device=self.device)
            check(lib().cp360_wino_pack_weights(C.byref(d), ptr(w), ptr(t), stream()))
            self._packed = t
        return self._packed

    def workspace(self, d):
        key = (self.device, self.dtype, int(torch.cuda.current_stream(self.device).cuda_stream))
        need_v, need_m = lib().cp360_wino_v_bytes(C.byref(d)), lib().cp360_wino_m_bytes(C.byref(d))
        v, m = WinoConv._ws.get(key, (None, None))
        if v is None or v.numel() < need_v:
            v = torch.empty(need_v, dtype=torch.uint8, device=self.device)
        if m is None or m.numel() * 4 < need_m:
            m = torch.empty(need_m // 4, dtype=torch.float32, device=self.device)
        WinoConv._ws[key] = (v, m)
        return v, m

    def _check_in(self, x):
        require_gpu(x)
        if x.dim() != 4 or x.dtype != self.dtype or not x.is_contiguous() or x.shape[1] != x.shape[2] or x.shape[3] < self.c_in \
                or x.shape[0] % 6:
            raise ValueError("x must be a contiguous %s [6B, w, w, >= %d] tensor" % (self.dtype, self.c_in))

    def input(self, x):
        """Input transform of x: returns (V workspace, desc)."""
        self._check_in(x)
        d = self.desc(x.shape[0], x.shape[1], pix_stride=x.shape[3])
        v, _ = self.workspace(d)
        check(lib().cp360_wino_input(C.byref(d), ptr(x), ptr(v), stream()))
        return v, d

    def gemm(self, v, d):
        """The 16 GEMMs on a transformed input: returns the M workspace (f32 [16, m_pad, c_out])."""
        _, m = self.workspace(d)
        L = lib()
        if LAUNCH_TIMER is None:
            check(L.cp360_wino_gemm(C.byref(d), ptr(v), ptr(self.packed), ptr(m), stream()))
        else:
            flops = 2.0 * d.n_img * d.face * d.face * self.c_out * self.c_in * 9       # quoted on the DIRECT form's flops
            packed = self.packed
            check(LAUNCH_TIMER.wrap(self.tag, flops, lambda: L.cp360_wino_gemm(C.byref(d), ptr(v), ptr(packed), ptr(m), stream())))
        return m

    def sums(self, x):
        """Input transform + the 16 GEMMs: returns (M workspace, desc) for an output transform."""
        v, d = self.input(x)
        return self.gemm(v, d), d

    def output(self, m, d, out=None, out_coff=0):
        n_img, w = d.n_img, d.face
        if out is None:
            out = torch.empty((n_img, w, w, self.c_out), dtype=self.dtype, device=self.device)
        require_gpu(out)
        _check_buf('out', out, self.dtype, (n_img, w, w, self.c_out + out_coff))
        d.ld_out, d.out_coff = out.shape[3], out_coff
        check(lib().cp360_wino_output(C.byref(d), ptr(m), ptr(self.bias), ptr(out), stream()))
        return out

    def output_input(self, m, d, nxt):
        """This convolution's output transform fused with ``nxt``'s input transform (cp360_wino_output_input): returns
        (V workspace, nxt's desc), or None where the fused kernel does not apply (faces above 9 x 9)."""
        if nxt.c_in != self.c_out or nxt.dtype != self.dtype:
            raise ValueError("the next convolution reads this one's output")
        dn = nxt.desc(d.n_img, d.face)
        v, _ = self.workspace(dn)
        rc = lib().cp360_wino_output_input(C.byref(d), ptr(m), ptr(self.bias), ptr(v), stream())
        if rc == -8:                                           # CP360_ERR_UNSUPPORTED
            return None
        check(rc)
        return v, dn

    def __call__(self, x, out=None, out_coff=0):
        m, d = self.sums(x)
        return self.output(m, d, out, out_coff)

    def gates_from(self, m, d, bias, c_prev, c_next, h_out, h_coff, h_f32=None, x_next=None):
        """The gate epilogue (clstm.py:68-80) on the Gates convolution's M; x_next as ops.lstm_gates."""
        n_img, w = d.n_img, d.face
        M, Hc = n_img * w * w, self.c_out // 4
        require_gpu(bias, c_prev, c_next, h_out, h_f32)
        _check_buf('gates bias', bias, torch.float32, numel=4 * Hc)
        _check_buf('c_prev', c_prev, torch.float32, numel=M * Hc)
        _check_buf('c_next', c_next, torch.float32, numel=M * Hc)
        _check_buf('h_f32', h_f32, torch.float32, numel=M * Hc)
        if h_out.dtype != self.dtype or not h_out.is_contiguous() or h_out.numel() < M * h_out.shape[-1] or h_coff + Hc > h_out.shape[-1]:
            raise ValueError("h_out must be a contiguous %s [.., ld] tensor with M pixels and h_coff + Hc <= ld" % self.dtype)
        xp, mm, x_coff, stride = None, None, 0, 0
        if x_next is not None:
            cam, minmax, x_coff, P, stride, t_next = x_next
            require_gpu(cam, minmax)
            _check_buf('cam', cam, torch.float32, numel=(M // P - 1) * stride + (t_next + 1) * P * Hc)
            _check_buf('minmax', minmax, torch.float32, numel=2 * (M // P))
            xp, mm = C.c_void_p(cam.data_ptr() + 4 * t_next * P * Hc), ptr(minmax)
        check(lib().cp360_wino_output_gates(C.byref(d), ptr(m), ptr(bias), ptr(c_prev), ptr(c_next), ptr(h_out), h_out.shape[-1],
                                            h_coff, ptr(h_f32), xp, mm, x_coff, stride, stream()))

    def gates(self, x, bias, c_prev, c_next, h_out, h_coff, h_f32=None, x_next=None):
        """The Gates convolution + the cell update (clstm.py:68-80) in the output transform; x_next as ops.lstm_gates."""
        m, d = self.sums(x)
        self.gates_from(m, d, bias, c_prev, c_next, h_out, h_coff, h_f32, x_next)


def window_minmax(x, B, per_clip, minmax, scratch, clip_stride=0):
    require_gpu(x, minmax, scratch)
    _check_buf('x', x, torch.float32, numel=(B - 1) * (clip_stride or per_clip) + per_clip)
    _check_buf('minmax', minmax, torch.float32, numel=2 * B)
    _check_buf('scratch', scratch, torch.float32, numel=B * 256 * 2)
    check(lib().cp360_window_minmax(ptr(x), ptr(minmax), ptr(scratch), B, per_clip, clip_stride, stream()))


def window_normalize(x, minmax, y, y_coff, y2, B, T, t, P, Cc, clip_stride=0):
    require_gpu(x, minmax, y, y2)
    _check_buf('x', x, torch.float32, numel=(B - 1) * (clip_stride or T * P * Cc) + (t + 1) * P * Cc)
    _check_buf('minmax', minmax, torch.float32, numel=2 * B)
    _check_buf('y2', y2, torch.float32, numel=B * P * Cc)
    if not y.is_contiguous() or y.numel() < B * P * y.shape[-1] or y_coff + Cc > y.shape[-1]:
        raise ValueError("y must be contiguous [.., ld] with B*P pixels and y_coff + C <= ld")
    check(lib().cp360_window_normalize(ptr(x), ptr(minmax), ptr(y), dtype_code(y.dtype), y.shape[-1], y_coff,
                                       ptr(y2), B, T, t, P, Cc, clip_stride, stream()))


def window_normalize_frames(x, minmax, y, B, T, P, Cc, clip_stride=0):
    """All T frames of every window at once into y [T, B, P, Cc] (dense; f32 / bf16 / fp16)."""
    require_gpu(x, minmax, y)
    _check_buf('x', x, torch.float32, numel=(B - 1) * (clip_stride or T * P * Cc) + T * P * Cc)
    _check_buf('minmax', minmax, torch.float32, numel=2 * B)
    _check_buf('y', y, y.dtype, numel=T * B * P * Cc)
    check(lib().cp360_window_normalize_frames(ptr(x), ptr(minmax), ptr(y), dtype_code(y.dtype), B, T, P, Cc, clip_stride,
                                              stream()))


def held_clock_ghz(device='cuda', ms=6.0, launches=3):
    """Diagnostic (never on the hot path): the shader clock the chip holds under a dense bf16 MFMA load on random operands -
    cp360_clock_probe (csrc/misc.hip), one wave per SIMD on every CU, median over the waves of the last of ``launches``
    back-to-back launches of about ``ms`` milliseconds each.  MI355X boxes differ in the clock they hold (DVFS), which moves
    a bench line by more than a round of kernel work: bench.py prints this next to its numbers."""
    dev = torch.device(device)
    n_wg = torch.cuda.get_device_properties(dev).multi_processor_count
    stamps = torch.zeros((n_wg * 4, 2), dtype=torch.int64, device=dev)
    iters = max(1, int(ms * 1e-3 * 1.8e9 / (16 * 16)))            # 16 MFMAs of 16 cycles per iteration at about 1.8 GHz
    with torch.cuda.device(dev):
        for _ in range(launches):
            check(lib().cp360_clock_probe(ptr(stamps), n_wg, iters, stream()))
        torch.cuda.synchronize()
    s = stamps.cpu().double()
    ok = s[:, 1] > 0
    if not bool(ok.any()):
        return None
    ghz = 0.1 * s[ok, 0] / s[ok, 1]
    return round(float(ghz.median()), 4)


# ----------------------------------------------------------------------------- K5t: ConvLSTM training
_TRAIN_DTYPES = (torch.float32, torch.bfloat16)


def _train_dtype(dt):
    if dt not in _TRAIN_DTYPES:
        raise ValueError("ConvLSTM training runs in f32 or bf16 operands (got %s)" % dt)
    return dtype_code(dt)


def train_gates(partial, splits, bias, c_prev, c_next, h_out, h_coff, h_f32, acts, M, Hc):
    """cp360_train_gates: lstm_gates on plain [splits, M, 4 Hc] slabs that also keeps the activated gates acts f32 [M, 4 Hc]."""
    require_gpu(partial, bias, c_prev, c_next, h_out, h_f32, acts)
    _check_buf('gates partial', partial, torch.float32, numel=splits * M * 4 * Hc)
    _check_buf('gates bias', bias, torch.float32, numel=4 * Hc)
    for name, t, n in (('c_prev', c_prev, M * Hc), ('c_next', c_next, M * Hc), ('h_f32', h_f32, M * Hc), ('acts', acts, M * 4 * Hc)):
        _check_buf(name, t, torch.float32, numel=n)
    if not h_out.is_contiguous() or h_out.numel() < M * h_out.shape[-1] or h_coff + Hc > h_out.shape[-1]:
        raise ValueError("h_out must be contiguous [.., ld] with M pixels and h_coff + Hc <= ld")
    check(lib().cp360_train_gates(ptr(partial), splits, ptr(bias), ptr(c_prev), ptr(c_next), ptr(h_out),
                                  _train_dtype(h_out.dtype), h_out.shape[-1], h_coff, ptr(h_f32), ptr(acts), M, Hc, stream()))


def train_gates_backward(dh, dc, acts, c_prev, c_next, dgates, M, Hc):
    """cp360_train_gates_backward: dgates [M, 4 Hc] (compute dtype) from dh, dc; dc becomes d c_prev in place."""
    require_gpu(dh, dc, acts, c_prev, c_next, dgates)
    for name, t, n in (('dh', dh, M * Hc), ('dc', dc, M * Hc), ('acts', acts, M * 4 * Hc), ('c_prev', c_prev, M * Hc),
                       ('c_next', c_next, M * Hc)):
        _check_buf(name, t, torch.float32, numel=n)
    _check_buf('dgates', dgates, dgates.dtype, numel=M * 4 * Hc)
    check(lib().cp360_train_gates_backward(ptr(dh), ptr(dc), ptr(acts), ptr(c_prev), ptr(c_next), ptr(dgates),
                                           _train_dtype(dgates.dtype), M, Hc, stream()))


def cubepad_inverse(face):
    """Host int32 (offsets [6 face^2 + 1], entries [6 (face+2)^2]): the padded positions of CubePad(1) that copy each source
    pixel of a cube, ascending (cp360_train_cubepad_inverse_host, no GPU needed)."""
    off = np.empty(6 * face * face + 1, dtype=np.int32)
    ent = np.empty(6 * (face + 2) * (face + 2), dtype=np.int32)
    check(lib().cp360_train_cubepad_inverse_host(int(face), off.ctypes.data_as(C.c_void_p), ent.ctypes.data_as(C.c_void_p)))
    return off, ent


def c2e_inverse(face_map, coord, w):
    """Host int32 (offsets [6 w^2 + 1], entries): the (output pixel << 2 | bilinear tap) pairs of cube -> equirectangular
    sampling that read each cube pixel, ascending (cp360_train_c2e_inverse_host)."""
    fm = np.ascontiguousarray(face_map, dtype=np.int8)
    pc = np.ascontiguousarray(coord, dtype=np.float32)
    if fm.shape != (2 * w, 4 * w) or pc.shape != (2 * w, 4 * w, 2):
        raise ValueError("face_map [2w, 4w] and coord [2w, 4w, 2] expected")
    off = np.empty(6 * w * w + 1, dtype=np.int32)
    ent = np.empty(32 * w * w, dtype=np.int32)
    n = lib().cp360_train_c2e_inverse_host(fm.ctypes.data_as(C.c_void_p), pc.ctypes.data_as(C.c_void_p), int(w),
                                           off.ctypes.data_as(C.c_void_p), ent.ctypes.data_as(C.c_void_p))
    check(min(n, 0))
    return off, ent[:n].copy()


class DgradPack:
    """The dgrad operand of one CubePad(1) + 3x3 convolution: filter f32 [c_out, c_in, 3, 3], input channels [ci0, ci0 + n)
    packed [n][9 c_out] in ``dtype`` (cp360_train_dgrad_pack).  Re-made by the owner when the weight's version changes."""

    def __init__(self, weight, ci0, n, dtype):
        require_gpu(weight)
        self.c_out, self.c_in = int(weight.shape[0]), int(weight.shape[1])
        if tuple(weight.shape[2:]) != (3, 3):
            raise ValueError("a [c_out, c_in, 3, 3] filter")
        self.ci0, self.n, self.dtype = int(ci0), int(n), dtype
        L = lib()
        code = _train_dtype(dtype)
        nbytes = L.cp360_train_dgrad_packed_bytes(code, self.c_out, self.n)
        self.packed = torch.empty(nbytes, dtype=torch.uint8, device=weight.device)
        w = weight.detach().float().contiguous()
        check(L.cp360_train_dgrad_pack(code, ptr(w), self.c_out, self.c_in, self.ci0, self.n, ptr(self.packed), stream()))

    def dgrad(self, dy, dxpad=None):
        """dy [n_img, face, face, c_out] -> f32 [n_img, face+2, face+2, n] (the full correlation onto the padded grid)."""
        require_gpu(dy, dxpad)
        n_img, face, _, co = dy.shape
        if co != self.c_out or dy.dtype != self.dtype or not dy.is_contiguous():
            raise ValueError("dy must be a contiguous %s [n_img, face, face, %d] tensor" % (self.dtype, self.c_out))
        if dxpad is None:
            dxpad = torch.empty((n_img, face + 2, face + 2, self.n), dtype=torch.float32, device=dy.device)
        _check_buf('dxpad', dxpad, torch.float32, numel=n_img * (face + 2) ** 2 * self.n)
        check(lib().cp360_train_dgrad(_train_dtype(self.dtype), ptr(dy), n_img, face, self.c_out, ptr(self.packed), self.n,
                                      ptr(dxpad), stream()))
        return dxpad


def cubepad_adjoint(dxpad, inv_off, inv_ent, dx, act=None, act_coff=0, accumulate=False):
    """cp360_train_cubepad_adjoint: dxpad f32 [n_img, face+2, face+2, n] -> dx [n_img, face, face, n] (written, or added
    onto with accumulate), masked by (act > 0) when act [n_img, face, face, ld] is given."""
    require_gpu(dxpad, inv_off, inv_ent, dx, act)
    n_img, fp, _, n = dxpad.shape
    face = fp - 2
    _check_buf('dxpad', dxpad, torch.float32)
    _check_buf('dx', dx, dx.dtype, (n_img, face, face, n))
    if inv_off.dtype != torch.int32 or inv_ent.dtype != torch.int32 or inv_off.numel() != 6 * face * face + 1 \
            or inv_ent.numel() != 6 * fp * fp:
        raise ValueError("inverse table of a different face size")
    act_ld = 0
    if act is not None:
        _check_buf('act', act, act.dtype)
        if tuple(act.shape[:3]) != (n_img, face, face) or act_coff + n > act.shape[3]:
            raise ValueError("act must be [n_img, face, face, >= act_coff + n]")
        act_ld = act.shape[3]
    check(lib().cp360_train_cubepad_adjoint(ptr(dxpad), ptr(inv_off), ptr(inv_ent), n_img, face, n, ptr(act),
                                            0 if act is None else _train_dtype(act.dtype), act_ld, act_coff, ptr(dx),
                                            _train_dtype(dx.dtype), int(bool(accumulate)), stream()))
    return dx


def conv_wgrad(dy, x, c_in, pad_table, dw, db=None, accumulate=False):
    """cp360_train_wgrad: dy [n_img, face, face, c_out], x [n_img, face, face, ld >= c_in] (same dtype; n_img may stack
    several steps) -> dw f32 [c_out, c_in, 3, 3] (+ db f32 [c_out]) of CubePad(1) + 3x3 convolution, in ONE launch."""
    require_gpu(dy, x, pad_table, dw, db)
    n_img, face, _, c_out = dy.shape
    if dy.dtype != x.dtype or not dy.is_contiguous() or not x.is_contiguous() or tuple(x.shape[:3]) != (n_img, face, face) \
            or x.shape[3] < c_in:
        raise ValueError("dy / x must be contiguous, of one dtype and of the same [n_img, face, face] geometry")
    if pad_table.dtype != torch.int32 or pad_table.numel() != 6 * (face + 2) ** 2:
        raise ValueError("pad_table must be the int32 CubePad(1) table of the face size")
    _check_buf('dw', dw, torch.float32, numel=c_out * c_in * 9)
    _check_buf('db', db, torch.float32, numel=c_out)
    check(lib().cp360_train_wgrad(_train_dtype(dy.dtype), ptr(dy), ptr(x), x.shape[3], ptr(pad_table), n_img, face, c_out,
                                  c_in, ptr(dw), ptr(db), int(bool(accumulate)), stream()))


def saliency_forward(h, face_map, coord, out_max, argmax):
    """cp360_train_saliency_forward: h f32 [6B, w, w, C] -> map f32 [B, 2w, 4w] and its argmax channel (int32)."""
    require_gpu(h, face_map, coord, out_max, argmax)
    n6, w, _, Cc = h.shape
    B = n6 // 6
    _check_buf('h', h, torch.float32)
    _check_buf('out_max', out_max, torch.float32, numel=B * 8 * w * w)
    _check_buf('argmax', argmax, torch.int32, numel=B * 8 * w * w)
    if n6 % 6 or face_map.dtype != torch.int8 or coord.dtype != torch.float32:
        raise ValueError("h needs 6B faces, face_map int8 and coord f32")
    check(lib().cp360_train_saliency_forward(ptr(h), ptr(face_map.contiguous()), ptr(coord.contiguous()), ptr(out_max),
                                             ptr(argmax), B, Cc, w, stream()))


def saliency_backward(dmap, argmax, coord, inv_off, inv_ent, dh):
    """cp360_train_saliency_backward: ADD d(map) f32 [B, 2w, 4w] onto dh f32 [6B, w, w, C] through the argmax channel."""
    require_gpu(dmap, argmax, coord, inv_off, inv_ent, dh)
    n6, w, _, Cc = dh.shape
    B = n6 // 6
    _check_buf('dh', dh, torch.float32)
    _check_buf('dmap', dmap, torch.float32, numel=B * 8 * w * w)
    _check_buf('argmax', argmax, torch.int32, numel=B * 8 * w * w)
    if inv_off.dtype != torch.int32 or inv_off.numel() != 6 * w * w + 1 or inv_ent.dtype != torch.int32:
        raise ValueError("inverse table of a different face size")
    check(lib().cp360_train_saliency_backward(ptr(dmap), ptr(argmax), ptr(coord.contiguous()), ptr(inv_off), ptr(inv_ent),
                                              ptr(dh), B, Cc, w, stream()))


# ----------------------------------------------------------------------------- K5o: fused Adam
def _adam_args(p, g, m, v, lr, betas, eps, weight_decay, step):
    """The checks and the scalar arguments the two Adam entry points share: the bias corrections in double, as torch."""
    require_gpu(p, g, m, v)
    for name, t in (('p', p), ('g', g), ('m', m), ('v', v)):
        _check_buf(name, t, torch.float32)
        if tuple(t.shape) != tuple(p.shape) or t.device != p.device:
            raise ValueError("%s must have the parameter's shape %s and device" % (name, tuple(p.shape)))
    step = int(step)
    if step < 1:
        raise ValueError("step counts from 1 (the step being taken), got %d" % step)
    b1, b2 = float(betas[0]), float(betas[1])
    if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0) or float(lr) < 0.0 or float(eps) < 0.0 or float(weight_decay) < 0.0:
        raise ValueError("Adam needs lr, eps, weight_decay >= 0 and betas in [0, 1)")
    return (float(lr), b1, b2, float(eps), float(weight_decay), 1.0 - b1 ** step, math.sqrt(1.0 - b2 ** step))


def adam_step(p, g, m, v, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1):
    """cp360_train_adam: step number ``step`` (from 1) of torch.optim.Adam (amsgrad False, maximize False) on f32 tensors of
    one shape, in place: parameter p, gradient g, exp_avg m, exp_avg_sq v.  The caller bumps p's version counter."""
    args = _adam_args(p, g, m, v, lr, betas, eps, weight_decay, step)
    if p.numel() == 0:
        raise ValueError("an empty parameter")
    check(lib().cp360_train_adam(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), *args, stream()))


def conv_pack_bytes(c_out, c_in, dtype, chan_major):
    """Bytes of a forward pack of a CubePad(1) + 3x3 filter [c_out, c_in, 3, 3] as the library sizes it (cp360_conv_packed_bytes;
    0: it has no kernel for that layout of this shape).  chan_major: cp360_conv_desc.clip_resident."""
    d = ConvDesc()
    for k, v in dict(dtype=dtype_code(dtype), n_img=6, h_in=7, w_in=7, c_in=c_in, pix_stride=c_in, kh=3, kw=3, sy=1, sx=1,
                     h_out=7, w_out=7, c_out=c_out, pad_mode=1, pad=1, ld_out=c_out, relu=1, splits=1,
                     clip_resident=int(bool(chan_major))).items():
        setattr(d, k, v)
    return lib().cp360_conv_packed_bytes(C.byref(d))


def adam_step_conv(p, g, m, v, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1, dtype=torch.float32,
                   fwd_tap_major=None, fwd_chan_major=None, dgrad_packed=None, ci0=0, n_dgrad=0):
    """cp360_train_adam_conv: ``adam_step`` on a filter [c_out, c_in, 3, 3] that also writes the new weights, rounded to
    ``dtype`` (f32 / bf16), into the packs given: the two forward layouts of ``Conv.packed_for(0 / 1)`` and ``DgradPack.packed``
    of input channels [ci0, ci0 + n_dgrad) (uint8 tensors as those classes keep them; None: not written)."""
    args = _adam_args(p, g, m, v, lr, betas, eps, weight_decay, step)
    if p.dim() != 4 or tuple(p.shape[2:]) != (3, 3):
        raise ValueError("a [c_out, c_in, 3, 3] filter")
    c_out, c_in = int(p.shape[0]), int(p.shape[1])
    code = _train_dtype(dtype)
    es = torch.empty((), dtype=dtype).element_size()
    require_gpu(fwd_tap_major, fwd_chan_major, dgrad_packed)
    ci0, n_dgrad = int(ci0), int(n_dgrad)
    if dgrad_packed is None:
        ci0 = n_dgrad = 0
    elif ci0 < 0 or n_dgrad < 1 or ci0 + n_dgrad > c_in:
        raise ValueError("the dgrad pack's channels [%d, %d) are not inside [0, %d)" % (ci0, ci0 + n_dgrad, c_in))
    for name, t, chan_major in (('fwd_tap_major', fwd_tap_major, False), ('fwd_chan_major', fwd_chan_major, True),
                                ('dgrad_packed', dgrad_packed, None)):
        if t is None:
            continue
        nbytes = n_dgrad * 9 * c_out * es if chan_major is None else conv_pack_bytes(c_out, c_in, dtype, chan_major)
        if nbytes == 0 or not t.is_contiguous() or t.device != p.device or t.numel() * t.element_size() != nbytes:
            raise ValueError("%s must be the contiguous %d-byte pack of this filter on its device" % (name, nbytes))
    check(lib().cp360_train_adam_conv(ptr(p), ptr(g), ptr(m), ptr(v), c_out, c_in, *args, code, ptr(fwd_tap_major),
                                      ptr(fwd_chan_major), ptr(dgrad_packed), ci0, n_dgrad, stream()))


# ----------------------------------------------------------------------------- K5f: flow resize and flow loss
def flow_resize_coeffs(in_size, out_size):
    """Host tables of one axis of cv2.resize(INTER_CUBIC) (cp360_flow_resize_coeffs_host, no GPU needed): first-tap index + 1
    int32 [out_size] and the four Keys coefficients f32 [out_size, 4]."""
    ofs = np.empty(int(out_size), dtype=np.int32)
    coef = np.empty((int(out_size), 4), dtype=np.float32)
    check(lib().cp360_flow_resize_coeffs_host(int(in_size), int(out_size), ofs.ctypes.data_as(C.c_void_p),
                                              coef.ctypes.data_as(C.c_void_p)))
    return ofs, coef


_FLOW_TABLES = {}


def _flow_tables(in_size, out_size, dev):
    key = (int(in_size), int(out_size), str(dev))
    t = _FLOW_TABLES.get(key)
    if t is None:
        ofs, coef = flow_resize_coeffs(in_size, out_size)
        t = _FLOW_TABLES[key] = (torch.from_numpy(ofs).to(dev), torch.from_numpy(coef).to(dev))
    return t


def flow_resize(flow, h_out, w_out, fscale, out=None):
    """cp360_flow_resize: f32 [..., h_in, w_in, 2] on the GPU -> cv2.resize(INTER_CUBIC) to [..., h_out, w_out, 2] times fscale
    (equal sizes: the scale alone, as cv2 copies)."""
    require_gpu(flow, out)
    if flow.dim() < 3 or flow.shape[-1] != 2:
        raise ValueError("flow must be [..., H, W, 2], got %s" % (tuple(flow.shape),))
    lead = tuple(flow.shape[:-3])
    h_in, w_in = int(flow.shape[-3]), int(flow.shape[-2])
    F = int(np.prod(lead)) if lead else 1
    _check_buf('flow', flow, torch.float32)
    if out is None:
        out = torch.empty(lead + (int(h_out), int(w_out), 2), dtype=torch.float32, device=flow.device)
    _check_buf('out', out, torch.float32, numel=F * h_out * w_out * 2)
    if (h_in, w_in) == (h_out, w_out):
        yo = yc = xo = xc = None
    else:
        yo, yc = _flow_tables(h_in, h_out, flow.device)
        xo, xc = _flow_tables(w_in, w_out, flow.device)
    check(lib().cp360_flow_resize(_lib.F32, ptr(flow), F, h_in, w_in, ptr(out), int(h_out), int(w_out), ptr(yo), ptr(yc),
                                  ptr(xo), ptr(xc), float(fscale), stream()))
    return out


def _flow_loss_geometry(maps, flow):
    if maps.dim() != 4 or flow.dim() != 5 or flow.shape[-1] != 2:
        raise ValueError("maps must be [B, L + 1, 2w, 4w] and flow [B, L, H, W, 2]")
    B, n, mh, mw = (int(s) for s in maps.shape)
    L, h, wl = int(flow.shape[1]), int(flow.shape[2]), int(flow.shape[3])
    w = mh // 2
    if flow.shape[0] != B or n != L + 1 or mh != 2 * w or mw != 4 * w:
        raise ValueError("maps %s and flow %s disagree: maps must be [B, L + 1, 2w, 4w] for flow [B, L, H, W, 2]"
                         % (tuple(maps.shape), tuple(flow.shape)))
    _check_buf('maps', maps, torch.float32)
    _check_buf('flow', flow, torch.float32)
    nbytes = lib().cp360_flow_loss_work_bytes(B, L, w, h, wl)
    if nbytes == 0:
        raise ValueError("flow loss: unsupported geometry (faces up to 16 x 16, flow of at least 2 x 2): maps %s, flow %s"
                         % (tuple(maps.shape), tuple(flow.shape)))
    return B, L, w, h, wl, nbytes


def flow_loss_forward(maps, flow, mm_th):
    """cp360_flow_loss_forward: maps f32 [B, L + 1, 2w, 4w], scaled flow f32 [B, L, H, W, 2] -> f32 [3] (smooth, temporal,
    motion-mask sum-MSE terms over all B x L pairs)."""
    require_gpu(maps, flow)
    B, L, w, h, wl, nbytes = _flow_loss_geometry(maps, flow)
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=maps.device)
    loss = torch.empty(3, dtype=torch.float32, device=maps.device)
    check(lib().cp360_flow_loss_forward(_lib.F32, ptr(maps), ptr(flow), B, L, w, h, wl, float(mm_th), ptr(loss), ptr(work),
                                        stream()))
    return loss


def flow_loss_backward(maps, flow, grad_loss, mm_th):
    """cp360_flow_loss_backward: grad_loss f32 [3] (device) -> dmaps f32 [B, L + 1, 2w, 4w] (map 0 of each clip: zero)."""
    require_gpu(maps, flow, grad_loss)
    B, L, w, h, wl, nbytes = _flow_loss_geometry(maps, flow)
    _check_buf('grad_loss', grad_loss, torch.float32, numel=3)
    work = torch.empty(nbytes // 4, dtype=torch.float32, device=maps.device)
    dmaps = torch.empty_like(maps)
    check(lib().cp360_flow_loss_backward(_lib.F32, ptr(maps), ptr(flow), ptr(grad_loss), B, L, w, h, wl, float(mm_th),
                                         ptr(dmaps), ptr(work), stream()))
    return dmaps


# ----------------------------------------------------------------------------- K10: Farneback optical flow
def optflow_levels(H, W, pyr_scale=0.5, levels=7):
    """cp360_optflow_levels_host (no GPU needed): [(h, w, ksz, sigma)] of pyramid levels k = 0 (full size) .. L."""
    L = lib().cp360_optflow_levels_host(int(H), int(W), float(pyr_scale), int(levels), 0, None, None, None, None)
    if L < 0:
        check(L)
    hs, ws, ks = (np.empty(L + 1, dtype=np.int32) for _ in range(3))
    sg = np.empty(L + 1, dtype=np.float64)
    vp = C.c_void_p
    rc = lib().cp360_optflow_levels_host(int(H), int(W), float(pyr_scale), int(levels), L + 1, hs.ctypes.data_as(vp),
                                         ws.ctypes.data_as(vp), ks.ctypes.data_as(vp), sg.ctypes.data_as(vp))
    if rc < 0:
        check(rc)
    return [(int(hs[k]), int(ws[k]), int(ks[k]), float(sg[k])) for k in range(L + 1)]


def optflow_gauss_kernel(ksz, sigma):
    """cp360_optflow_gauss_host (no GPU needed): the f32 taps of a pyramid level's Gaussian."""
    taps = np.empty(max(int(ksz), 1), dtype=np.float32)
    check(lib().cp360_optflow_gauss_host(int(ksz), float(sigma), taps.ctypes.data_as(C.c_void_p)))
    return taps


def optflow_poly_tables(poly_n=5, poly_sigma=1.2):
    """cp360_optflow_poly_tables_host (no GPU needed): g, xg, xxg f32 [2n + 1] and ig f32 [4] = (ig11, ig03, ig33, ig55)."""
    n = int(poly_n)
    g, xg, xxg = (np.empty(2 * max(n, 0) + 1, dtype=np.float32) for _ in range(3))
    ig = np.empty(4, dtype=np.float32)
    vp = C.c_void_p
    check(lib().cp360_optflow_poly_tables_host(n, float(poly_sigma), g.ctypes.data_as(vp), xg.ctypes.data_as(vp),
                                               xxg.ctypes.data_as(vp), ig.ctypes.data_as(vp)))
    return g, xg, xxg, ig


def _optflow_images(name, t, trailing=()):
    """A contiguous f32 [..., h, w] + trailing tensor seen as [N, h, w] + trailing: (N, h, w)."""
    nd = 2 + len(trailing)
    if t.dim() < nd or tuple(t.shape[t.dim() - len(trailing):]) != tuple(trailing):
        raise ValueError("%s must be [..., h, w%s], got %s" % (name, ''.join(', %d' % s for s in trailing), tuple(t.shape)))
    _check_buf(name, t, torch.float32)
    h, w = int(t.shape[-nd]), int(t.shape[-nd + 1])
    return int(t.numel() // max(h * w * int(np.prod(trailing, dtype=np.int64)), 1)), h, w


def optflow_gray(rgb):
    """cp360_optflow_gray: u8 [..., 3] resized frames as the video reader delivers them -> f32 [...] gray 0 .. 255 (channels
    reversed, then cv2's BGR2GRAY integer arithmetic: the reference's quirk)."""
    require_gpu(rgb)
    if rgb.dtype != torch.uint8 or rgb.dim() < 1 or rgb.shape[-1] != 3 or rgb.numel() == 0:
        raise ValueError("rgb must be a non-empty uint8 [..., 3] tensor")
    rgb = rgb.contiguous()
    out = torch.empty(rgb.shape[:-1], dtype=torch.float32, device=rgb.device)
    check(lib().cp360_optflow_gray(ptr(rgb), ptr(out), out.numel(), stream()))
    return out


def optflow_pyr_level(gray, ksz, sigma, lh, lw):
    """cp360_optflow_pyr_level: f32 [..., H, W] -> [..., lh, lw] = bilinear resize of the ksz x ksz Gaussian blur."""
    require_gpu(gray)
    N, H, W = _optflow_images('gray', gray)
    out = torch.empty(tuple(gray.shape[:-2]) + (int(lh), int(lw)), dtype=torch.float32, device=gray.device)
    tmp = torch.empty_like(gray)
    check(lib().cp360_optflow_pyr_level(ptr(gray), N, H, W, int(ksz), float(sigma), ptr(out), int(lh), int(lw), ptr(tmp),
                                        stream()))
    return out


def optflow_poly_exp(img, poly_n=5, poly_sigma=1.2):
    """cp360_optflow_poly_exp: f32 [..., h, w] -> R [..., 5, h, w] (planar), the coefficients of [y, x, y^2, x^2, xy]."""
    require_gpu(img)
    N, h, w = _optflow_images('img', img)
    R = torch.empty(tuple(img.shape[:-2]) + (5, h, w), dtype=torch.float32, device=img.device)
    check(lib().cp360_optflow_poly_exp(ptr(img), N, h, w, int(poly_n), float(poly_sigma), ptr(R), stream()))
    return R


def optflow_matrices(R0, R1, flow):
    """cp360_optflow_matrices: R0 (prev), R1 (next) f32 [P, 5, h, w] or [5, h, w], flow f32 [P, h, w, 2] or [h, w, 2]
    -> M of R0's shape."""
    require_gpu(R0, R1, flow)
    if R0.shape != R1.shape or R0.dim() not in (3, 4) or R0.shape[-3] != 5:
        raise ValueError("R0 and R1 must both be [P, 5, h, w] or [5, h, w], got %s and %s" % (tuple(R0.shape), tuple(R1.shape)))
    h, w = int(R0.shape[-2]), int(R0.shape[-1])
    P = int(R0.shape[0]) if R0.dim() == 4 else 1
    _check_buf('R0', R0, torch.float32)
    _check_buf('R1', R1, torch.float32)
    _check_buf('flow', flow, torch.float32, numel=P * h * w * 2)
    if tuple(flow.shape[-3:]) != (h, w, 2):
        raise ValueError("flow must be [P, h, w, 2] for R [P, 5, h, w], got %s" % (tuple(flow.shape),))
    M = torch.empty_like(R0)
    check(lib().cp360_optflow_matrices(ptr(R0), ptr(R1), 5 * h * w, ptr(flow), ptr(M), P, h, w, stream()))
    return M


def optflow_blur_solve(M, winsize=15):
    """cp360_optflow_blur_solve: M f32 [P, 5, h, w] or [5, h, w] -> flow [P, h, w, 2] or [h, w, 2]."""
    require_gpu(M)
    if M.dim() not in (3, 4) or M.shape[-3] != 5:
        raise ValueError("M must be [P, 5, h, w] or [5, h, w], got %s" % (tuple(M.shape),))
    if int(winsize) < 1 or int(winsize) % 2 == 0:
        raise ValueError("winsize must be odd, got %s" % (winsize,))
    _check_buf('M', M, torch.float32)
    h, w = int(M.shape[-2]), int(M.shape[-1])
    P = int(M.shape[0]) if M.dim() == 4 else 1
    flow = torch.empty(tuple(M.shape[:-3]) + (h, w, 2), dtype=torch.float32, device=M.device)
    check(lib().cp360_optflow_blur_solve(ptr(M), ptr(flow), P, h, w, int(winsize), stream()))
    return flow


def optflow_flow_upsample(flow, h_out, w_out, mul):
    """cp360_optflow_flow_upsample: f32 [..., h, w, 2] -> [..., h_out, w_out, 2] = bilinear resize times mul."""
    require_gpu(flow)
    P, h, w = _optflow_images('flow', flow, (2,))
    out = torch.empty(tuple(flow.shape[:-3]) + (int(h_out), int(w_out), 2), dtype=torch.float32, device=flow.device)
    check(lib().cp360_optflow_flow_upsample(ptr(flow), P, h, w, ptr(out), int(h_out), int(w_out), float(mul), stream()))
    return out


# ----------------------------------------------------------------------------- K11: 360-degree stabilisation (csrc/stabilize.hip)
def _stab_work(F, H, W, device, work=None):
    """The workspace of one K11 call: `work` when it is large enough, else a new one (F = 0: the tables alone)."""
    return _work(lib().cp360_stab_work_bytes, "stabilisation", F, H, W, device, work)


def _stab_rotations(R, n=None):
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3) or R.shape[0] < 1 or (n is not None and R.shape[0] != n):
        raise ValueError("R must be [%s, 3, 3], got %s" % ('F' if n is None else n, tuple(R.shape)))
    _check_buf('R', R, torch.float32)


def rotation_fit(flow, iters=8, c_min_px=0.25, work=None):
    """cp360_stab_fit: flow f32 [F, H, W, 2] (K10's convention) -> (R f32 [F, 3, 3], diag f64 [F, 4]): the camera rotation of
    every pair (a scene direction p of frame t is seen at R_t p in frame t + 1) and (final scale in px, sum of weights, weighted
    RMS residual in px, |delta| of the last iteration)."""
    require_gpu(flow)
    if flow.dim() != 4 or flow.shape[3] != 2 or flow.numel() == 0:
        raise ValueError("flow must be a non-empty [F, H, W, 2], got %s" % (tuple(flow.shape),))
    _check_buf('flow', flow, torch.float32)
    if int(iters) < 1 or not float(c_min_px) > 0.0:
        raise ValueError("iters must be at least 1 and c_min_px positive, got %r, %r" % (iters, c_min_px))
    F, H, W = (int(s) for s in flow.shape[:3])
    work = _stab_work(F, H, W, flow.device, work)
    R = torch.empty((F, 3, 3), dtype=torch.float32, device=flow.device)
    diag = torch.empty((F, 4), dtype=torch.float64, device=flow.device)
    check(lib().cp360_stab_fit(ptr(flow), F, H, W, int(iters), float(c_min_px), ptr(R), ptr(diag), ptr(work), work.numel() * 8,
                               stream()))
    return R, diag


def rotation_flow(R, H, W, work=None):
    """cp360_stab_flow: R f32 [F, 3, 3] -> G f32 [F, H, W, 2] = pix(R dir(x, y)) - (x, y), x wrapped into [-W / 2, W / 2)."""
    require_gpu(R)
    _stab_rotations(R)
    F, H, W = int(R.shape[0]), int(H), int(W)
    work = _stab_work(0, H, W, R.device, work)
    G = torch.empty((F, H, W, 2), dtype=torch.float32, device=R.device)
    check(lib().cp360_stab_flow(ptr(R), F, H, W, ptr(G), ptr(work), work.numel() * 8, stream()))
    return G


def equirect_rotate(frames, R, out=None, work=None):
    """cp360_stab_rotate: out[n](x, y) = bilinear(frames[n], pix(R[n] dir(x, y))), columns wrap, rows clamp; frames u8
    [N, H, W, 3] or f32 [N, H, W, C], C <= 4; R f32 [N, 3, 3]; the output has the frames' type and size."""
    require_gpu(frames, R, out)
    N, H, W, C = _frames_nhwc(frames, u8_only=False)
    _stab_rotations(R, N)
    out = _out_for(out, (N, H, W, C), frames.dtype, frames.device, frames)
    work = _stab_work(0, H, W, frames.device, work)
    check(lib().cp360_stab_rotate(dtype_code(frames.dtype), ptr(frames), ptr(R), N, H, W, C, ptr(out), ptr(work),
                                  work.numel() * 8, stream()))
    return out


# ----------------------------------------------------------------------------- K23: ego-motion from flow (csrc/egomotion.hip)
def _ego_work(F, H, W, device, work=None):
    """The workspace of one K23 call: `work` when it is large enough, else a new one (F = 0: the tables alone).  It is never
    smaller than K11's for the same sizes, so the fit's internal K11 start runs in it first."""
    return _work(lib().cp360_ego_work_bytes, "ego-motion", F, H, W, device, work)


def _ego_flow(flow):
    if flow.dim() != 4 or flow.shape[3] != 2 or flow.numel() == 0:
        raise ValueError("flow must be a non-empty [F, H, W, 2], got %s" % (tuple(flow.shape),))
    _check_buf('flow', flow, torch.float32)
    return (int(s) for s in flow.shape[:3])


def egomotion_fit(flow, R0=None, iters=8, c_min_px=0.25, t_min_px=0.25, min_share=0.25, work=None):
    """cp360_ego_fit: flow f32 [F, H, W, 2] (K10's convention) -> (R f32 [F, 3, 3], e f32 [F, 3], diag f64 [F, 8]): the camera
    rotation of every pair (K11's convention) and the unit direction of its translation in frame t's axes, fitted from R0 f32
    [F, 3, 3] (None: ``rotation_fit`` of the same flow with the same iters and c_min_px).  A pair of which less than min_share of
    the sphere moves by more than t_min_px at R0 has no translation: e = (0, 0, 0) and R = R0 bit for bit (both thresholds are
    conventions).  diag = (share, sum of weights, weighted RMS of the epipolar residual in px, lambda_0 / lambda_2 and lambda_1 /
    lambda_2 of the last scatter matrix, |delta| of the last rotation step, the scale in px, flag: 0 fitted, 1 gated, 2 singular)."""
    require_gpu(flow, R0, work)
    F, H, W = _ego_flow(flow)
    if int(iters) < 1 or not float(c_min_px) > 0.0 or not float(t_min_px) >= 0.0 or not float(min_share) >= 0.0:
        raise ValueError("iters must be at least 1, c_min_px positive, t_min_px and min_share not negative, got %r, %r, %r, %r"
                         % (iters, c_min_px, t_min_px, min_share))
    work = _ego_work(F, H, W, flow.device, work)
    if R0 is None:
        R0 = rotation_fit(flow, iters, c_min_px, work=work)[0]
    _stab_rotations(R0, F)
    if R0.device != flow.device:
        raise ValueError("R0 must be on the flow's device")
    R = torch.empty((F, 3, 3), dtype=torch.float32, device=flow.device)
    e = torch.empty((F, 3), dtype=torch.float32, device=flow.device)
    diag = torch.empty((F, 8), dtype=torch.float64, device=flow.device)
    check(lib().cp360_ego_fit(ptr(flow), ptr(R0), F, H, W, int(iters), float(c_min_px), float(t_min_px), float(min_share), ptr(R),
                              ptr(e), ptr(diag), ptr(work), work.numel() * 8, stream()))
    return R, e, diag


def egomotion_residual(flow, R, e, out=None, want_mag=False, work=None):
    """cp360_ego_residual: flow f32 [F, H, W, 2], R f32 [F, 3, 3], e f32 [F, 3] (unit, or exactly 0: ``egomotion_fit``'s) -> res
    f32 [F, H, W, 2], the part of the flow that the camera motion (R, e) and a static scene cannot explain at any depth, a flow
    in K10's pixels (e = 0: the de-rotated flow); with want_mag also mag f32 [F, H, W], its size in equator pixels.  A non-finite
    flow value gives NaN in its pixel."""
    require_gpu(flow, R, e, out, work)
    F, H, W = _ego_flow(flow)
    _stab_rotations(R, F)
    if e.dim() != 2 or tuple(e.shape) != (F, 3):
        raise ValueError("e must be [%d, 3], got %s" % (F, tuple(e.shape)))
    _check_buf('e', e, torch.float32)
    if R.device != flow.device or e.device != flow.device:
        raise ValueError("R and e must be on the flow's device")
    out = _out_for(out, (F, H, W, 2), torch.float32, flow.device, flow)
    mag = torch.empty((F, H, W), dtype=torch.float32, device=flow.device) if want_mag else None
    work = _ego_work(0, H, W, flow.device, work)
    check(lib().cp360_ego_residual(ptr(flow), ptr(R), ptr(e), F, H, W, ptr(out), ptr(mag), ptr(work), work.numel() * 8, stream()))
    return (out, mag) if want_mag else out


# ----------------------------------------------------------------------------- K12: the viewport pilot (csrc/viewport.hip)
def _view_geometry(hw, hfov_deg):
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1 or not 0.0 < float(hfov_deg) < 180.0:
        raise ValueError("a view needs h, w >= 1 and 0 < hfov_deg < 180, got %r, %r" % (hw, hfov_deg))
    return h, w, math.radians(float(hfov_deg))


def _supersample(supersample, K=None):
    """K21's factor(s): one int 1 .. 4 - or, for the K tiles of a canvas, one per tile - as a list of ints; ValueError otherwise."""
    many = K is not None and np.ndim(supersample) != 0
    ss = list(supersample) if many else [supersample] * (K or 1)
    if len(ss) != (K or 1) or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 1 <= v <= 4 for v in ss):
        raise ValueError("supersample must be an int 1 .. 4%s, got %r" % (" or one per tile" if K is not None else "", supersample))
    return [int(v) for v in ss]


def viewport_render(frames, R, hw, hfov_deg, out=None, supersample=1):
    """cp360_view_render: the perspective view of hw = (h, w) pixels and hfov_deg degrees of every frame under its camera R[n]
    (f32 [N, 3, 3], camera-to-world, columns forward / up / right; I looks at the panorama's centre): frames u8 [N, H, W, 3] or
    f32 [N, H, W, C], C <= 4 -> [N, h, w, C] of the frames' type.  Bilinear, columns wrap, rows clamp.  ``supersample`` = n in
    2 .. 4 (cp360_view_render_aa, K21): every pixel is the mean of the n x n unrounded samples of the view (n h, n w), added in
    f32 row by row - anti-aliased for up to n source pixels per view pixel (``utils.viewport.supersample_for``); 1: no
    anti-aliasing, today's call."""
    ss = _supersample(supersample)[0]
    h, w, hfov = _view_geometry(hw, hfov_deg)
    N, H, W, C_, out = _render_args(frames, R, h, w, out)
    if ss == 1:
        check(lib().cp360_view_render(dtype_code(frames.dtype), ptr(frames), ptr(R), N, H, W, C_, hfov, ptr(out), h, w, stream()))
    else:
        check(lib().cp360_view_render_aa(dtype_code(frames.dtype), ptr(frames), ptr(R), N, H, W, C_, hfov, ss, ptr(out), h, w,
                                         stream()))
    return out


def viewport_outline(frames, R, hw, hfov_deg, border_px=3, rgb=(0, 255, 0), out=None, work=None):
    """cp360_view_outline: the frame of the view (hw, hfov_deg) of camera R[n], border_px view pixels wide, drawn in rgb on the
    panorama: frames u8 [N, H, W, 3] -> u8 [N, H, W, 3]; out may be frames (every other pixel is copied)."""
    h, w, hfov = _view_geometry(hw, hfov_deg)
    rgb = tuple(int(v) for v in rgb)
    if not float(border_px) > 0.0 or len(rgb) != 3 or min(rgb) < 0 or max(rgb) > 255:
        raise ValueError("border_px must be positive and rgb three values of 0 .. 255, got %r, %r" % (border_px, rgb))
    N, H, W, out, work, colour = _outline_args(frames, R, rgb, out, work)
    check(lib().cp360_view_outline(ptr(frames), ptr(R), N, H, W, hfov, h, w, float(border_px), colour, ptr(out), ptr(work),
                                   work.numel() * 8, stream()))
    return out


def _view_maps(maps, sigma_deg):
    F, hm, wm = _map_shape(maps, ' (all pairs)')
    if not float(sigma_deg) > 0.0 or not math.isfinite(float(sigma_deg)):
        raise ValueError("sigma_deg must be positive, got %r" % (sigma_deg,))
    return F, hm, wm, math.radians(float(sigma_deg))


def sphere_smooth(maps, sigma_deg=15.0, work=None):
    """cp360_view_smooth: maps f32 [F, hm, wm] smoothed on the sphere with a von Mises-Fisher kernel of sigma_deg degrees
    (kappa = 1 / sigma^2), weighted by solid angle and normalised; non-finite values count as 0."""
    require_gpu(maps)
    F, hm, wm, sigma = _view_maps(maps, sigma_deg)
    work = _stab_work(0, hm, wm, maps.device, work)
    out = torch.empty_like(maps)
    check(lib().cp360_view_smooth(ptr(maps), F, hm, wm, sigma, ptr(out), ptr(work), work.numel() * 8, stream()))
    return out


def sphere_peak(maps, sigma_deg=15.0, smooth=None, work=None):
    """cp360_view_peak: maps f32 [F, hm, wm] -> (dirs f32 [F, 3], idx i32 [F], val f32 [F]): the argmax of the smoothed map
    (``smooth``, default ``sphere_smooth(maps, sigma_deg)``; lowest index on ties), its value, and the unit direction after one
    mean-shift step on the raw map.  A frame with no finite value: idx -1, dir (1, 0, 0), val NaN."""
    require_gpu(maps, smooth)
    F, hm, wm, sigma = _view_maps(maps, sigma_deg)
    work = _stab_work(0, hm, wm, maps.device, work)
    if smooth is None:
        smooth = sphere_smooth(maps, sigma_deg, work=work)
    elif smooth.shape != maps.shape or smooth.device != maps.device:
        raise ValueError("smooth must have the maps' shape on their device")
    _check_buf('smooth', smooth, torch.float32)
    dirs = torch.empty((F, 3), dtype=torch.float32, device=maps.device)
    idx = torch.empty((F,), dtype=torch.int32, device=maps.device)
    val = torch.empty((F,), dtype=torch.float32, device=maps.device)
    check(lib().cp360_view_peak(ptr(smooth), ptr(maps), F, hm, wm, sigma, ptr(dirs), ptr(idx), ptr(val), ptr(work),
                                work.numel() * 8, stream()))
    return dirs, idx, val


# ----------------------------------------------------------------------------- K16: the camera path (csrc/viewport.hip)
_PATH_TABLES = {}


def _path_params(hm, wm, turn_cost, step_deg):
    hm, wm, turn_cost, step_deg = int(hm), int(wm), float(turn_cost), float(step_deg)
    if hm < 1 or wm < 1 or hm * wm > 16384:
        raise ValueError("a path needs a map of 1 .. 16384 pixels, got %d x %d" % (hm, wm))
    if not 0.0 <= turn_cost <= 4096.0 or not 0.0 < step_deg <= 180.0:
        raise ValueError("turn_cost must be in [0, 4096] and step_deg in (0, 180], got %r, %r" % (turn_cost, step_deg))
    if step_deg < 180.0 / hm:
        raise ValueError("step_deg %g is below the map's row pitch of %g degrees: no move is ever allowed" % (step_deg, 180.0 / hm))
    return hm, wm, turn_cost, step_deg


def path_table_host(hm, wm, turn_cost, step_deg):
    """cp360_path_table_host: the turn costs of an hm x wm map as one int32 numpy array, cost [hm, hm, wm // 2 + 1] by (row of i,
    row of j, folded column difference) = rint(turn_cost * angle in degrees), -1 where the angle exceeds step_deg, and behind it
    span [hm, hm], the largest allowed column difference (``path_table_split`` gives the two views).  Host only: needs no GPU."""
    hm, wm, turn_cost, step_deg = _path_params(hm, wm, turn_cost, step_deg)
    out = np.empty(lib().cp360_path_table_bytes(hm, wm) // 4, np.int32)
    check(lib().cp360_path_table_host(hm, wm, turn_cost, math.radians(step_deg), out.ctypes.data_as(C.c_void_p)))
    return out


def path_table_split(table, hm, wm):
    """A table of ``path_table_host`` -> (cost [hm, hm, wm // 2 + 1], span [hm, hm]), views of it."""
    n = hm * hm * (wm // 2 + 1)
    return table[:n].reshape(hm, hm, wm // 2 + 1), table[n:].reshape(hm, hm)


def path_table(hm, wm, turn_cost, step_deg, device):
    """The table on `device`, uploaded once per (hm, wm, turn_cost, step_deg, device)."""
    key = _path_params(hm, wm, turn_cost, step_deg) + (torch.device(device),)
    if key not in _PATH_TABLES:
        _PATH_TABLES[key] = torch.from_numpy(path_table_host(*key[:4])).to(key[4])
    return _PATH_TABLES[key]


def sphere_path(smooth, gain, turn_cost=16.0, step_deg=15.0, starts=None, work=None):
    """cp360_view_path: the path over the pixels of smooth f32 [F, hm, wm] that collects the most votes q = rint(clamp(smooth *
    gain[t], 0, 4096)) (gain f32 [F]) minus turn_cost per degree turned, turning at most step_deg a frame -> (idx i32 [F], dirs
    f32 [F, 3] = the pixel centres, score i32 [S]).  ``starts`` i32 [S + 1] on the device (ascending, from 0 to F) cuts the video
    into S independent sequences; None: one.  Exact integers: bit-identical between runs."""
    require_gpu(smooth, gain, starts, work)
    if smooth.dim() != 3 or smooth.numel() == 0:
        raise ValueError("smooth must be a non-empty float32 [F, hm, wm], got %s" % (tuple(smooth.shape),))
    _check_buf('smooth', smooth, torch.float32)
    F, hm, wm = (int(s) for s in smooth.shape)
    hm, wm, turn_cost, step_deg = _path_params(hm, wm, turn_cost, step_deg)
    if tuple(gain.shape) != (F,) or gain.device != smooth.device:
        raise ValueError("gain must be float32 [%d] on the maps' device" % F)
    _check_buf('gain', gain, torch.float32)
    if starts is None:
        starts = torch.tensor([0, F], dtype=torch.int32, device=smooth.device)
    elif starts.dim() != 1 or not 2 <= starts.numel() <= F + 1 or starts.device != smooth.device:
        raise ValueError("starts must be int32 [S + 1] with 1 <= S <= %d on the maps' device" % F)
    _check_buf('starts', starts, torch.int32)
    S = starts.numel() - 1
    table = path_table(hm, wm, turn_cost, step_deg, smooth.device)
    work = _work(lib().cp360_path_work_bytes, "sphere_path", F, hm, wm, smooth.device, work, " (F <= 65535, hm wm <= 16384)")
    idx = torch.empty((F,), dtype=torch.int32, device=smooth.device)
    dirs = torch.empty((F, 3), dtype=torch.float32, device=smooth.device)
    score = torch.empty((S,), dtype=torch.int32, device=smooth.device)
    check(lib().cp360_view_path(ptr(smooth), ptr(gain), F, hm, wm, ptr(table), ptr(starts), S, ptr(idx), ptr(dirs), ptr(score),
                                ptr(work), work.numel() * 8, stream()))
    return idx, dirs, score


def sphere_refine(maps, idx, sigma_deg=15.0, work=None):
    """cp360_view_refine: ``sphere_peak``'s mean-shift step on the raw maps f32 [F, hm, wm] about the pixels idx i32 [F] -> dirs
    f32 [F, 3]; with ``sphere_peak``'s idx, its dirs bit for bit.  idx < 0: (1, 0, 0)."""
    require_gpu(maps, idx, work)
    F, hm, wm, sigma = _view_maps(maps, sigma_deg)
    if tuple(idx.shape) != (F,) or idx.device != maps.device:
        raise ValueError("idx must be int32 [%d] on the maps' device" % F)
    _check_buf('idx', idx, torch.int32)
    work = _stab_work(0, hm, wm, maps.device, work)
    dirs = torch.empty((F, 3), dtype=torch.float32, device=maps.device)
    check(lib().cp360_view_refine(ptr(maps), ptr(idx), F, hm, wm, sigma, ptr(dirs), ptr(work), work.numel() * 8, stream()))
    return dirs


# ----------------------------------------------------------------------------- K20: several cameras at once (csrc/viewport.hip)
def sphere_exclude(maps, dirs, radius_deg, out=None, work=None):
    """cp360_view_exclude: maps f32 [F, hm, wm] with the caps of radius_deg degrees about the directions dirs f32 [F, Kx, 3]
    (1 <= Kx <= 7) set to +0: a pixel goes where the f32 dot of its centre with any direction of its frame is at least
    cos(radius_deg); every other pixel keeps its bits.  A direction with a non-finite component excludes nothing.  out may be
    maps."""
    F, hm, wm = _map_shape(maps)
    if dirs.dim() != 3 or dirs.shape[0] != maps.shape[0] or not 1 <= dirs.shape[1] <= 7 or dirs.shape[2] != 3:
        raise ValueError("dirs must be float32 [%d, Kx, 3] with 1 <= Kx <= 7, got %s" % (maps.shape[0], tuple(dirs.shape)))
    if not 0.0 < float(radius_deg) <= 180.0:
        raise ValueError("radius_deg must be in (0, 180], got %r" % (radius_deg,))
    require_gpu(maps, dirs, out, work)
    if dirs.device != maps.device:
        raise ValueError("dirs must be on the maps' device")
    _check_buf('dirs', dirs, torch.float32)
    out = _out_for(out, maps.shape, torch.float32, maps.device, maps, same_ok=True)
    work = _stab_work(0, hm, wm, maps.device, work)
    check(lib().cp360_view_exclude(ptr(maps), ptr(dirs), F, hm, wm, int(dirs.shape[1]), math.radians(float(radius_deg)), ptr(out),
                                   ptr(work), work.numel() * 8, stream()))
    return out


def check_tiles(tiles, canvas_hw):
    """The tiles of a canvas: K rectangles (x0, y0, w, h), 1 <= K <= 8, none empty, all on the canvas of canvas_hw = (hc, wc),
    no two sharing a pixel -> ([(x0, y0, w, h)] as ints, (hc, wc)); ValueError otherwise."""
    hc, wc = (int(v) for v in canvas_hw)
    tiles = [tuple(int(v) for v in t) for t in tiles]
    if hc < 1 or wc < 1 or not 1 <= len(tiles) <= 8 or any(len(t) != 4 for t in tiles):
        raise ValueError("a canvas needs hc, wc >= 1 and 1 .. 8 tiles (x0, y0, w, h), got %r, %r" % (canvas_hw, tiles))
    for k, (x0, y0, w, h) in enumerate(tiles):
        if w < 1 or h < 1:
            raise ValueError("tile %d is empty: %r" % (k, tiles[k]))
        if x0 < 0 or y0 < 0 or x0 + w > wc or y0 + h > hc:
            raise ValueError("tile %d %r leaves the canvas of %d x %d" % (k, tiles[k], hc, wc))
        for m, (mx, my, mw, mh) in enumerate(tiles[:k]):
            if x0 < mx + mw and mx < x0 + w and y0 < my + mh and my < y0 + h:
                raise ValueError("tiles %d and %d overlap: %r, %r" % (m, k, tiles[m], tiles[k]))
    return tiles, (hc, wc)


def viewport_render_multi(frames, R, tiles, hfov_deg, canvas_hw, fill=None, out=None, supersample=1):
    """cp360_view_render_multi: K views of every frame on one canvas in one launch.  frames as ``viewport_render``'s, R f32
    [N, K, 3, 3], tiles K rectangles (x0, y0, w, h) on the canvas of canvas_hw = (hc, wc), hfov_deg a scalar or one value per
    tile -> [N, hc, wc, C] of the frames' type.  Tile k is ``viewport_render(frames, R[:, k], (h, w), hfov_deg[k])`` bit for bit;
    a pixel in no tile, and the tile of a camera with a non-finite entry, take fill (C values, default 0).  ``supersample``: one
    factor 1 .. 4 or one per tile (cp360_view_render_multi_aa, K21): tile k is ``viewport_render(.., supersample=s_k)`` bit for
    bit; all 1: today's call."""
    tiles, (hc, wc) = check_tiles(tiles, canvas_hw)
    ss = _supersample(supersample, len(tiles))
    require_gpu(frames, R, out)
    N, H, W, C_ = _frames_nhwc(frames, u8_only=False)
    K = len(tiles)
    if R.dim() != 4 or tuple(R.shape) != (N, K, 3, 3):
        raise ValueError("R must be [%d, %d, 3, 3], got %s" % (N, K, tuple(R.shape)))
    _check_buf('R', R, torch.float32)
    hfov = [float(hfov_deg)] * K if np.ndim(hfov_deg) == 0 else [float(v) for v in hfov_deg]
    if len(hfov) != K or not all(0.0 < v < 180.0 for v in hfov):
        raise ValueError("hfov_deg must be one value or one per tile, each in (0, 180), got %r" % (hfov_deg,))
    u8 = frames.dtype == torch.uint8
    fill = [0] * C_ if fill is None else list(fill)
    if len(fill) != C_ or (u8 and any(int(v) != v or not 0 <= v <= 255 for v in fill)):
        raise ValueError("fill must be %d values of the frames' type, got %r" % (C_, fill))
    out = _out_for(out, (N, hc, wc, C_), frames.dtype, frames.device, frames)
    rects = (C.c_int32 * (4 * K))(*[v for t in tiles for v in t])
    fovs = (C.c_double * K)(*[math.radians(v) for v in hfov])
    colour = (C.c_ubyte * C_)(*[int(v) for v in fill]) if u8 else (C.c_float * C_)(*[float(v) for v in fill])
    if all(v == 1 for v in ss):
        check(lib().cp360_view_render_multi(dtype_code(frames.dtype), ptr(frames), ptr(R), N, H, W, C_, K, C.cast(rects, C.c_void_p),
                                            C.cast(fovs, C.c_void_p), C.cast(colour, C.c_void_p), ptr(out), hc, wc, stream()))
    else:
        factors = (C.c_int32 * K)(*ss)
        check(lib().cp360_view_render_multi_aa(dtype_code(frames.dtype), ptr(frames), ptr(R), N, H, W, C_, K,
                                               C.cast(rects, C.c_void_p), C.cast(fovs, C.c_void_p), C.cast(factors, C.c_void_p),
                                               C.cast(colour, C.c_void_p), ptr(out), hc, wc, stream()))
    return out


# ----------------------------------------------------------------------------- K22: zoom, a lens per frame (csrc/viewport.hip)
def viewport_lens_host(hfov_deg, hw, border_px=0.0, n=None):
    """cp360_view_lens_host: the lenses of views of hw = (h, w) pixels as a float32 numpy [N, 4] = (tx, ty, b, 0) per frame, tx =
    tan(hfov / 2), ty = tx h / w, b = border_px 2 tx / w, each formed in double and rounded once - the values ``viewport_render``
    and ``viewport_outline`` hand their kernels.  hfov_deg: N values in degrees, or a scalar repeated ``n`` times (default 1).
    Host only: needs no GPU."""
    h, w = (int(v) for v in hw)
    fov = np.asarray(hfov_deg, np.float64)
    if fov.ndim == 0:
        fov = np.full(1 if n is None else int(n), float(fov))
    if fov.ndim != 1 or fov.size < 1 or (n is not None and fov.size != int(n)):
        raise ValueError("hfov_deg must be a scalar or %s values, got shape %s" % ('N' if n is None else int(n), fov.shape))
    if h < 1 or w < 1 or not all(0.0 < v < 180.0 for v in fov) or not (float(border_px) >= 0.0 and math.isfinite(float(border_px))):
        raise ValueError("a lens needs h, w >= 1, 0 < hfov_deg < 180 and a finite border_px >= 0, got %r, %r, %r"
                         % (hw, hfov_deg, border_px))
    rad = (C.c_double * fov.size)(*[math.radians(float(v)) for v in fov])
    out = np.empty((fov.size, 4), np.float32)
    check(lib().cp360_view_lens_host(C.cast(rad, C.c_void_p), int(fov.size), h, w, float(border_px), out.ctypes.data_as(C.c_void_p)))
    return out


def viewport_lens(hfov_deg, hw, border_px=0.0, device='cuda', n=None):
    """``viewport_lens_host`` on `device`: f32 [N, 4], what the ``_zoom`` ops take."""
    return torch.from_numpy(viewport_lens_host(hfov_deg, hw, border_px, n)).to(device)


def _lens(lens, N, device, name='lens'):
    if lens.dim() != 2 or tuple(lens.shape) != (N, 4) or lens.device != device:
        raise ValueError("%s must be float32 [%d, 4] on the frames' device (viewport_lens), got %s" % (name, N, tuple(lens.shape)))
    _check_buf(name, lens, torch.float32)
    if lens.data_ptr() % 16:
        raise ValueError("%s must be 16-byte aligned" % name)


def viewport_render_zoom(frames, R, hw, lens, out=None, supersample=None):
    """cp360_view_render_zoom: ``viewport_render`` with a lens per frame (``viewport_lens``, f32 [N, 4]) in one launch: frame n is
    ``viewport_render(frames[n:n + 1], R[n:n + 1], hw, hfov_n, supersample=ss_n)`` bit for bit.  ``supersample``: None (one
    sample per pixel), or int32 [N] on the device, a factor per frame; a value outside 2 .. 4 renders as 1."""
    if supersample is not None and not torch.is_tensor(supersample):
        raise ValueError("supersample must be None or an int32 tensor [N] on the frames' device, got %r" % (supersample,))
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1:
        raise ValueError("a view needs h, w >= 1, got %r" % (hw,))
    N, H, W, C_, out = _render_args(frames, R, h, w, out, lens, supersample)
    _lens(lens, N, frames.device)
    if supersample is not None:
        if tuple(supersample.shape) != (N,) or supersample.device != frames.device:
            raise ValueError("supersample must be None or int32 [%d] on the frames' device" % N)
        _check_buf('supersample', supersample, torch.int32)
    check(lib().cp360_view_render_zoom(dtype_code(frames.dtype), ptr(frames), ptr(R), ptr(lens), ptr(supersample), N, H, W, C_,
                                       ptr(out), h, w, stream()))
    return out


def viewport_outline_zoom(frames, R, lens, rgb=(0, 255, 0), out=None, work=None):
    """cp360_view_outline_zoom: ``viewport_outline`` with a lens per frame (``viewport_lens(hfov_deg, hw, border_px)``): frame n is
    ``viewport_outline`` with that frame's field of view and border, bit for bit; a frame whose b is not above 0 draws nothing.
    out may be frames."""
    N, H, W, out, work, colour = _outline_args(frames, R, rgb, out, work, lens)
    _lens(lens, N, frames.device)
    check(lib().cp360_view_outline_zoom(ptr(frames), ptr(R), ptr(lens), N, H, W, colour, ptr(out), ptr(work), work.numel() * 8,
                                        stream()))
    return out


def sphere_spread(maps, dirs, window_deg=45.0, level=0.5, work=None):
    """cp360_view_spread: how wide the target about dirs f32 [F, 3] (``sphere_peak``'s or ``sphere_refine``'s) is on maps f32
    [F, hm, wm] -> q f32 [F]: the mean of 1 - cos(angle to dirs[f]), weighted by solid angle times the map's excess over ``level``
    times its peak, both inside the cap of window_deg degrees about dirs[f].  For a Gaussian blob of width sigma_b that is narrow
    against the cap q = ``utils.viewport.spread_constant(level)`` sigma_b^2.  NaN for a non-finite direction, a cap without a
    finite pixel or a peak that is not positive."""
    require_gpu(maps, dirs, work)
    F, hm, wm = _map_shape(maps)
    if tuple(dirs.shape) != (F, 3) or dirs.device != maps.device:
        raise ValueError("dirs must be float32 [%d, 3] on the maps' device, got %s" % (F, tuple(dirs.shape)))
    _check_buf('dirs', dirs, torch.float32)
    if not 0.0 < float(window_deg) <= 180.0 or not 0.0 < float(level) < 1.0:
        raise ValueError("window_deg must be in (0, 180] and level in (0, 1), got %r, %r" % (window_deg, level))
    work = _stab_work(0, hm, wm, maps.device, work)
    q = torch.empty((F,), dtype=torch.float32, device=maps.device)
    check(lib().cp360_view_spread(ptr(maps), ptr(dirs), F, hm, wm, math.radians(float(window_deg)), float(level), ptr(q), ptr(work),
                                  work.numel() * 8, stream()))
    return q


# ----------------------------------------------------------------------------- K13: shot detection (csrc/shots.hip)
_SHOT_WEIGHTS = {}


def shot_weights_host(H):
    """cp360_shot_weights_host: (a int32 numpy [H], sum_y a_y): a_y = floor(cos(phi_y) 1024 + 1/2), the solid-angle weight of row
    y of an H-row equirectangular image.  Host only: needs no GPU."""
    H = int(H)
    if H < 1:
        raise ValueError("H must be at least 1, got %d" % H)
    a = np.empty(H, np.int32)
    total = C.c_longlong(0)
    check(lib().cp360_shot_weights_host(H, a.ctypes.data_as(C.c_void_p), C.cast(C.byref(total), C.c_void_p)))
    return a, int(total.value)


def shot_weights(H, device):
    """The weight table of H rows on `device`, uploaded once per (H, device)."""
    key = (int(H), torch.device(device))
    if key not in _SHOT_WEIGHTS:
        _SHOT_WEIGHTS[key] = torch.from_numpy(shot_weights_host(H)[0]).to(key[1])
    return _SHOT_WEIGHTS[key]


def _shot_work(F, H, W, device, work=None):
    """The workspace of one cp360_shot_signatures call: `work` when it is large enough, else a new one."""
    return _work(lib().cp360_shot_work_bytes, "shot signatures", F, H, W, device, work)


def shot_signatures(frames, work=None, weights=None):
    """cp360_shot_signatures: frames u8 [F, H, W, 3] (contiguous; a slice may start at any byte) -> sig int64 [F, 3, 64] on the
    device: sig[f, c, b] = the sum of the row weights a_y over the pixels with frames[f, y, x, c] >> 2 == b.  Exact integers:
    bit-identical between runs and batch sizes."""
    require_gpu(frames, work, weights)
    F, H, W, _ = _frames_nhwc(frames, u8_only=True, n='F')
    if weights is None:
        weights = shot_weights(H, frames.device)
    elif tuple(weights.shape) != (H,) or weights.device != frames.device:
        raise ValueError("weights must be int32 [%d] on the frames' device" % H)
    _check_buf('weights', weights, torch.int32)
    work = _shot_work(F, H, W, frames.device, work)
    sig = torch.empty((F, 3, 64), dtype=torch.int64, device=frames.device)
    check(lib().cp360_shot_signatures(ptr(frames), F, H, W, ptr(weights), ptr(sig), ptr(work), work.numel() * 8, stream()))
    return sig


def shot_distances(sig):
    """sig int64 [F, 3, 64] -> (sad int64 [F - 1], T int64 scalar), both on sig's device, without a synchronisation:
    sad_t = sum_{c, b} |sig_t - sig_t+1| and T = the sum of one channel's histogram; d_t = sad_t / (6 T) lies in [0, 1]."""
    if sig.dim() != 3 or tuple(sig.shape[1:]) != (3, 64) or sig.shape[0] < 1 or sig.dtype != torch.int64:
        raise ValueError("sig must be int64 [F, 3, 64] with F >= 1, got %s %s" % (sig.dtype, tuple(sig.shape)))
    sad = (sig[1:] - sig[:-1]).abs().sum(dim=(1, 2))
    return sad, sig[0, 0].sum()


# ----------------------------------------------------------------------------- K14: metrics on the sphere (csrc/sphere_eval.hip)
_EVAL_WEIGHTS = {}


def sphere_eval_weights(h, mode, device):
    """The int32 [h] row weights of an h-row evaluation grid on `device`: K13's solid-angle table ('solid_angle') or 1024 in every
    row ('uniform', a flat grid).  Uploaded once per (h, mode, device)."""
    if mode not in ('solid_angle', 'uniform'):
        raise ValueError("weights must be 'solid_angle' or 'uniform', got %r" % (mode,))
    key = (int(h), mode, torch.device(device))
    if key not in _EVAL_WEIGHTS:
        a = shot_weights_host(h)[0] if mode == 'solid_angle' else np.full(int(h), 1024, np.int32)
        _EVAL_WEIGHTS[key] = torch.from_numpy(a).to(key[2])
    return _EVAL_WEIGHTS[key]


def _eval_maps(name, t):
    if t.dim() != 3 or t.numel() == 0:
        raise ValueError("%s must be a non-empty float32 [F, h, w], got %s" % (name, tuple(t.shape)))
    _check_buf(name, t, torch.float32)
    return tuple(int(s) for s in t.shape)


def sphere_eval_work(F, h, w, device, work=None):
    """The workspace of one cp360_seval_scores call: `work` when it is large enough, else a new one."""
    return _work(lib().cp360_seval_work_bytes, "sphere_eval", F, h, w, device, work, " (F <= 65535, h w <= 2^21)")


def sphere_eval_resample(maps, hw, out=None):
    """cp360_seval_resample: maps f32 [F, hs, ws] -> f32 [F, h, w], bilinear on the sphere's pixel centres (columns wrap, rows
    clamp, no anti-aliasing); maps that are already h x w are copied bit for bit."""
    require_gpu(maps, out)
    F, hs, ws = _eval_maps('maps', maps)
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1:
        raise ValueError("the grid must be at least 1 x 1, got %d x %d" % (h, w))
    if out is None:
        out = torch.empty((F, h, w), dtype=torch.float32, device=maps.device)
    elif tuple(out.shape) != (F, h, w) or out.device != maps.device:
        raise ValueError("out must be float32 [%d, %d, %d] on the maps' device" % (F, h, w))
    _check_buf('out', out, torch.float32)
    check(lib().cp360_seval_resample(ptr(maps), F, hs, ws, ptr(out), h, w, stream()))
    return out


# ----------------------------------------------------------------------------- K25: the conservative remap (csrc/sphere_resample.hip)
RESAMPLERS = ('bilinear', 'conservative')
_RESAMPLE_PLANS = {}


def check_resampler(resample):
    """The ``resample=`` argument of the consumers: 'bilinear' (``sphere_eval_resample``, the default everywhere) or
    'conservative' (``sphere_resample``); ValueError otherwise."""
    if resample not in RESAMPLERS:
        raise ValueError("resample must be 'bilinear' or 'conservative', got %r" % (resample,))
    return resample


def resample_maps(maps, hw, resample='bilinear'):
    """maps f32 [F, hs, ws] on the GPU -> f32 [F, h, w] by the named resampler: what the consumers call."""
    if check_resampler(resample) == 'conservative':
        return sphere_resample(maps, hw)
    return sphere_eval_resample(maps, hw)


def _resample_shapes(src_hw, hw):
    hs, ws = (int(v) for v in src_hw)
    h, w = (int(v) for v in hw)
    if hs < 1 or ws < 1 or h < 1 or w < 1:
        raise ValueError("the source and the grid must be at least 1 x 1, got %d x %d and %d x %d" % (hs, ws, h, w))
    return hs, ws, h, w


def sphere_resample_tables_host(n_src, n_dst, axis):
    """cp360_sresample_axis_host: the runs and weights of one axis (0: rows, 1: columns) of the conservative remap from n_src to
    n_dst pixels -> (start int32 [n_dst], count int32 [n_dst], weights float32 [n_dst, R]) as numpy arrays, the weights
    zero-padded to the pair's run cap R.  Where the source is not finer the run is ``sphere_sample``'s two taps: start = i0, the
    second index start + 1 wrapped (columns) or clamped (rows).  Host only: needs no GPU."""
    n_src, n_dst, axis = int(n_src), int(n_dst), int(axis)
    R = lib().cp360_sresample_run_cap(n_src, n_dst)
    if R < 1 or axis not in (0, 1):
        raise ValueError("n_src, n_dst must be at least 1 and axis 0 or 1, got %d, %d, %d" % (n_src, n_dst, axis))
    if R > 256:
        raise ValueError("a run of up to %d source pixels per grid pixel is not supported (at most 256)" % R)
    start, count = np.empty(n_dst, np.int32), np.empty(n_dst, np.int32)
    weights = np.empty((n_dst, R), np.float32)
    check(lib().cp360_sresample_axis_host(n_src, n_dst, axis, start.ctypes.data_as(C.c_void_p), count.ctypes.data_as(C.c_void_p),
                                          weights.ctypes.data_as(C.c_void_p)))
    return start, count, weights


def sphere_resample_plan(src_hw, hw, device):
    """The tables of the conservative remap from src_hw to hw on `device` (a uint8 tensor, cp360_sresample_plan_host's layout):
    made on the host in float64 and uploaded once per (src_hw, hw, device)."""
    hs, ws, h, w = _resample_shapes(src_hw, hw)
    device = torch.device(device)
    if device.type != 'cuda':
        raise RuntimeError("cp360 ops run on the GPU only (HIP); got the device %s - there is no CPU fallback" % device)
    key = (hs, ws, h, w, device)
    if key not in _RESAMPLE_PLANS:
        n = int(lib().cp360_sresample_plan_bytes(hs, ws, h, w))
        if n == 0:
            raise ValueError("a conservative remap from %d x %d to %d x %d is not supported (h w <= 2^21, hs <= 65535, hs ws <= "
                             "2^28, at most 256 source rows or columns per grid pixel)" % (hs, ws, h, w))
        host = np.zeros(n // 8 + 2, np.int64)                          # 16-byte aligned: the first or the second word
        off = (-host.ctypes.data) % 16
        buf = host.view(np.uint8)[off:off + n]
        check(lib().cp360_sresample_plan_host(hs, ws, h, w, buf.ctypes.data_as(C.c_void_p), n))
        _RESAMPLE_PLANS[key] = torch.from_numpy(buf.copy()).to(device)
    return _RESAMPLE_PLANS[key]


def _resample_plan(plan, hs, ws, h, w, device):
    if plan is None:
        return sphere_resample_plan((hs, ws), (h, w), device)
    require_gpu(plan)
    need = int(lib().cp360_sresample_plan_bytes(hs, ws, h, w))
    if plan.device != device or plan.dim() != 1 or need == 0 or plan.numel() != need:
        raise ValueError("plan must be sphere_resample_plan((%d, %d), (%d, %d)) on the maps' device" % (hs, ws, h, w))
    _check_buf('plan', plan, torch.uint8)
    return plan


def sphere_resample(maps, hw, plan=None, out=None):
    """cp360_sresample_forward: maps f32 [F, hs, ws] (F = 0 is valid) -> f32 [F, h, w], the conservative remap on the sphere: a
    grid pixel is the solid-angle-weighted mean of the source pixels it overlaps on every axis on which the source is finer, and
    ``sphere_eval_resample``'s two taps on the others (neither finer: its bits).  One fixed order: a frame's numbers depend
    neither on F nor on its place in the batch."""
    require_gpu(maps, out, plan)
    if maps.dim() != 3 or maps.shape[1] < 1 or maps.shape[2] < 1:
        raise ValueError("maps must be float32 [F, hs, ws], got %s" % (tuple(maps.shape),))
    _check_buf('maps', maps, torch.float32)
    F = int(maps.shape[0])
    hs, ws, h, w = _resample_shapes(maps.shape[1:], hw)
    plan = _resample_plan(plan, hs, ws, h, w, maps.device)
    if out is None:
        out = torch.empty((F, h, w), dtype=torch.float32, device=maps.device)
    elif tuple(out.shape) != (F, h, w) or out.device != maps.device:
        raise ValueError("out must be float32 [%d, %d, %d] on the maps' device" % (F, h, w))
    _check_buf('out', out, torch.float32)
    check(lib().cp360_sresample_forward(ptr(maps), F, hs, ws, ptr(out), h, w, ptr(plan), plan.numel(), stream()))
    return out


def sphere_resample_adjoint(d_out, src_hw, plan=None):
    """cp360_sresample_adjoint: d_out f32 [F, h, w] -> f32 [F, hs, ws], the transpose of ``sphere_resample`` from src_hw to d_out's
    grid, gathered per source pixel in float64 and rounded once."""
    require_gpu(d_out, plan)
    if d_out.dim() != 3 or d_out.shape[1] < 1 or d_out.shape[2] < 1:
        raise ValueError("d_out must be float32 [F, h, w], got %s" % (tuple(d_out.shape),))
    _check_buf('d_out', d_out, torch.float32)
    F = int(d_out.shape[0])
    hs, ws, h, w = _resample_shapes(src_hw, d_out.shape[1:])
    plan = _resample_plan(plan, hs, ws, h, w, d_out.device)
    d_src = torch.empty((F, hs, ws), dtype=torch.float32, device=d_out.device)
    check(lib().cp360_sresample_adjoint(ptr(d_out), F, h, w, ptr(d_src), hs, ws, ptr(plan), plan.numel(), stream()))
    return d_src


def sphere_eval(S, G, weights, fixations=None, work=None):
    """cp360_seval_scores: S, G f32 [F, h, w] on the evaluation grid, weights int32 [h] (``sphere_eval_weights``), fixations u8 /
    bool [F, h, w] or None (the rule G > mean + 2 std, weighted) -> (scores f64 [F, 5] = (auc, nss, cc, sim, kl), n_fix int32
    [F]), both on the device, without a synchronisation.  A frame's numbers do not depend on F or on its place in the batch."""
    require_gpu(S, G, weights, fixations, work)
    F, h, w = _eval_maps('S', S)
    if _eval_maps('G', G) != (F, h, w) or G.device != S.device:
        raise ValueError("G must have S's shape %s on its device, got %s" % ((F, h, w), tuple(G.shape)))
    if tuple(weights.shape) != (h,) or weights.device != S.device:
        raise ValueError("weights must be int32 [%d] on the maps' device" % h)
    _check_buf('weights', weights, torch.int32)
    if fixations is not None:
        if fixations.dtype not in (torch.uint8, torch.bool):
            raise ValueError("fixations must be uint8 or bool, got %s" % fixations.dtype)
        if tuple(fixations.shape) != (F, h, w) or fixations.device != S.device:
            raise ValueError("fixations must be [%d, %d, %d] on the maps' device, got %s" % (F, h, w, tuple(fixations.shape)))
        _check_buf('fixations', fixations, fixations.dtype)
    work = sphere_eval_work(F, h, w, S.device, work)
    scores = torch.empty((F, 5), dtype=torch.float64, device=S.device)
    n_fix = torch.empty((F,), dtype=torch.int32, device=S.device)
    check(lib().cp360_seval_scores(ptr(S), ptr(G), ptr(fixations), ptr(weights), F, h, w, ptr(scores), ptr(n_fix), ptr(work),
                                   work.numel() * 8, stream()))
    return scores, n_fix


# ----------------------------------------------------------------------------- K15: fixations and shuffled AUC (csrc/fixations.hip)
def _fix_points(lonlat, offsets, hw):
    """The checks the three point ops share -> (N, F, h, w)."""
    if lonlat.dim() != 2 or lonlat.shape[1] != 2:
        raise ValueError("lonlat must be float64 [N, 2], got %s" % (tuple(lonlat.shape),))
    _check_buf('lonlat', lonlat, torch.float64)
    if offsets.dim() != 1 or offsets.shape[0] < 2 or offsets.device != lonlat.device:
        raise ValueError("offsets must be int32 [F + 1] with F >= 1 on lonlat's device, got %s" % (tuple(offsets.shape),))
    _check_buf('offsets', offsets, torch.int32)
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1:
        raise ValueError("the grid must be at least 1 x 1, got %d x %d" % (h, w))
    return int(lonlat.shape[0]), int(offsets.shape[0]) - 1, h, w


def fixation_work(F, h, w, device, work=None):
    """The workspace of cp360_fix_sauc for F frames (F = 0: of cp360_fix_density): `work` when it is large enough, else a new one."""
    return _work(lib().cp360_fix_work_bytes, "fixations", F, h, w, device, work, " (F <= 65535, h w <= 2^21)")


def fixation_counts(lonlat, offsets, hw):
    """cp360_fix_counts: lonlat f64 [N, 2] (longitude, latitude in radians), offsets int32 [F + 1] (CSR: frame f owns the points
    offsets[f] .. offsets[f + 1] - 1) -> (counts int32 [F, h, w], n_points int32 [F]), both on the device, without a
    synchronisation.  Longitudes wrap, latitudes clamp, points with a non-finite coordinate are dropped and not counted."""
    require_gpu(lonlat, offsets)
    N, F, h, w = _fix_points(lonlat, offsets, hw)
    counts = torch.empty((F, h, w), dtype=torch.int32, device=lonlat.device)
    n_points = torch.empty((F,), dtype=torch.int32, device=lonlat.device)
    check(lib().cp360_fix_counts(ptr(lonlat), ptr(offsets), N, F, h, w, ptr(counts), ptr(n_points), stream()))
    return counts, n_points


def fixation_density(lonlat, offsets, hw, sigma_rad, work=None):
    """cp360_fix_density: the points of ``fixation_counts`` -> f32 [F, h, w], per frame the sum over its points of the von
    Mises-Fisher kernel exp((p . q - 1) / sigma_rad^2) on the sphere (``sphere_smooth``'s kernel), un-normalised.  A frame's map does
    not depend on F or on its place in the batch; a frame without points is zero."""
    require_gpu(lonlat, offsets, work)
    N, F, h, w = _fix_points(lonlat, offsets, hw)
    sigma_rad = float(sigma_rad)
    if not (sigma_rad > 0.0 and math.isfinite(sigma_rad)):
        raise ValueError("sigma_rad must be finite and positive, got %r" % (sigma_rad,))
    work = fixation_work(0, h, w, lonlat.device, work)
    out = torch.empty((F, h, w), dtype=torch.float32, device=lonlat.device)
    check(lib().cp360_fix_density(ptr(lonlat), ptr(offsets), N, F, h, w, sigma_rad, ptr(out), ptr(work), work.numel() * 8, stream()))
    return out


def shuffled_auc(S, pos, neg, work=None):
    """cp360_fix_sauc: S f32 [F, h, w], pos int32 [F, h, w] (the fixation counts of each frame, clamped to 0 .. 1023), neg int32
    [1, h, w] or [F, h, w] (the counts the negatives are drawn from, clamped to 0 .. 2^20) -> (auc f64 [F], c_tot int64 [F], a_neg
    int64 [F]) on the device, without a synchronisation.  An exact quotient of integers: no jitter, no random draw."""
    require_gpu(S, pos, neg, work)
    F, h, w = _eval_maps('S', S)
    if pos.dim() != 3 or tuple(pos.shape) != (F, h, w) or pos.device != S.device:
        raise ValueError("pos must be int32 %s on S's device, got %s" % ((F, h, w), tuple(pos.shape)))
    if neg.dim() != 3 or tuple(neg.shape) not in ((1, h, w), (F, h, w)) or neg.device != S.device:
        raise ValueError("neg must be int32 [1 or %d, %d, %d] on S's device, got %s" % (F, h, w, tuple(neg.shape)))
    _check_buf('pos', pos, torch.int32)
    _check_buf('neg', neg, torch.int32)
    work = fixation_work(F, h, w, S.device, work)
    auc = torch.empty((F,), dtype=torch.float64, device=S.device)
    c_tot = torch.empty((F,), dtype=torch.int64, device=S.device)
    a_neg = torch.empty((F,), dtype=torch.int64, device=S.device)
    check(lib().cp360_fix_sauc(ptr(S), ptr(pos), ptr(neg), int(neg.shape[0]), F, h, w, ptr(auc), ptr(c_tot), ptr(a_neg), ptr(work),
                               work.numel() * 8, stream()))
    return auc, c_tot, a_neg


# ----------------------------------------------------------------------------- K19: the ceiling and the baselines, per point (csrc/fixations.hip)
def fixation_point_work(F, h, w, device, work=None):
    """The workspace of one cp360_fix_point_scores call over F frames (the tables and 8 F h w bytes): `work` when it is large
    enough, else a new one."""
    return _work(lib().cp360_fix_point_work_bytes, "fixation point scores", F, h, w, device, work, " (F <= 65535, h w <= 2^21)")


def fixation_point_scores(lonlat, offsets, hw, weights, sigma_rad=None, maps=None, work=None):
    """cp360_fix_point_scores: the points of ``fixation_counts`` (the points of one frame are taken as different viewers'), weights
    int32 [h] (``sphere_eval_weights``) -> f64 [N, 2] = (auc, nss) of every point on the device, without a synchronisation.
    Exactly one of sigma_rad and maps is given.  sigma_rad: leave-one-out - point k is scored against the density of the other
    points of its frame (``fixation_density``'s terms, the frame's f64 total minus the point's own term).  maps f32 [1 or F, h, w]:
    every point of frame f is scored against maps[f] (or maps[0]).  The AUC is ``sphere_eval``'s AUC-Judd with the point's pixel as
    the one fixation.  A point's numbers do not depend on F, N or its place in the batch; a non-finite point gets NaN."""
    if (sigma_rad is None) == (maps is None):
        raise ValueError("exactly one of sigma_rad (leave-one-out) and maps must be given")
    require_gpu(lonlat, offsets, weights, maps, work)
    N, F, h, w = _fix_points(lonlat, offsets, hw)
    if tuple(weights.shape) != (h,) or weights.device != lonlat.device:
        raise ValueError("weights must be int32 [%d] on lonlat's device" % h)
    _check_buf('weights', weights, torch.int32)
    if maps is None:
        sigma_rad, Fs = float(sigma_rad), 0
        if not (sigma_rad > 0.0 and math.isfinite(sigma_rad)):
            raise ValueError("sigma_rad must be finite and positive, got %r" % (sigma_rad,))
    else:
        if maps.dim() != 3 or tuple(maps.shape) not in ((1, h, w), (F, h, w)) or maps.device != lonlat.device:
            raise ValueError("maps must be float32 [1 or %d, %d, %d] on lonlat's device, got %s" % (F, h, w, tuple(maps.shape)))
        _check_buf('maps', maps, torch.float32)
        sigma_rad, Fs = 0.0, int(maps.shape[0])
    work = fixation_point_work(F, h, w, lonlat.device, work)
    scores = torch.empty((N, 2), dtype=torch.float64, device=lonlat.device)
    check(lib().cp360_fix_point_scores(ptr(maps), Fs, ptr(lonlat), ptr(offsets), N, F, h, w, sigma_rad, ptr(weights), ptr(scores),
                                       ptr(work), work.numel() * 8, stream()))
    return scores


# ----------------------------------------------------------------------------- K17: head-tracking ground truth (csrc/headtrack.hip)
def _head_view(view_hw, hfov_deg):
    """A view (h_v, w_v) of hfov_deg degrees -> (hfov in radians, the aspect h_v / w_v) as the library takes it."""
    hv, wv = (float(v) for v in view_hw)
    hfov_deg = float(hfov_deg)
    if not (hv > 0.0 and wv > 0.0 and math.isfinite(hv / wv) and hv / wv > 0.0 and 0.0 < hfov_deg < 180.0):
        raise ValueError("a view needs h_v, w_v > 0 and 0 < hfov_deg < 180, got %r, %r" % (view_hw, hfov_deg))
    return math.radians(hfov_deg), hv / wv


def _head_cameras(R, offsets, hw):
    """The checks the two head ops share -> (N, F, h, w)."""
    if R.dim() != 3 or tuple(R.shape[1:]) != (3, 3):
        raise ValueError("R must be float32 [N, 3, 3], got %s" % (tuple(R.shape),))
    _check_buf('R', R, torch.float32)
    if offsets.dim() != 1 or offsets.shape[0] < 2 or offsets.device != R.device:
        raise ValueError("offsets must be int32 [F + 1] with F >= 1 on R's device, got %s" % (tuple(offsets.shape),))
    _check_buf('offsets', offsets, torch.int32)
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1:
        raise ValueError("the grid must be at least 1 x 1, got %d x %d" % (h, w))
    return int(R.shape[0]), int(offsets.shape[0]) - 1, h, w


def head_work(h, w, device, work=None):
    """The workspace of the two head ops, the grid's tables: `work` when it is large enough, else a new one."""
    return _work(lib().cp360_fix_work_bytes, "head tracking", 0, h, w, device, work, " (h w <= 2^21)")


def head_footprints(R, offsets, hw, view_hw, hfov_deg, work=None):
    """cp360_head_footprints: the viewers' cameras R f32 [N, 3, 3] (camera-to-world, columns forward / up / right), offsets int32
    [F + 1] (CSR: frame f owns the cameras offsets[f] .. offsets[f + 1] - 1), each with the view (view_hw, hfov_deg) ->
    (counts int32 [F, h, w] = the number of the frame's cameras that have the grid pixel in view, n_views int32 [F] = the number
    of its finite cameras), both on the device, without a synchronisation.  A non-finite camera sees nothing."""
    require_gpu(R, offsets, work)
    N, F, h, w = _head_cameras(R, offsets, hw)
    hfov, aspect = _head_view(view_hw, hfov_deg)
    work = head_work(h, w, R.device, work)
    counts = torch.empty((F, h, w), dtype=torch.int32, device=R.device)
    n_views = torch.empty((F,), dtype=torch.int32, device=R.device)
    check(lib().cp360_head_footprints(ptr(R), ptr(offsets), N, F, h, w, hfov, aspect, ptr(counts), ptr(n_views), ptr(work),
                                      work.numel() * 8, stream()))
    return counts, n_views


def _agreement_args(Rc, R, offsets, hw, weights, work, *more):
    """What the two agreement ops check alike; the workspace and the two results -> (N, F, h, w, work, inter, uni)."""
    require_gpu(Rc, R, offsets, weights, work, *more)
    N, F, h, w = _head_cameras(R, offsets, hw)
    _stab_rotations(Rc, F)
    if Rc.device != R.device or tuple(weights.shape) != (h,) or weights.device != R.device:
        raise ValueError("Rc [%d, 3, 3] and weights int32 [%d] must be on R's device" % (F, h))
    _check_buf('weights', weights, torch.int32)
    work = head_work(h, w, R.device, work)
    inter = torch.empty((N,), dtype=torch.int64, device=R.device)
    uni = torch.empty((N,), dtype=torch.int64, device=R.device)
    return N, F, h, w, work, inter, uni


def head_agreement(Rc, cam_view, R, offsets, hw, view, weights, work=None):
    """cp360_head_agreement: the camera Rc f32 [F, 3, 3] with cam_view = ((h_c, w_c), hfov_deg) against every viewer of its frame
    (R, offsets as in ``head_footprints``, view = ((h_v, w_v), hfov_deg)); weights int32 [h] (``sphere_eval_weights``) -> (inter
    int64 [N], uni int64 [N]): the weighted pixels inside both windows and inside either, on the device, without a
    synchronisation."""
    N, F, h, w, work, inter, uni = _agreement_args(Rc, R, offsets, hw, weights, work)
    (cam_hfov, cam_aspect), (hfov, aspect) = _head_view(*cam_view), _head_view(*view)
    check(lib().cp360_head_agreement(ptr(Rc), cam_hfov, cam_aspect, ptr(R), ptr(offsets), N, F, h, w, hfov, aspect, ptr(weights),
                                     ptr(inter), ptr(uni), ptr(work), work.numel() * 8, stream()))
    return inter, uni


def head_agreement_zoom(Rc, cam_lens, R, offsets, hw, view, weights, work=None):
    """cp360_head_agreement_zoom (K22c): ``head_agreement`` with a lens per frame for the camera, cam_lens f32 [F, 4]
    (``viewport_lens`` of the camera's view and its field of view per frame); the viewers' window stays ``view``."""
    N, F, h, w, work, inter, uni = _agreement_args(Rc, R, offsets, hw, weights, work, cam_lens)
    _lens(cam_lens, F, R.device, 'cam_lens')
    hfov, aspect = _head_view(*view)
    check(lib().cp360_head_agreement_zoom(ptr(Rc), ptr(cam_lens), ptr(R), ptr(offsets), N, F, h, w, hfov, aspect, ptr(weights),
                                          ptr(inter), ptr(uni), ptr(work), work.numel() * 8, stream()))
    return inter, uni


# ----------------------------------------------------------------------------- K24: viewport-adaptive streaming (csrc/streaming.hip)
STREAM_MAX_SOURCE = 4096                                               # S = hs ws and T = rows cols
STREAM_MAX_LEVELS = 8


def _stream_grid(hw, tiles=None):
    """The grid (h, w) and the tiles (rows, cols) on it -> (h, w, rows, cols); without tiles rows = cols = 1."""
    h, w = (int(v) for v in hw)
    if h < 1 or w < 1 or h * w > 1 << 21:
        raise ValueError("the grid must be between 1 x 1 and 2^21 pixels, got %d x %d" % (h, w))
    rows, cols = (1, 1) if tiles is None else (int(v) for v in tiles)
    if not (1 <= rows <= h and 1 <= cols <= w and rows * cols <= STREAM_MAX_SOURCE):
        raise ValueError("tiles must be 1 .. %d rows and 1 .. %d columns, at most %d in all, got %d x %d"
                         % (h, w, STREAM_MAX_SOURCE, rows, cols))
    return h, w, rows, cols


def _stream_bits(name, bits, S, P, device):
    """A bit matrix of S rows over P elements: int32 [S, ceil(P / 32)], the u32 words' bit patterns."""
    if bits.dim() != 2 or tuple(bits.shape) != (S, (P + 31) // 32) or bits.device != device:
        raise ValueError("%s must be int32 [%d, %d] on the device of the other operands, got %s"
                         % (name, S, (P + 31) // 32, tuple(bits.shape)))
    _check_buf(name, bits, torch.int32)


def _stream_out(out, shape, dtype, device, *srcs):
    """A new destination, or the caller's when it has this shape and dtype on this device and shares no byte with an operand."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    if tuple(out.shape) != tuple(shape) or out.device != device:
        raise ValueError("out must be %s %s on the operands' device, got %s" % (dtype, tuple(shape), tuple(out.shape)))
    _check_buf('out', out, dtype)
    if any(_shares_bytes(out, s) for s in srcs if s.numel() and out.numel()):
        raise ValueError("out must not share memory with an operand")
    return out


def view_quality_work(h, w, device, work=None):
    """The workspace of the streaming ops on an h x w grid (the grid's tables and the tile of every column and row; it also
    serves ``view_incidence``): `work` when it is large enough, else a new one."""
    return _work(lambda F, hh, ww: lib().cp360_view_quality_work_bytes(hh, ww), "streaming", 0, h, w, device, work, " (h w <= 2^21)")


def view_incidence(cams, hw, view_hw, hfov_deg, work=None, out=None):
    """cp360_view_incidence: cams f32 [S, 3, 3] (camera-to-world, columns forward / up / right; S <= 4096), each with the view
    (view_hw, hfov_deg) -> int32 [S, ceil(h w / 32)]: bit i % 32 of word i / 32 of row j says whether grid pixel i is in the view
    of cams[j], ``head_footprints``' decision bit for bit; the bits past h w are 0.  The int32 hold the u32 words' bit patterns."""
    require_gpu(cams, work, out)
    if cams.dim() != 3 or tuple(cams.shape[1:]) != (3, 3) or not 1 <= cams.shape[0] <= STREAM_MAX_SOURCE:
        raise ValueError("cams must be float32 [S, 3, 3] with 1 <= S <= %d, got %s" % (STREAM_MAX_SOURCE, tuple(cams.shape)))
    _check_buf('cams', cams, torch.float32)
    h, w, _, _ = _stream_grid(hw)
    hfov, aspect = _head_view(view_hw, hfov_deg)
    S = int(cams.shape[0])
    work = head_work(h, w, cams.device, work)
    out = _stream_out(out, (S, (h * w + 31) // 32), torch.int32, cams.device, cams)
    check(lib().cp360_view_incidence(ptr(cams), S, h, w, hfov, aspect, ptr(out), ptr(work), work.numel() * 8, stream()))
    return out


def tile_incidence(inc, hw, tiles, out=None):
    """cp360_tile_incidence: inc int32 [S, ceil(h w / 32)] (``view_incidence``), tiles = (rows, cols) on the grid (pixel (x, y) in
    tile ((y rows) / h) cols + (x cols) / w) -> int32 [S, ceil(rows cols / 32)]: bit t of row j is the OR of inc[j, i] over the
    pixels of tile t."""
    require_gpu(inc, out)
    h, w, rows, cols = _stream_grid(hw, tiles)
    if inc.dim() != 2 or not 1 <= inc.shape[0] <= STREAM_MAX_SOURCE:
        raise ValueError("inc must be int32 [S, %d] with 1 <= S <= %d, got %s" % ((h * w + 31) // 32, STREAM_MAX_SOURCE, tuple(inc.shape)))
    S = int(inc.shape[0])
    _stream_bits('inc', inc, S, h * w, inc.device)
    out = _stream_out(out, (S, (rows * cols + 31) // 32), torch.int32, inc.device, inc)
    check(lib().cp360_tile_incidence(ptr(inc), S, h, w, rows, cols, ptr(out), stream()))
    return out


def view_expect(sal, weights, bits, P, out=None):
    """cp360_view_expect: sal f32 [F, hs, ws] (F = 0 is valid), weights int32 [hs] (``sphere_eval_weights``), bits int32 [hs ws,
    ceil(P / 32)] (``view_incidence`` with P = h w, or ``tile_incidence`` with P = rows cols) -> (out f32 [F, P], total f32 [F]):
    with m[f, j] = sal[f, j] (float)a_y where sal[f, j] > 0 and finite, else 0, out[f, i] = (the sum of m[f, j] over the j whose
    bit i is set) / total[f], total[f] the sum over every j, both summed in float32 for j ascending; 0 where total is 0.  On the
    device, without a synchronisation; a frame's numbers do not depend on F or on its place in the batch."""
    require_gpu(sal, weights, bits, out)
    if sal.dim() != 3 or sal.shape[1] < 1 or sal.shape[2] < 1 or sal.shape[1] * sal.shape[2] > STREAM_MAX_SOURCE or sal.shape[0] > 65535:
        raise ValueError("sal must be float32 [F, hs, ws] with F <= 65535 and 1 <= hs ws <= %d, got %s" % (STREAM_MAX_SOURCE, tuple(sal.shape)))
    _check_buf('sal', sal, torch.float32)
    F, hs, ws = (int(s) for s in sal.shape)
    P = int(P)
    if not 1 <= P <= 1 << 21:
        raise ValueError("P must be 1 .. 2^21, got %d" % P)
    if tuple(weights.shape) != (hs,) or weights.device != sal.device:
        raise ValueError("weights must be int32 [%d] on sal's device" % hs)
    _check_buf('weights', weights, torch.int32)
    _stream_bits('bits', bits, hs * ws, P, sal.device)
    out = _stream_out(out, (F, P), torch.float32, sal.device, sal, bits, weights)
    total = torch.empty((F,), dtype=torch.float32, device=sal.device)
    check(lib().cp360_view_expect(ptr(sal), F, hs, ws, ptr(weights), ptr(bits), P, ptr(out), ptr(total), stream()))
    return out, total


def view_quality(R, offsets, hw, view, weights, levels, tiles, L, work=None):
    """cp360_view_quality: the viewers R f32 [N, 3, 3], offsets int32 [F + 1] of ``head_footprints`` with view = ((h_v, w_v),
    hfov_deg), weights int32 [h], levels uint8 [F, rows cols] (the quality level of every tile in every frame; a value >= L counts
    as L - 1), tiles = (rows, cols), 1 <= L <= 8 -> qarea int64 [N, L]: the weighted pixels in viewer k's window whose tile has
    level l in its frame.  Exact integers, on the device, without a synchronisation; a non-finite viewer gets zeros."""
    require_gpu(R, offsets, weights, levels, work)
    N, F, _, _ = _head_cameras(R, offsets, hw)
    h, w, rows, cols = _stream_grid(hw, tiles)
    L = int(L)
    if not 1 <= L <= STREAM_MAX_LEVELS:
        raise ValueError("L must be 1 .. %d, got %d" % (STREAM_MAX_LEVELS, L))
    if tuple(weights.shape) != (h,) or weights.device != R.device:
        raise ValueError("weights must be int32 [%d] on R's device" % h)
    _check_buf('weights', weights, torch.int32)
    if tuple(levels.shape) != (F, rows * cols) or levels.device != R.device:
        raise ValueError("levels must be uint8 [%d, %d] on R's device, got %s" % (F, rows * cols, tuple(levels.shape)))
    _check_buf('levels', levels, torch.uint8)
    hfov, aspect = _head_view(*view)
    work = view_quality_work(h, w, R.device, work)
    qarea = torch.empty((N, L), dtype=torch.int64, device=R.device)
    check(lib().cp360_view_quality(ptr(R), ptr(offsets), N, F, h, w, hfov, aspect, ptr(weights), ptr(levels), rows, cols, L, ptr(qarea),
                                   ptr(work), work.numel() * 8, stream()))
    return qarea


# ----------------------------------------------------------------------------- K26: video quality on the sphere (csrc/sphere_quality.hip)
def _quality_cells(H, W, cells):
    rows, cols = (int(v) for v in cells)
    H, W = int(H), int(W)
    if H < 1 or W < 1 or not 1 <= rows <= H or not 1 <= cols <= W:
        raise ValueError("cells must be (rows, cols) with 1 <= rows <= %d and 1 <= cols <= %d, got %r" % (H, W, tuple(cells)))
    return H, W, rows, cols


def _quality_ssim_ok(H, W):
    return H % 4 == 0 and W % 4 == 0 and H >= 8 and W >= 8


def quality_cell_weights(H, W, cells):
    """int64 numpy [rows cols]: the sum of the row weights a_y (``shot_weights_host``) over the cell's pixels, pixel (y, x) in cell
    ((y rows) // H, (x cols) // W).  Exact; host only: needs no GPU."""
    H, W, rows, cols = _quality_cells(H, W, cells)
    per_row = np.zeros(rows, np.int64)
    np.add.at(per_row, (np.arange(H, dtype=np.int64) * rows) // H, shot_weights_host(H)[0].astype(np.int64))
    per_col = np.bincount((np.arange(W, dtype=np.int64) * cols) // W, minlength=cols).astype(np.int64)
    return (per_row[:, None] * per_col[None, :]).reshape(-1)


def quality_window_weights(H, W, cells):
    """int64 numpy [rows cols]: the sum of ww_i = a_4i + .. + a_4i+7 over the windows (i, j), i = 0 .. H / 4 - 2, j = 0 .. W / 4 - 1,
    whose pixel (4 i + 4, (4 j + 4) % W) lies in the cell; 0 for a cell without a window, and everywhere where the frame has no
    windows (H, W not multiples of 4 or below 8).  Exact; host only."""
    H, W, rows, cols = _quality_cells(H, W, cells)
    out = np.zeros((rows, cols), np.int64)
    if not _quality_ssim_ok(H, W):
        return out.reshape(-1)
    a = shot_weights_host(H)[0].astype(np.int64)
    i = np.arange(H // 4 - 1, dtype=np.int64)
    ww = np.array([a[4 * k:4 * k + 8].sum() for k in i], np.int64)
    per_row = np.zeros(rows, np.int64)
    np.add.at(per_row, ((4 * i + 4) * rows) // H, ww)
    per_col = np.bincount((((4 * np.arange(W // 4, dtype=np.int64) + 4) % W) * cols) // W, minlength=cols).astype(np.int64)
    return (per_row[:, None] * per_col[None, :]).reshape(-1)


def sphere_quality_work(F, H, W, cells, device, work=None):
    """The workspace of one cp360_sphere_quality call: `work` when it is large enough, else a new one."""
    H, W, rows, cols = _quality_cells(H, W, cells)
    return _work(lambda f, h, w: lib().cp360_sphere_quality_work_bytes(f, h, w, rows, cols), "sphere quality", F, H, W, device, work,
                 " (F, H <= 65535, H W <= 2^28, W <= 2^21)")


def sphere_quality(ref, dist, cells, ssim=True, work=None, weights=None):
    """cp360_sphere_quality: ref, dist u8 [F, H, W, 3] (contiguous; either may start at any byte), cells = (rows, cols) ->
    (sse int64 [F, rows cols, 3], ssim_q int64 [F, rows cols] or None with ssim=False), on the device, without a synchronisation.
    sse[f, t, c] = the sum over the pixels of cell t of a_y (ref - dist)^2; ssim_q[f, t] = the sum over the cell's windows of
    ww q, q = the window's structural similarity on integer luma times 2^24 (needs H, W multiples of 4, at least 8).
    Exact integers: the same bits whatever F, the frames' addresses and the launch."""
    require_gpu(ref, dist, work, weights)
    F, H, W, _ = _frames_nhwc(ref, u8_only=True, n='F')
    if _frames_nhwc(dist, u8_only=True, n='F') != (F, H, W, 3) or dist.device != ref.device:
        raise ValueError("dist must be uint8 %s on ref's device, got %s" % ((F, H, W, 3), tuple(dist.shape)))
    H, W, rows, cols = _quality_cells(H, W, cells)
    if ssim and not _quality_ssim_ok(H, W):
        raise ValueError("the structural similarity needs H and W multiples of 4 and at least 8, got %d x %d (ssim=False measures "
                         "the squared error alone)" % (H, W))
    if weights is None:
        weights = shot_weights(H, ref.device)
    elif tuple(weights.shape) != (H,) or weights.device != ref.device:
        raise ValueError("weights must be int32 [%d] on the frames' device" % H)
    _check_buf('weights', weights, torch.int32)
    if work is None:
        work = sphere_quality_work(F, H, W, (rows, cols), ref.device)
    else:
        need = int(lib().cp360_sphere_quality_work_bytes(F, H, W, rows, cols))
        _check_buf('work', work, torch.float64)
        if need == 0 or work.device != ref.device or work.numel() * 8 < need:
            raise ValueError("work must be float64 of at least %d bytes on the frames' device (sphere_quality_work)" % need)
    sse = torch.empty((F, rows * cols, 3), dtype=torch.int64, device=ref.device)
    ssim_q = torch.empty((F, rows * cols), dtype=torch.int64, device=ref.device) if ssim else None
    check(lib().cp360_sphere_quality(ptr(ref), ptr(dist), F, H, W, rows, cols, ptr(weights), ptr(sse), ptr(ssim_q), ptr(work),
                                     work.numel() * 8, stream()))
    return sse, ssim_q


# ----------------------------------------------------------------------------- K18: the supervised loss (csrc/suploss.hip)
SUP_LOSS_STATS = 16                                                    # CP360_SUP_LOSS_STATS


def sup_loss_work(N, mhw, hw, device, work=None):
    """The workspace of one cp360_sup_loss_forward / _backward call: `work` when it is large enough, else a new one."""
    mh, mw = (int(v) for v in mhw)
    return _work(lambda n, h, w: lib().cp360_sup_loss_work_bytes(n, mh, mw, h, w), "sup_loss", N, hw[0], hw[1], device, work,
                 " from maps of %d x %d (N <= 65535, h w <= 2^21, mh mw <= 2^21)" % (mh, mw))


def _sup_loss_args(maps, G, fix, weights, kl_eps):
    """The checks the two passes share -> (N, mh, mw, h, w, kl_eps)."""
    N, mh, mw = _eval_maps('maps', maps)
    if _eval_maps('G', G)[0] != N or G.device != maps.device:
        raise ValueError("G must be float32 [%d, h, w] on the maps' device, got %s" % (N, tuple(G.shape)))
    h, w = int(G.shape[1]), int(G.shape[2])
    if tuple(weights.shape) != (h,) or weights.device != maps.device:
        raise ValueError("weights must be int32 [%d] on the maps' device" % h)
    _check_buf('weights', weights, torch.int32)
    if fix is not None:
        if fix.dtype not in (torch.uint8, torch.bool):
            raise ValueError("fix must be uint8 or bool, got %s" % fix.dtype)
        if tuple(fix.shape) != (N, h, w) or fix.device != maps.device:
            raise ValueError("fix must be [%d, %d, %d] on the maps' device, got %s" % (N, h, w, tuple(fix.shape)))
        _check_buf('fix', fix, fix.dtype)
    kl_eps = float(kl_eps)
    if not (kl_eps > 0.0 and kl_eps < float('inf')):
        raise ValueError("kl_eps must be finite and > 0, got %r" % (kl_eps,))
    return N, mh, mw, h, w, kl_eps


def sup_loss_forward(maps, G, weights, fix=None, kl_eps=2.0 ** -52, work=None):
    """cp360_sup_loss_forward: maps f32 [N, mh, mw], G f32 [N, h, w], weights int32 [h] (``sphere_eval_weights``), fix u8 / bool
    [N, h, w] or None (K14's derived mask) -> (terms f64 [N, 3] = (kl, cc, nss), valid u8 [N, 3], stats f64 [N, 16]) on the
    device, without a synchronisation: K14's numbers of ``sphere_eval_resample(maps, (h, w))``, and what the backward pass needs."""
    require_gpu(maps, G, weights, fix, work)
    N, mh, mw, h, w, kl_eps = _sup_loss_args(maps, G, fix, weights, kl_eps)
    work = sup_loss_work(N, (mh, mw), (h, w), maps.device, work)
    terms = torch.empty((N, 3), dtype=torch.float64, device=maps.device)
    valid = torch.empty((N, 3), dtype=torch.uint8, device=maps.device)
    stats = torch.empty((N, SUP_LOSS_STATS), dtype=torch.float64, device=maps.device)
    check(lib().cp360_sup_loss_forward(ptr(maps), ptr(G), ptr(fix), ptr(weights), N, mh, mw, h, w, kl_eps, ptr(terms), ptr(valid),
                                       ptr(stats), ptr(work), work.numel() * 8, stream()))
    return terms, valid, stats


def sup_loss_backward(maps, G, weights, stats, valid, gterms, fix=None, kl_eps=2.0 ** -52, work=None):
    """cp360_sup_loss_backward: the inputs of ``sup_loss_forward``, its stats f64 [N, 16] and valid u8 [N, 3], and gterms f64
    [N, 3] -> dmaps f32 [N, mh, mw] = sum_t gterms[n, t] valid[n, t] dterm_t/dmaps[n]; an invalid term contributes +0."""
    require_gpu(maps, G, weights, stats, valid, gterms, fix, work)
    N, mh, mw, h, w, kl_eps = _sup_loss_args(maps, G, fix, weights, kl_eps)
    for name, t, dtype, cols in (('stats', stats, torch.float64, SUP_LOSS_STATS), ('valid', valid, torch.uint8, 3),
                                 ('gterms', gterms, torch.float64, 3)):
        if tuple(t.shape) != (N, cols) or t.device != maps.device:
            raise ValueError("%s must be %s [%d, %d] on the maps' device, got %s" % (name, dtype, N, cols, tuple(t.shape)))
        _check_buf(name, t, dtype)
    work = sup_loss_work(N, (mh, mw), (h, w), maps.device, work)
    dmaps = torch.empty_like(maps)
    check(lib().cp360_sup_loss_backward(ptr(maps), ptr(G), ptr(fix), ptr(weights), ptr(stats), ptr(valid), ptr(gterms), N, mh, mw,
                                        h, w, kl_eps, ptr(dmaps), ptr(work), work.numel() * 8, stream()))
    return dmaps
