"""CPU emulation of the UNet engine's bf16 and f16 modes (fdsr_set_precision: FDSR_PREC_BF16 / FDSR_PREC_F16), operator by operator:
the yardstick of the modes' arithmetic, written from oracle/fdsr_oracle.py's pieces (block, resnet_block, clam, slam,
noise_level_mlp) plus the modes' rounding points.  It takes nothing from the device code at run time; every rounding point below was
read from the kernel source named beside it (paths under fastdiffsr_amd/csrc/).

Formats.  'bf16' rounds to nearest even; 'f16' clamps to +-65504, then rounds to nearest even (fdsr_act_io.h:13 the bf16 cast,
:39-41 v_med3 + cast); fmt=None turns EVERY rounding off (weights, operands, stores), which leaves the oracle's network.

Rounding points
  * Staged operand.  A convolution rounds what it stages to the format, once: the stored tensor widened and used raw (stride-2 and
    upsample convs, the res_conv rider: it is a format value already), swish(GN(x)) (fdsr_conv_k32.hip:286-322: widen, v*sc+sh,
    silu_fast, stage4_16; fdsr_conv_h.hip:152-166; fdsr_conv_up2.hip:97; fdsr_conv_strip.hip:281-306 the same operations cut into
    three stages; stage4_16 = one RNE cast, no clamp: fdsr_act_io.h:106-116 -- `rnd` below clamps in f16, which is vacuous here:
    |swish(v)| <= |v| and a GroupNorm'ed v beyond 65504 needs a gamma or beta of that size), or the raw fp32 network input (conv_in8,
    fdsr_conv_tail.hip:149-153 through to_planes :28-49: f16 clamps to +-65504 first, bf16 casts).  Zero padding applies to the
    ACTIVATED tensor (k32 :320-321, tail :359).
  * Packed weights (fdsr_forms.cpp:153-181, chosen in fdsr_engine.cpp:434-438).  bf16: rn_bf16(w).  f16: the hi plane of the f16x3
    form, rn_f16(w * 2^e) with e = min(12, floor(log2(32768 / max|w|))) per tensor; the epilogue multiplies the accumulator by 2^-e
    (exact), so the effective weight is rn_f16(w 2^e) 2^-e.
  * Up path.  nearest x2 + conv3x3 runs as four 2x2 convolutions on the source grid (fdsr_forms.cpp:193-215): the 3x3 taps that land
    on one source pixel are summed in fp32, ky outer and kx inner, starting from 0.f, and THE SUM is rounded (bf16: :242; f16: :236-241
    with a scale of its own from the largest sum, :216-219).
  * conv_in8 (downs.0) and conv_out3 (final_conv) read the fp32 master copy and convert it in the kernel (fdsr_conv_tail.hip:87-106,
    :291-311).  bf16: rn_bf16(w), the packed value.  f16: the power-of-two scale is computed for PREC_F16X3 only (:88, :292), so the f16
    mode rounds w itself, rn_f16(clamp(w)) -- NOT the hi plane of the scaled form: the two differ for |w| < 2^-14, where the unscaled
    value is an f16 subnormal.  (A finding: every other conv of the f16 mode keeps 11 bits of such a weight, these two keep fewer.)
  * fp32 parts.  Products accumulate in fp32 (MFMA).  The epilogue is acc * 2^-e + (bias [+ rider bias] + noise shift)
    [+ residual read back widened], all fp32, rounded once at the store (fdsr_conv_dev.h:104-109 the constant; k32 :652-656;
    fdsr_conv_h.hip:377-380; strip :447-456; up2 :189-191; split K: fdsr_conv_h.hip:499-519, slices summed in fp32 first).
    The res_conv rider's products go into the SAME accumulators as block2's (fdsr_engine.cpp:350-360): the strip kernel needs the two
    weight scales equal (fdsr_conv_strip.hip:556-558, :699-701); the tile kernels multiply the accumulators by the ratio of the two
    scales between the two phases and un-scale by the rider's (fdsr_conv_h.hip:271-277, :323-329) -- a power of two, exact, so both
    are "sum of all products, each with its own effective weight".  With rider = 2 (the default) no res_conv output is ever stored.
    The noise shift is the fp32 MLP of fdsr_kernels.hip:494-532.  `input` and the eps output (final_conv) stay fp32: conv_out3 writes
    its 27 partial products per pixel * 2^-e to LDS and adds bias + nine of them in tap order (fdsr_conv_tail.hip:380, :391-394).
  * GroupNorm statistics come from the PRODUCER'S fp32 values BEFORE the store's rounding, in every producer: k32 tile
    (fdsr_conv_k32.hip:656-657, :673-674), sub-pixel k32 and up2 (fdsr_conv_up2.hip:189-191), strip (fdsr_conv_strip.hip:455-456),
    conv_h (fdsr_conv_h.hip:379-380, :403-404), split-K reduce (:511-513), conv_in8 (fdsr_conv_tail.hip:181-182), SLAM
    (fdsr_kernels.hip:767-773).  All agree.  Per-tile fp32 (sum, sumsq) are folded in fp64: mean, var = E[x^2] - mean^2 clamped at 0,
    rstd = 1/sqrt(var + 1e-5), then fp32 scale = rstd*gamma, shift = beta - mean*scale (fdsr_kernels.hip:389-443).  So an operator's
    GroupNorm takes its statistics from a second input: the producer's pre-rounding value (`*_pre` below; None: the stored tensor).
    These sums are an input no stored tensor shows: one operand rounding the producer took the other way moves a group mean by
    ~1e-6 of the group's deviation, which is enough to move operand roundings of the consumer (measured on an MI355X: the device's
    block outputs differed from the emulation's in 1-7 % of the elements, in steps of one consumer operand each, and the steps went
    away under mean shifts of 1e-6 .. 4e-6 deviations).  So an operator can take the device's own GroupNorm table (scale, shift:
    fdsr_debug_gn_table) as an input like its tensors (`gn=`); the table itself is then judged against the statistics separately.
  * CLAM / SLAM (fdsr_kernels.hip:583-651, :677-697, :703-775) read the stored tensor widened; pools, MLP, gate, y = gate * x, the
    (mean, max) map and the 7x7 conv are fp32 and nothing in between is rounded; out = sig * (gate * x) is rounded once at the store.

Each operator below takes its inputs as tensors and returns (pre-rounding value, stored value) in the evaluation precision:
E64 (`Emu(..., dtype=torch.float64)`: everything that is not a rounding point in fp64, products of rounded operands summed in fp64) or
E32 (torch fp32 throughout; it stages E64's rounding of swish(GN(x)) and says which of those roundings fp32 evaluation cannot
decide: Emu._stage_act).  `forward` chains them over a whole network; `judge` is the per-element rule of
tests/test_gpu_unet_16bit_layerwise.py."""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from oracle import fdsr_oracle as O
from oracle.layers import wiring

F16_MAX = 65504.0
# what Emu.run returns: pre-rounding value, stored value, F_e of Emu._stage_act (E32, GroupNorm'ed operators; else None), and the
# GroupNorm table (scale, shift, group mean, group variance) the statistics give (None where there is no GroupNorm)
Result = namedtuple('Result', 'pre stored widening table')
_FMT = {'bf16': (8, -126), 'f16': (11, -14), 'f32': (24, -126)}     # significand bits, smallest normal exponent


def ulp(v, fmt):
    """the format's spacing at magnitude v, as fp64"""
    p, emin = _FMT[fmt]
    a = v.detach().abs().double()
    _, e = torch.frexp(a)                                            # a = m 2^e, m in [0.5, 1)
    e = torch.where(a > 0, e - 1, torch.full_like(e, emin)).clamp(min=emin)
    return torch.ldexp(torch.ones_like(a), e - (p - 1))


def boundary_distance(v, fmt):
    """distance of v (fp64) to the nearest rounding boundary of the format: the midpoints between rnd(v) and its two neighbours.  (Just
    above a power of two the lower neighbour is half a spacing away, so the boundary below sits a quarter spacing under it.)"""
    a = v.double().abs()
    if fmt == 'f16':
        a = a.clamp(max=F16_MAX)
    ra = rnd(a, fmt)
    u = ulp(ra, fmt)
    m, _ = torch.frexp(ra)
    below = torch.where((m == 0.5) & (u > ulp(torch.zeros_like(ra), fmt)), u / 2, u)     # spacing under a power of two (not among the subnormals)
    return torch.minimum(ra + u / 2 - a, a - (ra - below / 2))


def rnd(v, fmt, trunc=False):
    """v -> the format's value nearest to it (ties to even; trunc: toward zero instead), in v's dtype.  fmt None: v."""
    if fmt is None:
        return v
    if fmt == 'f32':
        return v.float().to(v.dtype)
    if v.dtype == torch.float32 and not trunc:
        return v.bfloat16().float() if fmt == 'bf16' else v.clamp(-F16_MAX, F16_MAX).half().float()
    w = v.double()
    if fmt == 'f16':
        w = w.clamp(-F16_MAX, F16_MAX)
    u = ulp(w, fmt)
    q = w / u
    return ((torch.trunc(q) if trunc else torch.round(q)) * u).to(v.dtype)


def _pow2_scale(w):
    amax = w.abs().max().item()
    return 12 if amax <= 0 else min(12, math.floor(math.log2(32768.0 / amax)))


def packed_weight(w, fmt):
    """fdsr_forms.cpp:153-181: the value a packed conv weight stands for (fp32 tensor)"""
    w = w.float()
    if fmt is None:
        return w
    if fmt == 'bf16':
        return w.bfloat16().float()
    s = 2.0 ** _pow2_scale(w)
    return (w * s).half().float() / s


def tail_weight(w, fmt):
    """fdsr_conv_tail.hip:87-106, :291-311: conv_in8 / conv_out3 convert the master copy; no scale in the f16 mode"""
    w = w.float()
    if fmt is None:
        return w
    return w.bfloat16().float() if fmt == 'bf16' else w.clamp(-F16_MAX, F16_MAX).half().float()


_TAPS = {(0, 0): (0,), (0, 1): (1, 2), (1, 0): (0, 1), (1, 1): (2,)}        # (parity, source offset a) -> 3x3 taps


def up2_weight(w, fmt, dtype):
    """fdsr_forms.cpp:193-242: [py][px] -> the 2x2 kernel [Cout][Cin][a][b] of output parity (py, px), pre-summed then rounded"""
    w = w.to(dtype) if fmt is None else w.float()
    Co, Ci = w.shape[:2]
    w2 = torch.zeros(2, 2, Co, Ci, 2, 2, dtype=w.dtype)
    for py in range(2):
        for px in range(2):
            for a in range(2):
                for b in range(2):
                    acc = torch.zeros(Co, Ci, dtype=w.dtype)
                    for ky in _TAPS[(py, a)]:
                        for kx in _TAPS[(px, b)]:
                            acc = acc + w[:, :, ky, kx]
                    w2[py, px, :, :, a, b] = acc
    if fmt is None:
        return w2
    if fmt == 'bf16':
        return w2.bfloat16().float()
    s = 2.0 ** _pow2_scale(w2)
    return (w2 * s).half().float() / s


class Emu:
    """The operators of one UNet in one storage format and one evaluation precision.  mut: one deliberate fault (the host tests'
    mutations), {} for the arithmetic as read."""

    def __init__(self, sd, cfg, fmt, dtype=torch.float64, mut=None):
        assert fmt in ('bf16', 'f16', None) and dtype in (torch.float64, torch.float32)
        self.cfg, self.fmt, self.dt, self.mut = cfg, fmt, dtype, dict(mut or {})
        self.sd32 = {k: torch.as_tensor(v).float() for k, v in sd.items()}
        self.sd = {k: v.to(dtype) for k, v in self.sd32.items()}
        self.G = cfg.norm_groups
        self.layers = wiring(cfg)
        self._w, self._e64, self._und, self.widening, self._t32, self._gn, self.table = {}, None, None, None, None, None, None

    # ---- pieces -------------------------------------------------------------------------------------------------------------
    def _weight(self, key, form):
        if (key, form) not in self._w:
            w = self.sd32[key]
            fmt = None if 'unrounded_w' in self.mut else self.fmt
            if form == 'up2':
                v = up2_weight(w, fmt, self.dt)
            else:
                v = packed_weight(w, fmt) if form == 'packed' else tail_weight(w, fmt)
            self._w[(key, form)] = v.to(self.dt)
        return self._w[(key, form)]

    def _store(self, pre, fmt_out=None):
        fmt = self.fmt if fmt_out is None else (fmt_out if self.fmt is not None else None)
        return rnd(pre, fmt, trunc='trunc' in self.mut)

    def _conv(self, x, w, stride=1, padding=0, main=True, rider=False):
        """sum of products of the staged operand x (rounded by the caller) with w, in the evaluation precision"""
        m = self.mut if main else {}
        if rider:                                               # the same faults in the res_conv rider's products (a 1x1: tap 0, 0)
            m = {k[6:]: v for k, v in self.mut.items() if k.startswith('rider_')}
        if 'drop_block' in m:                                   # one (cout, cin-chunk of 16, tap) block of products left out
            co, ch, ky, kx = m['drop_block']
            w = w.clone()
            w[co, 16 * ch:16 * ch + 16, ky % w.shape[2], kx % w.shape[3]] = 0
        if 'swap' in m:                                         # two channels swapped inside a 16-channel chunk
            a, b = m['swap']
            idx = list(range(x.shape[1]))
            idx[a], idx[b] = idx[b], idx[a]
            x = x[:, idx]
        if padding:
            x = F.pad(x, (padding,) * 4)
            if 'halo' in m:                                     # the right halo of the last column reads its neighbour, not zero
                x = x.clone()
                x[..., -1] = x[..., -2]
        return F.conv2d(x, w, None, stride)

    def _gn_swish(self, x, stat, key, mag=False):
        """GroupNorm (statistics of `stat`, folded in fp64; scale / shift and their application in the evaluation precision), Swish"""
        B, C = x.shape[:2]
        G, cpg = self.G, C // self.G
        s = stat.double().reshape(B, G, -1)
        mean = s.mean(-1)
        var = ((s * s).mean(-1) - mean * mean).clamp(min=0)
        rstd = 1.0 / torch.sqrt(var + 1e-5)
        if 'gn_seam' in self.mut:                               # group g takes the scale of group g + 1
            g = self.mut['gn_seam']
            rstd = rstd.clone()
            rstd[:, g] = rstd[:, g + 1]
        sc = rstd.repeat_interleave(cpg, 1).to(self.dt) * self.sd[key + '.weight']
        sh = self.sd[key + '.bias'] - mean.repeat_interleave(cpg, 1).to(self.dt) * sc
        self.table = (sc, sh, mean, var)                        # what the statistics give
        if self._gn is not None:                                # the device's own table, read back: an INPUT of the operator
            sc, sh = self._gn[0].to(self.dt), self._gn[1].to(self.dt)
        y = x.to(self.dt) * sc[:, :, None, None] + sh[:, :, None, None]
        # E32 takes the Swish in the kernels' order of operations: v * rcp(1 + exp2(v * -log2(e))), the product rounded to fp32 before the
        # exponential (silu_fast = v * rcp(1 + __expf(-v)), fdsr_conv_dev.h:22; fdsr_conv_strip.hip:281-295)
        act = y * torch.sigmoid(y) if self.dt == torch.float64 else y * (1.0 / (1.0 + torch.exp2(y * -1.44269504088896340736)))
        if mag:                                                 # ... and |x sc| + |sh|, the size of the terms fp32 rounds
            return act, (x.to(self.dt) * sc[:, :, None, None]).abs() + sh[:, :, None, None].abs()
        return act

    def _stage_act(self, x, stat, key, stat_ref=None):
        """the staged operand rnd(swish(GN(x))), and -- E32 only, kept in self._und -- which of its roundings fp32 evaluation cannot
        decide.  y32: the activation in fp32 on E32's own statistics `stat` (the pre-rounding value E32 computed for the producer: it
        carries the fp32 noise shift and whatever fp32 did to the producer).  y64: in fp64 on E64's statistics `stat_ref`.  The device's
        statistics are sums of ITS fp32 pre-rounding values, which no stored tensor shows: the difference between the two evaluations is
        the measure of what is not known about them.  With r = max |y32 - y64| / (|x sc| + |sh|) over each (image, channel) of THIS
        tensor, an operand whose fp64 value lies within 4 r (|x sc| + |sh|) of a rounding boundary is undecided: the device may take
        either neighbour, and its product then moves by ulp(h) |w|.  Both precisions stage E64's rounding, so P32 - P64 is the spread
        of the accumulation and of the fp32 constants; what the undecided roundings can move output element e,
        F_e = sum over them of ulp(h_k) |w_ek|, is kept beside P32 (`Emu.widening`) and added to that element's bar by `judge`.
        (Why D cannot carry this term by itself: EXPERIMENTS.md, "Judging the 16-bit modes per operator".)"""
        self._und = None
        if self.fmt is None or self.dt == torch.float64:
            return rnd(self._gn_swish(x, stat, key), self.fmt)
        if self._e64 is None:
            self._e64 = Emu(self.sd32, self.cfg, self.fmt, torch.float64)
        y = self._gn_swish(x, stat, key)
        self._e64._gn = self._gn
        y64, m64 = self._e64._gn_swish(x, stat if stat_ref is None else stat_ref, key, mag=True)
        r = ((y.double() - y64).abs() / m64.clamp(min=1e-300)).amax(dim=(2, 3), keepdim=True)     # per (image, channel), as scale and shift are
        self._und = ulp(y64, self.fmt) * (boundary_distance(y64, self.fmt) <= 4 * r * m64)
        return rnd(y64, self.fmt).to(self.dt)

    def _widen(self, w):
        """F_e of the conv (padding 1) just staged, fp64"""
        self.widening = None if self._und is None else F.conv2d(self._und, w.double().abs(), None, 1, 1)

    def _cat(self, x, skip):
        return x if skip is None else torch.cat((x, skip), dim=1)

    @staticmethod
    def _linear_fma32(x, w, b):
        """fp32 Linear in the order of fdsr_kernels.hip:509-531: a = b; a = fmaf(w[k], x[k], a) for k = 0, 1, ... (the fp64 sum of an
        fp32 product and an fp32 value, rounded to fp32, is that fma)"""
        a = b.float().expand(x.shape[0], -1).clone()
        for k in range(x.shape[1]):
            a = (a.double() + x[:, k:k + 1].double() * w[:, k].double().view(1, -1)).float()
        return a

    def noise_shift(self, p, nl):
        """[B, Cout] the block's Linear of the noise-level embedding.  E32: fp32 in the device's order of operations (temb_kernel,
        fdsr_kernels.hip:494-532: sequential fma chains; a / (1 + exp(-a)) for the Swish)"""
        r = p + '.res_block.noise_func.noise_func.0'
        if self.dt == torch.float64:
            t = O.noise_level_mlp(self.sd, nl.to(self.dt).reshape(-1, 1), self.cfg.inner_channel)
            s = F.linear(t, self.sd[r + '.weight'], self.sd[r + '.bias']).reshape(t.shape[0], -1)
        else:
            key = tuple(nl.reshape(-1).tolist())
            if self._t32 is None or self._t32[0] != key:
                sd = self.sd32
                enc = O.positional_encoding(nl.float().reshape(-1, 1), self.cfg.inner_channel).reshape(len(key), -1)
                a = self._linear_fma32(enc, sd['noise_level_mlp.1.weight'], sd['noise_level_mlp.1.bias'])
                a = a / (1.0 + torch.exp(-a))
                self._t32 = (key, self._linear_fma32(a, sd['noise_level_mlp.3.weight'], sd['noise_level_mlp.3.bias']))
            s = self._linear_fma32(self._t32[1], self.sd32[r + '.weight'], self.sd32[r + '.bias'])
        if 'shift_img' in self.mut:                             # the shift of image 0 used for image 1
            s = s.clone()
            s[1] = s[0]
        return s

    # ---- operators: (pre-rounding value, stored value) -----------------------------------------------------------------------
    def conv_in(self, inp):
        """downs.0: the raw fp32 network input, rounded when staged; weights converted in the kernel"""
        x = rnd(inp.to(self.dt), self.fmt)
        pre = self._conv(x, self._weight('downs.0.weight', 'tail'), padding=1) + self.sd['downs.0.bias'].view(1, -1, 1, 1)
        return pre, self._store(pre)

    def block1(self, p, x, nl, x_pre=None, skip=None, skip_pre=None, x_ref=None, skip_ref=None):
        """<p>.res_block.block1: conv3x3(rnd(swish(GN(x | skip)))) + bias + noise shift"""
        r = p + '.res_block.block1'
        xin = self._cat(x, skip)
        stat = self._cat(x if x_pre is None else x_pre, None if skip is None else (skip if skip_pre is None else skip_pre))
        ref = None if x_ref is None else self._cat(x_ref, None if skip is None else skip_ref)
        h = self._stage_act(xin, stat, r + '.block.0', ref)
        pre = self._conv(h, self._weight(r + '.block.3.weight', 'packed'), padding=1)
        self._widen(self._weight(r + '.block.3.weight', 'packed'))
        pre = pre + (self.sd[r + '.block.3.bias'].view(1, -1) + self.noise_shift(p, nl))[:, :, None, None]
        return pre, self._store(pre)

    def block_out(self, p, h1, x, h1_pre=None, skip=None, h1_ref=None):
        """the ResnetBlock's output: conv3x3(rnd(swish(GN(h1)))) + bias + res_conv(x | skip) (same accumulators) or + x"""
        r = p + '.res_block'
        h = self._stage_act(h1, h1 if h1_pre is None else h1_pre, r + '.block2.block.0', h1_ref)
        pre = self._conv(h, self._weight(r + '.block2.block.3.weight', 'packed'), padding=1)
        self._widen(self._weight(r + '.block2.block.3.weight', 'packed'))
        add = self.sd[r + '.block2.block.3.bias']
        if r + '.res_conv.weight' in self.sd:
            pre = pre + self._conv(self._cat(x, skip).to(self.dt), self._weight(r + '.res_conv.weight', 'packed'), main=False, rider=True)
            pre = pre + (add + self.sd[r + '.res_conv.bias']).view(1, -1, 1, 1)
        else:
            pre = pre + add.view(1, -1, 1, 1) + x.to(self.dt)
        return pre, self._store(pre)

    def attn(self, p, x):
        """<p> after CLAM + SLAM of the stored block output"""
        pre = O.slam(self.sd, p + '.sa', O.clam(self.sd, p + '.ca', x.to(self.dt)))
        return pre, self._store(pre)

    def down(self, p, x):
        """downs.k: conv3x3 stride 2 of the stored tensor, raw"""
        pre = self._conv(x.to(self.dt), self._weight(p + '.conv.weight', 'packed'), stride=2, padding=1)
        pre = pre + self.sd[p + '.conv.bias'].view(1, -1, 1, 1)
        return pre, self._store(pre)

    def up(self, p, x):
        """ups.k: nearest x2 + conv3x3 as four 2x2 convolutions of the stored tensor on pre-summed weights"""
        w2 = self._weight(p + '.conv.weight', 'up2')
        B, C, H, W = x.shape
        pre = torch.zeros(B, w2.shape[2], 2 * H, 2 * W, dtype=self.dt)
        for py in range(2):
            for px in range(2):
                full = self._conv(x.to(self.dt), w2[py, px], padding=1)          # (H + 1) x (W + 1): [i, j] = sum K[a, b] xp[i + a, j + b]
                pre[:, :, py::2, px::2] = full[:, :, py:py + H, px:px + W]
        pre = pre + self.sd[p + '.conv.bias'].view(1, -1, 1, 1)
        return pre, self._store(pre)

    def final(self, x, x_pre=None, x_ref=None):
        """final_conv: conv3x3(rnd(swish(GN(x)))) + bias, stored fp32 (eps)"""
        h = self._stage_act(x, x if x_pre is None else x_pre, 'final_conv.block.0', x_ref)
        pre = self._conv(h, self._weight('final_conv.block.3.weight', 'tail'), padding=1)
        self._widen(self._weight('final_conv.block.3.weight', 'tail'))
        pre = pre + self.sd['final_conv.block.3.bias'].view(1, -1, 1, 1)
        return pre, self._store(pre, 'f32')

    # ---- the planned operators in forward order ------------------------------------------------------------------------------
    def operators(self):
        """[(name of the output tensor in fdsr_plan.cpp, kind, module, names of the input tensors)]; a res module gives two or three"""
        ops, feats, cur = [], [], 'input'
        n_down = sum(1 for L in self.layers if L.name.startswith('downs.'))
        for i, L in enumerate(self.layers):
            if L.kind == 'conv_in':
                ops.append((L.name, 'conv_in', L, (cur,)))
            elif L.kind in ('down', 'up'):
                ops.append((L.name, L.kind, L, (cur,)))
            elif L.kind == 'final':
                ops.append((L.name, 'final', L, (cur,)))
            else:
                skip = feats.pop() if L.name.startswith('ups.') else None
                ins = (cur,) if skip is None else (cur, skip)
                out = L.name + '.res_block' if L.with_attn else L.name
                ops.append((L.name + '.res_block.block1', 'block1', L, ins))
                ops.append((out, 'block_out', L, (L.name + '.res_block.block1',) + ins))
                if L.with_attn:
                    ops.append((L.name, 'attn', L, (out,)))
            cur = L.name
            if i < n_down:
                feats.append(cur)
        return ops

    def run(self, op, stored, pre, nl, pre_ref=None, gn=None):
        """one operator on the stored tensors `stored[name]` (and, for GroupNorm statistics, the producers' pre-rounding values
        `pre[name]` where the dict has them) -> Result"""
        name, kind, L, ins = op
        g = lambda n: None if n is None else pre.get(n)
        f = lambda n: None if (n is None or pre_ref is None) else pre_ref.get(n)     # E64's value of the same tensor: Emu._stage_act
        self.widening, self.table, self._gn = None, None, gn
        if kind == 'conv_in':
            out = self.conv_in(stored[ins[0]])
        elif kind == 'down':
            out = self.down(L.name, stored[ins[0]])
        elif kind == 'up':
            out = self.up(L.name, stored[ins[0]])
        elif kind == 'final':
            out = self.final(stored[ins[0]], g(ins[0]), f(ins[0]))
        elif kind == 'attn':
            out = self.attn(L.name, stored[ins[0]])
        elif kind == 'block1':
            sk = ins[1] if len(ins) > 1 else None
            out = self.block1(L.name, stored[ins[0]], nl, g(ins[0]), None if sk is None else stored[sk], g(sk), f(ins[0]), f(sk))
        else:
            sk = ins[2] if len(ins) > 2 else None
            out = self.block_out(L.name, stored[ins[0]], stored[ins[1]], g(ins[0]), None if sk is None else stored[sk], f(ins[0]))
        return Result(out[0], out[1], self.widening, self.table)

    def forward(self, x, nl):
        """the whole network, every operator fed its predecessors' stored values: ({name: pre}, {name: stored})"""
        stored, pre = {'input': x.to(self.dt)}, {}
        with torch.no_grad():
            for op in self.operators():
                pre[op[0]], stored[op[0]] = self.run(op, stored, pre, nl)[:2]
        return pre, stored


def gn_conv_name(op):
    """name of the GroupNorm'ed convolution op of an operator (fdsr_plan.cpp), or None"""
    name, kind, L, ins = op
    return {'block1': name, 'block_out': L.name + '.res_block.block2', 'final': 'final_conv'}.get(kind)


def gn_key(op):
    """state_dict prefix of that GroupNorm's affine parameters"""
    name, kind, L, ins = op
    return {'block1': L.name + '.res_block.block1.block.0', 'block_out': L.name + '.res_block.block2.block.0', 'final': 'final_conv.block.0'}[kind]


def per_operator(e64, e32, stored, nl, gn_tables=None):
    """Every operator of the plan on the stored tensors of some forward (`stored[name]`: the device's debug taps, or an emulation's
    stored values; 'input' the fp32 network input), in both precisions.  GroupNorm statistics come from the pre-rounding value the
    same precision computed for the producer -- from the producer's stored inputs, so nothing accumulates.
    gn_tables: {name of the conv op: (scale, shift)} read from the device, used in place of the statistics' table (e64.table keeps
    what the statistics give).  Yields (op, P64, P32, stored value of E32, F: what undecided operand roundings can move each element or
    None, E64's statistics table or None)."""
    pre64, pre32 = {}, {}
    with torch.no_grad():
        for op in e64.operators():
            gn = None if gn_tables is None else gn_tables.get(gn_conv_name(op))
            r64 = e64.run(op, stored, pre64, nl, gn=gn)
            r32 = e32.run(op, stored, pre32, nl, pre64, gn=gn)
            pre64[op[0]], pre32[op[0]] = r64.pre, r32.pre
            yield op, r64.pre, r32.pre, r32.stored, r32.widening, r64.table


def out_format(name, fmt):
    """the format an operator's output is stored in"""
    return 'f32' if name == 'final_conv' else fmt


def judge(dev, p64, p32, fmt, cap_fmt=None, widening=None):
    """The per-element rule.  dev: the stored output under judgement; p64 / p32: the two pre-rounding values; fmt: its format;
    widening: F_e of Emu._stage_act (None: 0).
      D = max |p32 - p64|: what ordering and fp32 evaluation of the same accumulation move a value before its rounding
      S_e = 4 D + F_e: what the device is granted on element e -- four times the CPU spread, plus the operand roundings nobody can decide
      bound: |dev - rnd(p64)| <= ulp(max(|dev|, |p64|)) + S_e for every element
      tie:   the grant is a pre-rounding value within S_e of p64, so an element may differ from rnd(p64) only where p64 lies within S_e
             of a rounding boundary of the format (with the bound alone a store that truncates, exactly one spacing off, would pass)
      cap:   D <= ulp(rms(p64)) and rms(F) <= ulp(rms(p64)): a broken emulation must not widen its own bar.  cap_fmt: the format this
             spacing is taken in -- the mode's 16-bit format also for final_conv, whose fp32 store (fmt 'f32') leaves the bound at S_e.
    Returns the figures; 'ok' = bound and tie rule hold for every element, 'cap_ok' separately."""
    dev, p64, p32 = dev.double(), p64.double(), p32.double()
    D = (p32 - p64).abs().max().item()
    S = 4 * D + (0 if widening is None else widening.double())
    r = rnd(p64, fmt)
    err = (dev - r).abs()
    u = ulp(torch.maximum(dev.abs(), p64.abs()), fmt)
    ratio = err / (u + S)
    uw = ulp(p64, fmt)
    tie_dist = boundary_distance(p64, fmt)                                   # of p64 to the nearest rounding boundary
    differs = err > 0
    unexplained = differs & (tie_dist > S)
    u_rms = ulp(p64.pow(2).mean().sqrt(), cap_fmt or fmt).item()
    F_rms = 0.0 if widening is None else widening.double().pow(2).mean().sqrt().item()
    return {
        'worst_spacings': (err / u).max().item(), 'delta_spacings': D / u_rms, 'share_diff': differs.double().mean().item(),
        'margin': ratio.max().item(), 'unexplained': int(unexplained.sum().item()),
        'tie_margin': (tie_dist / S).masked_fill(~differs, 0).max().item() if D > 0 else float(differs.any()),
        'widening_rms': F_rms / u_rms, 'widening_max': 0.0 if widening is None else widening.max().item() / u_rms,
        'sharp_share': ((S < 0.25 * uw).double().mean().item()),
        'ok': bool((ratio <= 1).all()) and not bool(unexplained.any()), 'cap_ok': D <= u_rms and F_rms <= u_rms, 'delta': D,
    }
