"""HAT on the HIP engine (include/fdsr.h: fdsr_hat_*): an nn.Module that takes the constructor arguments of the reference's
GeneratorResNet (MSI_SR_model/model/hat.py) with the reference's defaults, owns its parameters and buffers under the
reference's names -- `generator_param.pkl` loads with load_state_dict(strict=True) -- and whose forward runs the device
kernels.  Inference only, exact fp32; there is no PyTorch fallback.  As in the reference, the output is NOT cropped: a
[B,3,H,W] input returns [B,3,Hp*scale,Wp*scale] with Hp, Wp the sides rounded up to a multiple of 16."""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..swinir.model import to_u8  # noqa: F401  (save_img1 is the same function in hat.py)
from .arch import RGB_MEAN, HATConfig, alias_of, buffer_value, is_buffer, state_schema, tap_names


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()


class HAT(nn.Module):
    def __init__(self, img_size=64, patch_size=1, in_chans=3, embed_dim=180, depths=(6, 6, 6, 6, 6, 6), num_heads=(6, 6, 6, 6, 6, 6),
                 window_size=16, compress_ratio=3, squeeze_factor=30, conv_scale=0.01, overlap_ratio=0.5, mlp_ratio=4., qkv_bias=True,
                 qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.1, norm_layer=nn.LayerNorm, ape=False, patch_norm=True,
                 use_checkpoint=False, upscale=2, img_range=1., upsampler='pixelshuffle', resi_connection='1conv', **kwargs):
        super().__init__()
        for what, ok in (("upsampler %r (only 'pixelshuffle')" % (upsampler,), upsampler == 'pixelshuffle'),
                         ("resi_connection %r (only '1conv')" % (resi_connection,), resi_connection == '1conv'),
                         ('patch_size %r (only 1)' % (patch_size,), patch_size == 1), ('ape=True', not ape),
                         ('in_chans %r (only 3)' % (in_chans,), in_chans == 3), ('qkv_bias=False', bool(qkv_bias)),
                         ('qk_scale %r (only None)' % (qk_scale,), qk_scale is None),
                         ('norm_layer %r (only nn.LayerNorm)' % (norm_layer,), norm_layer is nn.LayerNorm),
                         ('window_size %r (only 16)' % (window_size,), window_size == 16),
                         ('overlap_ratio %r (only 0.5)' % (overlap_ratio,), overlap_ratio == 0.5),
                         ('compress_ratio %r' % (compress_ratio,), isinstance(compress_ratio, int) and compress_ratio >= 1),
                         ('squeeze_factor %r' % (squeeze_factor,), isinstance(squeeze_factor, int) and squeeze_factor >= 1),
                         # at img_size <= window the reference shrinks the window and never shifts
                         ('img_size %r (must exceed the window)' % (img_size,), isinstance(img_size, int) and img_size > window_size),
                         ('upscale %r (only 2, 3, 4, 8)' % (upscale,), upscale in (2, 3, 4, 8))):
            if not ok:
                raise NotImplementedError('HAT on the HIP engine does not run ' + what)
        self.cfg = HATConfig(img_size, embed_dim, list(depths), list(num_heads), window_size, compress_ratio, squeeze_factor,
                             float(conv_scale), float(overlap_ratio), mlp_ratio, upscale, float(img_range), bool(patch_norm))
        self.upscale, self.window_size, self.img_range = upscale, window_size, img_range
        self.schema = state_schema(self.cfg)
        # dotted names cannot be registered on an nn.Module: the tensors live under p<i> and state_dict / load_state_dict speak
        # the reference's keys.  An aliased key (upsample.upsampling.2.*) has no tensor of its own: it is p<i> of the key it
        # repeats, as in the reference, where one Conv2d sits at several places of the list.
        self._names = list(self.schema)
        self._slot = {}
        for i, (k, shape) in enumerate(self.schema.items()):
            if alias_of(k) != k:
                self._slot[k] = self._slot[alias_of(k)]
                continue
            self._slot[k] = 'p%d' % i
            if is_buffer(k):
                self.register_buffer('p%d' % i, torch.from_numpy(buffer_value(self.cfg, k)))
            else:
                self.register_parameter('p%d' % i, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self._h = None
        self._uploaded = {}
        self._ws = {}
        self._static = {}
        self._handle()     # refuses what the kernels do not cover (head_dim, embed_dim, ...) with the library's message

    # ---- the reference's keys ----
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for k in self._names:
            p = getattr(self, self._slot[k])
            destination[prefix + k] = p if keep_vars else p.detach()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for k in self._names:
            key = prefix + k
            if key not in state_dict:
                if strict:
                    missing_keys.append(key)
                continue
            src, p = state_dict[key], getattr(self, self._slot[k])
            if is_buffer(k):
                # a function of the geometry, never sent to the device
                if tuple(src.shape) != tuple(p.shape) or not torch.equal(src.to(p.device, p.dtype), p):
                    error_msgs.append('buffer %s differs from what the window geometry gives' % key)
                continue
            if tuple(src.shape) != tuple(p.shape):
                error_msgs.append('size mismatch for %s: copying a param with shape %s from checkpoint, the shape in current '
                                  'model is %s.' % (key, tuple(src.shape), tuple(p.shape)))
                continue
            first = prefix + alias_of(k)
            if alias_of(k) != k and first in state_dict:
                # the reference holds ONE tensor under these keys
                if not torch.equal(src, state_dict[first]):
                    error_msgs.append('%s differs from %s: the reference runs one shared convolution in every upsampling stage, '
                                      'its state_dict repeats one tensor' % (key, first))
                continue
            with torch.no_grad():
                p.copy_(src)
        if strict:
            known = {prefix + k for k in self._names}
            unexpected_keys += [k for k in state_dict if k.startswith(prefix) and k not in known]

    def named_reference_parameters(self):
        return [(k, getattr(self, self._slot[k])) for k in self._names if not is_buffer(k) and alias_of(k) == k]

    # ---- the engine ----
    def _handle(self):
        if self._h is None:
            cfg = self.cfg
            if len(cfg.depths) > _lib.FDSR_HAT_MAX_LAYERS:
                raise NotImplementedError('at most %d layers' % _lib.FDSR_HAT_MAX_LAYERS)
            c = _lib.FdsrHatConfig()
            c.embed_dim, c.n_layers, c.window_size, c.mlp_hidden = cfg.embed_dim, len(cfg.depths), cfg.window_size, cfg.mlp_hidden
            c.upscale, c.patch_norm, c.img_range = cfg.upscale, int(cfg.patch_norm), cfg.img_range
            c.compress_ratio, c.squeeze_factor, c.conv_scale = cfg.compress_ratio, cfg.squeeze_factor, cfg.conv_scale
            c.overlap_win_size = cfg.overlap_win_size
            for i, (d, h) in enumerate(zip(cfg.depths, cfg.num_heads)):
                c.depths[i], c.num_heads[i] = d, h
            for i in range(3):
                c.mean[i] = RGB_MEAN[i]
            h = C.c_void_p()
            try:
                _lib.check(None, _lib.load().fdsr_hat_create(C.byref(c), C.byref(h)))
            except _lib.FdsrError as e:
                raise NotImplementedError(str(e)) from e
            self._h = h
        return self._h

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and _lib._lib is not None:
            _lib._lib.fdsr_hat_destroy(h)
            self._h = None

    def __getstate__(self):
        """copy.deepcopy and pickle carry the tensors and the configuration; a copy creates an engine of its own on first use."""
        d = dict(self.__dict__)
        d['_h'], d['_uploaded'], d['_ws'], d['_static'] = None, {}, {}, {}
        return d

    def sync_weights(self, device):
        """Upload the parameters that changed since their last upload, by (_version, data_ptr)."""
        lib, h = _lib.load(), self._handle()
        if self._uploaded.get('device') != str(device):
            self._uploaded = {'device': str(device)}
        with torch.cuda.device(device):
            for k, p in self.named_reference_parameters():
                stamp = (p._version, p.data_ptr())
                if self._uploaded.get(k) == stamp:
                    continue
                a = p.detach().to('cpu', torch.float32).contiguous()
                shape = (C.c_int64 * a.dim())(*a.shape)
                _lib.check(None, lib.fdsr_hat_load(h, k.encode(), _ptr(a), shape, a.dim()))
                self._uploaded[k] = stamp

    def workspace_bytes(self, b, h, w):
        need = C.c_size_t()
        _lib.check(None, _lib.load().fdsr_hat_workspace_bytes(self._handle(), b, h, w, C.byref(need)))
        return need.value

    def workspace(self, b, h, w, device=None):
        device = device or next(self.parameters()).device
        need = self.workspace_bytes(b, h, w)
        key = (str(device), torch.cuda.current_stream(device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=device)
        return ws

    @staticmethod
    def _check(x):
        if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.shape[1] == 3):
            raise ValueError('HAT takes a [B,3,H,W] tensor on the GPU (there is no CPU path)')
        return x.float().contiguous()

    def padded(self, h, w):
        ws = self.window_size
        return -(-h // ws) * ws, -(-w // ws) * ws

    def output_shape(self, b, h, w):
        hp, wp = self.padded(h, w)
        return (b, 3, hp * self.upscale, wp * self.upscale)

    def forward(self, x, graph=False):
        """[B,3,H,W] fp32 in [0, 1] on the GPU -> [B,3,Hp*scale,Wp*scale] (the padded size: the reference does not crop).
        graph=True replays one captured graph per (B, H, W): the call copies x into, and the result out of, buffers that the
        graph keeps."""
        x = self._check(x)
        b, _, h, w = x.shape
        self.sync_weights(x.device)
        lib, hd = _lib.load(), self._handle()
        with torch.cuda.device(x.device):
            if not graph:
                ws = self.workspace(b, h, w, x.device)      # first: it refuses a shape that cannot be padded
                out = torch.empty(self.output_shape(b, h, w), dtype=torch.float32, device=x.device)
                st = torch.cuda.current_stream(x.device).cuda_stream
                _lib.check(None, lib.fdsr_hat_forward(hd, _ptr(x), b, h, w, _ptr(out), _ptr(ws), ws.numel(), C.c_void_p(st), 0))
                return out
            stream = torch.cuda.current_stream(x.device)
            if stream.cuda_stream == 0:           # capture cannot run on the NULL stream
                if not hasattr(self, '_graph_stream'):
                    self._graph_stream = torch.cuda.Stream(x.device)
                side = self._graph_stream
                side.wait_stream(stream)
                with torch.cuda.stream(side):
                    out = self._graph_call(x, b, h, w, side)
                stream.wait_stream(side)
                return out
            return self._graph_call(x, b, h, w, stream)

    def _graph_call(self, x, b, h, w, stream):
        key = (str(x.device), stream.cuda_stream, b, h, w)
        if key not in self._static:
            ws = torch.empty(self.workspace_bytes(b, h, w), dtype=torch.uint8, device=x.device)
            self._static[key] = (torch.empty_like(x), torch.empty(self.output_shape(b, h, w), dtype=torch.float32, device=x.device), ws)
        xin, out, ws = self._static[key]
        xin.copy_(x)
        _lib.check(None, _lib.load().fdsr_hat_forward(self._handle(), _ptr(xin), b, h, w, _ptr(out), _ptr(ws), ws.numel(),
                                                      C.c_void_p(stream.cuda_stream), _lib.FDSR_HAT_GRAPH))
        return out.clone()

    def debug_tensor(self, name, x):
        """The named tap of one forward (arch.tap_names), NCHW at the padded size."""
        x = self._check(x)
        b, _, h, w = x.shape
        if name not in tap_names(self.cfg):
            raise KeyError(name)
        self.sync_weights(x.device)
        hp, wp = self.padded(h, w)
        with torch.cuda.device(x.device):
            ws = self.workspace(b, h, w, x.device)
            cap = b * hp * wp * self.upscale ** 2 * max(self.cfg.embed_dim, 64)
            out = torch.empty(cap, dtype=torch.float32, device=x.device)
            dims = (C.c_int * 3)()
            st = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(None, _lib.load().fdsr_hat_debug_tensor(self._handle(), name.encode(), _ptr(x), b, h, w, _ptr(out), cap, dims,
                                                               _ptr(ws), ws.numel(), C.c_void_p(st)))
        th, tw, tc = dims[0], dims[1], dims[2]
        return out[:b * th * tw * tc].view(b, th, tw, tc).permute(0, 3, 1, 2).contiguous()


def load_synthetic(model, seed=0):
    """Fill a HAT with synth.synth_hat's weights (tests, timing, smoke runs)."""
    from ..synth import synth_hat
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth_hat(model.cfg, seed).items()}
    model.load_state_dict(sd, strict=False)
    return model
