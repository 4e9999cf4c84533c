"""TransENet on the HIP engine (include/fdsr.h: fdsr_transenet_*): an nn.Module that takes the constructor arguments of the
reference's TransENet (MSI_SR_model/model/transenet.py) with the reference's defaults, owns its parameters under the
reference's names -- `generator_param.pkl` loads with load_state_dict -- and whose forward runs the device kernels.  Inference
only, exact fp32; there is no PyTorch fallback.  As in the reference, a module built for hr_patch_size computes images of LR
height hr_patch_size / scale only (the inverse patch rearrange is called with h = hr_patch_size // 8); the width is free."""
import ctypes as C

import numpy as np
import torch
import torch.nn as nn

from .. import _lib
from ..swinir.model import to_u8  # noqa: F401  (save_img1 is the same function in transenet.py)
from .arch import MIN_NUM_PATCHES, PATCH, DIM, TransENetConfig, state_schema, tap_names


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()


class TransENet(nn.Module):
    def __init__(self, n_feats=64, scale=4, n_basic_modules=10, n_colors=3, hr_patch_size=256, back_projection_iters=10, en_depth=8,
                 de_depth=1, conv=None):
        """n_basic_modules and back_projection_iters are unused by the reference too; conv must be its default_conv (or None)."""
        super().__init__()
        if conv is not None and getattr(conv, '__name__', '') != 'default_conv':
            raise NotImplementedError('TransENet on the HIP engine runs the reference\'s default_conv only')
        if n_colors != 3:
            raise NotImplementedError('TransENet on the HIP engine does not run n_colors %r (only 3)' % (n_colors,))
        if scale not in (2, 3, 4, 8):
            raise NotImplementedError('TransENet on the HIP engine does not run scale %r (only 2, 3, 4, 8)' % (scale,))
        image_size = hr_patch_size // scale
        # the reference's two constructor assertions
        if hr_patch_size % scale or image_size % PATCH:
            raise ValueError('Image dimensions must be divisible by the patch size: hr_patch_size %r / scale %r is no multiple of 8'
                             % (hr_patch_size, scale))
        if (image_size // PATCH) ** 2 <= MIN_NUM_PATCHES:
            raise ValueError('your number of patches (%d) is way too small for attention to be effective: the LR side '
                             'hr_patch_size / scale must be at least 32' % ((image_size // PATCH) ** 2))
        self.cfg = TransENetConfig(n_feats, scale, n_colors, hr_patch_size, en_depth, de_depth)
        self.scale, self.hr_patch_size, self.patch_size = scale, hr_patch_size, PATCH
        self.schema = state_schema(self.cfg)
        # dotted names cannot be registered on an nn.Module: the tensors live under p<i> and state_dict / load_state_dict speak
        # the reference's keys
        self._names = list(self.schema)
        for i, shape in enumerate(self.schema.values()):
            self.register_parameter('p%d' % i, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self._h = None
        self._uploaded = {}
        self._ws = {}
        self._static = {}
        self._handle()     # refuses what the kernels do not cover (n_feats, depths) with the library's message

    # ---- the reference's keys ----
    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for i, k in enumerate(self._names):
            p = getattr(self, 'p%d' % i)
            destination[prefix + k] = p if keep_vars else p.detach()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for i, k in enumerate(self._names):
            key = prefix + k
            if key not in state_dict:
                if strict:
                    missing_keys.append(key)
                continue
            src, p = state_dict[key], getattr(self, 'p%d' % i)
            if tuple(src.shape) != tuple(p.shape):
                error_msgs.append('size mismatch for %s: copying a param with shape %s from checkpoint, the shape in current '
                                  'model is %s.' % (key, tuple(src.shape), tuple(p.shape)))
                continue
            with torch.no_grad():
                p.copy_(src)
        if strict:
            known = {prefix + k for k in self._names}
            unexpected_keys += [k for k in state_dict if k.startswith(prefix) and k not in known]

    def load_reference_state_dict(self, state_dict, strict=False):
        """The reference's own TransENet.load_state_dict: a known key is copied; a shape mismatch is an error except under 'tail'
        (a checkpoint of another scale keeps its body); an unknown key counts only with strict, and not under 'tail'; with strict
        every key of the model must be there."""
        own = self.state_dict()
        for name, param in state_dict.items():
            if name in own:
                if tuple(param.shape) != tuple(own[name].shape):
                    if 'tail' in name:
                        continue
                    raise RuntimeError('While copying the parameter named {}, whose dimensions in the model are {} and whose '
                                       'dimensions in the checkpoint are {}.'.format(name, tuple(own[name].shape), tuple(param.shape)))
                with torch.no_grad():
                    own[name].copy_(param)     # bumps _version: the next forward uploads it
            elif strict and 'tail' not in name:
                raise KeyError('unexpected key "{}" in state_dict'.format(name))
        if strict:
            missing = set(own) - set(state_dict)
            if missing:
                raise KeyError('missing keys in state_dict: "{}"'.format(sorted(missing)))

    def named_reference_parameters(self):
        return [(k, getattr(self, 'p%d' % i)) for i, k in enumerate(self._names)]

    # ---- the engine ----
    def _handle(self):
        if self._h is None:
            cfg = self.cfg
            c = _lib.FdsrTransenetConfig()
            c.n_feats, c.scale, c.n_colors, c.en_depth, c.de_depth = cfg.n_feats, cfg.scale, cfg.n_colors, cfg.en_depth, cfg.de_depth
            h = C.c_void_p()
            try:
                _lib.check(None, _lib.load().fdsr_transenet_create(C.byref(c), C.byref(h)))
            except _lib.FdsrError as e:
                raise NotImplementedError(str(e)) from e
            self._h = h
        return self._h

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and _lib._lib is not None:
            _lib._lib.fdsr_transenet_destroy(h)
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
                _lib.check(None, lib.fdsr_transenet_load(h, k.encode(), _ptr(a), shape, a.dim()))
                self._uploaded[k] = stamp

    def workspace_bytes(self, b, h, w):
        need = C.c_size_t()
        _lib.check(None, _lib.load().fdsr_transenet_workspace_bytes(self._handle(), b, h, w, C.byref(need)))
        return need.value

    def workspace(self, b, h, w, device=None):
        device = device or next(self.parameters()).device
        need = self.workspace_bytes(b, h, w)
        key = (str(device), torch.cuda.current_stream(device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=device)
        return ws

    def _check(self, x):
        if not (torch.is_tensor(x) and x.dim() == 4 and x.shape[1] == 3):
            raise ValueError('TransENet takes a [B,3,H,W] tensor on the GPU (there is no CPU path)')
        h, w = int(x.shape[2]), int(x.shape[3])
        if h % PATCH or w % PATCH:
            raise ValueError('TransENet takes sides that are multiples of the patch size 8, not %dx%d' % (h, w))
        if h * self.scale != self.hr_patch_size:
            raise ValueError("TransENet built with hr_patch_size %d at scale %d computes inputs of height %d only, not %d: the "
                             "reference's rearrange(feat_ups, 'b (h w) (p1 p2 c) -> b c (h p1) (w p2)', h=self.hr_patch_size // p) "
                             "fixes the HR height (the width is inferred)" % (self.hr_patch_size, self.scale,
                                                                              self.hr_patch_size // self.scale, h))
        if not x.is_cuda:
            raise ValueError('TransENet takes a [B,3,H,W] tensor on the GPU (there is no CPU path)')
        return x.float().contiguous()

    def output_shape(self, b, h, w):
        return (b, 3, h * self.scale, w * self.scale)

    def forward(self, x, graph=False):
        """[B,3,H,W] fp32 on the GPU, H = hr_patch_size / scale -> [B,3,H*scale,W*scale].  graph=True replays one captured graph
        per (B, H, W): the call copies x into, and the result out of, buffers that the graph keeps."""
        x = self._check(x)
        b, _, h, w = x.shape
        self.sync_weights(x.device)
        lib, hd = _lib.load(), self._handle()
        with torch.cuda.device(x.device):
            if not graph:
                ws = self.workspace(b, h, w, x.device)
                out = torch.empty(self.output_shape(b, h, w), dtype=torch.float32, device=x.device)
                st = torch.cuda.current_stream(x.device).cuda_stream
                _lib.check(None, lib.fdsr_transenet_forward(hd, _ptr(x), b, h, w, _ptr(out), _ptr(ws), ws.numel(), C.c_void_p(st), 0))
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
        _lib.check(None, _lib.load().fdsr_transenet_forward(self._handle(), _ptr(xin), b, h, w, _ptr(out), _ptr(ws), ws.numel(),
                                                            C.c_void_p(stream.cuda_stream), _lib.FDSR_TRANSENET_GRAPH))
        return out.clone()

    def debug_tensor(self, name, x):
        """The named tap of one forward (arch.tap_names), NCHW; a token tensor is [B, 512, h, w] over the grid of patches."""
        x = self._check(x)
        b, _, h, w = x.shape
        if name not in tap_names(self.cfg):
            raise KeyError(name)
        self.sync_weights(x.device)
        with torch.cuda.device(x.device):
            ws = self.workspace(b, h, w, x.device)
            # the largest: n_feats channels at HR; tokens are DIM per 64 pixels
            cap = b * h * w * self.scale ** 2 * max(self.cfg.n_feats, DIM // (PATCH * PATCH))
            out = torch.empty(cap, dtype=torch.float32, device=x.device)
            dims = (C.c_int * 3)()
            st = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(None, _lib.load().fdsr_transenet_debug_tensor(self._handle(), name.encode(), _ptr(x), b, h, w, _ptr(out), cap, dims,
                                                                     _ptr(ws), ws.numel(), C.c_void_p(st)))
        th, tw, tc = dims[0], dims[1], dims[2]
        return out[:b * th * tw * tc].view(b, th, tw, tc).permute(0, 3, 1, 2).contiguous()


def load_synthetic(model, seed=0):
    """Fill a TransENet with synth.synth_transenet's weights (tests, timing, smoke runs)."""
    from ..synth import synth_transenet
    sd = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in synth_transenet(model.cfg, seed).items()}
    model.load_state_dict(sd, strict=True)
    return model
