"""ConditionalNAFNet on the HIP engine (include/fdsr.h: fdsr_nafnet_*): an nn.Module that owns the reference's parameters
under the reference's names -- `latest_G.pth` loads with load_state_dict(strict=True) -- and whose forward runs the device
kernels.  Training runs two ways, both on the engine's own backward (there is no PyTorch fallback):
  * train_grads / optim_step: the IR-SDE l1 / l2 loss head and Adam / AdamW / Lion built into the library
    (denoising_model.DenoisingModel drives them);
  * torch autograd: after model.requires_grad_(True), forward records a node (_NAFNetFunction) whose backward is
    fdsr_nafnet_backward, so any loss, torch.optim, an EMA copy or DDP hooks stand around the network as they do around the
    reference's.  One forward's activations are kept at a time: each forward wants its backward before the next forward
    under grad, and a backward runs once (no retain_graph, no double backward); anything else raises the engine's
    stale-ticket error.  Parameters are created with requires_grad=False, so nothing changes for callers who do not opt in."""
import contextlib
import ctypes as C

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from .. import _lib
from ..scene import check_origins
from .arch import NAFNetConfig, param_schema, tap_names


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()


class _NAFNetFunction(torch.autograd.Function):
    """out = module(x, cond, time) with the activations kept (fdsr_nafnet_forward_train); backward is fdsr_nafnet_backward on
    the current stream.  Inputs: the module (no tensor), x, cond, time [B] fp32, then every parameter in state_dict order --
    the parameters are inputs only so that autograd routes their gradients; the engine reads its own copies."""

    @staticmethod
    def forward(ctx, module, x, cond, time, *params):
        ctx.module = module
        ctx.shape = tuple(x.shape)
        out, ctx.ticket, ctx.ws = module._forward_train(x, cond, time)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, dout):
        m, (b, _, h, w) = ctx.module, ctx.shape
        need = ctx.needs_input_grad
        dev = dout.device
        dout = dout.float().contiguous()
        lib, hd = _lib.load(), m._handle()
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            dx = torch.empty_like(dout) if need[1] else None
            dc = torch.empty_like(dout) if need[2] else None
            _lib.check(None, lib.fdsr_nafnet_backward(hd, ctx.ticket, _ptr(dout), _ptr(dx), _ptr(dc), b, h, w, _ptr(ctx.ws), ctx.ws.numel(), st))
            pg = [None] * (len(need) - 4)
            if any(need[4:]):
                sizes = [p.numel() for _, p in m.named_reference_parameters()]
                flat = torch.empty(sum(sizes), dtype=torch.float32, device=dev)
                _lib.check(None, lib.fdsr_nafnet_copy_grads(hd, _ptr(flat), flat.numel(), st))
                views = flat.split(sizes)
                pg = [v.view(shape) if n else None for v, shape, n in zip(views, m.schema.values(), need[4:])]
        return (None, dx, dc, None) + tuple(pg)


class ConditionalNAFNet(nn.Module):
    def __init__(self, img_channel=3, width=16, middle_blk_num=1, enc_blk_nums=(), dec_blk_nums=(), upscale=1):
        super().__init__()
        self.upscale = upscale
        self.cfg = NAFNetConfig(img_channel, width, middle_blk_num, list(enc_blk_nums), list(dec_blk_nums))
        self.padder_size = self.cfg.padder_size
        self.schema = param_schema(self.cfg)
        # flat registration under dotted names is not allowed by nn.Module, so the tensors live in a ParameterDict-like
        # table of their own and state_dict / load_state_dict speak the reference's keys (see _save_to_state_dict)
        self._names = list(self.schema)
        for i, (k, shape) in enumerate(self.schema.items()):
            self.register_parameter('p%d' % i, nn.Parameter(torch.zeros(shape), requires_grad=False))
        self._h = None
        self._uploaded = None      # (device, versions) of the last upload
        self._ws = {}

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

    def named_reference_parameters(self):
        return [(k, getattr(self, 'p%d' % i)) for i, k in enumerate(self._names)]

    # ---- the engine ----
    def _handle(self):
        if self._h is None:
            lib = _lib.load()
            c = _lib.FdsrNafnetConfig()
            c.img_channel, c.width, c.middle_blk_num = self.cfg.img_channel, self.cfg.width, self.cfg.middle_blk_num
            c.n_levels = len(self.cfg.enc_blk_nums)
            if c.n_levels > _lib.FDSR_NAFNET_MAX_LEVELS:
                raise ValueError('at most %d levels' % _lib.FDSR_NAFNET_MAX_LEVELS)
            for i, (e, d) in enumerate(zip(self.cfg.enc_blk_nums, self.cfg.dec_blk_nums)):
                c.enc_blk_nums[i], c.dec_blk_nums[i] = e, d
            h = C.c_void_p()
            _lib.check(None, lib.fdsr_nafnet_create(C.byref(c), C.byref(h)))
            self._h = h
        return self._h

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and _lib._lib is not None:
            _lib._lib.fdsr_nafnet_destroy(h)
            self._h = None

    def __getstate__(self):
        """What copy.deepcopy and pickle carry: the parameters and the configuration.  The engine object and what belongs to
        it stay behind -- the handle, the upload stamp, the workspaces, the graph stream, and the precision, the training
        precision and the schedule that were set on that handle -- so a copy creates an engine of its own (in 'f32', training
        in 'f32', without a schedule) on first use."""
        d = dict(self.__dict__)
        d['_h'], d['_uploaded'], d['_ws'] = None, None, {}
        for k in ('_graph_stream', '_precision', '_train_precision', '_sde_T', '_noise_tiles'):
            d.pop(k, None)
        return d

    def engine_schema(self):
        """[(key, shape)] as the library lists them (fdsr_nafnet_weight_info)."""
        lib, h = _lib.load(), self._handle()
        out = []
        for i in range(lib.fdsr_nafnet_num_weights(h)):
            key, shape, nd = C.create_string_buffer(256), (C.c_int64 * 4)(), C.c_int()
            _lib.check(None, lib.fdsr_nafnet_weight_info(h, i, key, 256, shape, C.byref(nd)))
            out.append((key.value.decode(), tuple(shape[:nd.value])))
        return out

    def sync_weights(self, device):
        """Upload the parameters when they changed since the last upload (tensor versions, as unet.py does).  The first upload,
        and any in a 16-bit mode, packs on the host.  Once the engine has the weights, a module that requires grad (a torch
        optimizer steps its fp32 CUDA parameters in place) hands them over on the device: one torch.cat and
        fdsr_nafnet_set_weights_flat, no host round trip."""
        params = [p for _, p in self.named_reference_parameters()]
        stamp = (str(device), tuple((p.data_ptr(), p._version) for p in params))
        if stamp == self._uploaded:
            return
        lib, h = _lib.load(), self._handle()
        if (self._uploaded is not None and self._uploaded[0] == stamp[0] and self.precision == 'f32' and any(p.requires_grad for p in params)
                and all(p.is_cuda and p.dtype == torch.float32 and str(p.device) == stamp[0] for p in params)):
            with torch.cuda.device(device), torch.no_grad():
                flat = torch.cat([p.detach().reshape(-1) for p in params])
                st = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
                _lib.check(None, lib.fdsr_nafnet_set_weights_flat(h, _ptr(flat), flat.numel(), st))
            self._uploaded = stamp
            return
        with torch.cuda.device(device):
            for k, p in zip(self._names, params):
                a = p.detach().to('cpu', torch.float32).contiguous()
                shape = (C.c_int64 * a.dim())(*a.shape)
                _lib.check(None, lib.fdsr_nafnet_load_weight(h, k.encode(), _ptr(a), shape, a.dim()))
        self._uploaded = stamp

    def workspace(self, b, h, w, device):
        need = C.c_size_t()
        _lib.check(None, _lib.load().fdsr_nafnet_workspace_bytes(self._handle(), b, h, w, C.byref(need)))
        key = (str(device), torch.cuda.current_stream(device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need.value:
            ws = self._ws[key] = torch.empty(need.value, dtype=torch.uint8, device=device)
        return ws

    @staticmethod
    def _check_pair(x, cond):
        if not (x.is_cuda and cond.is_cuda and x.dim() == 4 and x.shape[1] == 3 and x.shape == cond.shape):
            raise ValueError('ConditionalNAFNet takes two [B,3,H,W] tensors on the GPU (there is no CPU path)')
        return x.float().contiguous(), cond.float().contiguous()

    def _times(self, time, b, device):
        if isinstance(time, (int, float)):
            time = torch.tensor([time])
        t = torch.as_tensor(time).to(device=device, dtype=torch.float32).reshape(-1)
        if t.numel() == 1:
            t = t.expand(b)
        if t.numel() != b:
            raise ValueError('time must be a scalar or one value per image')
        return t.contiguous()

    def _train_ws(self, b, h, w, device):
        need = C.c_size_t()
        _lib.check(None, _lib.load().fdsr_nafnet_train_workspace_bytes(self._handle(), b, h, w, C.byref(need)))
        key = ('train', str(device))
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need.value:
            ws = self._ws[key] = torch.empty(need.value, dtype=torch.uint8, device=device)
        return ws

    def _forward_train(self, x, cond, t):
        """(out, ticket, workspace) of fdsr_nafnet_forward_train: forward's out, with the activations kept for one backward."""
        b, _, h, w = x.shape
        with torch.cuda.device(x.device):
            out = torch.empty_like(x)
            ws = self._train_ws(b, h, w, x.device)
            ticket = C.c_int64()
            st = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(None, _lib.load().fdsr_nafnet_forward_train(self._handle(), _ptr(x), _ptr(cond), _ptr(t), _ptr(out), b, h, w, _ptr(ws),
                                                                   ws.numel(), C.byref(ticket), C.c_void_p(st)))
        return out, ticket.value, ws

    def forward(self, inp, cond, time):
        x, cond = self._check_pair(inp, cond)
        b, _, h, w = x.shape
        self.sync_weights(x.device)
        params = [p for _, p in self.named_reference_parameters()]
        with torch.cuda.device(x.device):
            t = self._times(time, b, x.device)
            if torch.is_grad_enabled() and (x.requires_grad or cond.requires_grad or any(p.requires_grad for p in params)):
                return _NAFNetFunction.apply(self, x, cond, t, *params)
            out = torch.empty_like(x)
            ws = self.workspace(b, h, w, x.device)
            st = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(None, _lib.load().fdsr_nafnet_forward(self._handle(), _ptr(x), _ptr(cond), _ptr(t), _ptr(out), b, h, w,
                                                             _ptr(ws), ws.numel(), C.c_void_p(st)))
        return out

    def debug_tensor(self, name, inp, cond, time):
        """The named tap of one forward (arch.tap_names), NCHW at the tap's padded size."""
        x, cond = self._check_pair(inp, cond)
        b, _, h, w = x.shape
        self.sync_weights(x.device)
        pad = self.padder_size
        hp, wp = -(-h // pad) * pad, -(-w // pad) * pad
        with torch.cuda.device(x.device):
            t = self._times(time, b, x.device)
            cap = b * hp * wp * self.cfg.width
            out = torch.empty(cap, dtype=torch.float32, device=x.device)
            dims = (C.c_int * 3)()
            ws = self.workspace(b, h, w, x.device)
            st = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(None, _lib.load().fdsr_nafnet_debug_tensor(self._handle(), name.encode(), _ptr(x), _ptr(cond), _ptr(t), b, h, w,
                                                                  _ptr(out), cap, dims, _ptr(ws), ws.numel(), C.c_void_p(st)))
        th, tw, tc = dims[0], dims[1], dims[2]
        return out[:b * th * tw * tc].view(b, th, tw, tc).permute(0, 3, 1, 2).contiguous()

    # ---- precision of the GEMMs and storage of the activations (include/fdsr.h: fdsr_nafnet_set_precision, _set_storage) ----
    PRECISIONS = ('f32', 'f16x3', 'f16')

    @property
    def precision(self):
        return getattr(self, '_precision', 'f32')

    def set_precision(self, mode):
        """'f32' (exact, the default), 'f16x3' (fp32-grade, three f16 MFMAs per product, fp32 activations) or 'f16' (PSNR-grade:
        f16 activations in memory, one f16 MFMA per product, fp32 accumulators).  forward, debug_tensor and sample follow the
        mode; training runs in 'f32' only: train_grads and optim_step raise what the engine says under 'f16x3' and 'f16'.
        'f16x3' and 'f16' are two settings of one switch: 'f16' is not reached from 'f16x3' directly (ValueError, as the engine
        refuses f16 storage under the f16x3 precision) but through 'f32'."""
        if mode not in self.PRECISIONS:
            raise ValueError('precision must be one of %s, not %r' % (self.PRECISIONS, mode))
        if mode == 'f16' and self.precision == 'f16x3':
            raise ValueError("precision 'f16' is not set over 'f16x3': set 'f32' first")
        lib, h = _lib.load(), self._handle()
        dev = next(self.parameters()).device
        with torch.cuda.device(dev) if dev.type == 'cuda' else contextlib.nullcontext():
            # two settings of one switch in the engine: 'f16' is f16 storage over the F32 GEMM precision
            if mode != 'f16':
                _lib.check(None, lib.fdsr_nafnet_set_storage(h, _lib.FDSR_NAF_STORE_F32))
            _lib.check(None, lib.fdsr_nafnet_set_precision(h, _lib.PRECISIONS['f32' if mode == 'f16' else mode]))
            if mode == 'f16':
                _lib.check(None, lib.fdsr_nafnet_set_storage(h, _lib.FDSR_NAF_STORE_F16))
        self._precision = mode

    # ---- storage of the activations a training call keeps (include/fdsr.h: fdsr_nafnet_set_train_storage) ----
    TRAIN_PRECISIONS = ('f32', 'f16')

    @property
    def train_precision(self):
        return getattr(self, '_train_precision', 'f32')

    def set_train_precision(self, mode):
        """'f32' (the default) or 'f16': mixed-precision training.  Under 'f16' train_grads, the autograd bridge and optim_step
        run the f16-storage forward into a training workspace of about half the bytes and keep every gradient in fp32 (no loss
        scaling); check_saturation after train_grads tells whether a stored value left the f16 range.  The setting is the
        training calls' own: forward, debug_tensor and sample follow set_precision as before, and it takes effect only while
        that is 'f32' (under 'f16x3' and 'f16' training refuses as it always did)."""
        if mode not in self.TRAIN_PRECISIONS:
            raise ValueError('train precision must be one of %s, not %r' % (self.TRAIN_PRECISIONS, mode))
        dev = next(self.parameters()).device
        with torch.cuda.device(dev) if dev.type == 'cuda' else contextlib.nullcontext():
            _lib.check(None, _lib.load().fdsr_nafnet_set_train_storage(
                self._handle(), _lib.FDSR_NAF_STORE_F16 if mode == 'f16' else _lib.FDSR_NAF_STORE_F32))
        self._train_precision = mode

    def check_saturation(self):
        """f16x3 clamps GEMM inputs beyond +-65504 and raises a sticky flag, f16 does so for every value it stores or stages:
        synchronises, reads and clears it.  Raises _lib.FdsrSaturated when it was set (re-run the calls since the last check
        in 'f32'); a no-op in 'f32'.  Training under set_train_precision('f16') raises the same flag from the
        stores of its forward: the gradients of that train_grads are then not to be used."""
        dev = next(self.parameters()).device
        with torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            rc = _lib.load().fdsr_nafnet_check_saturation(self._handle(), C.c_void_p(st))
        if rc == _lib.FDSR_E_SATURATED:
            msg = _lib.load().fdsr_last_error(None)
            raise _lib.FdsrSaturated(rc, msg.decode() if msg else '?')
        _lib.check(None, rc)

    def set_sde(self, thetas, sigmas, sigma_bars, dt, device, thetas_cumsum=None):
        T = thetas.numel() - 1
        arr = [a.detach().to('cpu', torch.float32).contiguous() for a in (thetas, sigmas, sigma_bars)]
        f = C.POINTER(C.c_float)
        with torch.cuda.device(device):
            _lib.check(None, _lib.load().fdsr_nafnet_set_sde(self._handle(), T, *[C.cast(a.data_ptr(), f) for a in arr], float(dt)))
            if thetas_cumsum is not None:
                cum = thetas_cumsum.detach().to('cpu', torch.float32).contiguous()
                _lib.check(None, _lib.load().fdsr_nafnet_set_thetas_cumsum(self._handle(), T, C.cast(cum.data_ptr(), f)))

    # ---- training ----
    LOSSES = {'l1': 0, 'l2': 1}
    OPTIMIZERS = {'Adam': 0, 'AdamW': 1, 'Lion': 2}

    def train_grads(self, state, cond, gt, timesteps, loss_type='l1', weight=1.0, is_weighted=False):
        """The loss of DenoisingModel.optimize_parameters and its gradients (kept in the engine: read_grad).  Returns a
        device tensor [1 + B]: the loss, then every image's own mean."""
        x, cond = self._check_pair(state, cond)
        gt = gt.to(x.device).float().contiguous()
        if gt.shape != x.shape:
            raise ValueError('GT must have the state\'s shape')
        if loss_type not in self.LOSSES:
            raise ValueError('invalid loss type %s' % (loss_type,))
        b, _, h, w = x.shape
        self.sync_weights(x.device)
        lib, hd = _lib.load(), self._handle()
        with torch.cuda.device(x.device):
            t = torch.as_tensor(timesteps).to(x.device).reshape(-1).to(torch.int32).contiguous()
            if t.numel() != b:
                raise ValueError('one timestep per image')
            ws = self._train_ws(b, h, w, x.device)
            out = torch.empty(1 + b, dtype=torch.float32, device=x.device)
            st = torch.cuda.current_stream(x.device).cuda_stream
            code = self.LOSSES[loss_type] | (_lib.FDSR_NAFNET_LOSS_WEIGHTED if is_weighted else 0)
            _lib.check(None, lib.fdsr_nafnet_train_grads(hd, _ptr(x), _ptr(cond), _ptr(gt), _ptr(t), code, float(weight), _ptr(out), b, h, w,
                                                         _ptr(ws), ws.numel(), C.c_void_p(st)))
        return out

    def train_workspace_bytes(self, b, h, w):
        need = C.c_size_t()
        _lib.check(None, _lib.load().fdsr_nafnet_train_workspace_bytes(self._handle(), b, h, w, C.byref(need)))
        return need.value

    def read_grad(self, key):
        shape = self.schema[key]
        out = torch.empty(shape, dtype=torch.float32)
        _lib.check(None, _lib.load().fdsr_nafnet_read_grad(self._handle(), key.encode(), _ptr(out)))
        return out

    def grads(self):
        return {k: self.read_grad(k) for k in self._names}

    def grad_buffer(self):
        """(device pointer, floats) of the flat gradient buffer."""
        p, cnt = C.c_void_p(), C.c_size_t()
        _lib.check(None, _lib.load().fdsr_nafnet_grad_buffer(self._handle(), C.byref(p), C.byref(cnt)))
        return p.value, cnt.value

    def optim_step(self, kind, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0):
        """One optimizer step from the engine's gradients; afterwards the nn.Parameters hold the new values (device copies
        into their storage, which leaves their versions -- the upload stamp -- as they were)."""
        params = self.named_reference_parameters()
        dev = params[0][1].device
        lib, hd = _lib.load(), self._handle()
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            _lib.check(None, lib.fdsr_nafnet_optim_step(hd, self.OPTIMIZERS[kind], float(lr), float(betas[0]), float(betas[1]), float(eps),
                                                        float(weight_decay), st))
            for k, p in params:
                if p.dtype != torch.float32 or not p.is_contiguous():
                    raise TypeError('training needs contiguous fp32 parameters')
                _lib.check(None, lib.fdsr_nafnet_read_weight(hd, k.encode(), _ptr(p), 1, st))
        self._uploaded = (str(dev), tuple((p.data_ptr(), p._version) for _, p in params))

    def optim_state(self, key):
        shape = self.schema[key]
        m, v, step = torch.empty(shape), torch.empty(shape), C.c_int64()
        _lib.check(None, _lib.load().fdsr_nafnet_optim_get_state(self._handle(), key.encode(), _ptr(m), _ptr(v), C.byref(step)))
        return m, v, step.value

    def set_optim_state(self, key, exp_avg, exp_avg_sq, step):
        dev = next(self.parameters()).device
        self.sync_weights(dev)
        m = None if exp_avg is None else exp_avg.detach().to('cpu', torch.float32).contiguous()
        v = None if exp_avg_sq is None else exp_avg_sq.detach().to('cpu', torch.float32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(None, _lib.load().fdsr_nafnet_optim_set_state(self._handle(), key.encode(), _ptr(m), _ptr(v), int(step)))

    def sample(self, state, cond, noise=None, seed=0, first_image=0, graph=False, ode=False, trajectory=False):
        """IRSDE.reverse_sde / reverse_ode in one engine call (set_sde first).  noise [T,B,3,H,W] or None (engine draws)."""
        x, cond = self._check_pair(state, cond)
        b, _, h, w = x.shape
        self.sync_weights(x.device)
        flags = (_lib.FDSR_SAMPLE_GRAPH if graph else 0) | (_lib.FDSR_NAFNET_ODE if ode else 0)
        with torch.cuda.device(x.device):
            if noise is not None:
                noise = noise.to(x.device, torch.float32).contiguous()
                if noise.dim() != 5 or tuple(noise.shape[1:]) != tuple(x.shape) or noise.shape[0] != self._T():
                    raise ValueError('noise must be [T,B,3,H,W] with the schedule\'s T')
            out = torch.empty_like(x)
            traj = torch.empty((self._T(),) + tuple(x.shape), dtype=torch.float32, device=x.device) if trajectory else None
            ws = self.workspace(b, h, w, x.device)
            stream = torch.cuda.current_stream(x.device)
            if graph and stream.cuda_stream == 0:
                if not hasattr(self, '_graph_stream'):
                    self._graph_stream = torch.cuda.Stream(x.device)
                side = self._graph_stream
                side.wait_stream(stream)
                with torch.cuda.stream(side):
                    ws = self.workspace(b, h, w, x.device)
                    self._sample_call(x, cond, noise, seed, first_image, flags, out, traj, b, h, w, ws, side.cuda_stream)
                stream.wait_stream(side)
            else:
                self._sample_call(x, cond, noise, seed, first_image, flags, out, traj, b, h, w, ws, stream.cuda_stream)
        return (out, traj) if trajectory else out

    def _T(self):
        if getattr(self, '_sde_T', None) is None:
            raise RuntimeError('set an IRSDE first (IRSDE.set_model)')
        return self._sde_T

    def _sample_call(self, x, cond, noise, seed, first_image, flags, out, traj, b, h, w, ws, st):
        _lib.check(None, _lib.load().fdsr_nafnet_sample(self._handle(), _ptr(x), _ptr(cond), _ptr(noise), int(seed), int(first_image), flags,
                                                        _ptr(out), _ptr(traj), b, h, w, _ptr(ws), ws.numel(), C.c_void_p(st)))

    def set_noise_tiles(self, origins, scene_w):
        """Tile-addressed noise (include/fdsr.h: fdsr_nafnet_set_noise_tiles): origins [n,2] int32 on the device, (y0, x0) of image
        i of a call in a scene `scene_w` wide.  Until clear_noise_tiles, what sample draws itself (noise=None) and randn are the
        crops of the scene's planes at those origins; first_image must then be 0.  The table is read when the kernels run: the
        module keeps the tensor, and the caller may rewrite it in place between calls."""
        _lib.check(None, _lib.load().fdsr_nafnet_set_noise_tiles(self._handle(), _ptr(origins), check_origins(origins), int(scene_w)))
        self._noise_tiles = (origins, int(scene_w))

    def clear_noise_tiles(self):
        _lib.check(None, _lib.load().fdsr_nafnet_set_noise_tiles(self._handle(), None, 0, 0))
        self._noise_tiles = None

    def randn(self, b, h, w, plane, seed, first_image=0, device=None):
        """Plane `plane` of the engine's own noise stream (include/fdsr.h), [B,3,H,W]; under set_noise_tiles, the B crops of the
        scene's plane at the table's first B origins (first_image must then be 0)."""
        device = device or next(self.parameters()).device
        tiles = getattr(self, '_noise_tiles', None)
        if tiles is not None and (int(first_image) != 0 or b > tiles[0].shape[0]):
            raise ValueError('randn under a noise-tile table of %d: first_image must be 0 and B at most that (got %d, %d)'
                             % (tiles[0].shape[0], first_image, b))
        out = torch.empty((b, 3, h, w), dtype=torch.float32, device=device)
        with torch.cuda.device(device):
            st = torch.cuda.current_stream(device).cuda_stream
            if tiles is not None:
                _lib.check(None, _lib.load().fdsr_nafnet_randn_tiles(_ptr(out), b, h, w, plane, int(seed), _ptr(tiles[0]), tiles[1], C.c_void_p(st)))
            else:
                _lib.check(None, _lib.load().fdsr_nafnet_randn(_ptr(out), b, h, w, plane, int(seed), int(first_image), C.c_void_p(st)))
        return out


def upscale(x, scale):
    """util.upscale on the device: F.interpolate(x, scale_factor=scale, mode='bicubic') for fp32 NCHW CUDA tensors."""
    if not x.is_cuda or x.dim() != 4:
        raise ValueError('upscale takes a [B,C,H,W] tensor on the GPU')
    x = x.float().contiguous()
    b, c, h, w = x.shape
    out = torch.empty((b, c, h * scale, w * scale), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        st = torch.cuda.current_stream(x.device).cuda_stream
        _lib.check(None, _lib.load().fdsr_upscale_bicubic_f32(_ptr(x), _ptr(out), b, c, h, w, int(scale), C.c_void_p(st)))
    return out
