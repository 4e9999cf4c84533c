"""What the comparator modules (swinir.SwinIR, hat.HAT, transenet.TransENet, hsenet.HSENet) share: an nn.Module over one engine handle of
include/fdsr.h's fdsr_<family>_* functions.  The tensors live under p<i> (dotted names cannot be registered on an nn.Module)
and state_dict / load_state_dict speak the reference's keys.

A family sets `_family` ('hat': the fdsr_hat_ symbols and FDSR_HAT_GRAPH) and `_tap_names` (its arch.tap_names), fills
self.cfg, self._names and p<i> in __init__ and ends it with _init_engine(), and supplies _fill_config(), _check(x),
output_shape(b, h, w), _debug_capacity(b, h, w) and named_reference_parameters().  Its key rules are the small methods
_tensor, _is_buffer, _buffer_differs and _repeats."""
import ctypes as C

import torch
import torch.nn as nn

from . import _lib


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p()


class EngineModule(nn.Module):
    _family = None
    _tap_names = None

    def _init_engine(self):
        self._h = None
        self._uploaded = {}
        self._ws = {}
        self._static = {}
        self._handle()     # refuses what the kernels do not cover with the library's message

    def _fn(self, what):
        return getattr(_lib.load(), 'fdsr_%s_%s' % (self._family, what))

    # ---- the reference's keys ----
    def _tensor(self, i, k):
        return getattr(self, 'p%d' % i)

    def _is_buffer(self, k):
        """A function of the geometry, never sent to the device."""
        return False

    def _buffer_differs(self, src, p):
        raise NotImplementedError

    def _repeats(self, k, key, src, state_dict, prefix, error_msgs):
        """True: `key` has no tensor of its own to copy into."""
        return False

    def _save_to_state_dict(self, destination, prefix, keep_vars):
        for i, k in enumerate(self._names):
            p = self._tensor(i, k)
            destination[prefix + k] = p if keep_vars else p.detach()

    def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        for i, k in enumerate(self._names):
            key = prefix + k
            if key not in state_dict:
                if strict:
                    missing_keys.append(key)
                continue
            src, p = state_dict[key], self._tensor(i, k)
            if self._is_buffer(k):
                if self._buffer_differs(src, p):
                    error_msgs.append('buffer %s differs from what the window geometry gives' % key)
                continue
            if tuple(src.shape) != tuple(p.shape):
                error_msgs.append('size mismatch for %s: copying a param with shape %s from checkpoint, the shape in current '
                                  'model is %s.' % (key, tuple(src.shape), tuple(p.shape)))
                continue
            if self._repeats(k, key, src, state_dict, prefix, error_msgs):
                continue
            with torch.no_grad():
                p.copy_(src)
        if strict:
            known = {prefix + k for k in self._names}
            unexpected_keys += [k for k in state_dict if k.startswith(prefix) and k not in known]

    # ---- the engine ----
    def _handle(self):
        if self._h is None:
            c = self._fill_config()
            h = C.c_void_p()
            try:
                _lib.check(None, self._fn('create')(C.byref(c), C.byref(h)))
            except _lib.FdsrError as e:
                raise NotImplementedError(str(e)) from e
            self._h = h
        return self._h

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and _lib._lib is not None:
            getattr(_lib._lib, 'fdsr_%s_destroy' % self._family)(h)
            self._h = None

    def __getstate__(self):
        """copy.deepcopy and pickle carry the tensors and the configuration; a copy creates an engine of its own on first use."""
        d = dict(self.__dict__)
        d['_h'], d['_uploaded'], d['_ws'], d['_static'] = None, {}, {}, {}
        return d

    def sync_weights(self, device):
        """Upload the parameters that changed since their last upload, by (_version, data_ptr)."""
        load, h = self._fn('load'), self._handle()
        if self._uploaded.get('device') != str(device):
            self._uploaded = {'device': str(device)}
        with torch.cuda.device(device):
            for k, p in self.named_reference_parameters():
                stamp = (p._version, p.data_ptr())
                if self._uploaded.get(k) == stamp:
                    continue
                a = p.detach().to('cpu', torch.float32).contiguous()
                shape = (C.c_int64 * a.dim())(*a.shape)
                _lib.check(None, load(h, k.encode(), _ptr(a), shape, a.dim()))
                self._uploaded[k] = stamp

    def workspace_bytes(self, b, h, w):
        need = C.c_size_t()
        _lib.check(None, self._fn('workspace_bytes')(self._handle(), b, h, w, C.byref(need)))
        return need.value

    def workspace(self, b, h, w, device=None):
        device = device or next(self.parameters()).device
        need = self.workspace_bytes(b, h, w)
        key = (str(device), torch.cuda.current_stream(device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=device)
        return ws

    def forward(self, x, graph=False):
        """[B,3,H,W] fp32 on the GPU -> output_shape(B, H, W).  graph=True replays one captured graph per (B, H, W): the call
        copies x into, and the result out of, buffers that the graph keeps."""
        x = self._check(x)
        b, _, h, w = x.shape
        self.sync_weights(x.device)
        with torch.cuda.device(x.device):
            if not graph:
                ws = self.workspace(b, h, w, x.device)      # first: it refuses a shape the family does not compute
                out = torch.empty(self.output_shape(b, h, w), dtype=torch.float32, device=x.device)
                st = torch.cuda.current_stream(x.device).cuda_stream
                _lib.check(None, self._fn('forward')(self._handle(), _ptr(x), b, h, w, _ptr(out), _ptr(ws), ws.numel(), C.c_void_p(st), 0))
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
        _lib.check(None, self._fn('forward')(self._handle(), _ptr(xin), b, h, w, _ptr(out), _ptr(ws), ws.numel(),
                                             C.c_void_p(stream.cuda_stream), getattr(_lib, 'FDSR_%s_GRAPH' % self._family.upper())))
        return out.clone()

    def debug_tensor(self, name, x):
        """The named tap of one forward (arch.tap_names), NCHW as the engine holds it: at the padded size where the family pads;
        a token tensor is [B, C, h, w] over the grid of tokens."""
        x = self._check(x)
        b, _, h, w = x.shape
        if name not in self._tap_names(self.cfg):
            raise KeyError(name)
        self.sync_weights(x.device)
        with torch.cuda.device(x.device):
            ws = self.workspace(b, h, w, x.device)
            cap = self._debug_capacity(b, h, w)
            out = torch.empty(cap, dtype=torch.float32, device=x.device)
            dims = (C.c_int * 3)()
            st = torch.cuda.current_stream(x.device).cuda_stream
            _lib.check(None, self._fn('debug_tensor')(self._handle(), name.encode(), _ptr(x), b, h, w, _ptr(out), cap, dims, _ptr(ws),
                                                      ws.numel(), C.c_void_p(st)))
        th, tw, tc = dims[0], dims[1], dims[2]
        return out[:b * th * tw * tc].view(b, th, tw, tc).permute(0, 3, 1, 2).contiguous()
