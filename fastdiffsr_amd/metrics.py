"""Image metrics of the reference's val loop (FastDiffSR/core/metrics.py), host side, plus the
GPU `tensor2img` (clamp -> uint8 on the device, so only 1 byte/channel crosses PCIe instead of the
fp32 copy `DDPM.get_current_visuals` makes, model/model.py:97-111).

tensor2img and PSNR are pinned by goldens generated from the reference's own functions
(tests/golden/metrics.npz).  SSIM / ERGAS follow the reference formulas (metrics.py:103-152) but the
reference needs cv2 / skimage to run them, which this image lacks: those two are unpinned.
LPIPS (AlexNet, v0.1 heads; calculate_lpips, metrics.py:154-163) runs on the device from the user's own weight files
(class LPIPS below, csrc/fdsr_lpips.hip); it is pinned by tests/golden/lpips_alex.npz, made by the reference's own
calculate_lpips on a synthetic backbone (synth.synth_alexnet_features) and the real v0.1 heads.
"""
import ctypes as C
import math
import os
from collections import OrderedDict

import numpy as np
import torch

from . import _lib


def tensor2img(tensor, out_type=np.uint8, min_max=(-1, 1)):
    """metrics.py:16-42 for 3D (C,H,W) / 2D (H,W) tensors (after squeeze) -> HWC / HW numpy array.
    CUDA tensors are converted on the device (uint8 output only)."""
    t = tensor.squeeze()
    if t.dim() not in (2, 3):
        raise TypeError('Only support 3D and 2D tensor. But received with dimension: {:d}'.format(t.dim()))
    if t.is_cuda and out_type == np.uint8:
        t3 = (t if t.dim() == 3 else t[None]).float().contiguous()
        c, h, w = t3.shape
        dst = torch.empty(h, w, c, dtype=torch.uint8, device=t3.device)
        lib = _lib.load()
        st = torch.cuda.current_stream(t3.device).cuda_stream
        _lib.check(None, lib.fdsr_tensor2img_u8(None, C.c_void_p(t3.data_ptr()), C.c_void_p(dst.data_ptr()), 1, c, h, w,
                                                float(min_max[0]), float(min_max[1]), C.c_void_p(st)))
        out = dst.cpu().numpy()
        return out if t.dim() == 3 else out[:, :, 0]
    t = t.float().cpu().clamp_(*min_max)
    t = (t - min_max[0]) / (min_max[1] - min_max[0])
    img = t.numpy()
    if t.dim() == 3:
        img = np.transpose(img, (1, 2, 0))
    if out_type == np.uint8:
        img = (img * 255.0).round()
    return img.astype(out_type)


# --- device-side forms for the evaluation loop (val.py): the batch stays on the GPU as uint8, the per-pixel work of the
# metrics runs in libfdsr_hip.so (csrc/fdsr_val.hip) and only B x 8 doubles come back ---------------------------------
def tensor2img_batch(t4, min_max=(-1, 1)):
    """tensor2img of every image of a [B,C,H,W] CUDA batch in ONE launch -> [B,H,W,C] uint8 CUDA tensor (stays on the device)."""
    if not t4.is_cuda or t4.dim() != 4:
        raise ValueError('tensor2img_batch takes a [B,C,H,W] CUDA tensor')
    t4 = t4.float().contiguous()
    b, c, h, w = t4.shape
    dst = torch.empty(b, h, w, c, dtype=torch.uint8, device=t4.device)
    st = torch.cuda.current_stream(t4.device).cuda_stream
    _lib.check(None, _lib.load().fdsr_tensor2img_u8(None, C.c_void_p(t4.data_ptr()), C.c_void_p(dst.data_ptr()), b, c, h, w,
                                                    float(min_max[0]), float(min_max[1]), C.c_void_p(st)))
    return dst


def u8_to_tensor(u8, min_max=(-1, 1)):
    """The dataset transform (data/util.py:66-75: ToTensor() then * (max - min) + min) of a decoded [B,H,W,C] uint8 CUDA batch
    -> [B,C,H,W] fp32, bit-identical to dataset.to_tensor on the host."""
    if not u8.is_cuda or u8.dtype != torch.uint8 or u8.dim() != 4:
        raise ValueError('u8_to_tensor takes a [B,H,W,C] uint8 CUDA tensor')
    u8 = u8.contiguous()
    b, h, w, c = u8.shape
    dst = torch.empty(b, c, h, w, dtype=torch.float32, device=u8.device)
    st = torch.cuda.current_stream(u8.device).cuda_stream
    _lib.check(None, _lib.load().fdsr_u8_to_tensor(None, C.c_void_p(u8.data_ptr()), C.c_void_p(dst.data_ptr()), b, c, h, w,
                                                   float(min_max[0]), float(min_max[1]), C.c_void_p(st)))
    return dst


_metric_ws = {}


def image_metric_sums(test_u8, truth_u8, gauss=False, out=None):
    """include/fdsr.h: fdsr_image_metrics_u8 -> [B,8] fp64 CUDA tensor of per-image sums (asynchronous on the current stream)."""
    if (not test_u8.is_cuda or test_u8.dtype != torch.uint8 or test_u8.dim() != 4 or truth_u8.shape != test_u8.shape or
            truth_u8.dtype != torch.uint8 or truth_u8.device != test_u8.device):
        raise ValueError('image_metric_sums takes two [B,H,W,C] uint8 CUDA tensors of one shape')
    test_u8, truth_u8 = test_u8.contiguous(), truth_u8.contiguous()
    b, h, w, c = test_u8.shape
    lib = _lib.load()
    need = C.c_size_t()
    _lib.check(None, lib.fdsr_image_metrics_workspace_bytes(b, h, w, C.byref(need)))
    key = (test_u8.device, torch.cuda.current_stream(test_u8.device).cuda_stream)
    ws = _metric_ws.get(key)
    if ws is None or ws.numel() < need.value:
        ws = _metric_ws[key] = torch.empty(int(need.value), dtype=torch.uint8, device=test_u8.device)
    if out is None:
        out = torch.empty(b, _lib.FDSR_METRIC_FIELDS, dtype=torch.float64, device=test_u8.device)
    flags = _lib.FDSR_SSIM_UNIFORM7 | (_lib.FDSR_SSIM_GAUSS11 if gauss else 0)
    _lib.check(None, lib.fdsr_image_metrics_u8(None, C.c_void_p(test_u8.data_ptr()), C.c_void_p(truth_u8.data_ptr()), b, h, w, c, flags,
                                               C.c_void_p(out.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(key[1])))
    return out


def metrics_from_sums(sums, shape_hwc, scale=4):
    """Per-image (mse, psnr, ssim, ergas[, ssim_gauss]) from one row of image_metric_sums, with the scalar formulas of
    compare_mse / compare_psnr / calculate_ergas above (the sums are exact integers, so these three equal the host path
    bit for bit) and SSIM = map sum / positions."""
    h, w, c = shape_hwc
    n = float(h * w * c)
    sse, s_test, ss7, n7, ss11, n11 = (float(x) for x in sums[:6])
    mse = sse / n
    psnr = float('inf') if mse == 0 else 10 * math.log10((255.0 ** 2) / mse)
    mean2 = (s_test / n) ** 2
    ergas = float(100.0 * np.sqrt(np.float64(mse) / mean2 / c) / scale)
    out = {'mse': mse, 'psnr': psnr, 'ssim': ss7 / n7 if n7 else float('nan'), 'ergas': ergas}
    if n11:
        out['ssim_gauss'] = ss11 / n11
    return out


def calculate_mse(img1, img2):                       # skimage.measure.compare_mse
    return float(np.mean((img1.astype(np.float64) - img2.astype(np.float64)) ** 2))


def calculate_psnr(img1, img2):                      # metrics.py:94-101
    mse = np.mean((img1.astype(np.float64) - img2.astype(np.float64)) ** 2)
    if mse == 0:
        return float('inf')
    return 20 * math.log10(255.0 / math.sqrt(mse))


def _gauss_window(size=11, sigma=1.5):               # cv2.getGaussianKernel(11, 1.5) outer product
    x = np.arange(size, dtype=np.float64) - (size - 1) / 2.0
    k = np.exp(-(x ** 2) / (2 * sigma ** 2))
    k /= k.sum()
    return np.outer(k, k)


def _filter_valid(img, win):
    """cv2.filter2D(img, -1, win)[5:-5, 5:-5]: the border-independent ('valid') part, per channel."""
    from numpy.lib.stride_tricks import sliding_window_view
    if img.ndim == 3:
        return np.stack([_filter_valid(img[..., c], win) for c in range(img.shape[2])], axis=-1)
    v = sliding_window_view(img, win.shape)
    return np.einsum('ijkl,kl->ij', v, win)


def ssim(img1, img2):                                # metrics.py:103-123
    C1, C2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    a, b = img1.astype(np.float64), img2.astype(np.float64)
    win = _gauss_window()
    mu1, mu2 = _filter_valid(a, win), _filter_valid(b, win)
    mu1_sq, mu2_sq, mu12 = mu1 ** 2, mu2 ** 2, mu1 * mu2
    s1 = _filter_valid(a ** 2, win) - mu1_sq
    s2 = _filter_valid(b ** 2, win) - mu2_sq
    s12 = _filter_valid(a * b, win) - mu12
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s1 + s2 + C2))
    return float(m.mean())


def calculate_ssim(img1, img2):                      # metrics.py:126-145 (3-channel: ssim of the whole array, as there)
    if img1.shape != img2.shape:
        raise ValueError('Input images must have the same dimensions.')
    if img1.ndim == 2:
        return ssim(img1, img2)
    if img1.ndim == 3:
        if img1.shape[2] == 3:
            return float(np.array([ssim(img1, img2) for _ in range(3)]).mean())
        if img1.shape[2] == 1:
            return ssim(np.squeeze(img1), np.squeeze(img2))
    raise ValueError('Wrong input image dimensions.')


def calculate_ergas(img1, img2, scale=4):            # metrics.py:147-152
    channel = img1.shape[2]
    mse = calculate_mse(img1, img2)
    mean2 = np.mean(img1, dtype=np.float64) ** 2
    return float(100.0 * np.sqrt(mse / mean2 / channel) / scale)


# --- what sr_mfe.py's val loop actually calls for MSE / PSNR / SSIM (sr_mfe.py:313-333): the
# skimage.measure functions of skimage 0.16 with their defaults.  skimage is not in this image, so these are
# restated from its published algorithm (compare_ssim: uniform 7x7 window via scipy.ndimage.uniform_filter,
# sample covariance, K1 = 0.01, K2 = 0.03, data range of the dtype, borders cropped, mean over channels) and
# are unpinned.
def compare_mse(im1, im2):
    return float(np.mean(np.square(im1.astype(np.float64) - im2.astype(np.float64)), dtype=np.float64))


def compare_psnr(im_true, im_test):
    err = compare_mse(im_true, im_test)
    return float('inf') if err == 0 else 10 * math.log10((255.0 ** 2) / err)


def compare_ssim(X, Y, multichannel=True, win_size=7):
    from scipy.ndimage import uniform_filter
    if multichannel:
        return float(np.mean([compare_ssim(X[..., c], Y[..., c], multichannel=False, win_size=win_size)
                              for c in range(X.shape[-1])]))
    K1, K2, R = 0.01, 0.03, 255.0
    X, Y = X.astype(np.float64), Y.astype(np.float64)
    NP = win_size ** X.ndim
    cov_norm = NP / (NP - 1)
    ux, uy = uniform_filter(X, size=win_size), uniform_filter(Y, size=win_size)
    uxx, uyy, uxy = uniform_filter(X * X, size=win_size), uniform_filter(Y * Y, size=win_size), uniform_filter(X * Y, size=win_size)
    vx, vy, vxy = cov_norm * (uxx - ux * ux), cov_norm * (uyy - uy * uy), cov_norm * (uxy - ux * uy)
    C1, C2 = (K1 * R) ** 2, (K2 * R) ** 2
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
    pad = (win_size - 1) // 2
    return float(S[pad:-pad, pad:-pad].mean())


# --- LPIPS (core/metrics.py:154-163 calculate_lpips: lpips.LPIPS(net='alex'), the v0.1 linear heads), on the device --------
LPIPS_BACKBONE = OrderedDict([('features.0.weight', (64, 3, 11, 11)), ('features.0.bias', (64,)),
                              ('features.3.weight', (192, 64, 5, 5)), ('features.3.bias', (192,)),
                              ('features.6.weight', (384, 192, 3, 3)), ('features.6.bias', (384,)),
                              ('features.8.weight', (256, 384, 3, 3)), ('features.8.bias', (256,)),
                              ('features.10.weight', (256, 256, 3, 3)), ('features.10.bias', (256,))])
LPIPS_CHANNELS = (64, 192, 384, 256, 256)
LPIPS_LIN = OrderedDict(('lin%d.model.1.weight' % k, (1, c, 1, 1)) for k, c in enumerate(LPIPS_CHANNELS))
LPIPS_BACKBONE_FILE = 'alexnet-owt-7be5be79.pth'     # torchvision's ImageNet AlexNet, as its hub cache names it


def _as_state_dict(src):
    if isinstance(src, (str, os.PathLike)):
        return torch.load(os.fspath(src), map_location='cpu', weights_only=True)
    return src


def lpips_state(backbone, lin):
    """The 15 tensors fdsr_lpips_load takes, as float32 numpy arrays in load order, from a torchvision AlexNet state dict
    (its `classifier.*` tensors are ignored) and an `lpips` v0.1 alex.pth state dict.  Any other name, a missing tensor or a
    wrong shape raises KeyError / ValueError: nothing is guessed."""
    out = OrderedDict()
    for sd, table, ignore in ((backbone, LPIPS_BACKBONE, 'classifier.'), (lin, LPIPS_LIN, None)):
        extra = [k for k in sd if k not in table and not (ignore and k.startswith(ignore))]
        if extra:
            raise KeyError('unexpected LPIPS tensor(s): %s' % ', '.join(sorted(extra)))
        for k, shape in table.items():
            if k not in sd:
                raise KeyError('LPIPS tensor %r is missing' % k)
            v = sd[k]
            a = (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float32)
            if tuple(a.shape) != shape:
                raise ValueError('LPIPS tensor %r has shape %s, expected %s' % (k, tuple(a.shape), shape))
            out[k] = np.ascontiguousarray(a)
    return out


class LPIPS:
    """LPIPS (AlexNet, v0.1 heads) of uint8 images on the device (include/fdsr.h: fdsr_lpips_*), the reference's
    calculate_lpips: the [0,1] ToTensor image goes into the network as it is (no normalize=True), so the values match the
    reference's log, not `lpips` called with normalize=True.

        lp = LPIPS(backbone, lin)          # two state dicts or two .pth paths (torch.load(weights_only=True))
        lp = LPIPS(*LPIPS.default_paths())
        out = lp.lpips_u8(truth, test_a, test_b=None)    # [n_tests, B, 6] fp64 CUDA: (LPIPS, per-layer terms 0..4)
    """

    def __init__(self, backbone, lin, device=None):
        tensors = lpips_state(_as_state_dict(backbone), _as_state_dict(lin))
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(None, lib.fdsr_lpips_create(C.byref(h)))
        self._h = h
        with torch.cuda.device(self.device):
            for k, a in tensors.items():
                shape = (C.c_int64 * a.ndim)(*a.shape)
                _lib.check(None, lib.fdsr_lpips_load(h, k.encode(), C.c_void_p(a.ctypes.data), shape, a.ndim))
        self._ws = {}

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and _lib._lib is not None:
            _lib._lib.fdsr_lpips_destroy(h)
            self._h = None

    @staticmethod
    def default_paths():
        """Where a user of the reference already has the two files (lpips.LPIPS(net='alex') reads them from there); nothing is
        ever downloaded:  $TORCH_HOME/hub/checkpoints/alexnet-owt-7be5be79.pth (TORCH_HOME defaults to ~/.cache/torch) and the
        `lpips` package's weights/v0.1/alex.pth (located with importlib, without importing the package)."""
        import importlib.util
        torch_home = os.path.expanduser(os.environ.get('TORCH_HOME', os.path.join('~', '.cache', 'torch')))
        backbone = os.path.join(torch_home, 'hub', 'checkpoints', LPIPS_BACKBONE_FILE)
        if not os.path.isfile(backbone):
            raise FileNotFoundError('LPIPS backbone %s not found: put torchvision\'s ImageNet AlexNet weights (%s) there, or pass '
                                    '--lpips-backbone PATH' % (backbone, LPIPS_BACKBONE_FILE))
        spec = importlib.util.find_spec('lpips')
        lin = None
        if spec is not None and spec.submodule_search_locations:
            for d in spec.submodule_search_locations:
                cand = os.path.join(d, 'weights', 'v0.1', 'alex.pth')
                if os.path.isfile(cand):
                    lin = cand
                    break
        if lin is None:
            raise FileNotFoundError('LPIPS heads lpips/weights/v0.1/alex.pth not found: install the `lpips` package (it ships the '
                                    'file) or pass --lpips-lin PATH')
        return backbone, lin

    def workspace(self, b, h, w):
        need = C.c_size_t()
        _lib.check(None, _lib.load().fdsr_lpips_workspace_bytes(self._h, b, h, w, C.byref(need)))
        key = (self.device, torch.cuda.current_stream(self.device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need.value:
            ws = self._ws[key] = torch.empty(int(need.value), dtype=torch.uint8, device=self.device)
        return ws

    def lpips_u8(self, truth, test_a, test_b=None, out=None):
        """[B,H,W,3] uint8 CUDA images -> [n_tests, B, 6] fp64 CUDA tensor (asynchronous on the current stream)."""
        imgs = [truth, test_a] + ([test_b] if test_b is not None else [])
        for t in imgs:
            if (not t.is_cuda or t.dtype != torch.uint8 or t.dim() != 4 or t.shape != truth.shape or t.shape[-1] != 3 or
                    t.device != truth.device):
                raise ValueError('lpips_u8 takes [B,H,W,3] uint8 CUDA tensors of one shape')
        imgs = [t.contiguous() for t in imgs]
        b, h, w, _ = truth.shape
        ws = self.workspace(b, h, w)
        if out is None:
            out = torch.empty(len(imgs) - 1, b, 6, dtype=torch.float64, device=truth.device)
        st = torch.cuda.current_stream(truth.device).cuda_stream
        ptr = [C.c_void_p(t.data_ptr()) for t in imgs] + ([None] if test_b is None else [])
        _lib.check(None, _lib.load().fdsr_lpips_u8(self._h, ptr[0], ptr[1], ptr[2], b, h, w, C.c_void_p(out.data_ptr()),
                                                   C.c_void_p(ws.data_ptr()), ws.numel(), C.c_void_p(st)))
        return out


# --- FID (FastDiffSR/FID.py: pytorch_fid.fid_score.calculate_fid_given_paths(..., dims=2048)), features on the device -------
def _fid_layers():
    """The 94 BasicConv2d of pytorch_fid's InceptionV3 up to pool3 (use_fid_inception=True), in state-dict order:
    (name, cin, cout, kh, kw, stride, pad_h, pad_w).  csrc/fdsr_fid.hip walks the same table."""
    out = []

    def c(name, cin, cout, k, s=1, p=(0, 0)):
        out.append((name, cin, cout, k[0], k[1], s, p[0], p[1]))
    c('Conv2d_1a_3x3', 3, 32, (3, 3), 2)
    c('Conv2d_2a_3x3', 32, 32, (3, 3))
    c('Conv2d_2b_3x3', 32, 64, (3, 3), 1, (1, 1))
    c('Conv2d_3b_1x1', 64, 80, (1, 1))
    c('Conv2d_4a_3x3', 80, 192, (3, 3))
    for m, cin, pf in (('Mixed_5b', 192, 32), ('Mixed_5c', 256, 64), ('Mixed_5d', 288, 64)):      # FIDInceptionA
        c(m + '.branch1x1', cin, 64, (1, 1))
        c(m + '.branch5x5_1', cin, 48, (1, 1))
        c(m + '.branch5x5_2', 48, 64, (5, 5), 1, (2, 2))
        c(m + '.branch3x3dbl_1', cin, 64, (1, 1))
        c(m + '.branch3x3dbl_2', 64, 96, (3, 3), 1, (1, 1))
        c(m + '.branch3x3dbl_3', 96, 96, (3, 3), 1, (1, 1))
        c(m + '.branch_pool', cin, pf, (1, 1))
    c('Mixed_6a.branch3x3', 288, 384, (3, 3), 2)                                                  # InceptionB
    c('Mixed_6a.branch3x3dbl_1', 288, 64, (1, 1))
    c('Mixed_6a.branch3x3dbl_2', 64, 96, (3, 3), 1, (1, 1))
    c('Mixed_6a.branch3x3dbl_3', 96, 96, (3, 3), 2)
    for m, c7 in (('Mixed_6b', 128), ('Mixed_6c', 160), ('Mixed_6d', 160), ('Mixed_6e', 192)):     # FIDInceptionC
        c(m + '.branch1x1', 768, 192, (1, 1))
        c(m + '.branch7x7_1', 768, c7, (1, 1))
        c(m + '.branch7x7_2', c7, c7, (1, 7), 1, (0, 3))
        c(m + '.branch7x7_3', c7, 192, (7, 1), 1, (3, 0))
        c(m + '.branch7x7dbl_1', 768, c7, (1, 1))
        c(m + '.branch7x7dbl_2', c7, c7, (7, 1), 1, (3, 0))
        c(m + '.branch7x7dbl_3', c7, c7, (1, 7), 1, (0, 3))
        c(m + '.branch7x7dbl_4', c7, c7, (7, 1), 1, (3, 0))
        c(m + '.branch7x7dbl_5', c7, 192, (1, 7), 1, (0, 3))
        c(m + '.branch_pool', 768, 192, (1, 1))
    c('Mixed_7a.branch3x3_1', 768, 192, (1, 1))                                                   # InceptionD
    c('Mixed_7a.branch3x3_2', 192, 320, (3, 3), 2)
    c('Mixed_7a.branch7x7x3_1', 768, 192, (1, 1))
    c('Mixed_7a.branch7x7x3_2', 192, 192, (1, 7), 1, (0, 3))
    c('Mixed_7a.branch7x7x3_3', 192, 192, (7, 1), 1, (3, 0))
    c('Mixed_7a.branch7x7x3_4', 192, 192, (3, 3), 2)
    for m, cin in (('Mixed_7b', 1280), ('Mixed_7c', 2048)):                                       # FIDInceptionE_1 / _2
        c(m + '.branch1x1', cin, 320, (1, 1))
        c(m + '.branch3x3_1', cin, 384, (1, 1))
        c(m + '.branch3x3_2a', 384, 384, (1, 3), 1, (0, 1))
        c(m + '.branch3x3_2b', 384, 384, (3, 1), 1, (1, 0))
        c(m + '.branch3x3dbl_1', cin, 448, (1, 1))
        c(m + '.branch3x3dbl_2', 448, 384, (3, 3), 1, (1, 1))
        c(m + '.branch3x3dbl_3a', 384, 384, (1, 3), 1, (0, 1))
        c(m + '.branch3x3dbl_3b', 384, 384, (3, 1), 1, (1, 0))
        c(m + '.branch_pool', cin, 192, (1, 1))
    return out


FID_LAYERS = _fid_layers()
FID_TENSORS = OrderedDict()           # the 470 tensors fdsr_fid_load takes, in load order
for _n, _ci, _co, _kh, _kw, _s, _ph, _pw in FID_LAYERS:
    FID_TENSORS[_n + '.conv.weight'] = (_co, _ci, _kh, _kw)
    for _b in ('weight', 'bias', 'running_mean', 'running_var'):
        FID_TENSORS[_n + '.bn.' + _b] = (_co,)
del _n, _ci, _co, _kh, _kw, _s, _ph, _pw, _b
# include/fdsr.h's module table: (name, output side, output channels) at the fixed 299 x 299 input
FID_MODULES = [('Conv2d_1a_3x3', 149, 32), ('Conv2d_2a_3x3', 147, 32), ('Conv2d_2b_3x3', 147, 64), ('MaxPool_1', 73, 64),
               ('Conv2d_3b_1x1', 73, 80), ('Conv2d_4a_3x3', 71, 192), ('MaxPool_2', 35, 192), ('Mixed_5b', 35, 256),
               ('Mixed_5c', 35, 288), ('Mixed_5d', 35, 288), ('Mixed_6a', 17, 768), ('Mixed_6b', 17, 768), ('Mixed_6c', 17, 768),
               ('Mixed_6d', 17, 768), ('Mixed_6e', 17, 768), ('Mixed_7a', 8, 1280), ('Mixed_7b', 8, 2048), ('Mixed_7c', 8, 2048)]
FID_DIMS = 2048
FID_WEIGHTS_FILE = 'pt_inception-2015-12-05-6726825d.pth'     # pytorch_fid's FID Inception weights, as its hub cache names it


def fid_state(sd):
    """The 470 tensors fdsr_fid_load takes, as float32 numpy arrays in load order, from the FID Inception state dict
    (pt_inception-2015-12-05-6726825d.pth, torchvision names).  `fc.*` and `*.num_batches_tracked` are ignored; any other
    name, a missing tensor or a wrong shape raises KeyError / ValueError naming it: nothing is guessed."""
    extra = [k for k in sd if k not in FID_TENSORS and not k.startswith('fc.') and not k.endswith('.num_batches_tracked')]
    if extra:
        raise KeyError('unexpected FID Inception tensor(s): %s' % ', '.join(sorted(extra)))
    out = OrderedDict()
    for k, shape in FID_TENSORS.items():
        if k not in sd:
            raise KeyError('FID Inception tensor %r is missing' % k)
        v = sd[k]
        a = (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float32)
        if tuple(a.shape) != shape:
            raise ValueError('FID Inception tensor %r has shape %s, expected %s' % (k, tuple(a.shape), shape))
        out[k] = np.ascontiguousarray(a)
    return out


class FID:
    """pytorch_fid's pool3 features (InceptionV3, dims=2048) of uint8 images on the device (include/fdsr.h: fdsr_fid_*).

        fid = FID(state_dict_or_path)              # pt_inception-2015-12-05-6726825d.pth (torch.load(weights_only=True))
        fid = FID(FID.default_path())
        f = fid.features_u8(imgs)                  # [B,H,W,3] uint8 CUDA -> [B,2048] fp32 CUDA
        frechet_distance(*activation_statistics(f1), *activation_statistics(f2))

    Any H, W: every image is resized to 299 x 299 first.  Features are per image (bitwise independent of the batch), so B is
    cut into chunks whose workspace stays within MAX_WORKSPACE bytes."""

    MAX_WORKSPACE = 2 << 30

    def __init__(self, weights, device=None):
        tensors = fid_state(_as_state_dict(weights))
        self.device = torch.device(device) if device is not None else torch.device('cuda', torch.cuda.current_device())
        lib = _lib.load()
        h = C.c_void_p()
        _lib.check(None, lib.fdsr_fid_create(C.byref(h)))
        self._h = h
        with torch.cuda.device(self.device):
            for k, a in tensors.items():
                shape = (C.c_int64 * a.ndim)(*a.shape)
                _lib.check(None, lib.fdsr_fid_load(h, k.encode(), C.c_void_p(a.ctypes.data), shape, a.ndim))
        self._ws = {}

    def __del__(self):
        h = getattr(self, '_h', None)
        if h is not None and _lib._lib is not None:
            _lib._lib.fdsr_fid_destroy(h)
            self._h = None

    @staticmethod
    def default_path():
        """Where pytorch_fid caches the weights for the reference's users: torch.hub.get_dir()/checkpoints/<FID_WEIGHTS_FILE>.
        Nothing is ever downloaded."""
        p = os.path.join(torch.hub.get_dir(), 'checkpoints', FID_WEIGHTS_FILE)
        if not os.path.isfile(p):
            raise FileNotFoundError('FID Inception weights %s not found: put pytorch_fid\'s %s there, or pass --fid-weights PATH'
                                    % (p, FID_WEIGHTS_FILE))
        return p

    def _workspace_bytes(self, b, h, w):
        need = C.c_size_t()
        _lib.check(None, _lib.load().fdsr_fid_workspace_bytes(self._h, b, h, w, C.byref(need)))
        return int(need.value)

    def chunk(self, h, w):
        """Images per device call: the most whose workspace fits MAX_WORKSPACE (at least 1)."""
        one = self._workspace_bytes(1, h, w)
        per = max(self._workspace_bytes(2, h, w) - one, 1)
        return max(1, 1 + (self.MAX_WORKSPACE - one) // per)

    def workspace(self, b, h, w):
        need = self._workspace_bytes(b, h, w)
        key = (self.device, torch.cuda.current_stream(self.device).cuda_stream)
        ws = self._ws.get(key)
        if ws is None or ws.numel() < need:
            ws = self._ws[key] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return ws

    def features_u8(self, imgs, module=-1):
        """[B,H,W,3] uint8 CUDA images -> [B,2048] fp32 CUDA pool3 features (asynchronous on the current stream).
        module = k: the raw NHWC output of module k of FID_MODULES, [B,S,S,C]; module = -2: the normalised 299 x 299 input."""
        if not imgs.is_cuda or imgs.dtype != torch.uint8 or imgs.dim() != 4 or imgs.shape[-1] != 3:
            raise ValueError('features_u8 takes [B,H,W,3] uint8 CUDA images')
        imgs = imgs.contiguous()
        b, h, w, _ = imgs.shape
        if module == -1:
            shape = (FID_DIMS,)
        elif module == -2:
            shape = (299, 299, 3)
        else:
            _, s, c = FID_MODULES[module]
            shape = (s, s, c)
        out = torch.empty((b,) + shape, dtype=torch.float32, device=imgs.device)
        if b == 0:
            return out
        n = min(b, self.chunk(h, w))
        ws = self.workspace(n, h, w)
        st = torch.cuda.current_stream(imgs.device).cuda_stream
        for i in range(0, b, n):
            m = min(n, b - i)
            _lib.check(None, _lib.load().fdsr_fid_features_u8(self._h, C.c_void_p(imgs[i].data_ptr()), m, h, w, module,
                                                              C.c_void_p(out[i].data_ptr()), C.c_void_p(ws.data_ptr()),
                                                              ws.numel(), C.c_void_p(st)))
        return out


def activation_statistics(feats):
    """pytorch_fid's calculate_activation_statistics on [N, D] features, in fp64: (mu = mean, sigma = np.cov(rowvar=False))."""
    a = (feats.detach().cpu().numpy() if isinstance(feats, torch.Tensor) else np.asarray(feats)).astype(np.float64)
    return np.mean(a, axis=0), np.cov(a, rowvar=False)


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """pytorch_fid's calculate_frechet_distance: |mu1 - mu2|^2 + tr s1 + tr s2 - 2 tr sqrtm(s1 s2), scipy.linalg.sqrtm in fp64;
    a non-finite root is retried with eps * I added to both covariances; a diagonal imaginary part above 1e-3 raises ValueError,
    a smaller one is dropped."""
    from scipy import linalg
    mu1, mu2 = np.atleast_1d(np.asarray(mu1, dtype=np.float64)), np.atleast_1d(np.asarray(mu2, dtype=np.float64))
    sigma1, sigma2 = np.atleast_2d(np.asarray(sigma1, dtype=np.float64)), np.atleast_2d(np.asarray(sigma2, dtype=np.float64))
    if mu1.shape != mu2.shape or sigma1.shape != sigma2.shape:
        raise ValueError('frechet_distance: the two statistics have different dimensions')
    diff = mu1 - mu2
    covmean = linalg.sqrtm(sigma1.dot(sigma2))
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError('frechet_distance: imaginary component %g' % np.max(np.abs(covmean.imag)))
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))
