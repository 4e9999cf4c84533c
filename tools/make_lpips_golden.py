"""Generate tests/golden/lpips_alex.npz by RUNNING THE REFERENCE's calculate_lpips (CPU).

TEST INFRASTRUCTURE.  Runs only where the reference checkout exists (never on the GPU box).  It imports the reference's
core/metrics.py and calls its calculate_lpips (metrics.py:154-163) for real, with stub modules around it:
  * `lpips.LPIPS(net='alex')` builds the reference's own PNetLin(pnet_type='alex', version='0.1')
    (MSI_SR_model/utils/PerceptualSimilarity/networks_basic.py) with the real weights/v0.1/alex.pth heads, in eval mode
  * `torchvision.models.alexnet` returns torchvision's AlexNet `features` layer list, filled from
    fastdiffsr_amd.synth.synth_alexnet_features(SEED) (no ImageNet AlexNet is available here; 2.5 M parameters are too
    large for a fixture)
  * `torchvision.transforms.ToTensor` has torchvision's semantics (HWC uint8 -> CHW float32 / 255)
  * cv2 / skimage / matplotlib are stubbed as oracle/make_goldens.py stubs them
The fixture holds DATA only: the seed, a checksum per synthetic tensor, the five real head vectors, the image pairs and
the reference's LPIPS and per-layer (retPerLayer) values.

Usage:  python tools/make_lpips_golden.py [REFERENCE_DIR]      (writes tests/golden/lpips_alex.npz)
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = sys.argv[1] if len(sys.argv) > 1 else os.environ.get('FDSR_REFERENCE', '/root/reference/FastDiffSR')
OUT = os.path.join(ROOT, 'tests', 'golden', 'lpips_alex.npz')
SEED = 7

from fastdiffsr_amd.synth import synth_alexnet_features  # noqa: E402


def checksum(a):
    """fp64 (sum, sum |x|, sum x * ramp) of one tensor: a drift of the random generator shows up tensor by tensor."""
    x = a.astype(np.float64).ravel()
    return np.array([x.sum(), np.abs(x).sum(), (x * np.linspace(-1.0, 1.0, x.size)).sum()])


def alexnet_features(sd):
    """torchvision.models.AlexNet().features (torchvision/models/alexnet.py), filled from a state dict."""
    nn = torch.nn
    f = nn.Sequential(nn.Conv2d(3, 64, kernel_size=11, stride=4, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
                      nn.Conv2d(64, 192, kernel_size=5, padding=2), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2),
                      nn.Conv2d(192, 384, kernel_size=3, padding=1), nn.ReLU(inplace=True),
                      nn.Conv2d(384, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True),
                      nn.Conv2d(256, 256, kernel_size=3, padding=1), nn.ReLU(inplace=True), nn.MaxPool2d(kernel_size=3, stride=2))
    f.load_state_dict({k[len('features.'):]: torch.from_numpy(v) for k, v in sd.items()})
    return f


def install_stubs(backbone_sd, lin_path, made):
    def ToTensor():
        def f(pic):
            return torch.from_numpy(np.ascontiguousarray(pic.transpose((2, 0, 1)))).contiguous().to(torch.float32).div(255)
        return f

    tv, tvm, tvt, tvu = (types.ModuleType(n) for n in ('torchvision', 'torchvision.models', 'torchvision.transforms', 'torchvision.utils'))
    tvm.alexnet = lambda pretrained=True, **kw: types.SimpleNamespace(features=alexnet_features(backbone_sd))
    tvt.ToTensor = ToTensor
    tvu.make_grid = None
    tv.models, tv.transforms, tv.utils = tvm, tvt, tvu
    for name, mod in (('torchvision', tv), ('torchvision.models', tvm), ('torchvision.transforms', tvt), ('torchvision.utils', tvu)):
        sys.modules[name] = mod
    for name in ('cv2', 'skimage', 'skimage.measure', 'skimage.color', 'skimage.transform', 'matplotlib', 'matplotlib.pyplot',
                 'core.PerceptualSimilarity', 'lpips'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['skimage.measure'].compare_mse = None
    sys.modules['skimage.measure'].compare_ssim = None
    sys.modules['skimage'].io = sys.modules['skimage'].data = None
    sys.modules['skimage'].color = sys.modules['skimage.color']
    sys.modules['skimage'].transform = sys.modules['skimage.transform']

    sys.path.insert(0, os.path.join(REF, 'MSI_SR_model'))
    from utils.PerceptualSimilarity import networks_basic as nb

    def LPIPS(net='alex', **kw):
        assert net == 'alex'
        m = nb.PNetLin(pnet_type='alex', version='0.1', use_gpu=False)
        sd = torch.load(lin_path, map_location='cpu', weights_only=True)
        m.load_state_dict(sd, strict=False)
        m.eval()
        made.append(m)
        return m

    sys.modules['lpips'].LPIPS = LPIPS
    sys.path.insert(0, REF)
    import core
    core.PerceptualSimilarity = sys.modules['core.PerceptualSimilarity']
    from core import metrics as ref_metrics
    return ref_metrics, tvt.ToTensor()


def texture(rng, h, w, smooth=6.0, noise=10.0):
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.zeros((h, w, 3))
    for c in range(3):
        for _ in range(4):
            fx, fy, ph = rng.uniform(0.02, 0.4, 2).tolist() + [rng.uniform(0, 6.28)]
            base[..., c] += 40 * np.sin(fx * xx + fy * yy + ph) * np.cos(fy * xx / smooth + ph)
    return (128 + base + rng.normal(0, noise, base.shape)).clip(0, 255).astype(np.uint8)


def main():
    from PIL import Image
    lin_path = os.path.join(REF, 'MSI_SR_model', 'utils', 'PerceptualSimilarity', 'weights', 'v0.1', 'alex.pth')
    backbone = synth_alexnet_features(SEED)
    made = []
    ref_metrics, to_tensor = install_stubs(backbone, lin_path, made)
    lin_sd = torch.load(lin_path, map_location='cpu', weights_only=True)

    rng = np.random.default_rng(2025)
    pairs = {}
    t64 = texture(rng, 64, 64)
    pairs['p64_noise'] = (t64, (t64 + rng.normal(0, 12, t64.shape)).clip(0, 255).astype(np.uint8))
    pairs['p64_shift'] = (t64, np.roll(t64, (1, 2), axis=(0, 1)))
    pairs['p64_other'] = (t64, texture(rng, 64, 64, smooth=2.0))
    toff = texture(rng, 72, 104)
    pairs['p72x104'] = (toff, (toff * 0.85 + rng.normal(0, 6, toff.shape)).clip(0, 255).astype(np.uint8))
    hr = texture(rng, 256, 256, smooth=3.0, noise=8.0)
    lr = Image.fromarray(hr).resize((64, 64), Image.BICUBIC)
    bic = np.asarray(lr.resize((256, 256), Image.BICUBIC))
    noisy = (hr + rng.normal(0, 4, hr.shape)).clip(0, 255).astype(np.uint8)
    pairs['p256_bic'] = (bic, hr)           # (fake_img, hr_img) as the reference's val loop calls it
    pairs['p256_noisy'] = (noisy, hr)
    # each image is stored once: pair/test and pair/truth name an entry of img/
    images, names = {}, {}
    for name, ims in pairs.items():
        for role, im in zip(('test', 'truth'), ims):
            key = next((k for k, v in images.items() if v is im), None) or '%s_%s' % (name, role)
            images[key] = im
            names[name + '/' + role] = key

    out = {'seed': np.array(SEED), 'names': np.array(sorted(pairs))}
    out.update({'img/' + k: v for k, v in images.items()})
    out.update({k: np.array(v) for k, v in names.items()})
    lin0 = []
    for k, v in backbone.items():
        out['checksum/' + k] = checksum(v)
    for k in range(5):
        out['lin%d' % k] = lin_sd['lin%d.model.1.weight' % k].float().numpy().reshape(-1)
    for name, (test, truth) in pairs.items():
        total = ref_metrics.calculate_lpips(test, truth)
        hook = made[-1].lin0.model.register_forward_hook(lambda mod, inp, o: lin0.append(o.mean([2, 3]).item()))
        with torch.no_grad():
            val, per = made[-1](to_tensor(test).to(torch.float32), to_tensor(truth).to(torch.float32), retPerLayer=True)
        hook.remove()
        assert abs(float(val) - total) <= 1e-6 * abs(total), (name, float(val), total)
        # PNetLin.forward adds the layers into res[0] in place, so retPerLayer[0] comes back as the total: layer 0's own term
        # is taken where lin0 produced it (spatial_average of its output, the op the forward applies)
        out[name + '/lpips'] = np.array(total, dtype=np.float64)
        out[name + '/layers'] = np.array([lin0[-1]] + [float(p) for p in per[1:]], dtype=np.float64)
        print(f'{name}: {test.shape} lpips {total:.6e} layers {out[name + "/layers"]}')
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT), 'bytes')


if __name__ == '__main__':
    main()
