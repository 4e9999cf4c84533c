"""The test flow of MSI_SR_model/model/hsenet.py (mfeNew_validateByClass) on the HIP engine:

    python -m fastdiffsr_amd.hsenet.test --model generator_param.pkl (--hr DIR | --lr DIR) [--scale 4] -o OUT
                                         [--batch 16] [--graph] [--max-images N]

The flow is fastdiffsr_amd.swinir.test's (the reference's files differ in the network's name): DIR is a folder of images or
of class folders; with --hr the LR input is made from the HR image as the reference's TestDatasetFromFolder makes it and MSE /
PSNR / SSIM / ERGAS of the SR image and of the bicubic upscale are printed per class and overall; with --lr the images are
super-resolved and written.  The checkpoint loads by the reference's own lenient rule (HSENET.load_state_dict, strict=False):
a shape mismatch is tolerated only under `tail`.  The architecture defaults to the one the reference tests with (n_feats 64,
n_basic_modules 10); --n-feats and --n-basic-modules describe another checkpoint."""
import argparse

import torch

from ..swinir.test import list_classes, run
from .model import HSENet


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--model', required=True, help='generator.state_dict() as the reference saves it (generator_param.pkl)')
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument('--hr', help='HR images: LR is made from them and the results are scored')
    src.add_argument('--lr', help='LR images: super-resolved and written')
    ap.add_argument('--scale', type=int, default=4)
    ap.add_argument('-o', '--out', required=True)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--graph', action='store_true', help='replay one captured graph per (batch, height, width)')
    ap.add_argument('--max-images', type=int, default=None)
    ap.add_argument('--n-feats', type=int, default=64)
    ap.add_argument('--n-basic-modules', type=int, default=10)
    a = ap.parse_args(argv)
    device = torch.device('cuda', torch.cuda.current_device())
    model = HSENet(n_feats=a.n_feats, scale=a.scale, n_basic_modules=a.n_basic_modules, n_colors=3)
    sd = torch.load(a.model, map_location='cpu', weights_only=True)
    model.load_reference_state_dict({k[7:] if k.startswith('module.') else k: v for k, v in sd.items()}, strict=False)
    model.to(device).eval()
    run(model, list_classes(a.hr or a.lr), a.out, a.scale, a.hr is not None, batch=a.batch, graph=a.graph, max_images=a.max_images,
        label='HSENet ')
    return 0


if __name__ == '__main__':
    raise SystemExit(main())
