"""FastDiffSR/FID.py on the HIP engine: the Frechet Inception Distance between two image folders (pytorch_fid's
calculate_fid_given_paths, dims=2048), the pool3 features computed on the device (metrics.FID, csrc/fdsr_fid.hip):

    python -m fastdiffsr_amd.fid RESULTS_DIR HR_DIR [--weights pt_inception-2015-12-05-6726825d.pth] [--batch 50]
    python -m fastdiffsr_amd.fid RESULTS_DIR --save-stats results.npz          # the statistics of the first path only

A path is a folder or an .npz holding `mu` / `sigma`, as in pytorch_fid.  A folder is listed as pytorch_fid lists it: its own
files (not recursive) with the extensions bmp jpg jpeg pgm png ppm tif tiff webp, in that letter case, sorted; each is read with
PIL as RGB.  Images of different sizes run in same-size batches: the features are per image, so batching changes nothing.
The weights are read from pytorch_fid's hub cache (torch.hub.get_dir()/checkpoints) unless --weights is given; nothing is
ever downloaded.  Prints FID.py's line `- SR_FID : {:.3f}`."""
import argparse
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import metrics as M
from .parallel import host_threads_per_rank

IMAGE_EXTENSIONS = ('bmp', 'jpg', 'jpeg', 'pgm', 'png', 'ppm', 'tif', 'tiff', 'webp')


def list_images(folder):
    """pytorch_fid's listing: sorted(file for ext in IMAGE_EXTENSIONS for file in Path(folder).glob('*.' + ext))"""
    names = [n for n in os.listdir(folder) if '.' in n and n.rsplit('.', 1)[1] in IMAGE_EXTENSIONS]
    return sorted(os.path.join(folder, n) for n in names)


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert('RGB'))


def folder_features(fid, files, batch=50, workers=None):
    """[len(files), 2048] fp32 host features, in the order of `files`."""
    with ThreadPoolExecutor(max_workers=workers or host_threads_per_rank(cap=8, floor=2)) as pool:
        imgs = list(pool.map(_read, files))
    out = np.zeros((len(files), M.FID_DIMS), dtype=np.float32)
    by_size = {}
    for i, im in enumerate(imgs):
        by_size.setdefault(im.shape, []).append(i)
    for idx in by_size.values():
        for b0 in range(0, len(idx), batch):
            part = idx[b0:b0 + batch]
            x = torch.from_numpy(np.stack([imgs[i] for i in part])).to(fid.device)
            out[part] = fid.features_u8(x).cpu().numpy()
    return out


def path_statistics(fid, path, batch=50, workers=None):
    """(mu, sigma) of a folder (features on the device, statistics in fp64) or of an .npz holding mu / sigma"""
    if path.endswith('.npz'):
        with np.load(path) as f:
            return f['mu'][:], f['sigma'][:]
    if not os.path.isdir(path):
        raise FileNotFoundError('invalid path: %s' % path)
    files = list_images(path)
    if not files:
        raise ValueError('no images in %s' % path)
    return M.activation_statistics(folder_features(fid, files, batch, workers))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('path', nargs='+', help='two folders / .npz files (one with --save-stats)')
    ap.add_argument('--weights', default=None, metavar='PATH', help="pytorch_fid's FID Inception state dict (default: its hub cache)")
    ap.add_argument('--batch', type=int, default=50)
    ap.add_argument('--save-stats', default=None, metavar='OUT.npz', help='write mu / sigma of the first path')
    ap.add_argument('--workers', type=int, default=None, help='image reader threads (default: the rank\'s share of the cores)')
    a = ap.parse_args(argv)
    if len(a.path) > 2 or (len(a.path) < 2 and a.save_stats is None):
        ap.error('give two paths, or one path and --save-stats')
    # the device is needed for folders only (two .npz files are compared on the host)
    fid = M.FID(a.weights or M.FID.default_path()) if any(not p.endswith('.npz') for p in a.path) else None
    stats = [path_statistics(fid, p, a.batch, a.workers) for p in a.path]
    if a.save_stats:
        np.savez_compressed(a.save_stats, mu=stats[0][0], sigma=stats[0][1])
    if len(stats) < 2:
        return None
    value = M.frechet_distance(*stats[0], *stats[1])
    print('- SR_FID : {:.3f}'.format(value))        # FID.py
    return value


if __name__ == '__main__':
    main()
