"""A CPU restatement of pytorch_fid's InceptionV3(output_blocks=[3], resize_input=True, normalize_input=True,
use_fid_inception=True) with torch.nn.functional, in fp32 or fp64 (a test helper, not collected).  Written from the network's
published definition, independently of csrc/fdsr_fid.hip: the BN is applied unfolded (F.batch_norm, eval, eps 1e-3), the input
transform is not fused (u8 / 255, F.interpolate, 2x - 1), and every module's output is tapped.

    out = forward(sd, u8, dtype=torch.float64)    # sd: name -> array (metrics.FID_TENSORS keys); u8: [B,H,W,3] uint8
    out['input']      [B,3,299,299]
    out[k]            module k of metrics.FID_MODULES, NCHW
    out['pool3']      [B,2048]
    out['convs']      [(name, cin, cout, kh, kw, stride, (ph, pw), hout, wout), ...] in call order
"""
import numpy as np
import torch
import torch.nn.functional as F


class _Net:
    def __init__(self, sd, dtype):
        self.sd = sd
        self.dtype = dtype
        self.convs = []

    def t(self, k):
        return torch.as_tensor(np.asarray(self.sd[k])).to(self.dtype)

    def conv(self, name, x, stride=1, padding=(0, 0)):
        w = self.t(name + '.conv.weight')
        y = F.conv2d(x, w, stride=stride, padding=padding)
        self.convs.append((name, w.shape[1], w.shape[0], w.shape[2], w.shape[3], stride, tuple(padding), y.shape[2], y.shape[3]))
        y = F.batch_norm(y, self.t(name + '.bn.running_mean'), self.t(name + '.bn.running_var'), self.t(name + '.bn.weight'),
                         self.t(name + '.bn.bias'), training=False, eps=0.001)
        return F.relu(y)

    def block_a(self, m, x):                      # FIDInceptionA
        b1 = self.conv(m + '.branch1x1', x)
        b5 = self.conv(m + '.branch5x5_2', self.conv(m + '.branch5x5_1', x), padding=(2, 2))
        b3 = self.conv(m + '.branch3x3dbl_1', x)
        b3 = self.conv(m + '.branch3x3dbl_2', b3, padding=(1, 1))
        b3 = self.conv(m + '.branch3x3dbl_3', b3, padding=(1, 1))
        bp = self.conv(m + '.branch_pool', F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False))
        return torch.cat([b1, b5, b3, bp], 1)

    def block_b(self, m, x):                      # torchvision InceptionB
        b3 = self.conv(m + '.branch3x3', x, stride=2)
        bd = self.conv(m + '.branch3x3dbl_1', x)
        bd = self.conv(m + '.branch3x3dbl_2', bd, padding=(1, 1))
        bd = self.conv(m + '.branch3x3dbl_3', bd, stride=2)
        return torch.cat([b3, bd, F.max_pool2d(x, 3, stride=2)], 1)

    def block_c(self, m, x):                      # FIDInceptionC
        b1 = self.conv(m + '.branch1x1', x)
        b7 = self.conv(m + '.branch7x7_1', x)
        b7 = self.conv(m + '.branch7x7_2', b7, padding=(0, 3))
        b7 = self.conv(m + '.branch7x7_3', b7, padding=(3, 0))
        bd = self.conv(m + '.branch7x7dbl_1', x)
        bd = self.conv(m + '.branch7x7dbl_2', bd, padding=(3, 0))
        bd = self.conv(m + '.branch7x7dbl_3', bd, padding=(0, 3))
        bd = self.conv(m + '.branch7x7dbl_4', bd, padding=(3, 0))
        bd = self.conv(m + '.branch7x7dbl_5', bd, padding=(0, 3))
        bp = self.conv(m + '.branch_pool', F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False))
        return torch.cat([b1, b7, bd, bp], 1)

    def block_d(self, m, x):                      # torchvision InceptionD
        b3 = self.conv(m + '.branch3x3_2', self.conv(m + '.branch3x3_1', x), stride=2)
        b7 = self.conv(m + '.branch7x7x3_1', x)
        b7 = self.conv(m + '.branch7x7x3_2', b7, padding=(0, 3))
        b7 = self.conv(m + '.branch7x7x3_3', b7, padding=(3, 0))
        b7 = self.conv(m + '.branch7x7x3_4', b7, stride=2)
        return torch.cat([b3, b7, F.max_pool2d(x, 3, stride=2)], 1)

    def block_e(self, m, x, max_pool):            # FIDInceptionE_1 (avg, count_include_pad=False) / FIDInceptionE_2 (max)
        b1 = self.conv(m + '.branch1x1', x)
        b3 = self.conv(m + '.branch3x3_1', x)
        b3 = torch.cat([self.conv(m + '.branch3x3_2a', b3, padding=(0, 1)), self.conv(m + '.branch3x3_2b', b3, padding=(1, 0))], 1)
        bd = self.conv(m + '.branch3x3dbl_1', x)
        bd = self.conv(m + '.branch3x3dbl_2', bd, padding=(1, 1))
        bd = torch.cat([self.conv(m + '.branch3x3dbl_3a', bd, padding=(0, 1)), self.conv(m + '.branch3x3dbl_3b', bd, padding=(1, 0))], 1)
        if max_pool:
            p = F.max_pool2d(x, 3, stride=1, padding=1)
        else:
            p = F.avg_pool2d(x, 3, stride=1, padding=1, count_include_pad=False)
        return torch.cat([b1, b3, bd, self.conv(m + '.branch_pool', p)], 1)


def input_transform(u8, dtype=torch.float32):
    """ToTensor (u8 / 255), F.interpolate(size=(299, 299), mode='bilinear', align_corners=False), 2x - 1: [B,3,299,299]"""
    x = torch.as_tensor(np.asarray(u8)).permute(0, 3, 1, 2).to(dtype) / 255
    x = F.interpolate(x, size=(299, 299), mode='bilinear', align_corners=False)
    return 2 * x - 1


def forward(sd, u8, dtype=torch.float32, taps=True):
    net = _Net(sd, dtype)
    out = {}
    with torch.no_grad():
        x = input_transform(u8, dtype)
        out['input'] = x
        seq = [lambda x: net.conv('Conv2d_1a_3x3', x, stride=2),
               lambda x: net.conv('Conv2d_2a_3x3', x),
               lambda x: net.conv('Conv2d_2b_3x3', x, padding=(1, 1)),
               lambda x: F.max_pool2d(x, 3, stride=2),
               lambda x: net.conv('Conv2d_3b_1x1', x),
               lambda x: net.conv('Conv2d_4a_3x3', x),
               lambda x: F.max_pool2d(x, 3, stride=2),
               lambda x: net.block_a('Mixed_5b', x),
               lambda x: net.block_a('Mixed_5c', x),
               lambda x: net.block_a('Mixed_5d', x),
               lambda x: net.block_b('Mixed_6a', x),
               lambda x: net.block_c('Mixed_6b', x),
               lambda x: net.block_c('Mixed_6c', x),
               lambda x: net.block_c('Mixed_6d', x),
               lambda x: net.block_c('Mixed_6e', x),
               lambda x: net.block_d('Mixed_7a', x),
               lambda x: net.block_e('Mixed_7b', x, False),
               lambda x: net.block_e('Mixed_7c', x, True)]
        for k, f in enumerate(seq):
            x = f(x)
            if taps:
                out[k] = x
        out['pool3'] = F.adaptive_avg_pool2d(x, (1, 1)).flatten(1)
    out['convs'] = net.convs
    return out


def seeded_images(seed, n, h, w):
    """n smooth-ish uint8 RGB images (a random low-resolution field bicubically enlarged, plus noise): natural enough that
    the features differ from image to image."""
    g = torch.Generator().manual_seed(seed)
    lo = torch.rand(n, 3, max(2, h // 16), max(2, w // 16), generator=g)
    x = F.interpolate(lo, size=(h, w), mode='bicubic', align_corners=False) + 0.08 * torch.randn(n, 3, h, w, generator=g)
    return (x.clamp(0, 1) * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
