"""`GaussianDiffusion` facade of the TESR sibling (FastDiffSR/model/tesr_modules/diffusion.py:66-252) over the HIP
engine.  Same reverse process as FastDiffSR's (continuous noise level sqrt(alpha_bar), :154-181) but the network
predicts the image itself: no img2res / res2img, `p_sample_loop` returns `ret_img[-1]` (:183-204), and the 'l1'
loss is the Charbonnier mean (:85-90, unet.py:956-967)."""
import numpy as np
import torch
from torch import nn

from .. import diffusion as _d


class CharbonnierLoss(nn.Module):                                 # tesr_modules/unet.py:956-967
    def __init__(self, eps=1e-3):
        super().__init__()
        self.eps = eps

    def forward(self, x, y):
        diff = x - y
        return torch.mean(torch.sqrt((diff * diff) + (self.eps * self.eps)))


class GaussianDiffusion(_d.GaussianDiffusion):
    residual = False                                              # the network predicts the image itself (:225)
    long_schedules = True                                         # T = 2000 in the reference's configs

    def __init__(self, denoise_fn, image_size, channels=3, loss_type='l1', conditional=True, schedule_opt=None, scale=None):
        super().__init__(denoise_fn, image_size, channels=channels, loss_type=loss_type, conditional=conditional,
                         schedule_opt=schedule_opt)

    def set_loss(self, device):                                   # :85-94
        if self.loss_type == 'l1':
            self.loss_func = CharbonnierLoss().to(device)
        elif self.loss_type == 'l2':
            self.loss_func = nn.MSELoss(reduction='sum').to(device)
        else:
            raise NotImplementedError()

    def _result(self, img):                                       # ret_img[-1]: the last image of the batch (:203-204)
        return img[-1]

    def _training_batch(self, x_in, noise=None):                  # :224-244, the part before the network
        x_start = x_in['HR'].float()                              # the image itself, not a residual (:225)
        b = x_start.shape[0]
        t = np.random.randint(1, self.num_timesteps + 1)
        gamma = torch.FloatTensor(np.random.uniform(self.sqrt_alphas_cumprod_prev[t - 1],
                                                    self.sqrt_alphas_cumprod_prev[t], size=b)).to(x_start.device)
        gamma = gamma.view(b, -1)
        noise = torch.randn_like(x_start) if noise is None else noise
        x_noisy = self.q_sample(x_start, gamma.view(-1, 1, 1, 1), noise)
        return torch.cat([x_in['SR'].float(), x_noisy], dim=1).contiguous(), gamma, noise.contiguous()

    def _engine_loss(self):                                       # 'l1' is the Charbonnier MEAN (:85-90)
        return ('charbonnier', True) if self.loss_type == 'l1' else ('l2', False)
