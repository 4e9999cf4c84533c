"""`GaussianDiffusion` facade of the GDP sibling (FastDiffSR/model/gdp_modules/diffusion.py:64-300) over the HIP engine.
The network predicts x_0 (clamped, :189-195) from cat([x_t, cond]) and the integer time step; every step draws noise
(masked at t = 0, :206-211); `p_sample_loop` returns `ret_img[-1]` (:238-241); both loss types are the summed MSE (:83-89)."""
import torch
from torch import nn

from .. import diffusion as _d


class GaussianDiffusion(_d.GaussianDiffusion):
    residual = False                                              # the network predicts x_0 of the image itself (:277-290)
    long_schedules = True                                         # T = 1000 in the reference's configs
    noise_at_t0 = True                                            # every step draws noise, masked at t = 0 (:206-211)

    def __init__(self, denoise_fn, image_size, channels=3, loss_type='l2', conditional=True, schedule_opt=None, scale=4):
        super().__init__(denoise_fn, image_size, channels=channels, loss_type=loss_type, conditional=conditional,
                         schedule_opt=schedule_opt)

    def set_loss(self, device):                                   # :83-89: 'l1' is MSE too
        if self.loss_type in ('l1', 'l2'):
            self.loss_func = nn.MSELoss(reduction='sum').to(device)
        else:
            raise NotImplementedError()

    def _result(self, img):                                       # ret_img[-1]: the last image of the batch (:238-241)
        return img[-1]

    def q_sample(self, x_start, t, noise=None):                   # :258-265
        noise = torch.randn_like(x_start) if noise is None else noise
        a = self.sqrt_alphas_cumprod[t].view(-1, 1, 1, 1)
        s = self.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1)
        return a * x_start + s * noise

    def _engine_loss(self):                                       # :83-89: both loss types are the summed MSE
        return 'l2', False

    def _training_batch(self, x_in, noise=None):                  # :277-290, the part before the network
        """The reference's draws: t = torch.randint(0, T, (b,)), then noise = randn_like(x_start), both from torch's generator of
        x_start's device; the network sees cat([x_t, SR]) and its target is x_start = HR itself (it predicts x_0)."""
        x_start = x_in['HR'].float()
        b = x_start.shape[0]
        t = torch.randint(0, self.num_timesteps, (b,), device=x_start.device).long()
        noise = torch.randn_like(x_start) if noise is None else noise
        x_t = self.q_sample(x_start, t, noise)
        return torch.cat([x_t, x_in['SR'].float()], dim=1).contiguous(), t, x_start.contiguous()
