"""`GaussianDiffusion` facade of the SR3 sibling (FastDiffSR/model/ddpm_modules/diffusion.py:78-300) over the
HIP engine: discrete-time reverse process, the network sees the integer t, the output is x_0 itself."""
import torch
from torch import nn

from .. import diffusion as _d


class GaussianDiffusion(_d.GaussianDiffusion):
    residual = False                                              # the network sees the image itself (:279-291)
    long_schedules = True                                         # T = 1000 in the reference's configs
    noise_at_t0 = True                                            # one noise_like draw per step, t = 0 included (:189-196, :215)

    def __init__(self, denoise_fn, image_size, channels=3, loss_type='l1', conditional=True, schedule_opt=None):
        super().__init__(denoise_fn, image_size, channels=channels, loss_type=loss_type, conditional=conditional,
                         schedule_opt=schedule_opt)

    def set_loss(self, device):                                   # :96-102
        if self.loss_type == 'l1':
            self.loss_func = nn.L1Loss(reduction='sum').to(device)
        elif self.loss_type == 'l2':
            self.loss_func = nn.MSELoss(reduction='sum').to(device)
        else:
            raise NotImplementedError()

    def _result(self, img):                                       # ret_img[-1] of one image, a batch whole (:198-227)
        return img[-1] if img.shape[0] == 1 else img

    # -- training (ddpm_modules/diffusion.py:260-300; DDPM.optimize_parameters, model/model.py:47-57) ------------------
    def q_sample(self, x_start, t, noise=None):                   # :260-268 (the "fix gama" branch)
        noise = torch.randn_like(x_start) if noise is None else noise
        a = self.sqrt_alphas_cumprod[t].view(-1, 1, 1, 1)
        b = self.sqrt_one_minus_alphas_cumprod[t].view(-1, 1, 1, 1)
        return a * x_start + b * noise

    def _training_batch(self, x_in, noise=None):                  # :279-291, the part before the network
        """The reference's draws: t = torch.randint(0, T, (b,)) then noise = randn_like(x_start), both from torch's generator of
        x_start's device; x_start is the HR image itself (SR3 predicts the noise of the image, not of a residual)."""
        x_start = x_in['HR'].float()
        b = x_start.shape[0]
        t = torch.randint(0, self.num_timesteps, (b,), device=x_start.device).long()
        noise = torch.randn_like(x_start) if noise is None else noise
        x_noisy = self.q_sample(x_start, t, noise)
        return torch.cat([x_in['SR'].float(), x_noisy], dim=1).contiguous(), t, noise.contiguous()
