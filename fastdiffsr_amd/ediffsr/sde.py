"""IRSDE (EDiffSR/codes/utils/sde_utils.py) as far as sampling and training need it.  The tables are built with the reference's own
fp32 torch operations, so they equal the reference's bit for bit.  With this package's ConditionalNAFNet as the model,
reverse_sde / reverse_ode are one engine call; with any other callable they run the reference's Python loop."""
import math

import torch

from .model import ConditionalNAFNet


def theta_schedule(schedule, timesteps):
    if schedule == 'constant':
        return torch.ones(timesteps + 1, dtype=torch.float32)
    if schedule == 'linear':
        n = timesteps + 1
        scale = 1000 / n
        return torch.linspace(scale * 0.0001, scale * 0.02, n, dtype=torch.float32)
    if schedule == 'cosine':
        s = 0.008
        n = timesteps + 2
        x = torch.linspace(0, n, n + 1, dtype=torch.float32)
        alphas_cumprod = torch.cos(((x / n) + s) / (1 + s) * math.pi * 0.5) ** 2
        alphas_cumprod = alphas_cumprod / alphas_cumprod[0]
        return 1 - alphas_cumprod[1:-1]
    raise ValueError('unknown schedule %r (cosine, linear, constant)' % (schedule,))


class IRSDE:
    """Timesteps run from 1 to T; state t = 0 is never used."""

    def __init__(self, max_sigma, T=100, schedule='cosine', eps=0.01, device=None, rng='torch', graph=False, seed=0):
        if rng not in ('torch', 'engine'):
            raise ValueError("rng is 'torch' or 'engine'")
        self.T = T
        self.device = device
        self.rng, self.graph, self.seed = rng, graph, seed
        self.first_image = 0
        self.max_sigma = max_sigma / 255 if max_sigma >= 1 else max_sigma
        thetas = theta_schedule(schedule, T)
        sigmas = torch.sqrt(self.max_sigma ** 2 * 2 * thetas)
        thetas_cumsum = torch.cumsum(thetas, dim=0) - thetas[0]
        self.dt = -1 / thetas_cumsum[-1] * math.log(eps)
        sigma_bars = torch.sqrt(self.max_sigma ** 2 * (1 - torch.exp(-2 * thetas_cumsum * self.dt)))
        self.thetas = thetas.to(device)
        self.sigmas = sigmas.to(device)
        self.thetas_cumsum = thetas_cumsum.to(device)
        self.sigma_bars = sigma_bars.to(device)
        self.mu = 0.
        self.model = None

    def set_mu(self, mu):
        self.mu = mu

    def set_model(self, model):
        self.model = model
        if isinstance(model, ConditionalNAFNet):
            dev = self.device if self.device is not None and torch.device(self.device).type == 'cuda' else torch.device('cuda', torch.cuda.current_device())
            model.set_sde(self.thetas, self.sigmas, self.sigma_bars, float(self.dt), dev, thetas_cumsum=self.thetas_cumsum)
            model._sde_T = self.T

    def mu_bar(self, x0, t):
        return self.mu + (x0 - self.mu) * torch.exp(-self.thetas_cumsum[t] * self.dt)

    def sigma_bar(self, t):
        return self.sigma_bars[t]

    def sigma(self, t):
        return self.sigmas[t]

    def theta(self, t):
        return self.thetas[t]

    def noise_state(self, tensor):
        return tensor + torch.randn_like(tensor) * self.max_sigma

    def noise_fn(self, x, t, **kwargs):
        return self.model(x, self.mu, t, **kwargs)

    def score_fn(self, x, t, **kwargs):
        return -self.noise_fn(x, t, **kwargs) / self.sigma_bar(t)

    def sde_reverse_drift(self, x, score, t):
        return (self.thetas[t] * (self.mu - x) - self.sigmas[t] ** 2 * score) * self.dt

    def ode_reverse_drift(self, x, score, t):
        return (self.thetas[t] * (self.mu - x) - 0.5 * self.sigmas[t] ** 2 * score) * self.dt

    def dispersion(self, x, t):
        return self.sigmas[t] * (torch.randn_like(x) * math.sqrt(self.dt)).to(self.device)

    def _engine(self, xt, T, ode, noise, trajectory):
        if T not in (-1, self.T):
            raise NotImplementedError('the engine samples the whole schedule (T = %d)' % self.T)
        if noise is None and not ode and self.rng == 'torch':
            # the reference draws randn_like per step from torch's generator: same draws, in the same order
            noise = torch.stack([torch.randn_like(xt) for _ in range(self.T)])
        return self.model.sample(xt, self.mu, noise=noise, seed=self.seed, first_image=self.first_image, graph=self.graph, ode=ode,
                                 trajectory=trajectory)

    def reverse_sde(self, xt, T=-1, noise=None, trajectory=False, **kwargs):
        if isinstance(self.model, ConditionalNAFNet):
            return self._engine(xt, T, False, noise, trajectory)
        T = self.T if T < 0 else T
        x = xt.clone()
        for t in reversed(range(1, T + 1)):
            score = self.score_fn(x, t, **kwargs)
            x = x - self.sde_reverse_drift(x, score, t) - self.dispersion(x, t)
        return x

    def reverse_ode(self, xt, T=-1, trajectory=False, **kwargs):
        if isinstance(self.model, ConditionalNAFNet):
            return self._engine(xt, T, True, None, trajectory)
        T = self.T if T < 0 else T
        x = xt.clone()
        for t in reversed(range(1, T + 1)):
            score = self.score_fn(x, t, **kwargs)
            x = x - self.ode_reverse_drift(x, score, t)
        return x

    def get_score_from_noise(self, noise, t):
        return -noise / self.sigma_bar(t)

    def reverse_sde_step_mean(self, x, score, t):
        return x - self.sde_reverse_drift(x, score, t)

    def reverse_optimum_step(self, xt, x0, t):
        A = torch.exp(-self.thetas[t] * self.dt)
        B = torch.exp(-self.thetas_cumsum[t] * self.dt)
        C = torch.exp(-self.thetas_cumsum[t - 1] * self.dt)
        term1 = A * (1 - C ** 2) / (1 - B ** 2)
        term2 = C * (1 - A ** 2) / (1 - B ** 2)
        return term1 * (xt - self.mu) + term2 * (x0 - self.mu) + self.mu

    def generate_random_states(self, x0, mu):
        """The training states: timesteps by randint, then the noise by randn_like, in the reference's order.  As in the
        reference's train.py, the model is set first (set_model): an IRSDE without one has nothing to train and refuses."""
        if self.model is None:
            raise NotImplementedError('IRSDE.generate_random_states: no model is set (set_model); EDiffSR trains through '
                                      'fastdiffsr_amd.ediffsr.DenoisingModel')
        x0 = x0.to(self.device)
        mu = mu.to(self.device)
        self.set_mu(mu)
        batch = x0.shape[0]
        timesteps = torch.randint(1, self.T + 1, (batch, 1, 1, 1)).long()
        state_mean = self.mu_bar(x0, timesteps)
        noises = torch.randn_like(state_mean)
        noise_level = self.sigma_bar(timesteps)
        noisy_states = noises * noise_level + state_mean
        return timesteps, noisy_states.to(torch.float32)
