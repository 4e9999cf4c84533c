"""`GaussianDiffusion` facade: the surface DDPM (FastDiffSR/model/model.py) calls on
`netG`, over the HIP engine.  Mirrors the constructor and methods of
FastDiffSR/model/fastdiffsr_modules/diffusion.py:76-289.

Deviation from the reference, documented: the reference's
p_sample_loop raises for batch >= 2 (diffusion.py:215-216); here a batch is B
independent B=1 runs and `continous=True` returns the frames concatenated along
dim 0 exactly as the reference's torch.cat would ([8*B,3,H,W]; for B=1 identical).
"""
import numpy as np
import torch
from torch import nn

from .long_schedule import frame_every, use_stepwise
from .schedule import schedule_buffers, sampling_scalars


class _EngineLoss(torch.autograd.Function):
    """loss = the engine's summed loss of kind `kind` with the engine's backward pass behind autograd: backward() copies the engine's
    gradients (scaled by the incoming gradient of the loss, e.g. 1 / (b*c*h*w)) into the Parameters' .grad."""

    @staticmethod
    def forward(ctx, diffusion, kind, x6, gamma, target, *params):
        eng = diffusion._engine_for_training()
        loss = eng.train_grads(x6, gamma, target, kind, 1.0)
        ctx.eng = eng
        ctx.keys = [k for k, p in diffusion.denoise_fn.named_parameters() if p.requires_grad]
        ctx.live = {k for k, _, live in eng.schema() if live}
        return torch.tensor(loss, device=x6.device, dtype=torch.float32)

    @staticmethod
    def backward(ctx, grad_out):
        scale = float(grad_out)
        grads = []
        for k in ctx.keys:          # never-executed tensors (unet.py:212) get no gradient, as in torch
            grads.append(torch.from_numpy(ctx.eng.get_grad(k)).to(grad_out.device) * scale if k in ctx.live else None)
        return (None, None, None, None, None) + tuple(grads)


class GaussianDiffusion(nn.Module):
    """The flagship's facade, and the base of its siblings' (sr3 / tesr / gdp): the sampling path (p_sample_loop) and the training
    step (optimize_step, p_losses' autograd bridge) are here once; a sibling overrides only what the reference's own diffusion.py
    differs in -- the attributes and the small methods marked `variant` below, next to its set_loss / q_sample / _training_batch."""

    # variant: the network's images are residuals over the upsampled LR image: frames go through res2img, and a training pair through
    # the engine's own img2res + q_sample input kernel (fdsr_train_grads_pairs); the siblings work on the image itself
    residual = True
    # variant: SR3 / GDP draw noise at t = 0 too (masked): T + 1 planes
    noise_at_t0 = False
    # variant: the siblings' schedules run to T = 1000 / 2000; above long_schedule.STEPWISE_ABOVE steps they sample through
    # fdsr_sample_stepwise (chunks of steps as graphs, only the kept frames), and only that path of theirs captures graphs
    long_schedules = False

    def __init__(self, denoise_fn, image_size, channels=3, loss_type='l1', conditional=True, schedule_opt=None, scale=4):
        super().__init__()
        self.channels = channels
        self.image_size = image_size
        self.denoise_fn = denoise_fn
        self.loss_type = loss_type
        self.conditional = conditional
        # conv arithmetic of the HIP engine: 'f16x3' (fp32-grade split-f16 MFMA, default), 'f32' (exact
        # fp32 MFMA) or 'bf16' (PSNR-grade); see include/fdsr.h
        self.precision = 'f16x3'
        # where the sampling noise comes from when the caller passes none: 'torch' = torch.randn on the
        # device in the reference's order (reproducible with torch.manual_seed, like the reference; all planes are drawn up
        # front); 'engine' = drawn inside the HIP loop (Philox, denoise_fn.engine.set_seed)
        self.rng = 'torch'
        # the loop as a captured hipGraph (north_star; include/fdsr.h FDSR_SAMPLE_GRAPH) -- the flagship's T steps as ONE graph, a
        # sibling's long schedule as chunks of steps: 'auto' replays from the second call of a shape on (capture + instantiation of
        # ~3 600 nodes is not worth it for a one-off shape), 'on' from the first, 'off' never.  See _graph_buffers.
        self.graph = 'auto'
        self._gbuf = {}
        # like the reference (:96-98) the schedule is NOT set here; DDPM calls set_new_noise_schedule

    def set_loss(self, device):                                   # :101-107
        if self.loss_type == 'l1':
            self.loss_func = nn.L1Loss(reduction='sum').to(device)
        elif self.loss_type == 'l2':
            self.loss_func = nn.MSELoss(reduction='sum').to(device)
        else:
            raise NotImplementedError()

    def set_new_noise_schedule(self, schedule_opt, device):       # :109-155
        bufs, sqrt_prev = schedule_buffers(schedule_opt)
        self.sqrt_alphas_cumprod_prev = sqrt_prev
        self.num_timesteps = int(bufs['betas'].shape[0])
        for k, v in bufs.items():
            self.register_buffer(k, torch.tensor(v, dtype=torch.float32, device=device))
        self.denoise_fn.engine.set_schedule(sampling_scalars(bufs, sqrt_prev))

    # -- sampling ------------------------------------------------------------------
    def _graph_buffers(self, key, x, traj_slots):
        """The cond / out / trajectory (and, once needed, 'noise') buffers of one shape.  Graph replays need stable addresses, so the
        caller's tensors are copied in and results are cloned out, and the buffers stay allocated between calls, for the last few
        shapes: with noise (explicit or rng = 'torch') that includes the [planes,B,3,H,W] noise buffer, 12.6 GB at B = 16, 256^2,
        T = 1000.  graph = 'off' keeps nothing; long_schedule.release_buffers(self) frees the long schedules' buffers (the next
        graph call of a shape captures again)."""
        buf = self._gbuf.setdefault(key, {})
        if 'cond' not in buf:
            if len(self._gbuf) > 4:                               # shapes come and go: keep the buffers of the last few
                for old in [k_ for k_ in self._gbuf if k_ != key][:len(self._gbuf) - 4]:
                    del self._gbuf[old]
            buf['cond'] = torch.empty_like(x)
            buf['out'] = torch.empty_like(x)
            buf['traj'] = torch.empty((traj_slots,) + tuple(x.shape), device=x.device, dtype=torch.float32) if traj_slots else None
        return buf

    @torch.no_grad()
    def p_sample_loop(self, x_in, continous=False, noise=None):   # :192-221
        if not self.conditional:
            raise NotImplementedError('only the conditional (super-resolution) branch is implemented')
        device = self.betas.device
        x = x_in.to(device=device, dtype=torch.float32).contiguous()
        T = self.num_timesteps
        unet = self.denoise_fn
        unet.sync_weights()
        eng = unet.engine
        eng.set_precision(self.precision)
        # the reference samples after netG.eval() (model.py:60), which turns off the Dropout a training step left live; in .train()
        # mode its Dropout would be live here too, and so it is (the engine then insists on the fp32 kernels)
        live_dropout = bool(unet.training and unet.cfg.dropout > 0)
        eng.set_training(live_dropout, seed_from_torch=True)
        stepwise = self.long_schedules and use_stepwise(T)
        every = frame_every(T)                                    # sample_inter (:195)
        route = dict(stepwise=True, traj_every=every) if stepwise else {}
        # graphs: the flagship's fdsr_sample loop and a sibling's stepwise loop, per shape, and never with live dropout (a replay
        # would repeat its masks)
        key = ('stepwise' if stepwise else 'loop', tuple(x.shape), bool(continous), str(device), T)
        seen = self._gbuf.get(key)
        can_graph = self.graph != 'off' and (stepwise or not self.long_schedules)
        use_graph = can_graph and not live_dropout and (self.graph == 'on' or seen is not None)
        if can_graph and self.graph == 'auto' and seen is None:
            self._gbuf[key] = {}          # this shape has been sampled once: the next call captures
        traj_slots = (eng.traj_slots(every) if stepwise else T) if continous else 0
        buf = self._graph_buffers(key, x, traj_slots) if use_graph else {}          # eager: nothing is kept
        if noise is not None or self.rng != 'engine':            # else None: the engine draws inside the loop (Philox)
            given = noise
            if use_graph or given is None:
                noise = buf.get('noise')
                if noise is None:
                    planes = T + (1 if self.noise_at_t0 else 0)
                    noise = buf['noise'] = torch.empty((planes,) + tuple(x.shape), device=device, dtype=torch.float32)
            if given is None:
                # torch's stream as the reference consumes it: randn(shape) (:207), then one randn_like per step (:189)
                for plane in noise:
                    torch.randn(x.shape, device=device, out=plane)
            elif use_graph:
                noise.copy_(given)
        # (the f16x3 range guard and its exact-fp32 re-run live in Engine.sample: Engine.on_saturation)
        if use_graph:
            buf['cond'].copy_(x)
            res = eng.sample(buf['cond'], noise, want_traj=bool(continous), graph=True, out=buf['out'], traj=buf['traj'], **route)
        else:
            res = eng.sample(x, noise, want_traj=bool(continous), graph=False, **route)
        if not continous:
            return self._result(res.clone() if use_graph else res)
        traj = res[1]                     # (stepwise: the kept frames only) no clone of a graph's buffer: res2img / torch.cat make new tensors
        kept = traj if stepwise else [traj[k] for k, t in enumerate(reversed(range(T))) if t % every == 0]
        return torch.cat([self._frame(x, x)] + [self._frame(x_t, x) for x_t in kept], dim=0)

    def _result(self, img):               # variant: what continous=False returns of the batch
        return img

    def _frame(self, x_t, x):             # one frame of ret_img; ret_img[0] = res2img(x_in, x_in) (:215-216)
        return self.res2img(x_t, x) if self.residual else x_t

    @torch.no_grad()
    def sample(self, batch_size=1, continous=False):              # :223-227 (crashes in the reference)
        raise NotImplementedError('unconditional sampling is broken in the reference (diffusion.py:224-227)')

    @torch.no_grad()
    def super_resolution(self, x_in, continous=False):            # :229-231
        return self.p_sample_loop(x_in, continous)

    # -- training surface -------------------------------------------------------------
    def q_sample(self, x_start, continuous_sqrt_alpha_cumprod, noise=None):   # :233-241
        noise = torch.randn_like(x_start) if noise is None else noise
        return continuous_sqrt_alpha_cumprod * x_start + (1 - continuous_sqrt_alpha_cumprod ** 2).sqrt() * noise

    def _training_batch(self, x_in, noise=None):                  # :242-266, the part before the network
        """x_start, the numpy draws of t and gamma (reference: numpy global RNG), noise, q_sample."""
        x_start = self.img2res(x_in['HR'], x_in['SR'])
        b = x_start.shape[0]
        t = np.random.randint(1, self.num_timesteps + 1)
        gamma = torch.FloatTensor(np.random.uniform(self.sqrt_alphas_cumprod_prev[t - 1],
                                                    self.sqrt_alphas_cumprod_prev[t], size=b)).to(x_start.device)
        gamma = gamma.view(b, -1)
        noise = torch.randn_like(x_start) if noise is None else noise
        x_noisy = self.q_sample(x_start, gamma.view(-1, 1, 1, 1), noise)
        return torch.cat([x_in['SR'], x_noisy], dim=1).contiguous(), gamma, noise.contiguous()

    def _engine_loss(self):
        """variant: (the engine's loss kind, whether loss_func is the MEAN of the engine's sum)"""
        return self.loss_type, False

    def p_losses(self, x_in, noise=None):                         # :242-270
        """What loss_func gives for the network's prediction, RNG draws as in the reference (_training_batch).  In train mode with
        autograd on, the result carries a grad_fn whose backward is the ENGINE's backward pass: the reference's
        `l_pix.sum() / n; l_pix.backward(); optG.step()` (model.py:49-56) then works unchanged on the module's
        Parameters.  The all-device fast path is optimize_step()."""
        x6, t, target = self._training_batch(x_in, noise)
        if self.denoise_fn.training and torch.is_grad_enabled():
            kind, mean = self._engine_loss()
            params = [p for p in self.denoise_fn.parameters() if p.requires_grad]
            loss = _EngineLoss.apply(self, kind, x6, t.float(), target, *params)
            return loss / target.numel() if mean else loss
        with torch.no_grad():
            x_recon = self.denoise_fn(x6, t)
        return self.loss_func(target, x_recon)

    def _engine_for_training(self):
        unet = self.denoise_fn
        unet.sync_weights(for_training=True)
        eng = unet.engine
        # 'f32' (everything exact fp32) or 'f16x3' (every convolution -- forward, input and weight gradients -- fp32-grade on
        # split-f16 MFMAs)
        eng.set_precision('f32' if self.precision in ('bf16', 'f16') else self.precision)
        eng.set_training(unet.training and unet.cfg.dropout > 0, seed_from_torch=True)   # Dropout(p) of block2 is live in .train() mode
        return eng

    def optimize_step(self, x_in, lr, betas=(0.9, 0.999), eps=1e-8, noise=None, grad_hook=None, global_batch=None):
        """DDPM.optimize_parameters (model/model.py:47-57) entirely on the device: forward, loss / (b*c*h*w),
        backward, Adam on the engine's master copy.  Returns the SUMMED loss of this rank's samples divided by the
        global element count (a python float; summed over ranks it is the reference's l_pix).  grad_hook(engine) runs
        between backward and the optimiser (data-parallel all-reduce of the gradient arena, parallel.allreduce_grads).
        Where loss_func is a mean (TESR's Charbonnier), l_pix is that mean divided by b*c*h*w once more (model.py:50-52 divides
        whatever netG returned): sum / (b*c*h*w)^2, which is what this returns and what the engine back-propagates.

        Data parallel: `global_batch` is the number of samples of the WHOLE step over all ranks -- every rank divides by
        global_batch*c*h*w and the all-reduce SUMS the arenas, so per-sample weights are right for ragged shards too; a
        rank whose shard is empty (b == 0) contributes a zero arena and still takes part in the all-reduce."""
        b, c, h, w = x_in['HR'].shape
        gb = int(global_batch) if global_batch is not None else int(b)
        if gb < 1:
            raise ValueError('optimize_step: the global batch is empty')
        n = gb * int(c * h * w)
        kind, mean = self._engine_loss()
        div = float(n) * float(n) if mean else n
        eng = self._engine_for_training()
        if b == 0:
            eng.zero_grads(x_in['HR'].device)
            loss = 0.0
        elif self.residual:
            # the RNG draws are the reference's (numpy for t and gamma, torch for the noise: diffusion.py:246-259); img2res,
            # q_sample and the channel concat happen in the engine's input kernel (the arithmetic of _training_batch's tensors)
            hr, sr = x_in['HR'].float().contiguous(), x_in['SR'].float().contiguous()
            t = np.random.randint(1, self.num_timesteps + 1)
            gamma = torch.FloatTensor(np.random.uniform(self.sqrt_alphas_cumprod_prev[t - 1], self.sqrt_alphas_cumprod_prev[t],
                                                        size=b)).to(hr.device)
            noise = torch.randn_like(hr) if noise is None else noise
            loss = eng.train_grads_pairs(hr, sr, gamma, noise.contiguous(), kind, 1.0 / div)
        else:
            x6, t, target = self._training_batch(x_in, noise)
            loss = eng.train_grads(x6, t.float(), target, kind, 1.0 / div)
        if grad_hook is not None:
            grad_hook(eng)
        eng.adam_step(lr, betas, eps)
        self.denoise_fn._engine_ahead = True
        return loss / div

    def forward(self, x, *args, **kwargs):                        # :272-273
        return self.p_losses(x, *args, **kwargs)

    def res2img(self, img_, img_lr_up, clip_input=None):          # :275-281
        if clip_input is None or clip_input:
            img_ = img_.clamp(-1, 1)
        return img_ / 2.0 + img_lr_up

    def img2res(self, x, img_lr_up, clip_input=None):             # :283-289
        x = (x - img_lr_up) * 2.0
        if clip_input is None or clip_input:
            x = x.clamp(-1, 1)
        return x
