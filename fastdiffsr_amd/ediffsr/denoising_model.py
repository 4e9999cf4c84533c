"""DenoisingModel (EDiffSR/codes/config/sisr/models/denoising_model.py) on the HIP engine: the reference's training surface
around ConditionalNAFNet.  optimize_parameters is one engine call for the loss and the gradients and one for the optimizer; the
learning-rate schedules are evaluated on the host.  Not on this engine-only path: the EMA copy, multi-rank training,
is_weighted, any loss other than l1 / l2.  All four are reached the other way round: the reference's own DenoisingModel around
this package's ConditionalNAFNet with requires_grad_(True), whose forward is differentiable through torch autograd (model.py;
INTEGRATION 6).  On neither path: f16x3 or bf16 training, DenoisingUNet_arch.

train_precision='f16' trains with f16 activation storage and fp32 gradients (ConditionalNAFNet.set_train_precision).  Its range
guard is read after every train_grads: a step whose forward left the f16 range is skipped -- the weights and the optimizer state
stay as they were -- with a warning that names the iteration; skipped_steps counts them and consecutive_skips the current run,
which ediffsr.train stops on."""
import math
import os
import warnings
from collections import OrderedDict

import torch

from .. import _lib
from .model import ConditionalNAFNet


def cosine_annealing_lr(base_lr, step, t_max, eta_min):
    """torch.optim.lr_scheduler.CosineAnnealingLR's closed form (TrueCosineAnnealingLR) after `step` scheduler steps."""
    return eta_min + (base_lr - eta_min) * (1 + math.cos(math.pi * step / t_max)) / 2


def multistep_restart_lr(base_lr, step, milestones, gamma=0.1, restarts=None, weights=None):
    """MultiStepLR_Restart (models/lr_scheduler.py) after `step` scheduler steps: the rate decays by gamma at every milestone;
    at a restart it becomes base_lr * weight and the decay starts again."""
    restarts = list(restarts) if restarts else [0]
    weights = list(weights) if weights else [1]
    start, w = 0, None
    for r, wt in zip(restarts, weights):
        if r and step >= r:
            start, w = r, wt
    lr = base_lr * w if w is not None else base_lr
    for ms in sorted(milestones or []):
        if start < ms <= step:
            lr *= gamma
    return lr


class DenoisingModel:
    def __init__(self, opt, train_precision='f32'):
        self.opt = opt
        self.train_precision = train_precision
        self.skipped_steps = 0        # optimizer steps skipped because the f16 forward saturated
        self.consecutive_skips = 0    # ... since the last step that was taken
        self.is_train = opt.get('is_train', True)
        self.device = torch.device('cuda', torch.cuda.current_device())
        net = opt['network_G']
        if net.get('which_model_G', 'ConditionalNAFNet') != 'ConditionalNAFNet':
            raise NotImplementedError('only ConditionalNAFNet trains on this engine (not %s)' % net['which_model_G'])
        self.model = ConditionalNAFNet(**net['setting']).to(self.device)
        if train_precision != 'f32':
            self.model.set_train_precision(train_precision)
        self.schedulers, self.optimizers = [], []
        self.log_dict = OrderedDict()
        self.load()
        if self.is_train:
            t = opt['train']
            if t.get('is_weighted'):
                raise NotImplementedError('is_weighted is not supported (the reference passes no weights to MatchingLoss)')
            self.loss_type = t.get('loss_type', 'l1')
            self.weight = t.get('weight', 1.0)
            self.optimizer = t.get('optimizer', 'Adam')
            if self.optimizer not in ConditionalNAFNet.OPTIMIZERS:
                raise NotImplementedError('optimizer %s (Adam, AdamW, Lion)' % self.optimizer)
            self.base_lr = float(t['lr_G'])
            self.lr = self.base_lr
            self.betas = (t.get('beta1', 0.9), t.get('beta2', 0.999))
            self.wd = t.get('weight_decay_G') or 0
            self.scheme = t.get('lr_scheme', 'TrueCosineAnnealingLR')
            if self.scheme not in ('TrueCosineAnnealingLR', 'MultiStepLR'):
                raise NotImplementedError('MultiStepLR learning rate scheme is enough.')
            self.sched_step = 0

    # ---- data ----
    def feed_data(self, state, LQ, GT=None):
        self.state = state.to(self.device)
        self.condition = LQ.to(self.device)
        if GT is not None:
            self.state_0 = GT.to(self.device)

    def optimize_parameters(self, step, timesteps, sde=None):
        sde.set_mu(self.condition)
        out = self.model.train_grads(self.state, self.condition, self.state_0, timesteps, loss_type=self.loss_type, weight=self.weight)
        self.log_dict['loss'] = out[0].item()
        if self.train_precision == 'f16':   # the .item() above has synchronised already
            try:
                self.model.check_saturation()
            except _lib.FdsrSaturated:
                self.skipped_steps += 1
                self.consecutive_skips += 1
                warnings.warn('iteration %d: an activation left the f16 range, the optimizer step is skipped (%d skipped so far)'
                              % (step, self.skipped_steps))
                return
        self.consecutive_skips = 0
        self.model.optim_step(self.optimizer, self.lr, self.betas, 1e-8, self.wd)

    def test(self, sde=None, save_states=False):
        sde.set_mu(self.condition)
        with torch.no_grad():
            self.output = sde.reverse_sde(self.state)

    def get_current_log(self):
        return self.log_dict

    def get_current_visuals(self, need_GT=True):
        out = OrderedDict()
        out['Input'] = self.condition.detach()[0].float().cpu()
        out['Output'] = self.output.detach()[0].float().cpu()
        if need_GT:
            out['GT'] = self.state_0.detach()[0].float().cpu()
        return out

    # ---- learning rate ----
    def _lr_at(self, k):
        t = self.opt['train']
        if self.scheme == 'TrueCosineAnnealingLR':
            return cosine_annealing_lr(self.base_lr, k, t['niter'], t.get('eta_min', 0))
        return multistep_restart_lr(self.base_lr, k, t.get('lr_steps'), t.get('lr_gamma', 0.1), t.get('restarts'), t.get('restart_weights'))

    def update_learning_rate(self, cur_iter, warmup_iter=-1):
        self.sched_step += 1
        self.lr = self._lr_at(self.sched_step)
        if cur_iter < warmup_iter:
            self.lr = self.lr / warmup_iter * cur_iter

    def get_current_learning_rate(self):
        return self.lr

    # ---- files ----
    def load(self):
        path = self.opt['path'].get('pretrain_model_G')
        if path is not None:
            sd = torch.load(path, map_location='cpu', weights_only=True)
            self.model.load_state_dict({k[7:] if k.startswith('module.') else k: v for k, v in sd.items()},
                                       strict=self.opt['path'].get('strict_load', True))

    def save(self, iter_label):
        path = os.path.join(self.opt['path']['models'], '{}_G.pth'.format(iter_label))
        torch.save(OrderedDict((k, v.detach().cpu()) for k, v in self.model.state_dict().items()), path)
        return path

    def save_training_state(self, epoch, iter_step):
        st = {}
        for i, k in enumerate(self.model._names):
            m, v, step = self.model.optim_state(k)
            st[i] = {'step': step, 'exp_avg': m} if self.optimizer == 'Lion' else {'step': step, 'exp_avg': m, 'exp_avg_sq': v}
        state = {'epoch': epoch, 'iter': iter_step, 'lr': self.lr, 'sched_step': self.sched_step,
                 'optimizers': [{'state': st, 'kind': self.optimizer}], 'schedulers': [{'last_epoch': self.sched_step}]}
        path = os.path.join(self.opt['path']['training_state'], '{}.state'.format(iter_step))
        torch.save(state, path)
        return path

    def resume_training(self, resume_state):
        st = resume_state['optimizers'][0]['state']
        for i, k in enumerate(self.model._names):
            self.model.set_optim_state(k, st[i]['exp_avg'], st[i].get('exp_avg_sq'), int(st[i]['step']))
        self.sched_step = int(resume_state['sched_step'])
        self.lr = float(resume_state['lr'])
