"""Plain-torch, dtype-generic restatement of one EDiffSR training step (config/sisr/models/denoising_model.py:
optimize_parameters): autograd over ediffsr_restatement.forward, the IR-SDE terms of utils/sde_utils.py, MatchingLoss and the three
optimizers of the reference's driver (torch.optim.Adam / AdamW single-tensor updates, models/optimizer.py's Lion)."""
import math

import torch

import ediffsr_restatement as R


def cast_tables(sde, dtype):
    """(thetas, sigmas, sigma_bars, thetas_cumsum, dt) of sde.IRSDE in the compute dtype."""
    return tuple(torch.as_tensor(v).to('cpu', dtype) for v in (sde.thetas, sde.sigmas, sde.sigma_bars, sde.thetas_cumsum, sde.dt))


def reverse_sde_step_mean(tables, x, mu, score, t):
    thetas, sigmas, _, _, dt = tables
    return x - (thetas[t] * (mu - x) - sigmas[t] ** 2 * score) * dt


def reverse_optimum_step(tables, xt, x0, mu, t):
    thetas, _, _, cum, dt = tables
    A = torch.exp(-thetas[t] * dt)
    B = torch.exp(-cum[t] * dt)
    C = torch.exp(-cum[t - 1] * dt)
    term1 = A * (1 - C ** 2) / (1 - B ** 2)
    term2 = C * (1 - A ** 2) / (1 - B ** 2)
    return term1 * (xt - mu) + term2 * (x0 - mu) + mu


def matching_loss(predict, target, loss_type):
    d = predict - target
    if loss_type == 'l1':
        per = d.abs()
    elif loss_type == 'l2':
        per = d * d
    else:
        raise ValueError('invalid loss type %s' % loss_type)
    return per.flatten(1).mean(dim=1).mean()


def loss(sd, tables, state, mu, x0, timesteps, loss_type='l1', weight=1.0):
    """timesteps: long [B,1,1,1] (generate_random_states' shape).  Returns (loss, xt_1_expection, xt_1_optimum)."""
    t = timesteps.reshape(-1, 1, 1, 1).long()
    noise = R.forward(sd, state, mu, t.reshape(-1))
    score = -noise / tables[2][t]
    expect = reverse_sde_step_mean(tables, state, mu, score, t)
    optimum = reverse_optimum_step(tables, state, x0, mu, t)
    return weight * matching_loss(expect, optimum, loss_type), expect, optimum


def loss_and_grads(sd, tables, state, mu, x0, timesteps, loss_type='l1', weight=1.0):
    """sd in the compute dtype.  Returns (loss as a python float of that dtype's value, {key: gradient})."""
    leaves = {k: v.detach().clone().requires_grad_(True) for k, v in sd.items()}
    val, _, _ = loss(leaves, tables, state, mu, x0, timesteps, loss_type, weight)
    keys = list(leaves)
    gs = torch.autograd.grad(val, [leaves[k] for k in keys], allow_unused=True)
    return val.detach(), {k: (torch.zeros_like(leaves[k]) if g is None else g) for k, g in zip(keys, gs)}


def optim_step(kind, p, g, state, lr, beta1, beta2, eps, wd):
    """One update of one tensor in p's dtype; state: dict with 'step', 'exp_avg', 'exp_avg_sq' (created on first use).
    Returns the new parameter; state is updated in place."""
    if 'exp_avg' not in state:
        state.update(step=0, exp_avg=torch.zeros_like(p), exp_avg_sq=torch.zeros_like(p))
    state['step'] += 1
    m, v, step = state['exp_avg'], state['exp_avg_sq'], state['step']
    if kind == 'Lion':
        p = p * (1 - lr * wd)
        update = m * beta1 + g * (1 - beta1)
        p = p + torch.sign(update) * (-lr)
        state['exp_avg'] = m * beta2 + g * (1 - beta2)
        return p
    if kind == 'AdamW':
        p = p * (1 - lr * wd)
    elif kind == 'Adam':
        if wd != 0:
            g = g + wd * p
    else:
        raise ValueError(kind)
    m = m + (1 - beta1) * (g - m)
    v = v * beta2 + (1 - beta2) * g * g
    bc1, bc2 = 1 - beta1 ** step, 1 - beta2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    state['exp_avg'], state['exp_avg_sq'] = m, v
    return p + (m / denom) * (-(lr / bc1))
