"""Sampling of the sibling denoisers (SR3 / TESR / GDP) at their own schedule lengths (T = 1000, TESR 2000) through
fdsr_sample_stepwise (include/fdsr.h): the per-step inputs live on the device, a graph replays a chunk of steps, and
`continous=True` keeps only the frames the reference keeps instead of all T of them.  The rules are here; the sampling path that
follows them is fastdiffsr_amd.diffusion.GaussianDiffusion.p_sample_loop."""

# schedules longer than this go through the stepwise entry point; up to it the facades call fdsr_sample as before
STEPWISE_ABOVE = 50


def frame_every(T):
    """The reference's `sample_inter = (1 | (T // 10))` (ddpm_modules/diffusion.py:200 and its siblings)."""
    return 1 | (int(T) // 10)


def kept_steps(T):
    """The t whose x_t `continous=True` returns, in loop order (t descending): `t % sample_inter == 0`."""
    every = frame_every(T)
    return [t for t in reversed(range(int(T))) if t % every == 0]


def use_stepwise(T):
    return int(T) > STEPWISE_ABOVE


def release_buffers(facade):
    """Free the per-shape graph buffers a facade keeps for its long schedules (GaussianDiffusion._graph_buffers; the next graph call
    of a shape captures again)."""
    for k in [k_ for k_ in facade._gbuf if k_[0] == 'stepwise']:
        del facade._gbuf[k]
