"""Timestep respacing: host-side mirror of `improved_diffusion/respace.py`.

`space_timesteps` is integer arithmetic and must be bit-exact (pinned by
tests/golden/space_timesteps.json); `SpacedDiffusion` rebuilds the betas of the
retained steps in float64 (respace.py:68-82) and hands the timestep map to the
engine, which applies `_WrappedModel`'s gather + 1000/N rescale on device
(respace.py:111-119) instead of re-uploading the map every step.
"""
import numpy as np
import torch as th

from .gaussian_diffusion import GaussianDiffusion


def space_timesteps(num_timesteps, section_counts):
    """respace.py:7-58.  'ddimN' -> the first integer stride giving exactly N steps;
    'a,b,c' / [a,b,c] -> per-section fractional strides, rounded with round()."""
    if isinstance(section_counts, str):
        if section_counts.startswith("ddim"):
            desired_count = int(section_counts[len("ddim"):])
            for stride in range(1, num_timesteps):
                steps = range(0, num_timesteps, stride)
                if len(steps) == desired_count:
                    return set(steps)
            raise ValueError(f"cannot create exactly {num_timesteps} steps with an integer stride")
        section_counts = [int(x) for x in section_counts.split(",")]
    size_per, extra = divmod(num_timesteps, len(section_counts))
    taken, start = set(), 0
    for i, count in enumerate(section_counts):
        size = size_per + (1 if i < extra else 0)
        if size < count:
            raise ValueError(f"cannot divide section of {size} steps into {count}")
        stride = 1 if count <= 1 else (size - 1) / (count - 1)
        taken.update(start + round(k_stride) for k_stride in _walk(stride, count))
        start += size
    return taken


def logsnr_timesteps(betas, num_steps):
    """This project's extension (the reference has no such respacing; `timestep_respacing="logsnrN"` of create_gaussian_diffusion):
    exactly `num_steps` distinct indices of the base schedule, 0 and n - 1 among them, as uniform as the grid allows in
    lambda_i = log(acp_i / (1 - acp_i)) / 2 -- the spacing dpmpp_2m_sample is meant for: its extrapolation weights stay
    near 1/2, where steps uniform in t let them grow past 1 at the clean end.  float64 throughout: the targets
    linspace(lambda_0, lambda_{n-1}, num_steps), the nearest index of each (first minimum), then one pass upwards and one
    downwards that make the list strictly increasing inside 0..n - 1."""
    acp = np.cumprod(1.0 - np.asarray(betas, dtype=np.float64), axis=0)
    n = int(acp.shape[0])
    if not 2 <= num_steps <= n:
        raise ValueError(f"cannot pick {num_steps} logSNR-uniform steps from a schedule of {n}: 2 <= N <= {n}")
    lam = 0.5 * np.log(acp / (1.0 - acp))
    idx = [int(np.argmin(np.abs(lam - target))) for target in np.linspace(lam[0], lam[-1], num_steps)]
    for k in range(1, num_steps):
        idx[k] = max(idx[k], idx[k - 1] + 1)
    idx[-1] = min(idx[-1], n - 1)
    for k in range(num_steps - 2, -1, -1):
        idx[k] = min(idx[k], idx[k + 1] - 1)
    return idx


def repaint_schedule(t_start, jump_length, n_resample):
    """This project's extension: the walk of RePaint (Lugmayr et al. 2022, algorithm 1 with jumps) over respaced indices, as a list of
    ("step", t) -- one reverse step at index t, x_t -> x_{t-1} -- and ("jump", t) -- one forward step x_{t-1} -> x_t.  From t_start down
    to 0; every jump_length steps below t_start the chain goes jump_length steps back up and comes down again, until each such level
    has been left n_resample times.  n_resample == 1 is the plain descent; no jump passes t_start.  Steps in all:
    t_start + 1 + (n_resample - 1) * jump_length * (t_start // jump_length)."""
    if int(jump_length) != jump_length or jump_length < 1:
        raise ValueError(f"jump_length={jump_length!r}: an integer >= 1")
    if int(n_resample) != n_resample or n_resample < 1:
        raise ValueError(f"n_resample={n_resample!r}: an integer >= 1")
    if int(t_start) != t_start or t_start < 0:
        raise ValueError(f"t_start={t_start!r}: a respaced index >= 0")
    ops, done, level = [], {}, int(t_start)
    while level >= 0:
        ops.append(("step", level))
        level -= 1
        if level >= 0 and (t_start - level) % jump_length == 0 and done.get(level, 0) < n_resample - 1:
            done[level] = done.get(level, 0) + 1
            for _ in range(int(jump_length)):
                level += 1
                ops.append(("jump", level))
    return ops


def _walk(stride, count):
    pos = 0.0                      # accumulated, not k*stride: the reference's float drift is part of the contract
    for _ in range(count):
        yield pos
        pos += stride


class SpacedDiffusion(GaussianDiffusion):
    """respace.py:61-100."""

    def __init__(self, use_timesteps, **kwargs):
        self.use_timesteps = set(use_timesteps)
        self.timestep_map = []
        self.original_num_steps = len(kwargs["betas"])
        base_acp = np.cumprod(1.0 - np.array(kwargs["betas"], dtype=np.float64), axis=0)
        last, new_betas = 1.0, []
        for i, acp in enumerate(base_acp):
            if i in self.use_timesteps:
                new_betas.append(1 - acp / last)
                last = acp
                self.timestep_map.append(i)
        kwargs["betas"] = np.array(new_betas)
        super().__init__(**kwargs)

    def _timestep_map_and_scale(self):
        scale = 1000.0 / self.original_num_steps if self.rescale_timesteps else 1.0
        return self.timestep_map, scale

    def _wrap_model(self, model):
        if isinstance(model, _WrappedModel):
            return model
        return _WrappedModel(model, self.timestep_map, self.rescale_timesteps, self.original_num_steps)

    def _scale_timesteps(self, t):
        return t                   # scaling is done by the wrapped model (respace.py:98-100)


class _WrappedModel:
    """respace.py:103-119: index -> original step (-> 0..1000 scale), then the network."""

    def __init__(self, model, timestep_map, rescale_timesteps, original_num_steps):
        self.model = model
        self.timestep_map = timestep_map
        self.rescale_timesteps = rescale_timesteps
        self.original_num_steps = original_num_steps

    def __call__(self, x, timesteps, **kwargs):
        map_tensor = th.tensor(self.timestep_map, device=timesteps.device, dtype=timesteps.dtype)
        new_ts = map_tensor[timesteps]
        if self.rescale_timesteps:
            new_ts = new_ts.float() * (1000.0 / self.original_num_steps)
        return self.model(x, timesteps=new_ts, **kwargs)
