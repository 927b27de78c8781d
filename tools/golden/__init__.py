"""The golden fixtures of tests/golden/, minted from the IMPORTED reference on CPU/fp32 with the closed-form weights of
`video-diffusion_amd/weights_init.py`.  The reference has no tests or fixtures of its own, so parity is pinned by outputs
of the reference itself; it never travels: only the data written to tests/golden/ is committed.

    python -m tools.golden list | write [NAME ...] [--out DIR] | check [NAME ...] | probe      [--reference DIR]

Importing this package does not touch the reference: the producers load it when they run (`_reference.load()`).
Every producer takes the output directory, returns the paths it wrote, and gives the same output whether it runs alone
or after any other producer: inputs come from explicit generators, and a producer that lets the reference draw from
torch's global generator (loops, nll*, full_sampler) seeds it right before the call."""
from . import configs, full_size, guidance, jobs, long_window, loops_nll, optimal_schedule, room_seq, schedules, steps

# fixture file -> (producer, rough CPU seconds of the producer on 8 threads, needs a full-size model?)
MANIFEST = {
    "space_timesteps.json": (schedules.space_timesteps, 1, False),
    "schedule_linear1000_ddim250.json": (schedules.schedules, 1, False),
    "schedule_linear1000_full.json": (schedules.schedules, 1, False),
    "schedule_linear1000_ddim50.json": (schedules.schedules, 1, False),
    "schedule_cosine1000_ddim100.json": (schedules.schedules, 1, False),
    "schedule_linear1000_ddim5_small.json": (schedules.schedules, 1, False),
    "schedulers.json": (schedules.schedulers, 1, False),
    "schedulers_more.json": (schedules.schedulers_more, 1, False),
    "schedulers_adaptive.json": (schedules.schedulers_adaptive, 20, False),
    "param_specs.json": (schedules.param_specs, 5, False),
    "unet_tiny.npz": (steps.unet_tiny, 2, False),
    "unet_tiny_table.npz": (steps.unet_tiny_table, 1, False),
    "unet_tiny_frameenc.npz": (steps.unet_tiny_frameenc, 1, False),
    "unet_tiny_noss.npz": (steps.unet_tiny_noss, 1, False),
    "blocks_tiny.npz": (steps.blocks, 1, False),
    "psample_tiny.npz": (steps.psample, 2, False),
    "window_tiny.npz": (steps.window, 1, False),
    "denoised_fn_tiny.npz": (steps.denoised, 3, False),
    "xstart_tiny.npz": (steps.xstart, 4, False),
    "attn_tiny.npz": (steps.attn, 1, False),
    "attn_denoised_tiny.npz": (steps.attn_denoised, 1, False),
    "variants_tiny.npz": (steps.variants, 3, False),
    "loops_tiny.npz": (loops_nll.loops, 5, False),
    "ddim_reverse_tiny.npz": (loops_nll.ddim_reverse, 4, False),
    "nll_tiny.npz": (loops_nll.nll, 3, False),
    "nll_xstart_tiny.npz": (loops_nll.nll_xstart, 2, False),
    "grad_tiny.npz": (guidance.grad, 5, False),
    "unet_full64.npz": (full_size.full, 30, True),
    "unet_full128.npz": (full_size.full, 30, True),
    "full_size_reference_vs_oracle.json": (full_size.full, 30, True),
    "unet_full64_b8.npz": (full_size.b8, 30, True),
    "unet_tiny_long.npz": (long_window.unet_tiny_long, 4, False),
    "full_sampler_tiny.npz": (jobs.full_sampler, 5, False),
    "eval_paths.json": (jobs.eval_paths, 1, False),
    "script_imports.json": (jobs.script_imports, 1, False),
    "optimal_schedule_search.json": (optimal_schedule.search, 3, False),
    "room_seq_acc.json": (room_seq.room_seq, 1, False),
    "unet_configs.npz": (configs.unet_configs, 30, False),
}

# JSON keys that hold wall-clock seconds: `check` does not compare them, and `write` leaves an existing file alone when
# nothing else in it changed
SKIPPED_KEYS = {"full_size_reference_vs_oracle.json": full_size.TIMING_KEYS}
