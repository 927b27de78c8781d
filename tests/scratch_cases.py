"""What tests/test_gpu_scratch_history.py runs (host only: no engine, no torch): one row per engine entry that launches work, the
entries that are not run and why, the engine's device buffers as scratch or state, and the rows of the step's option matrix that are
served again here.  tests/test_scratch_cases_cpu.py keeps the three tables complete against include/vd_amd.h and csrc/engine.hip.

The question the GPU file asks of every row: do the bits of the call depend on what the engine's scratch memory held when the call
began?  The yardstick is the same call on a freshly created engine; a row names the runner that makes the call (a function of the GPU
file, on inputs that depend on nothing but their seed) and what is compared: every tensor the runner returns, and the state named here."""
import collections
import os
import re

import step_matrix_cases as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vd_amd.h")
ENGINE = os.path.join(ROOT, "video-diffusion_amd", "csrc", "engine.hip")

# run: the GPU file's runner;  outputs: the tensors it returns, each compared to the bit;  state: what the entry leaves in the engine and
# is read back and compared too ('flags': vd_device_errors; 'particles': vd_particle_state; 'history': vd_window_history; 'window': the
# window tensor, the graph count and the generation);  diffws: the entry lays DiffWs's tail over the workspace (the differentiated
# passes), which decides what the larger call in front of it is in the history 'grown'
Row = collections.namedtuple("Row", "run outputs state diffws")


def _r(run, outputs, state=("flags",), diffws=False):
    return Row(run, tuple(outputs.split()), tuple(state), diffws)


STEP_OUT = "sample pred_xstart"
ENTRIES = collections.OrderedDict([
    ("vd_unet_forward", _r("forward", "eps")),
    # the six samplers: the served rows of the option matrix (STEP_ROWS below), through tests/step_compose.py: fused_step
    ("vd_p_sample", _r("step", STEP_OUT, ("flags", "particles"))),
    ("vd_ddim_sample", _r("step", STEP_OUT, ("flags", "particles"))),
    ("vd_ddim_reverse_sample", _r("step", STEP_OUT)),
    ("vd_dpmpp_2m_sample", _r("step", STEP_OUT)),
    ("vd_dpmpp_2m_sde_sample", _r("step", STEP_OUT, ("flags", "particles"))),
    ("vd_unipc_sample", _r("step", STEP_OUT + " base d1 d2")),
    # the network-free passes: no workspace of the engine, but its tables and its flags
    ("vd_posterior_update", _r("posterior_update", STEP_OUT)),
    ("vd_posterior_from_xstart", _r("from_xstart", STEP_OUT + " mean")),
    ("vd_ddim_reverse_from_xstart", _r("from_xstart", STEP_OUT)),
    ("vd_dpmpp_2m_from_xstart", _r("from_xstart", STEP_OUT)),
    ("vd_dpmpp_2m_sde_from_xstart", _r("from_xstart", STEP_OUT)),
    ("vd_unipc_from_xstart", _r("from_xstart", STEP_OUT + " base d1 d2")),
    ("vd_q_sample", _r("q_sample", "x_t")),
    ("vd_q_jump", _r("q_jump", "x_t")),
    ("vd_known_merge", _r("known_merge", "sample")),
    ("vd_measurement_project", _r("measurement_project", "x0")),
    ("vd_op_linear_project", _r("linear_project", "x0")),
    ("vd_p_mean_variance", _r("p_mean_variance", "mean pred_xstart eps")),
    # the NLL path and the observed-frame search
    ("vd_vb_terms", _r("vb_terms", "vb xstart_mse mse pred_xstart")),
    ("vd_prior_bpd", _r("prior_bpd", "bpd")),
    ("vd_score_windows", _r("score_windows", "mse mse_skip")),
    ("vd_op_eps_mse", _r("eps_mse", "mse")),
    # the differentiated passes
    ("vd_guided_step", _r("guided_step", "mean pred_xstart grad sample", diffws=True)),
    ("vd_op_guided_grad", _r("guided_grad", "deps dxd mean xstart")),
    ("vd_op_guided_final", _r("guided_final", "grad mean_out sample")),
    ("vd_dps_step", _r("dps_step", STEP_OUT + " grad residual_norm", diffws=True)),
    ("vd_op_dps_seed", _r("dps_seed", "deps dxd rho xstart")),
    ("vd_deblur_step", _r("deblur_step", STEP_OUT + " grad residual_norm", diffws=True)),
    ("vd_op_deblur_seed", _r("deblur_seed", "deps dxd rho xstart")),
    ("vd_linear_dps_step", _r("linear_dps_step", STEP_OUT + " grad residual_norm", diffws=True)),
    ("vd_op_linear_dps_seed", _r("linear_dps_seed", "deps dxd rho xstart")),
    # (the two halves of one loss-guided step: one job of the GPU file makes both calls)
    ("vd_guide_begin", _r("loss_guidance", STEP_OUT + " grad grad_norm", diffws=True)),
    ("vd_guide_finish", _r("loss_guidance", STEP_OUT + " grad grad_norm", diffws=True)),
    ("vd_op_guide_seed", _r("guide_seed", "deps dxd")),
    ("vd_eps_vjp", _r("eps_vjp", "eps vjp", diffws=True)),
    ("vd_ode_nll_eval", _r("ode_nll_eval", "eps trace x_next", diffws=True)),
    ("vd_op_ode_heun", _r("ode_heun", "x_next")),
    ("vd_particle_apply", _r("particle_apply", STEP_OUT + " ancestors log_weights", ("flags", "particles"))),
    # the window executor: the rows of WINDOW_ROWS, the fill between begin and run and between two runs
    ("vd_window_begin", _r("window", "x", ("flags", "history", "window"))),
    ("vd_window_run", _r("window", "x", ("flags", "history", "window"))),
    ("vd_window_history", _r("window", "x", ("flags", "history", "window"))),
    ("vd_window_jump", _r("window_jump", "x", ("flags", "window"))),
])

_SETTER = "a setter: host state and uploads of tables the caller hands in; no stream, nothing computed on the device"
_QUERY = "a host-only query: reads the engine's host state, launches nothing"
_WEIGHTS = "weight storage and loading: packs on the host and copies into the caller's buffer; no kernel of the engine runs"
EXEMPT = collections.OrderedDict([
    ("vd_destroy", "frees the engine"),
    ("vd_param_count", _QUERY), ("vd_param_info", _QUERY), ("vd_weights_bytes", _QUERY), ("vd_weights_missing", _QUERY),
    ("vd_weights_layout_id", _QUERY), ("vd_pos_channels", _QUERY), ("vd_pos_resolution", _QUERY), ("vd_workspace_bytes", _QUERY),
    ("vd_window_generation", _QUERY), ("vd_window_graphs", _QUERY), ("vd_window_prefix_frames", _QUERY), ("vd_window_suffix_frames", _QUERY),
    ("vd_cfg_scale", _QUERY), ("vd_freeu", _QUERY), ("vd_freeu_stages", _QUERY), ("vd_guidance_rescale", _QUERY), ("vd_dynamic_threshold", _QUERY),
    ("vd_known_region", _QUERY), ("vd_measurement", _QUERY), ("vd_attn_blocks", _QUERY), ("vd_attn_block_info", _QUERY),
    ("vd_bwd_weights_bytes", _QUERY), ("vd_particles", _QUERY), ("vd_blur_kernel", _QUERY), ("vd_particle_blur", _QUERY),
    ("vd_linear_operator", _QUERY), ("vd_linear_measurement", _QUERY), ("vd_particle_linear", _QUERY),
    ("vd_set_weight_storage", _WEIGHTS), ("vd_set_weight_storage_host", _WEIGHTS), ("vd_load_weight", _WEIGHTS), ("vd_mark_weights_loaded", _WEIGHTS),
    ("vd_set_bwd_weight_storage", _WEIGHTS), ("vd_load_weight_bwd", _WEIGHTS),
    ("vd_set_freqs", _SETTER), ("vd_set_schedule", _SETTER), ("vd_set_model_mean_type", _SETTER), ("vd_set_multistep_weights", _SETTER),
    ("vd_set_unipc_rows", _SETTER), ("vd_set_window_prefix_cache", _SETTER), ("vd_set_window_suffix_skip", _SETTER), ("vd_set_cfg_scale", _SETTER),
    ("vd_set_freeu", _SETTER), ("vd_set_guidance_rescale", _SETTER), ("vd_set_dynamic_threshold", _SETTER), ("vd_set_known_region", _SETTER),
    ("vd_set_jump_rows", _SETTER), ("vd_set_measurement", _SETTER), ("vd_set_attn_capture", _SETTER), ("vd_set_particles", _SETTER),
    ("vd_particle_draws", _SETTER), ("vd_set_blur_kernel", _SETTER), ("vd_set_particle_blur", _SETTER), ("vd_set_linear_operator", _SETTER),
    ("vd_set_linear_measurement", _SETTER), ("vd_set_particle_linear", _SETTER),
    ("vd_particle_reset", "zeroes the particle state with blocking memsets; the rows of vd_particle_apply and of the steered steps read that state back"),
    ("vd_particle_state", "copies the particle state to the host: the read-back every row with state 'particles' goes through"),
    ("vd_device_errors", "reads and clears the sticky flags: the read-back of every row"),
    ("vd_scratch_fill", "the hook itself"),
    ("vd_guide_abort", "ends a held pass on the host; the held-pass test covers the endings"),
])

# The engine's device pointers (struct vd_engine in csrc/engine.hip, its nested structs included), as the comment above vd_scratch_fill
# classifies them: a buffer is scratch when no call reads it before that same call has written it
SCRATCH = ("ws", "d_fu", "d_lin_r", "d_part_scratch", "d_part_r", "d_part_partials", "d_part_x0", "d_part", "d_score_xt", "d_score_list")
STATE = ("d_freq_time", "d_freq_frame", "d_tab", "d_tmap", "d_w2m", "d_unipc", "d_jump", "d_hid", "d_out", "d_cfg_zero", "d_fu_trig",
         "d_blur_taps", "d_lin_mats", "d_part_sel", "d_part_logw", "d_part_rprev", "d_part_ess", "d_part_anc", "d_part_chosen",
         "d_part_counters", "d_err", "d_win_t", "d_win_rng", "d_win_hist", "d_win_ubase", "d_win_ud2", "d_win_xtm1", "d_lists")

# The evaluator handles: entry -> its fill
EVALUATORS = collections.OrderedDict([("vd_lpips_embed", "vd_lpips_scratch_fill"), ("vd_i3d_embed", "vd_i3d_scratch_fill"),
                                      ("vd_frame_metrics", "vd_frame_metrics_scratch_fill")])

FILLS = (0x00, 0x7F, 0xFF)              # in this order: a dependence shows as a difference on zeros before anything harsher runs
HISTORIES = ("filled", "grown", "leftovers")
SHAPE, LONG_SHAPE, GROWN_SHAPE = (2, 3), (1, 33), (3, 7)                         # (B, T)

SAMPLER_ENTRY = {"p_sample": "vd_p_sample", "ddim": "vd_ddim_sample", "ddim_reverse": "vd_ddim_reverse_sample", "dpmpp_2m": "vd_dpmpp_2m_sample",
                 "dpmpp_2m_sde": "vd_dpmpp_2m_sde_sample", "unipc": "vd_unipc_sample"}
DEEPEST = sm.Case("p_sample", "eps", "w2_phi0.7_p0.9", "adaptive", "part_linear", "none")       # stack_rows(): every option at once, particles included


def entry_of(case):
    return SAMPLER_ENTRY[sm.SAMPLER[case.sampler][0]]


def step_rows():
    """The served rows of the step entry that run again here: the deepest stack, then, greedily in matrix_rows()' order, every row
    that brings a value of an axis not seen yet (the window switches are no option of a step: WINDOW_ROWS)."""
    rows, seen = [DEEPEST], set()
    note = lambda r: {(a, getattr(r, a)) for a in sm.AXES if a != "switch"}      # noqa: E731
    seen |= note(DEEPEST)
    for r in sm.matrix_rows():
        if sm.status(r, "step") == "served" and note(r) - seen:
            rows.append(r._replace(switch="none"))
            seen |= note(r)
    return rows


def window_rows():
    """A plain window, the two switches, and one row each of cfg_scale, FreeU, the known region, a measurement and particles; with the
    samplers that carry history among them."""
    C = sm.Case
    return [C("p_sample", "eps", "off", "off", "none", "none"), C("dpmpp_2m_sde", "eps", "off", "off", "none", "prefix_cache"),
            C("unipc", "xstart", "off", "off", "none", "suffix_skip"), C("ddim_eta0.5", "eps", "w2", "off", "none", "none"),
            C("dpmpp_2m", "eps", "off", "adaptive", "none", "none"), C("p_sample", "eps", "off", "off", "known", "none"),
            C("unipc", "eps", "off", "off", "linear", "none"), C("p_sample", "eps", "off", "off", "part_blur5", "none")]


STEP_ROWS = step_rows()
WINDOW_ROWS = window_rows()


def option_cover(rows, windows):
    """What the two sets leave uncovered of the matrix's axes -> list of (axis, value); the deepest stack counts as a value of its own."""
    missing = []
    for axis, values in sm.AXES.items():
        have = {getattr(r, axis) for r in (windows if axis == "switch" else list(rows) + list(windows))}
        missing += [(axis, v) for v in values if v not in have]
    if not any(r in sm.stack_rows() and sm.particles(r) for r in rows):
        missing.append(("stack", "deepest"))
    missing += [("served", sm.case_id(r)) for r in rows if sm.status(r, "step") != "served"]
    missing += [("served", sm.case_id(r)) for r in windows if sm.status(r, "window") != "served"]
    return missing


# ------------------------------------------------------------------------------------------------ the sources, parsed
def _strip_comments(text):
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def header_entries(text):
    """include/vd_amd.h -> (entries whose first parameter is vd_engine* and that take a stream, the other vd_engine* entries)."""
    launch, other = [], []
    for name, args in re.findall(r"\b(vd_\w+)\s*\(([^;{)]*)\)\s*;", _strip_comments(text)):
        args = " ".join(args.split())
        if args.startswith("vd_engine*"):
            (launch if re.search(r"void\*\s*stream\b", args) else other).append(name)
    return launch, other


def entry_cover(launch, other, entries, exempt):
    """The mistakes of the two lists against the header -> list of strings (empty: complete)."""
    bad = [f"{n}: in ENTRIES and in EXEMPT" for n in entries if n in exempt]
    bad += [f"{n}: launches work (vd_engine*, a stream) and is no row of ENTRIES" for n in launch if n not in entries]
    bad += [f"{n}: in neither list" for n in other if n not in entries and n not in exempt]
    bad += [f"{n}: no vd_engine* entry of the header" for n in list(entries) + list(exempt) if n not in launch and n not in other]
    return bad


def _braces(text, start):
    """The text between the brace at or behind `start` and its partner."""
    i = text.index("{", start)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            return text[i + 1:j]
        j += 1


def engine_pointers(text):
    """csrc/engine.hip -> the names of the device pointers declared in struct vd_engine: `ws` and every pointer member d_*."""
    src = _strip_comments(text)
    body = _braces(src, src.index("struct vd_engine {"))
    names = re.findall(r"\*\s*(d_\w+|ws)\b\s*(?==|;|,)", body)
    return sorted(set(names))


def fill_body(text):
    src = _strip_comments(text)
    return _braces(src, src.index("int vd_scratch_fill("))


def buffer_cover(pointers, body, scratch, state):
    bad = [f"{n}: in SCRATCH and in STATE" for n in scratch if n in state]
    bad += [f"{n}: a device pointer of struct vd_engine in neither list" for n in pointers if n not in scratch and n not in state]
    bad += [f"{n}: listed, but no device pointer of struct vd_engine" for n in list(scratch) + list(state) if n not in pointers]
    named = lambda n: re.search(r"\b" + re.escape(n) + r"\b", body) is not None   # noqa: E731
    bad += [f"{n}: scratch that vd_scratch_fill does not fill" for n in scratch if not named(n)]
    bad += [f"{n}: state that vd_scratch_fill names" for n in state if named(n)]
    return bad
