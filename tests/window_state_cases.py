"""The engine state a captured window graph depends on, entry by entry (host only: no engine, no torch) -- shared by
tests/test_window_state_cpu.py, which holds the list against _lib.SIGNATURES, and tests/test_gpu_window_state.py, which runs every row.

csrc/engine.hip, above drop_window_graphs(): "Captured window graphs bake addresses ... and values ... into their kernel arguments:
whatever replaces one of those drops every graph first."  Every entry that changes engine state keeps that in one of four ways (the
fourth in two forms), and a row says which -- read from the entry's code (`cite` names the place), not from what a run gives:

  KEYED         the state is a field of WinKey (or decides one): the entry itself touches no graph; the next vd_window_begin captures one
                more graph, and with the old value back it finds the old graph and gives the old bits.
  DROPS         the entry replaces an address or a value the graphs hold: vd_window_graphs() is 0 at once, a window in flight is lost
                (vd_window_run refuses with "window graphs invalidated"; vd_window_generation does not move, so it is the engine's refusal
                and not the executor's _gen check that stops the run), and the next begin captures again.
  CONTENT       the state lives in a buffer whose address never changes and which the graph re-reads: the graph count stays, the next
                window replays the same graph on the new content.
  REFUSED       vd_window_begin refuses by name while the state is set; the captured graphs are not touched.
  NOT_CAPTURED  no captured launch reads the state: graph count and generation stay, and the window in flight goes on to the bits it
                would have had.

A recipe is what the GPU file does for the row on the tiny model (T = 6, 32 x 32, 32 channels, ddim10):
  options              before / after: values of step_matrix_cases' axes (the scopes of tests/step_compose.py call the setter); both
                       windows run at one batch size -- 4 where either side has particles, else 2 -- since B is a field of the key too
  restoration_content  the row's restoration with other content of the same shape (`vary`)
  reload               load_state_dict of a second set of weights
  call                 `apply` (then `restore`) name functions of the GPU file; `refusal`: what vd_window_begin says in between
  growth_eager         an eager step at a larger batch behind a window at a smaller one
  growth_begin         a window at B = 2, then the same window at B = 4, under `options`, `sampler`, `observed_frames`: the begin at the
                       larger batch is the growth event (the workspace and the step counters are grown to B = 4 beforehand)
"""
import collections

KEYED, DROPS, CONTENT, REFUSED, NOT_CAPTURED = "KEYED", "DROPS", "CONTENT", "REFUSED", "NOT_CAPTURED"
CLASSES = (KEYED, DROPS, CONTENT, REFUSED, NOT_CAPTURED)
RECIPES = ("options", "restoration_content", "reload", "call", "growth_eager", "growth_begin")

Row = collections.namedtuple("Row", "name cls cite recipe")

# what a symbol of _lib.SIGNATURES must look like to need a row ...
STATE_PREFIXES = ("vd_set_", "vd_enable")
STATE_NAMES = ("vd_load_weight", "vd_load_weight_bwd", "vd_mark_weights_loaded")
# ... and the read-only getters of that state: they need none.  Stated by name, so that a symbol `vd_X` beside a `vd_set_X` is known to
# be the getter and not a second setter (tests/test_window_state_cpu.py holds the two lists against each other)
READ_ONLY_GETTERS = (
    "vd_weights_bytes", "vd_weights_missing", "vd_weights_layout_id", "vd_bwd_weights_bytes", "vd_window_generation", "vd_window_graphs",
    "vd_window_prefix_frames", "vd_window_suffix_frames", "vd_cfg_scale", "vd_guidance_rescale", "vd_dynamic_threshold", "vd_freeu",
    "vd_freeu_stages", "vd_known_region", "vd_measurement", "vd_blur_kernel", "vd_particle_blur", "vd_linear_operator",
    "vd_linear_measurement", "vd_particle_linear", "vd_particles", "vd_attn_blocks", "vd_attn_block_info")


def is_state_changing(symbol):
    return symbol.startswith(STATE_PREFIXES) or symbol in STATE_NAMES


def _options(before, after):
    return dict(kind="options", before=before, after=after)


def _call(apply, restore=None, refusal=None):
    return dict(kind="call", apply=apply, restore=restore, refusal=refusal)


def _growth(sampler="p_sample", observed_frames="x_0", **options):
    return dict(kind="growth_begin", sampler=sampler, observed_frames=observed_frames, options=options)


ROWS = [
    # ---- weights
    Row("vd_set_weight_storage", DROPS, "vd_set_weight_storage: another buffer than the bound one drops the graphs (W() addresses are kernel arguments)",
        _call("move_weight_storage")),
    Row("vd_set_weight_storage_host", DROPS, "vd_set_weight_storage_host: drops like vd_set_weight_storage; check_ready then refuses every compute entry",
        _call("host_weight_storage", restore="device_weight_storage", refusal="the packed image must live in device memory")),
    Row("vd_load_weight", CONTENT, "vd_load_weight: e->put into e->wbuf + p.off, behind a device drain; the address stays", dict(kind="reload")),
    Row("vd_mark_weights_loaded", NOT_CAPTURED, "vd_mark_weights_loaded: Param::loaded is host state, read by check_ready alone", _call("mark_weights_loaded")),
    Row("vd_set_bwd_weight_storage", NOT_CAPTURED, "check_diff / backward(): wbuf_bwd is read by the differentiated passes, which no window graph holds",
        _call("set_bwd_weight_storage")),
    Row("vd_load_weight_bwd", NOT_CAPTURED, "vd_load_weight_bwd: writes e->wbuf_bwd + p.off_bwd (see vd_set_bwd_weight_storage)", _call("load_weight_bwd")),
    # ---- tables
    Row("vd_set_freqs", DROPS, "vd_set_freqs: frees d_freq_time / d_freq_frame, which every captured forward reads", _call("reupload_freqs")),
    Row("vd_set_schedule", DROPS, "vd_set_schedule: 'the tables' addresses, num_timesteps and rescale are kernel arguments of every captured window graph'",
        _call("set_schedule", restore="rebind")),
    Row("vd_set_multistep_weights", DROPS, "vd_set_multistep_weights: 'Captured sampler-3 graphs bake the row's address in: they are dropped when it moves'",
        _call("set_multistep_weights")),
    Row("vd_set_unipc_rows", DROPS, "vd_set_unipc_rows: 'Captured sampler-5 graphs bake the table's address in: they are dropped when it moves'",
        _call("set_unipc_rows")),
    Row("vd_set_jump_rows", NOT_CAPTURED, "vd_set_jump_rows: 'No captured graph reads them (vd_window_jump launches plainly): nothing is dropped'",
        _call("set_jump_rows")),
    Row("vd_set_model_mean_type", DROPS, "vd_set_model_mean_type: 'Captured window graphs bake it in: they are dropped on a change'",
        _call("flip_mean_type", restore="restore_mean_type")),
    # ---- the window switches: read by vd_window_begin alone, where WinKey::flags carries them (with nothing observed they change no key;
    # under the prefix cache the bits may be the plain window's: not a KEYED row, whose bits must differ)
    Row("vd_set_window_prefix_cache", NOT_CAPTURED, "vd_set_window_prefix_cache: sets prefix_cache_on, read at the next vd_window_begin (key.flags)",
        _call("toggle_prefix_cache", restore="window_switches_off")),
    Row("vd_set_window_suffix_skip", NOT_CAPTURED, "vd_set_window_suffix_skip: sets suffix_skip_on, read at the next vd_window_begin (key.flags)",
        _call("toggle_suffix_skip", restore="window_switches_off")),
    # ---- options in the key
    Row("vd_set_cfg_scale", KEYED, "WinKey::cfg_w", _options(dict(guidance="off"), dict(guidance="w2"))),
    Row("vd_set_guidance_rescale", KEYED, "WinKey::guid_phi (acts with cfg_w != 1)", _options(dict(guidance="w2"), dict(guidance="w2_phi0.7"))),
    Row("vd_set_dynamic_threshold", KEYED, "WinKey::dyn_p", _options(dict(guidance="off"), dict(guidance="p0.9"))),
    Row("vd_set_freeu", KEYED, "WinKey::fu_b, fu_s, fu_on, fu_adaptive", _options(dict(freeu="off"), dict(freeu="on"))),
    Row("vd_set_known_region", KEYED, "WinKey::known_src, known_mask", _options(dict(restoration="none"), dict(restoration="known"))),
    Row("vd_set_measurement", KEYED, "WinKey::meas_y, meas_scale, meas_gray", _options(dict(restoration="none"), dict(restoration="meas_s2_colour"))),
    Row("vd_set_linear_measurement", KEYED, "WinKey::lin_y, lin_Mh, lin_Mw", _options(dict(restoration="none"), dict(restoration="linear"))),
    Row("vd_set_particles", KEYED, "WinKey::part_y, part_K, part_scale, part_gray, part_lambda, part_tau, part_sigma",
        _options(dict(restoration="none"), dict(restoration="part_cell4"))),
    Row("vd_set_particle_blur", KEYED, "WinKey::part_blur_k", _options(dict(restoration="part_cell4"), dict(restoration="part_blur5"))),
    Row("vd_set_particle_linear", KEYED, "WinKey::part_lin_Mh, part_lin_Mw", _options(dict(restoration="part_cell4"), dict(restoration="part_linear"))),
    # ---- engine-owned buffers at fixed addresses (another k, another (Mh, Mw) is KEYED through part_blur_k, lin_Mh / lin_Mw)
    Row("vd_set_blur_kernel", CONTENT, "vd_set_blur_kernel: d_blur_taps is allocated once, written behind a device drain",
        dict(kind="restoration_content", restoration="part_blur5", vary="taps")),
    Row("vd_set_linear_operator", CONTENT, "vd_set_linear_operator: d_lin_mats is allocated once, written behind a device drain",
        dict(kind="restoration_content", restoration="linear", vary="matrices")),
    # ---- refused
    Row("vd_set_attn_capture", REFUSED, "vd_window_begin: 'a window graph together with return_attn_weights (vd_set_attn_capture) is not served'",
        _call("arm_attn_capture", restore="clear_attn_capture", refusal="return_attn_weights (vd_set_attn_capture)")),
    # ---- growth: every grow(..., held_by_graphs = true) drops the graphs before the buffer moves
    Row("grow:workspace", DROPS, "grow_ws -> grow(ws, ws_cap, ..., true)", dict(kind="growth_eager")),
    Row("grow:d_win_hist", DROPS, "window_buffers: grow(d_win_hist, ..., true)", _growth(sampler="dpmpp_2m")),
    Row("grow:d_win_ubase+d_win_ud2", DROPS, "window_buffers: grow(d_win_ubase, ..., true), grow(d_win_ud2, ..., true)", _growth(sampler="unipc")),
    Row("grow:d_win_xtm1", DROPS, "window_buffers: obs_mode == 2 -> grow(d_win_xtm1, ..., true)", _growth(observed_frames="x_t_minus_1")),
    Row("grow:d_cfg_zero", DROPS, "cfg_zero_mask: grow(d_cfg_zero, ..., true)", _growth(guidance="w2")),
    Row("grow:d_fu", DROPS, "freeu_workspace: grow(d_fu, ..., true)", _growth(freeu="on")),
    Row("grow:particles", DROPS, "particle_state_reset / ensure_particle_ws: grow(d_part_*, ..., true)", _growth(restoration="part_cell4")),
]
GROWTH_PREFIX = "grow:"


def entry_rows():
    """The rows of C entry points (the growth events are pseudo-entries)."""
    return [r for r in ROWS if not r.name.startswith(GROWTH_PREFIX)]


def row_id(row):
    return row.name
