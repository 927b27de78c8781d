"""The option matrix of one denoise step (host only: no engine, no torch): the axes, what each combination is -- served, refused by name
or documented as not honoured -- at each of the three entries, and the rows the GPU file runs.

`status` is written from the docstrings of gaussian_diffusion.py (the *_scope methods, the step methods), executor.py
(WindowExecutor.begin) and include/vd_amd.h, not by calling the engine.  What the docstrings do not state is the ORDER in which two
refusals that both apply are checked; that order is read from the code (begin()'s host checks stand in front of vd_window_begin's) and
is the order of the rules below.

A refusal's fragment names both parties.  Where the message is one literal of the source the fragment is that string; where the message
is formatted from a sampler's or a scope's name (gaussian_diffusion._refuse, _check_steered, executor._steering) it is the tuple of
the message's verbatim pieces, which the message holds in that order (`fragment_in`)."""
import collections
import itertools

AXES = collections.OrderedDict([
    ("sampler", ("p_sample", "ddim_eta0.5", "ddim_eta0", "ddim_reverse", "dpmpp_2m", "dpmpp_2m_sde", "unipc")),
    ("model", ("eps", "xstart")),
    ("guidance", ("off", "w2", "w2_phi0.7", "p0.9", "w2_phi0.7_p0.9")),
    ("freeu", ("off", "on", "adaptive")),
    ("restoration", ("none", "meas_s2_colour", "meas_s1_gray", "linear", "known", "part_cell4", "part_blur5", "part_linear")),
    ("switch", ("none", "prefix_cache", "suffix_skip")),
])
Case = collections.namedtuple("Case", list(AXES))
ENTRIES = ("step", "p_mean_variance", "window")

# axis value -> what the GPU file hands the entries
SAMPLER = {"p_sample": ("p_sample", 0.0), "ddim_eta0.5": ("ddim", 0.5), "ddim_eta0": ("ddim", 0.0), "ddim_reverse": ("ddim_reverse", 0.0),
           "dpmpp_2m": ("dpmpp_2m", 0.0), "dpmpp_2m_sde": ("dpmpp_2m_sde", 0.0), "unipc": ("unipc", 0.0)}
GUIDANCE = {"off": (1.0, 0.0, None), "w2": (2.0, 0.0, None), "w2_phi0.7": (2.0, 0.7, None), "p0.9": (1.0, 0.0, 0.9),
            "w2_phi0.7_p0.9": (2.0, 0.7, 0.9)}                                  # (cfg_scale, cfg_rescale, dynamic_threshold)
FREEU = {"off": None, "on": dict(b1=1.4, b2=1.2, s1=0.6, s2=0.8, adaptive=False), "adaptive": dict(b1=1.4, b2=1.2, s1=0.6, s2=0.8, adaptive=True)}
PARTICLES = 2                                                                    # K; the batch is 4 where particles are on, else 2

STEP_NAME = {"p_sample": "p_sample", "ddim": "ddim_sample", "ddim_reverse": "ddim_reverse_sample", "dpmpp_2m": "dpmpp_2m_sample",
             "dpmpp_2m_sde": "dpmpp_2m_sde_sample", "unipc": "unipc_sample"}
SCOPE = {"meas_s2_colour": "measurement", "meas_s1_gray": "measurement", "linear": "linear_measurement", "known": "known_region",
         "part_cell4": "steering", "part_blur5": "steering", "part_linear": "steering"}
ENGINE_NAME = {"measurement": "a measurement (vd_set_measurement)", "linear_measurement": "a linear measurement (vd_set_linear_measurement)"}
SWITCH_NAME = {"prefix_cache": "the window prefix cache (vd_set_window_prefix_cache)", "suffix_skip": "the window suffix skip (vd_set_window_suffix_skip)"}


def walks_up(case):
    return SAMPLER[case.sampler][0] == "ddim_reverse"


def draws_noise(case):
    """The step draws noise (steering_scope: 'ddim_sample at eta = 0, dpmpp_2m_sample, unipc_sample, ddim_reverse_sample ... draw no noise')."""
    name, eta = SAMPLER[case.sampler]
    return name in ("p_sample", "dpmpp_2m_sde") or (name == "ddim" and eta > 0.0)


def particles(case):
    return SCOPE.get(case.restoration) == "steering"


def batch(case):
    return 2 * PARTICLES if particles(case) else 2


def fragment_in(fragment, message):
    """The message holds the fragment: the string, or the tuple's pieces in their order."""
    pos = 0
    for piece in ((fragment,) if isinstance(fragment, str) else fragment):
        k = message.find(piece, pos)
        if k < 0:
            return False
        pos = k + len(piece)
    return True


def _no_noise(case, head, tail):
    name, eta = SAMPLER[case.sampler]
    return ("refused", (*head, *((" at eta = 0",) if name == "ddim" else ()), tail))


def _status_step(case):
    """A step method called inside the nested scopes."""
    name, _ = SAMPLER[case.sampler]
    scope = SCOPE.get(case.restoration)
    if scope is None:
        return "served"
    if name == "ddim_reverse":                                                   # every scope's docstring: 'Refused inside ...: ddim_reverse_sample'
        return ("refused", (STEP_NAME[name], scope, "_scope is not served"))
    if scope == "steering" and not draws_noise(case):                            # steering_scope: they draw no noise, duplicates would never separate
        return _no_noise(case, (STEP_NAME[name],), " inside steering_scope is not served")
    if scope == "known_region" and name == "unipc":                              # known_region_scope: the corrector rebuilds the state from its own
        return ("refused", (STEP_NAME[name], scope, "_scope is not served"))
    return "served"


def _status_pmv(case):
    """p_mean_variance inside the same scopes.  It is no sampler's: the row's sampler is not read (a measurement under it is served
    whatever step the caller makes next).  known_region_scope: 'Not honoured by model(...) itself, p_mean_variance'; steering_scope the
    same -- both act behind the sampler pass, which p_mean_variance does not run."""
    return "ignored" if SCOPE.get(case.restoration) in ("known_region", "steering") else "served"


def _status_window(case):
    """WindowExecutor(prefix_cache=, suffix_skip=).begin(..., cfg_scale=w) inside the FreeU, guidance and restoration scopes."""
    name, _ = SAMPLER[case.sampler]
    w, _, p = GUIDANCE[case.guidance]
    scope, sw = SCOPE.get(case.restoration), case.switch
    cut = sw != "none"
    if w != 1.0 and cut:                                                         # begin: 'cfg_scale ... Not served together with prefix_cache or suffix_skip'
        return ("refused", f"{sw} together with cfg_scale != 1")
    if scope == "steering":                                                      # begin: 'Refused by name too: a sampler that draws no noise ..., prefix_cache, suffix_skip'
        if not draws_noise(case):
            return _no_noise(case, ("sampler=", f"'{name}'"), " together with particles is not served")
        if cut:
            return ("refused", (sw, " together with particles is not served"))
    if scope == "known_region":                                                  # begin: 'Not served with 'ddim_reverse', prefix_cache or suffix_skip'; unipc: 'a known region is refused by name'
        if cut:
            return ("refused", (sw, " together with a known region"))
        if name in ("ddim_reverse", "unipc"):
            return ("refused", (f"sampler='{name}'", " together with a known region"))
    if cut and p is not None:                                                    # guidance_scope: 'Either option is refused together with ... prefix_cache or suffix_skip'
        return ("refused", (sw, " together with dynamic_threshold"))
    if cut and FREEU[case.freeu] is not None:                                    # freeu_scope: 'Refused ... a WindowExecutor with prefix_cache or suffix_skip'
        return ("refused", (sw, " together with FreeU (freeu_scope)"))
    if scope in ENGINE_NAME:                                                     # begin: 'The engine refuses it by name with 'ddim_reverse', prefix_cache, suffix_skip'
        if name == "ddim_reverse":
            return ("refused", (STEP_NAME[name], f" together with {ENGINE_NAME[scope]} is not served"))
        if cut:
            return ("refused", f"{ENGINE_NAME[scope]} together with {SWITCH_NAME[sw]} is not served")
    return "served"


def status(case, entry):
    """'served', ('refused', fragment) or 'ignored' for `case` at `entry` ('step', 'p_mean_variance' or 'window')."""
    return {"step": _status_step, "p_mean_variance": _status_pmv, "window": _status_window}[entry](case)


def all_pairs():
    """Every pair of values from two different axes, as ((axis, value), (axis, value)) with the axes in AXES' order."""
    names = list(AXES)
    return [((a, va), (b, vb)) for a, b in itertools.combinations(names, 2) for va in AXES[a] for vb in AXES[b]]


def pairs_of(case):
    d = case._asdict()
    return {((a, d[a]), (b, d[b])) for a, b in itertools.combinations(list(AXES), 2)}


def pairwise_rows(seed=0):
    """A deterministic greedy all-pairs covering set over the six axes: every row starts from the first pair still uncovered and takes,
    axis by axis, the value that covers the most uncovered pairs with the values already chosen (ties: the first value, counted from
    `seed` on, so another seed gives another set of about the same size)."""
    todo = all_pairs()
    left = set(todo)
    names = list(AXES)
    rows = []
    while left:
        first = next(pr for pr in todo if pr in left)
        chosen = dict(first)
        for axis in names:
            if axis in chosen:
                continue
            vals = AXES[axis]
            order = [vals[(k + seed + len(rows)) % len(vals)] for k in range(len(vals))]

            def gain(v):
                return sum(1 for other, ov in chosen.items()
                           if (((axis, v), (other, ov)) if names.index(axis) < names.index(other) else ((other, ov), (axis, v))) in left)
            chosen[axis] = max(order, key=gain)                                  # (max keeps the first of equal gains)
        row = Case(**chosen)
        rows.append(row)
        left -= pairs_of(row)
    return rows


def stack_rows():
    """The deep stack: FreeU adaptive + w=2 phi=0.7 p=0.9 on both models and every sampler that walks down, with a linear measurement, a
    known region and -- for the samplers that draw noise -- particles on the linear operator.  A combination that is refused (unipc with
    a known region) stays in, as a refusal."""
    rows = []
    for model in AXES["model"]:
        for sampler in AXES["sampler"]:
            probe = Case(sampler, model, "w2_phi0.7_p0.9", "adaptive", "none", "none")
            if walks_up(probe):
                continue
            for restoration in ("linear", "known") + (("part_linear",) if draws_noise(probe) else ()):
                rows.append(probe._replace(restoration=restoration))
    return rows


KEY_AXES = ("guidance", "freeu", "restoration")


def keying_partner(case, index):
    """The row a window of `case` is keyed against: it differs from `case` in exactly one value of the guidance, FreeU or restoration
    axis -- the axes tried in turn from `index` on, so that over the rows each of them is the differing one -- is served at the window
    entry and has `case`'s batch.  None where every such row is refused (a window switch is served with every other option off only)."""
    for j in range(len(KEY_AXES)):
        axis = KEY_AXES[(index + j) % len(KEY_AXES)]
        for v in AXES[axis]:
            other = case._replace(**{axis: v})
            if other != case and batch(other) == batch(case) and status(other, "window") == "served":
                return other
    return None


def case_id(case):
    return "-".join(case)


def plain_rows():
    """Every sampler with every option off, the models alternating -- the rows in which the window column serves each sampler whatever
    the pairwise set happened to pair it with -- and four samplers under each window switch."""
    rows = [Case(s, AXES["model"][k % 2], "off", "off", "none", "none") for k, s in enumerate(AXES["sampler"])]
    # a window switch is served with every other option off only, which no pairwise row is: a noise sampler, the one that walks up, and
    # the two kinds of carried state under each switch
    for sw in AXES["switch"][1:]:
        rows += [Case(s, m, "off", "off", "none", sw) for s, m in (("p_sample", "eps"), ("ddim_reverse", "xstart"), ("dpmpp_2m_sde", "eps"), ("unipc", "xstart"))]
    return rows


def matrix_rows():
    """The rows of the GPU file: the pairwise set, then the rows of the deep stack and the plain rows it does not hold already."""
    rows = pairwise_rows()
    for r in stack_rows() + plain_rows():
        if r not in rows:
            rows.append(r)
    return rows
