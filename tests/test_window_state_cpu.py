"""No GPU: tests/window_state_cases.py against the library's signature table, and the Python side of the window executor's protection
(executor.py: _check_gen) on a stand-in library.

The table says, entry by entry, how a change of engine state reaches the captured window graphs.  What keeps it complete is the first
test: every symbol of _lib.SIGNATURES that changes engine state by its name has exactly one row, so a setter added later without a
row -- without anyone having decided whether it is keyed, drops, rewrites content or is refused -- fails here."""
import contextlib
import ctypes
import re

import pytest
import torch

import step_matrix_cases as sm
import window_state_cases as ws
from video_diffusion_amd import _lib, executor
from video_diffusion_amd.script_util import create_gaussian_diffusion


def test_the_table_names_exactly_the_state_changing_symbols_of_the_signature_table():
    want = sorted(s for s in _lib.SIGNATURES if ws.is_state_changing(s))
    got = sorted(r.name for r in ws.entry_rows())
    assert got == want, (sorted(set(want) - set(got)), sorted(set(got) - set(want)))
    assert len(set(r.name for r in ws.ROWS)) == len(ws.ROWS)                      # one row per entry
    # the patterns are the ones a reader expects: every vd_set_*, the loaders, the storage setters, the attention capture
    for s in ("vd_set_freqs", "vd_set_weight_storage", "vd_set_weight_storage_host", "vd_set_bwd_weight_storage", "vd_set_attn_capture",
              "vd_load_weight", "vd_load_weight_bwd", "vd_mark_weights_loaded", "vd_set_window_prefix_cache", "vd_set_jump_rows"):
        assert ws.is_state_changing(s) and s in _lib.SIGNATURES, s
    # the getters: each exists, none is taken for a setter, and every `vd_X` that stands beside a `vd_set_X` is one of them
    for g in ws.READ_ONLY_GETTERS:
        assert g in _lib.SIGNATURES and not ws.is_state_changing(g), g
    for s in _lib.SIGNATURES:
        if s.startswith("vd_set_") and "vd_" + s[len("vd_set_"):] in _lib.SIGNATURES:
            assert "vd_" + s[len("vd_set_"):] in ws.READ_ONLY_GETTERS, s
    # the growth events the engine has: every buffer grown with held_by_graphs = true appears in a growth row's citation or recipe
    growth = [r for r in ws.ROWS if r.name.startswith(ws.GROWTH_PREFIX)]
    named = " ".join(r.name + " " + r.cite for r in growth)
    for buf in ("workspace", "d_win_hist", "d_win_ubase", "d_win_ud2", "d_win_xtm1", "d_cfg_zero", "d_fu", "d_part"):
        assert buf in named, buf


def test_a_setter_without_a_row_fails():
    """The first test's teeth: the table without one of its rows, and the signature table with one more setter."""
    want = sorted(s for s in _lib.SIGNATURES if ws.is_state_changing(s))
    short = [r for r in ws.entry_rows() if r.name != "vd_set_freqs"]
    assert sorted(r.name for r in short) != want
    assert ws.is_state_changing("vd_set_something_new") and ws.is_state_changing("vd_enable_something") and not ws.is_state_changing("vd_something_new")


def test_every_row_has_a_class_a_citation_and_a_recipe_the_gpu_file_knows():
    for r in ws.ROWS:
        assert r.cls in ws.CLASSES, r
        assert isinstance(r.cite, str) and len(r.cite) > 8, r
        k = r.recipe["kind"]
        assert k in ws.RECIPES, r
        if k == "options":
            assert r.cls == ws.KEYED
            for side in ("before", "after"):
                for axis, v in r.recipe[side].items():
                    assert v in sm.AXES[axis], (r.name, axis, v)
            assert r.recipe["before"] != r.recipe["after"]
            a, b = _case(r.recipe["before"]), _case({**r.recipe["before"], **r.recipe["after"]})
            assert sm.status(a, "window") == "served" and sm.status(b, "window") == "served", r.name
        elif k == "restoration_content":
            assert r.cls == ws.CONTENT and r.recipe["restoration"] in sm.AXES["restoration"] and r.recipe["vary"] in ("taps", "matrices")
        elif k == "reload":
            assert r.cls == ws.CONTENT
        elif k == "call":
            assert r.cls in (ws.DROPS, ws.NOT_CAPTURED, ws.REFUSED) and re.fullmatch(r"[a-z_]+", r.recipe["apply"])
            assert (r.cls == ws.REFUSED) <= (r.recipe["refusal"] is not None and r.recipe["restore"] is not None), r.name
        else:
            assert r.cls == ws.DROPS and r.name.startswith(ws.GROWTH_PREFIX)
            if k == "growth_begin":
                assert sm.status(_case(dict(r.recipe["options"], sampler=_axis_sampler(r.recipe["sampler"]))), "window") == "served", r.name
    # every class is met, and the keyed rows end in distinct keys (one executor could run them all)
    assert {r.cls for r in ws.ROWS} == set(ws.CLASSES)
    afters = [tuple(sorted({**r.recipe["before"], **r.recipe["after"]}.items())) for r in ws.ROWS if r.recipe["kind"] == "options"]
    assert len(set(afters)) == len(afters)


def _axis_sampler(name):
    return {"p_sample": "p_sample", "dpmpp_2m": "dpmpp_2m", "unipc": "unipc"}[name]


def _case(over):
    base = dict(sampler="p_sample", model="eps", guidance="off", freeu="off", restoration="none", switch="none")
    return sm.Case(**{**base, **over})


# ------------------------------------------------------------------------------------------------ the executor's Python side
class _Stream:
    cuda_stream = 4242

    def wait_stream(self, other):
        pass


class _Lib:
    """Stand-in library: a generation counter vd_window_begin bumps (as the engine does), a vd_window_run that can be told to refuse
    the way a dropped graph makes the engine refuse; every call is recorded."""

    def __init__(self):
        self.gen, self.lost, self.calls = 0, False, []

    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        res, argtypes = _lib.SIGNATURES[name]

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))
            self.calls.append(name)
            if name == "vd_window_generation":
                return self.gen
            if name == "vd_window_begin":
                self.gen += 1
                self.lost = False
            if name == "vd_window_run" and self.lost:
                return -1
            if name == "vd_last_error":
                return b"window graphs invalidated (workspace growth or a new schedule since vd_window_begin): begin the window again"
            return 0 if res is ctypes.c_int else (1.0 if name == "vd_cfg_scale" else 0.0)
        return call


class _Model:
    _handle = 17
    device = torch.device("cpu")
    image_size = 2

    def _pack_kwargs(self, x, kw):
        B, T = x.shape[:2]
        z = torch.zeros(B * T)
        return dict(obs_src=torch.zeros_like(x), obs_mask=z, latent_mask=z + 1, kinda_marg_mask=z, frame_indices=torch.zeros(B, T, dtype=torch.int64), obs_mode=0)


@pytest.fixture
def fake(monkeypatch):
    lib = _Lib()
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: _Stream())
    monkeypatch.setattr(torch.cuda, "stream", lambda s: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "Stream", lambda device=None: _Stream())
    diff = create_gaussian_diffusion(steps=1000, learn_sigma=False, noise_schedule="linear", timestep_respacing="ddim4")
    model = _Model()
    x = torch.zeros(2, 3, 3, 2, 2)
    return lib, model, diff, x


def test_executor_refuses_a_window_another_begin_has_replaced_and_runs_again_after_its_own_begin(fake):
    """executor.py, _check_gen: run / jump / particle_state compare the generation begin() read with the engine's.  A generation that
    moved (another executor's begin on the same engine) is refused in Python, in front of vd_window_run; the executor's own begin()
    reads the new generation and runs again."""
    lib, model, diff, x = fake
    a, b = executor.WindowExecutor(model, diff), executor.WindowExecutor(model, diff)
    a.begin(x, {}, seed=1)
    assert a._gen == lib.gen == 1 and a._left == diff.num_timesteps
    a.run(1)
    assert lib.calls.count("vd_window_run") == 1
    b.begin(x, {}, seed=2)                                                      # the engine's counters now belong to b
    assert lib.gen == 2 and a._gen == 1
    n_runs = lib.calls.count("vd_window_run")
    for what, call in (("run", lambda: a.run(1)), ("jump", lambda: a.jump(1))):
        with pytest.raises(RuntimeError, match=f"WindowExecutor.{what}: another window was begun"):
            call()
    assert lib.calls.count("vd_window_run") == n_runs and "vd_window_jump" not in lib.calls       # nothing reached the engine
    b.run(1)
    a.begin(x, {}, seed=1)                                                      # begin again: the window is a's
    assert a._gen == lib.gen == 3
    a.run(2)
    assert lib.calls.count("vd_window_run") == n_runs + 2 and a._left == diff.num_timesteps - 2
    with pytest.raises(RuntimeError, match="another window was begun"):
        b.run(1)


def test_executor_hands_on_the_engines_refusal_of_a_dropped_graph(fake):
    """A DROPS entry does not move the generation (vd_window_begin alone does): _check_gen passes, and it is vd_window_run's own
    refusal that reaches the caller, by name; begin() arms the window again."""
    lib, model, diff, x = fake
    ex = executor.WindowExecutor(model, diff)
    ex.begin(x, {}, seed=1)
    ex.run(1)
    lib.lost = True
    left = ex._left
    with pytest.raises(_lib.VdError, match="window graphs invalidated"):
        ex.run(1)
    assert ex._left == left                                                      # the refused run took no step off the window
    ex.begin(x, {}, seed=1)
    ex.run(1)
    assert ex._left == diff.num_timesteps - 1
