"""No GPU: what the Python step path hands the engine, per sampler -- on a recording stand-in library, for every sampler of
gaussian_diffusion.SAMPLERS and for the fused step as well as the step through `denoised_fn`: the entry called, the number of its
arguments against _lib.SIGNATURES, every scalar and every pointer slot (which tensor, or NULL), where the global generators are drawn
from between the calls, and for every public loop on a 3-step schedule the sequence of entries with the `t` handed to each.  The
expected values are literals, recorded from the step path as it stood before the sampler table existed; the table, executor._sampler_id
and the job's --sampler choices are held against each other."""
import contextlib
import ctypes

import pytest
import torch

from video_diffusion_amd import _lib, executor, gaussian_diffusion, video_sample
from video_diffusion_amd.script_util import create_gaussian_diffusion

B, T, PER = 4, 3, 3 * 3 * 2 * 2                                                  # batch, frames, elements per item: all distinct from
OBS_MODE, ETA, PHILOX, COUNT = 2, 0.5, (7, 11), 5                                # ... the flags and from each other


class _Recorder:
    """The event stream of one case: engine calls (name, arguments by label), draws from torch's global generators, the callback."""

    def __init__(self):
        self.events, self.labels, self.drawn = [], {}, 0

    def label(self, **tensors):
        for name, v in tensors.items():
            self.labels[id(v)] = (name, v)                                       # (the tensor is kept alive: ids are not reused)
        return self

    def arg(self, a, argtype):
        if argtype is not ctypes.c_void_p:
            return repr(a)
        if a is None:
            return "N"
        if not torch.is_tensor(a):
            return str(a)                                                        # the stand-in model's handle and window pointers
        return self.labels.get(id(a), ("p",))[0]                                 # a tensor this test did not make: an output, a copy

    def t_of(self, args):
        for a in args:
            if torch.is_tensor(a) and a.dtype == torch.int64 and a.dim() == 1 and bool((a == a[0]).all()):
                return int(a[0])
        return None


class _FakeLib:
    """Stand-in for the library: the getters answer with the engine's defaults, every other symbol records its arguments."""

    def __init__(self, rec, full):
        self.rec, self.full, self.cfg = rec, full, 1.0

    def __getattr__(self, name):
        if name not in _lib.SIGNATURES:
            raise AttributeError(name)
        argtypes = _lib.SIGNATURES[name][1]

        def call(*args):
            assert len(args) == len(argtypes), (name, len(args), len(argtypes))  # (b): the C entry's own argument count
            if name == "vd_set_cfg_scale":
                self.cfg = args[1]
            if self.full:
                self.rec.events.append(f"{name}({' '.join(self.rec.arg(a, ty) for a, ty in zip(args, argtypes))})")
            else:
                t = self.rec.t_of(args)
                philox = [a for a, ty in zip(args, argtypes) if ty is ctypes.c_ulonglong]      # (seed, offset) where the entry has them
                self.rec.events.append(name + ("" if t is None else f"@{t}") + (f"+{philox[1]}" if len(philox) == 2 and philox[1] else ""))
            if _lib.SIGNATURES[name][0] is ctypes.c_int:
                return 0
            return {"vd_cfg_scale": self.cfg}.get(name, 0.0)
        return call


class _FakeModel:
    _handle = 17
    device = torch.device("cpu")

    def __init__(self, rec):
        self.rec = rec

    def _pack_kwargs(self, x, kw):
        return dict(obs_src=x, obs_mask=x, latent_mask=x, kinda_marg_mask=x, frame_indices=x, obs_mode=OBS_MODE)

    @staticmethod
    def _window_ptrs(x, kw):
        return ("w1", "w2", "w3", "w4", "w5", "w6")

    def check_device_errors(self):
        self.rec.events.append("check_device_errors")


def _rand(*shape, seed=0):
    return torch.empty(*shape).uniform_(generator=torch.Generator().manual_seed(seed))      # (not one of the recorded draws)


@contextlib.contextmanager
def _recording(monkeypatch, respacing="ddim3", full=True):
    """(rec, model, diffusion, inputs) on the stand-in library; _lib.ptr hands the tensor itself on, so the recorder sees which one it
    is.  inputs: x, t, noise, prev_xstart and a unipc state, each known to the recorder by name."""
    rec = _Recorder()
    x, noise, prev, s0, s1, s2 = _rand(6, B, T, 3, 2, 2).unbind(0)
    x, noise, prev, s0, s1, s2 = (v.contiguous() for v in (x, noise, prev, s0, s1, s2))
    t = torch.tensor([1] * B)
    rec.label(x=x, t=t, noise=noise, prev=prev, s0=s0, s1=s1, s2=s2)
    with monkeypatch.context() as m:
        fake = _FakeLib(rec, full)
        m.setattr(_lib, "lib", lambda: fake)
        m.setattr(_lib, "current_stream", lambda: None)
        m.setattr(_lib, "ptr", lambda t: t)
        for fn in ("randn_like", "randn", "rand", "randint"):
            real = getattr(torch, fn)

            def draw(*a, _real=real, _fn=fn, **kw):
                out = _real(*a, **kw)
                rec.label(**{f"drawn{rec.drawn}": out})
                rec.drawn += 1
                rec.events.append(_fn)                                           # (d): every draw, in its place between the calls
                return out
            m.setattr(torch, fn, draw)
        model = _FakeModel(rec)
        diff = create_gaussian_diffusion(timestep_respacing=respacing)
        model._bound_schedule = diff                                             # (bound already: no upload)
        yield rec, model, diff, (x, t, noise, prev, (s0, s1, s2, COUNT))


def _denoised_fn(rec):
    def fn(x0):
        rec.events.append("denoised_fn")
        return x0
    return fn


# every case: name -> a call on (diffusion, model, x, t, noise, prev, state, kw, fn); fn is None on the fused path
STEP_CASES = {
    "p_sample": lambda d, m, x, t, noise, prev, state, kw, fn: d.p_sample(m, x, t, denoised_fn=fn, model_kwargs=kw),
    "p_sample/noise": lambda d, m, x, t, noise, prev, state, kw, fn: d._step(0, m, x, t, False, fn, kw, 0.0, noise),
    "ddim": lambda d, m, x, t, noise, prev, state, kw, fn: d.ddim_sample(m, x, t, denoised_fn=fn, model_kwargs=kw, eta=ETA),
    "ddim/noise": lambda d, m, x, t, noise, prev, state, kw, fn: d._step(1, m, x, t, True, fn, kw, ETA, noise),
    "ddim_reverse": lambda d, m, x, t, noise, prev, state, kw, fn: d.ddim_reverse_sample(m, x, t, denoised_fn=fn, model_kwargs=kw),
    "dpmpp_2m": lambda d, m, x, t, noise, prev, state, kw, fn: d.dpmpp_2m_sample(m, x, t, prev_xstart=prev, denoised_fn=fn, model_kwargs=kw),
    "dpmpp_2m/first": lambda d, m, x, t, noise, prev, state, kw, fn: d.dpmpp_2m_sample(m, x, t, clip_denoised=False, denoised_fn=fn,
                                                                                     model_kwargs=kw),
    "dpmpp_2m_sde": lambda d, m, x, t, noise, prev, state, kw, fn: d.dpmpp_2m_sde_sample(m, x, t, prev_xstart=prev, denoised_fn=fn,
                                                                                         model_kwargs=kw),
    "dpmpp_2m_sde/noise": lambda d, m, x, t, noise, prev, state, kw, fn: d._dpmpp_2m_sde(m, x, t, None, True, fn, kw, noise=noise),
    "dpmpp_2m_sde/philox": lambda d, m, x, t, noise, prev, state, kw, fn: d._dpmpp_2m_sde(m, x, t, prev, False, fn, kw, philox=PHILOX),
    "unipc": lambda d, m, x, t, noise, prev, state, kw, fn: d.unipc_sample(m, x, t, state=state, denoised_fn=fn, model_kwargs=kw),
    "unipc/first": lambda d, m, x, t, noise, prev, state, kw, fn: d.unipc_sample(m, x, t, clip_denoised=False, denoised_fn=fn,
                                                                               model_kwargs=kw),
}


def record_step(monkeypatch, case, through_fn):
    with _recording(monkeypatch) as (rec, model, diff, (x, t, noise, prev, state)):
        out = STEP_CASES[case](diff, model, x, t, noise, prev, state, {}, _denoised_fn(rec) if through_fn else None)
        assert out is not None
        return rec.events


def record_scoped(monkeypatch, case):
    """The set / restore pairs around a step: cfg_scale as a keyword and from the scope, a known region with and without its own noise."""
    with _recording(monkeypatch) as (rec, model, diff, (x, t, noise, prev, state)):
        src, mask = torch.zeros(B, T, 3, 2, 2), torch.ones(B, T, 2, 2)
        if case == "cfg/keyword":
            diff.ddim_sample(model, x, t, model_kwargs={}, cfg_scale=2.0)
        elif case == "cfg/scope":
            with diff.cfg_scale_scope(model, 2.0):
                diff.unipc_sample(model, x, t, model_kwargs={})
        elif case == "cfg/denoised":
            diff.p_sample(model, x, t, denoised_fn=_denoised_fn(rec), model_kwargs={}, cfg_scale=2.0)
        elif case == "known/drawn":
            with diff.known_region_scope(model, src, mask):
                diff.dpmpp_2m_sde_sample(model, x, t, prev_xstart=prev, model_kwargs={})
        elif case == "known/given":
            with diff.known_region_scope(model, src, mask, known_noise=noise):
                diff.p_sample(model, x, t, model_kwargs={})
        elif case == "measurement":
            with diff.measurement_scope(model, torch.zeros(B, T, 3, 1, 1), scale=2):
                diff.dpmpp_2m_sample(model, x, t, model_kwargs={})
        return rec.events


def _loop_kwargs(x0):
    return dict(x0=x0, observed_frames="x_0", latent_mask=torch.ones(B, T, 1, 1, 1))


LOOPS = ("p_sample_loop", "ddim_sample_loop", "dpmpp_2m_sample_loop", "dpmpp_2m_sde_sample_loop", "unipc_sample_loop")


def record_loop(monkeypatch, case):
    """(e): the sequence of entries of a public loop on a 3-step schedule, with the t handed to each, the draws and the device check."""
    name, _, variant = case.partition("/")
    with _recording(monkeypatch, full=False) as (rec, model, diff, (x, t, noise, prev, state)):
        shape, kw = tuple(x.shape), _loop_kwargs(x)
        extra = {"cfg": dict(cfg_scale=2.0), "noise": dict(noise=noise), "fn": dict(denoised_fn=_denoised_fn(rec))}.get(variant, {})
        if name in LOOPS:
            if variant == "progressive":
                outs = list(getattr(diff, name + "_progressive")(model, shape, model_kwargs=kw))
                assert len(outs) == 3 and all("sample" in o and "pred_xstart" in o for o in outs)
            else:
                out = getattr(diff, name)(model, shape, model_kwargs=kw, **extra)
                assert (out[0] if name == "p_sample_loop" else out).shape == x.shape
        elif name == "ddim_reverse_sample_loop":
            if variant == "progressive":
                assert len(list(diff.ddim_reverse_sample_loop_progressive(model, x, model_kwargs=kw, t_start=1))) == 2
            else:
                assert diff.ddim_reverse_sample_loop(model, x, model_kwargs=kw, **extra).shape == x.shape
        else:
            assert name == "repaint_sample_loop"
            out = diff.repaint_sample_loop(model, shape, torch.zeros(B, T, 3, 2, 2), torch.ones(B, T, 2, 2), sampler=variant, jump_length=1,
                                           n_resample=2, model_kwargs=kw, eta=ETA, cfg_scale=2.0 if variant == "dpmpp_2m" else 1.0)
            assert out.shape == x.shape
        return rec.events


def record_infer_video(monkeypatch, case):
    """The eager executor of infer_video, one window of two latent frames: every sampler plain, and with a known region on the walk of
    repaint_schedule (jump_length 1, n_resample 2)."""
    sampler, _, variant = case.partition("/")
    with _recording(monkeypatch, full=False) as (rec, model, diff, _):
        batch = _rand(2, 4, 3, 2, 2, seed=1)
        kw = dict(known_mask=torch.ones(4, 2, 2), n_resample=2) if variant == "known" else {}
        if variant == "cfg":
            kw = dict(cfg_scale=2.0)
        samples, _ = video_sample.infer_video("autoreg", model, diff, batch, 4, 2, 2, sampler=sampler, eta=ETA, **kw)
        assert samples.shape == tuple(batch.shape)
        return rec.events


def _compact(events):
    """Runs of one event as 'event*n'."""
    out = []
    for e in events:
        if out and out[-1][0] == e:
            out[-1][1] += 1
        else:
            out.append([e, 1])
    return " ".join(e if n == 1 else f"{e}*{n}" for e, n in out)


# recorded with the functions above from the step path of the parent commit, before any of it read the table
EXPECTED_STEP = {('p_sample', False): 'randn_like vd_p_sample(17 4 3 w1 w2 w3 w4 w5 w6 t 2 1 drawn0 0 0 p p N N)',
 ('p_sample', True): 'vd_dynamic_threshold(17) vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn randn_like '
                     'vd_posterior_from_xstart(17 0 4 36 x p t 1 0.0 drawn0 0 0 p p N N)',
 ('p_sample/noise', False): 'vd_p_sample(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 noise 0 0 p p N N)',
 ('p_sample/noise', True): 'vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn vd_posterior_from_xstart(17 0 4 '
                           '36 x p t 0 0.0 noise 0 0 p p N N)',
 ('ddim', False): 'randn_like vd_ddim_sample(17 4 3 w1 w2 w3 w4 w5 w6 t 2 1 0.5 drawn0 0 0 p p N N)',
 ('ddim', True): 'vd_dynamic_threshold(17) vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn randn_like '
                 'vd_posterior_from_xstart(17 1 4 36 x p t 1 0.5 drawn0 0 0 p p N N)',
 ('ddim/noise', False): 'vd_ddim_sample(17 4 3 w1 w2 w3 w4 w5 w6 t 2 1 0.5 noise 0 0 p p N N)',
 ('ddim/noise', True): 'vd_dynamic_threshold(17) vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn '
                       'vd_posterior_from_xstart(17 1 4 36 x p t 1 0.5 noise 0 0 p p N N)',
 ('ddim_reverse', False): 'vd_ddim_reverse_sample(17 4 3 w1 w2 w3 w4 w5 w6 t 2 1 p p N N)',
 ('ddim_reverse', True): 'vd_dynamic_threshold(17) vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn '
                         'vd_ddim_reverse_from_xstart(17 4 36 x p t 1 p p N)',
 ('dpmpp_2m', False): 'vd_dpmpp_2m_sample(17 4 3 w1 w2 w3 w4 w5 w6 t prev 2 1 p p N N)',
 ('dpmpp_2m', True): 'vd_dynamic_threshold(17) vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn '
                     'vd_dpmpp_2m_from_xstart(17 4 36 x p prev t 1 p p N)',
 ('dpmpp_2m/first', False): 'vd_dpmpp_2m_sample(17 4 3 w1 w2 w3 w4 w5 w6 t N 2 0 p p N N)',
 ('dpmpp_2m/first', True): 'vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn vd_dpmpp_2m_from_xstart(17 4 36 '
                           'x p N t 0 p p N)',
 ('dpmpp_2m_sde', False): 'randn_like vd_dpmpp_2m_sde_sample(17 4 3 w1 w2 w3 w4 w5 w6 t prev 2 1 drawn0 0 0 p p N N)',
 ('dpmpp_2m_sde', True): 'vd_dynamic_threshold(17) vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn '
                         'randn_like vd_dpmpp_2m_sde_from_xstart(17 4 36 x p prev t 1 drawn0 0 0 p p N)',
 ('dpmpp_2m_sde/noise', False): 'vd_dpmpp_2m_sde_sample(17 4 3 w1 w2 w3 w4 w5 w6 t N 2 1 noise 0 0 p p N N)',
 ('dpmpp_2m_sde/noise', True): 'vd_dynamic_threshold(17) vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn '
                               'vd_dpmpp_2m_sde_from_xstart(17 4 36 x p N t 1 noise 0 0 p p N)',
 ('dpmpp_2m_sde/philox', False): 'vd_dpmpp_2m_sde_sample(17 4 3 w1 w2 w3 w4 w5 w6 t prev 2 0 N 7 11 p p N N)',
 ('dpmpp_2m_sde/philox', True): 'vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn '
                                'vd_dpmpp_2m_sde_from_xstart(17 4 36 x p prev t 0 N 7 11 p p N)',
 ('unipc', False): 'vd_unipc_sample(17 4 3 w1 w2 w3 w4 w5 w6 t s0 s1 s2 5 2 1 p p p p p N N)',
 ('unipc', True): 'vd_dynamic_threshold(17) vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn '
                  'vd_unipc_from_xstart(17 4 36 x p s0 s1 s2 5 t 1 p p p p p N)',
 ('unipc/first', False): 'vd_unipc_sample(17 4 3 w1 w2 w3 w4 w5 w6 t N N N 0 2 0 p p p p p N N)',
 ('unipc/first', True): 'vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t 2 0 p p p N) denoised_fn vd_unipc_from_xstart(17 4 36 x p N '
                        'N N 0 t 0 p p p p p N)'}
EXPECTED_SCOPED = {'cfg/keyword': 'randn_like vd_cfg_scale(17) vd_set_cfg_scale(17 2.0) vd_ddim_sample(17 4 3 w1 w2 w3 w4 w5 w6 t 2 1 0.0 drawn0 0 0 '
                'p p N N) vd_set_cfg_scale(17 1.0)',
 'cfg/scope': 'vd_cfg_scale(17) vd_set_cfg_scale(17 2.0) vd_unipc_sample(17 4 3 w1 w2 w3 w4 w5 w6 t N N N 0 2 1 p p p p p N N) '
              'vd_set_cfg_scale(17 1.0)',
 'cfg/denoised': 'vd_dynamic_threshold(17) vd_cfg_scale(17) vd_set_cfg_scale(17 2.0) vd_p_mean_variance(17 4 3 w1 w2 w3 w4 w5 w6 t '
                 '2 0 p p p N) vd_set_cfg_scale(17 1.0) denoised_fn randn_like vd_posterior_from_xstart(17 0 4 36 x p t 1 0.0 '
                 'drawn0 0 0 p p N N)',
 'known/drawn': 'vd_set_known_region(17 p p N 0 0) randn_like*2 vd_set_known_region(17 p p drawn1 0 0) vd_dpmpp_2m_sde_sample(17 4 '
                '3 w1 w2 w3 w4 w5 w6 t prev 2 1 drawn0 0 0 p p N N) vd_set_known_region(17 p p N 0 0) vd_set_known_region(17 N N N '
                '0 0)',
 'known/given': 'vd_set_known_region(17 p p N 0 0) randn_like vd_set_known_region(17 p p noise 0 0) vd_p_sample(17 4 3 w1 w2 w3 w4 '
                'w5 w6 t 2 1 drawn0 0 0 p p N N) vd_set_known_region(17 p p N 0 0) vd_set_known_region(17 N N N 0 0)',
 'measurement': 'vd_set_measurement(17 p 2 0) vd_dpmpp_2m_sample(17 4 3 w1 w2 w3 w4 w5 w6 t N 2 1 p p N N) vd_set_measurement(17 N '
                '1 0)'}
EXPECTED_LOOP = {'p_sample_loop': 'randn randn_like vd_q_sample@1 rand randn_like*2 vd_p_sample@2 randn_like vd_q_sample@0 rand randn_like*2 '
                  'vd_p_sample@1 randn_like vd_q_sample@-1 rand randn_like*2 vd_p_sample@0 check_device_errors',
 'p_sample_loop/progressive': 'randn randn_like vd_q_sample@1 rand randn_like*2 vd_p_sample@2 randn_like vd_q_sample@0 rand '
                              'randn_like*2 vd_p_sample@1 randn_like vd_q_sample@-1 rand randn_like*2 vd_p_sample@0',
 'p_sample_loop/fn': 'randn randn_like vd_q_sample@1 rand randn_like vd_dynamic_threshold vd_p_mean_variance@2 denoised_fn '
                     'randn_like vd_posterior_from_xstart@2 randn_like vd_q_sample@0 rand randn_like vd_dynamic_threshold '
                     'vd_p_mean_variance@1 denoised_fn randn_like vd_posterior_from_xstart@1 randn_like vd_q_sample@-1 rand '
                     'randn_like vd_dynamic_threshold vd_p_mean_variance@0 denoised_fn randn_like vd_posterior_from_xstart@0 '
                     'check_device_errors',
 'p_sample_loop/noise': 'vd_q_sample@1 rand randn_like vd_p_sample@2 vd_q_sample@0 rand randn_like vd_p_sample@1 vd_q_sample@-1 '
                        'rand randn_like vd_p_sample@0 check_device_errors',
 'p_sample_loop/cfg': 'randn randn_like vd_q_sample@1 rand randn_like*2 vd_cfg_scale vd_set_cfg_scale vd_p_sample@2 '
                      'vd_set_cfg_scale randn_like vd_q_sample@0 rand randn_like*2 vd_cfg_scale vd_set_cfg_scale vd_p_sample@1 '
                      'vd_set_cfg_scale randn_like vd_q_sample@-1 rand randn_like*2 vd_cfg_scale vd_set_cfg_scale vd_p_sample@0 '
                      'vd_set_cfg_scale check_device_errors',
 'ddim_sample_loop': 'randn randn_like vd_ddim_sample@2 randn_like vd_ddim_sample@1 randn_like vd_ddim_sample@0 '
                     'check_device_errors',
 'ddim_sample_loop/progressive': 'randn randn_like vd_ddim_sample@2 randn_like vd_ddim_sample@1 randn_like vd_ddim_sample@0',
 'ddim_sample_loop/fn': 'randn vd_dynamic_threshold vd_p_mean_variance@2 denoised_fn randn_like vd_posterior_from_xstart@2 '
                        'vd_dynamic_threshold vd_p_mean_variance@1 denoised_fn randn_like vd_posterior_from_xstart@1 '
                        'vd_dynamic_threshold vd_p_mean_variance@0 denoised_fn randn_like vd_posterior_from_xstart@0 '
                        'check_device_errors',
 'ddim_sample_loop/noise': 'randn_like vd_ddim_sample@2 randn_like vd_ddim_sample@1 randn_like vd_ddim_sample@0 '
                           'check_device_errors',
 'ddim_sample_loop/cfg': 'randn randn_like vd_cfg_scale vd_set_cfg_scale vd_ddim_sample@2 vd_set_cfg_scale randn_like vd_cfg_scale '
                         'vd_set_cfg_scale vd_ddim_sample@1 vd_set_cfg_scale randn_like vd_cfg_scale vd_set_cfg_scale '
                         'vd_ddim_sample@0 vd_set_cfg_scale check_device_errors',
 'dpmpp_2m_sample_loop': 'randn vd_dpmpp_2m_sample@2 vd_dpmpp_2m_sample@1 vd_dpmpp_2m_sample@0 check_device_errors',
 'dpmpp_2m_sample_loop/progressive': 'randn vd_dpmpp_2m_sample@2 vd_dpmpp_2m_sample@1 vd_dpmpp_2m_sample@0',
 'dpmpp_2m_sample_loop/fn': 'randn vd_dynamic_threshold vd_p_mean_variance@2 denoised_fn vd_dpmpp_2m_from_xstart@2 '
                            'vd_dynamic_threshold vd_p_mean_variance@1 denoised_fn vd_dpmpp_2m_from_xstart@1 vd_dynamic_threshold '
                            'vd_p_mean_variance@0 denoised_fn vd_dpmpp_2m_from_xstart@0 check_device_errors',
 'dpmpp_2m_sample_loop/noise': 'vd_dpmpp_2m_sample@2 vd_dpmpp_2m_sample@1 vd_dpmpp_2m_sample@0 check_device_errors',
 'dpmpp_2m_sample_loop/cfg': 'randn vd_cfg_scale vd_set_cfg_scale vd_dpmpp_2m_sample@2 vd_set_cfg_scale vd_cfg_scale '
                             'vd_set_cfg_scale vd_dpmpp_2m_sample@1 vd_set_cfg_scale vd_cfg_scale vd_set_cfg_scale '
                             'vd_dpmpp_2m_sample@0 vd_set_cfg_scale check_device_errors',
 'dpmpp_2m_sde_sample_loop': 'randn randn_like vd_dpmpp_2m_sde_sample@2 randn_like vd_dpmpp_2m_sde_sample@1 randn_like '
                             'vd_dpmpp_2m_sde_sample@0 check_device_errors',
 'dpmpp_2m_sde_sample_loop/progressive': 'randn randn_like vd_dpmpp_2m_sde_sample@2 randn_like vd_dpmpp_2m_sde_sample@1 randn_like '
                                         'vd_dpmpp_2m_sde_sample@0',
 'dpmpp_2m_sde_sample_loop/fn': 'randn vd_dynamic_threshold vd_p_mean_variance@2 denoised_fn randn_like '
                                'vd_dpmpp_2m_sde_from_xstart@2 vd_dynamic_threshold vd_p_mean_variance@1 denoised_fn randn_like '
                                'vd_dpmpp_2m_sde_from_xstart@1 vd_dynamic_threshold vd_p_mean_variance@0 denoised_fn randn_like '
                                'vd_dpmpp_2m_sde_from_xstart@0 check_device_errors',
 'dpmpp_2m_sde_sample_loop/noise': 'randn_like vd_dpmpp_2m_sde_sample@2 randn_like vd_dpmpp_2m_sde_sample@1 randn_like '
                                   'vd_dpmpp_2m_sde_sample@0 check_device_errors',
 'dpmpp_2m_sde_sample_loop/cfg': 'randn vd_cfg_scale vd_set_cfg_scale randn_like vd_dpmpp_2m_sde_sample@2 vd_set_cfg_scale '
                                 'vd_cfg_scale vd_set_cfg_scale randn_like vd_dpmpp_2m_sde_sample@1 vd_set_cfg_scale vd_cfg_scale '
                                 'vd_set_cfg_scale randn_like vd_dpmpp_2m_sde_sample@0 vd_set_cfg_scale check_device_errors',
 'unipc_sample_loop': 'randn vd_unipc_sample@2 vd_unipc_sample@1 vd_unipc_sample@0 check_device_errors',
 'unipc_sample_loop/progressive': 'randn vd_unipc_sample@2 vd_unipc_sample@1 vd_unipc_sample@0',
 'unipc_sample_loop/fn': 'randn vd_dynamic_threshold vd_p_mean_variance@2 denoised_fn vd_unipc_from_xstart@2 vd_dynamic_threshold '
                         'vd_p_mean_variance@1 denoised_fn vd_unipc_from_xstart@1 vd_dynamic_threshold vd_p_mean_variance@0 '
                         'denoised_fn vd_unipc_from_xstart@0 check_device_errors',
 'unipc_sample_loop/noise': 'vd_unipc_sample@2 vd_unipc_sample@1 vd_unipc_sample@0 check_device_errors',
 'unipc_sample_loop/cfg': 'randn vd_cfg_scale vd_set_cfg_scale vd_unipc_sample@2 vd_set_cfg_scale vd_cfg_scale vd_set_cfg_scale '
                          'vd_unipc_sample@1 vd_set_cfg_scale vd_cfg_scale vd_set_cfg_scale vd_unipc_sample@0 vd_set_cfg_scale '
                          'check_device_errors',
 'ddim_reverse_sample_loop': 'vd_ddim_reverse_sample@0 vd_ddim_reverse_sample@1 vd_ddim_reverse_sample@2 check_device_errors',
 'ddim_reverse_sample_loop/progressive': 'vd_ddim_reverse_sample@1 vd_ddim_reverse_sample@2',
 'ddim_reverse_sample_loop/fn': 'vd_dynamic_threshold vd_p_mean_variance@0 denoised_fn vd_ddim_reverse_from_xstart@0 '
                                'vd_dynamic_threshold vd_p_mean_variance@1 denoised_fn vd_ddim_reverse_from_xstart@1 '
                                'vd_dynamic_threshold vd_p_mean_variance@2 denoised_fn vd_ddim_reverse_from_xstart@2 '
                                'check_device_errors',
 'repaint_sample_loop/p_sample': 'randn vd_set_known_region randn_like vd_q_sample@1 rand randn_like*3 vd_set_known_region '
                                 'vd_p_sample@2 vd_set_known_region randn_like vd_q_jump@2 randn_like vd_q_sample@1 rand '
                                 'randn_like*3 vd_set_known_region vd_p_sample@2 vd_set_known_region randn_like vd_q_sample@0 rand '
                                 'randn_like*3 vd_set_known_region vd_p_sample@1 vd_set_known_region randn_like vd_q_jump@1 '
                                 'randn_like vd_q_sample@0 rand randn_like*3 vd_set_known_region vd_p_sample@1 vd_set_known_region '
                                 'randn_like vd_q_sample@-1 rand randn_like*3 vd_set_known_region vd_p_sample@0 '
                                 'vd_set_known_region*2 check_device_errors',
 'repaint_sample_loop/ddim': 'randn vd_set_known_region randn_like*2 vd_set_known_region vd_ddim_sample@2 vd_set_known_region '
                             'randn_like vd_q_jump@2 randn_like*2 vd_set_known_region vd_ddim_sample@2 vd_set_known_region '
                             'randn_like*2 vd_set_known_region vd_ddim_sample@1 vd_set_known_region randn_like vd_q_jump@1 '
                             'randn_like*2 vd_set_known_region vd_ddim_sample@1 vd_set_known_region randn_like*2 '
                             'vd_set_known_region vd_ddim_sample@0 vd_set_known_region*2 check_device_errors',
 'repaint_sample_loop/dpmpp_2m': 'randn vd_set_known_region vd_cfg_scale vd_set_cfg_scale randn_like vd_set_known_region '
                                 'vd_dpmpp_2m_sample@2 vd_set_known_region vd_set_cfg_scale randn_like vd_q_jump@2 vd_cfg_scale '
                                 'vd_set_cfg_scale randn_like vd_set_known_region vd_dpmpp_2m_sample@2 vd_set_known_region '
                                 'vd_set_cfg_scale vd_cfg_scale vd_set_cfg_scale randn_like vd_set_known_region '
                                 'vd_dpmpp_2m_sample@1 vd_set_known_region vd_set_cfg_scale randn_like vd_q_jump@1 vd_cfg_scale '
                                 'vd_set_cfg_scale randn_like vd_set_known_region vd_dpmpp_2m_sample@1 vd_set_known_region '
                                 'vd_set_cfg_scale vd_cfg_scale vd_set_cfg_scale randn_like vd_set_known_region '
                                 'vd_dpmpp_2m_sample@0 vd_set_known_region vd_set_cfg_scale vd_set_known_region '
                                 'check_device_errors',
 'repaint_sample_loop/dpmpp_2m_sde': 'randn vd_set_known_region randn_like*2 vd_set_known_region vd_dpmpp_2m_sde_sample@2 '
                                     'vd_set_known_region randn_like vd_q_jump@2 randn_like*2 vd_set_known_region '
                                     'vd_dpmpp_2m_sde_sample@2 vd_set_known_region randn_like*2 vd_set_known_region '
                                     'vd_dpmpp_2m_sde_sample@1 vd_set_known_region randn_like vd_q_jump@1 randn_like*2 '
                                     'vd_set_known_region vd_dpmpp_2m_sde_sample@1 vd_set_known_region randn_like*2 '
                                     'vd_set_known_region vd_dpmpp_2m_sde_sample@0 vd_set_known_region*2 check_device_errors'}
EXPECTED_INFER = {'p_sample': 'randn_like vd_p_sample@2 randn_like vd_p_sample@1 randn_like vd_p_sample@0 check_device_errors',
 'p_sample/known': 'randint vd_randn+24 vd_set_known_region randn_like vd_set_known_region vd_p_sample@2 vd_set_known_region*2 '
                   'vd_randn+96 vd_q_jump@2 vd_randn+216 vd_set_known_region randn_like vd_set_known_region vd_p_sample@2 '
                   'vd_set_known_region*2 vd_randn+312 vd_set_known_region randn_like vd_set_known_region vd_p_sample@1 '
                   'vd_set_known_region*2 vd_randn+384 vd_q_jump@1 vd_randn+504 vd_set_known_region randn_like vd_set_known_region '
                   'vd_p_sample@1 vd_set_known_region*2 vd_randn+600 vd_set_known_region randn_like vd_set_known_region '
                   'vd_p_sample@0 vd_set_known_region*2 check_device_errors',
 'p_sample/cfg': 'randn_like vd_cfg_scale vd_set_cfg_scale vd_p_sample@2 vd_set_cfg_scale randn_like vd_cfg_scale vd_set_cfg_scale '
                 'vd_p_sample@1 vd_set_cfg_scale randn_like vd_cfg_scale vd_set_cfg_scale vd_p_sample@0 vd_set_cfg_scale '
                 'check_device_errors',
 'ddim': 'randn_like vd_ddim_sample@2 randn_like vd_ddim_sample@1 randn_like vd_ddim_sample@0 check_device_errors',
 'ddim/known': 'randint vd_randn+24 vd_set_known_region randn_like vd_set_known_region vd_ddim_sample@2 vd_set_known_region*2 '
               'vd_randn+96 vd_q_jump@2 vd_randn+216 vd_set_known_region randn_like vd_set_known_region vd_ddim_sample@2 '
               'vd_set_known_region*2 vd_randn+312 vd_set_known_region randn_like vd_set_known_region vd_ddim_sample@1 '
               'vd_set_known_region*2 vd_randn+384 vd_q_jump@1 vd_randn+504 vd_set_known_region randn_like vd_set_known_region '
               'vd_ddim_sample@1 vd_set_known_region*2 vd_randn+600 vd_set_known_region randn_like vd_set_known_region '
               'vd_ddim_sample@0 vd_set_known_region*2 check_device_errors',
 'ddim/cfg': 'randn_like vd_cfg_scale vd_set_cfg_scale vd_ddim_sample@2 vd_set_cfg_scale randn_like vd_cfg_scale vd_set_cfg_scale '
             'vd_ddim_sample@1 vd_set_cfg_scale randn_like vd_cfg_scale vd_set_cfg_scale vd_ddim_sample@0 vd_set_cfg_scale '
             'check_device_errors',
 'dpmpp_2m': 'vd_dpmpp_2m_sample@2 vd_dpmpp_2m_sample@1 vd_dpmpp_2m_sample@0 check_device_errors',
 'dpmpp_2m/known': 'randint vd_randn+24 vd_set_known_region*2 vd_dpmpp_2m_sample@2 vd_set_known_region*2 vd_randn+96 vd_q_jump@2 '
                   'vd_randn+216 vd_set_known_region*2 vd_dpmpp_2m_sample@2 vd_set_known_region*2 vd_randn+312 '
                   'vd_set_known_region*2 vd_dpmpp_2m_sample@1 vd_set_known_region*2 vd_randn+384 vd_q_jump@1 vd_randn+504 '
                   'vd_set_known_region*2 vd_dpmpp_2m_sample@1 vd_set_known_region*2 vd_randn+600 vd_set_known_region*2 '
                   'vd_dpmpp_2m_sample@0 vd_set_known_region*2 check_device_errors',
 'dpmpp_2m/cfg': 'vd_cfg_scale vd_set_cfg_scale vd_dpmpp_2m_sample@2 vd_set_cfg_scale vd_cfg_scale vd_set_cfg_scale '
                 'vd_dpmpp_2m_sample@1 vd_set_cfg_scale vd_cfg_scale vd_set_cfg_scale vd_dpmpp_2m_sample@0 vd_set_cfg_scale '
                 'check_device_errors',
 'dpmpp_2m_sde': 'randint vd_dpmpp_2m_sde_sample@2 vd_dpmpp_2m_sde_sample@1+96 vd_dpmpp_2m_sde_sample@0+192 check_device_errors',
 'dpmpp_2m_sde/known': 'randint vd_randn+24 vd_set_known_region*2 vd_dpmpp_2m_sde_sample@2 vd_set_known_region*2 vd_randn+96 '
                       'vd_q_jump@2 vd_randn+216 vd_set_known_region*2 vd_dpmpp_2m_sde_sample@2+192 vd_set_known_region*2 '
                       'vd_randn+312 vd_set_known_region*2 vd_dpmpp_2m_sde_sample@1+288 vd_set_known_region*2 vd_randn+384 '
                       'vd_q_jump@1 vd_randn+504 vd_set_known_region*2 vd_dpmpp_2m_sde_sample@1+480 vd_set_known_region*2 '
                       'vd_randn+600 vd_set_known_region*2 vd_dpmpp_2m_sde_sample@0+576 vd_set_known_region*2 check_device_errors',
 'dpmpp_2m_sde/cfg': 'randint vd_cfg_scale vd_set_cfg_scale vd_dpmpp_2m_sde_sample@2 vd_set_cfg_scale vd_cfg_scale '
                     'vd_set_cfg_scale vd_dpmpp_2m_sde_sample@1+96 vd_set_cfg_scale vd_cfg_scale vd_set_cfg_scale '
                     'vd_dpmpp_2m_sde_sample@0+192 vd_set_cfg_scale check_device_errors',
 'unipc': 'vd_unipc_sample@2 vd_unipc_sample@1 vd_unipc_sample@0 check_device_errors',
 'unipc/cfg': 'vd_cfg_scale vd_set_cfg_scale vd_unipc_sample@2 vd_set_cfg_scale vd_cfg_scale vd_set_cfg_scale vd_unipc_sample@1 '
              'vd_set_cfg_scale vd_cfg_scale vd_set_cfg_scale vd_unipc_sample@0 vd_set_cfg_scale check_device_errors'}


def test_table_executor_and_job_agree():
    rows = gaussian_diffusion.SAMPLERS
    assert list(rows) == ["p_sample", "ddim", "ddim_reverse", "dpmpp_2m", "dpmpp_2m_sde", "unipc"]
    assert [row.id for row in rows.values()] == [0, 1, 2, 3, 4, 5]
    for name, row in rows.items():
        assert executor._sampler_id(name) == row.id
        assert callable(getattr(gaussian_diffusion.GaussianDiffusion, row.step))
        assert row.fused in _lib.SIGNATURES and row.from_xstart in _lib.SIGNATURES
        assert row.noise in (None, "tensor", "philox") and row.carry in (None, "prev_xstart", "state")
    sampler = next(a for a in video_sample.build_parser()._actions if a.dest == "sampler")
    assert list(sampler.choices) == [name for name, row in rows.items() if not row.up] == ["p_sample", "ddim", "dpmpp_2m", "dpmpp_2m_sde", "unipc"]
    assert {name for name, row in rows.items() if set(STEP_CASES) & {name}} == set(rows)          # every sampler has its step cases
    assert [row.carry for row in rows.values()] == [None, None, None, "prev_xstart", "prev_xstart", "state"]
    assert [name for name, row in rows.items() if row.up] == ["ddim_reverse"] and [name for name, row in rows.items() if row.eta] == ["ddim"]


@pytest.mark.parametrize("case,through_fn", list(EXPECTED_STEP))
def test_step_entry_arguments_and_draws(monkeypatch, case, through_fn):
    events = record_step(monkeypatch, case, through_fn)
    row = gaussian_diffusion.SAMPLERS[case.partition("/")[0]]
    assert events[-1].startswith((row.from_xstart if through_fn else row.fused) + "(")             # (a) the entry; (b) held in the stand-in
    drawn = row.noise is not None and case.partition("/")[2] not in ("noise", "philox")
    assert sum(e in ("randn_like", "randn", "rand", "randint") for e in events) == (1 if drawn else 0)   # (d)
    if through_fn:                                                                                # ... behind the callback, in front of the entry
        assert events.index("denoised_fn") < len(events) - (2 if drawn else 1) and (not drawn or events[-2] == "randn_like")
    assert _compact(events) == EXPECTED_STEP[case, through_fn]                                    # (c) every scalar, every pointer slot


@pytest.mark.parametrize("case", list(EXPECTED_SCOPED))
def test_set_and_restore_pairs_around_a_step(monkeypatch, case):
    assert _compact(record_scoped(monkeypatch, case)) == EXPECTED_SCOPED[case]


@pytest.mark.parametrize("case", list(EXPECTED_LOOP))
def test_loop_entries_and_the_t_of_each(monkeypatch, case):
    assert _compact(record_loop(monkeypatch, case)) == EXPECTED_LOOP[case]                        # (e)


@pytest.mark.parametrize("case", list(EXPECTED_INFER))
def test_infer_video_eager_window(monkeypatch, case):
    assert _compact(record_infer_video(monkeypatch, case)) == EXPECTED_INFER[case]


def test_every_public_loop_is_recorded():
    loops = {n for n in dir(gaussian_diffusion.GaussianDiffusion)
             if n.endswith(("_sample_loop", "_sample_loop_progressive")) and not n.startswith("_")}
    assert len(loops) == 14                                                                       # two per sampler, and repaint's two
    seen = {c.partition("/")[0] + ("_progressive" if c.endswith("/progressive") else "") for c in EXPECTED_LOOP}
    assert seen | {"repaint_sample_loop_progressive"} == loops


def test_what_the_steps_return(monkeypatch):
    """The dict of every step on both paths: its keys in order, fresh tensors of x's shape, and unipc's state one step further."""
    with _recording(monkeypatch) as (rec, model, diff, (x, t, noise, prev, state)):
        for fn in (None, _denoised_fn(rec)):
            for case, call in STEP_CASES.items():
                if case.startswith("p_sample/") or case.startswith("ddim/"):
                    continue                                                     # (_step: a tuple)
                out = call(diff, model, x, t, noise, prev, state, {}, fn)
                name = case.partition("/")[0]
                keys = {"p_sample": ["sample", "pred_xstart", "attn"], "unipc": ["sample", "pred_xstart", "state"]}.get(name, ["sample", "pred_xstart"])
                assert list(out) == keys, case
                assert out["sample"].shape == out["pred_xstart"].shape == x.shape and out["sample"] is not x
                if name == "unipc":
                    assert len(out["state"]) == 4 and out["state"][3] == (COUNT + 1 if case == "unipc" else 1)
                    assert all(v.shape == x.shape and v is not s for v, s in zip(out["state"][:3], state[:3]))
            assert [len(r) for r in (diff._fused_step(0, model, x, t, True, {}, noise=noise), diff._fused_step(5, model, x, t, True, {}))] == [2, 3]
