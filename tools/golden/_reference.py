"""The only place that touches the reference checkout.  Nothing here runs when the package is imported: `load()` is
called by the producers, so `tools.golden` imports (and lists its manifest) on a machine without the reference."""
import contextlib
import functools
import importlib
import importlib.util
import os
import sys
import types

import torch

DIR = "/root/reference"          # set by the command's --reference option before any producer runs


def directory():
    if not os.path.isdir(DIR):
        raise SystemExit(f"tools.golden: the reference directory {DIR!r} does not exist (pass --reference DIR)")
    return DIR


@functools.lru_cache(maxsize=None)
def load():
    """Import `improved_diffusion` from the reference and return its modules as a namespace (su, iu, respace, tu).
    Third-party modules the reference imports but never reaches on the pinned paths (lpips, imageio, blobfile / mpi4py
    via dist_util, the dataset loaders) are empty stand-ins of our own; nothing of the reference is copied."""
    sys.dont_write_bytecode = True           # the reference's directory is read-only: leave no __pycache__ in it
    sys.path.insert(0, directory())
    torch.set_num_threads(8)                 # every fixture was minted with 8 threads

    lp = types.ModuleType("lpips")
    lp.LPIPS = type("LPIPS", (torch.nn.Module,), {})
    lp.normalize_tensor = lambda x: x
    sys.modules["lpips"] = lp
    sys.modules["imageio"] = types.ModuleType("imageio")
    du = types.ModuleType("improved_diffusion.dist_util")
    du.load_state_dict = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("not used"))
    sys.modules["improved_diffusion.dist_util"] = du
    ds = types.ModuleType("improved_diffusion.image_datasets")
    for n in ("get_test_dataset", "get_train_dataset", "get_variable_length_dataset"):
        setattr(ds, n, None)
    sys.modules["improved_diffusion.image_datasets"] = ds

    import improved_diffusion
    improved_diffusion.dist_util = du
    improved_diffusion.image_datasets = ds
    mod = lambda name: importlib.import_module("improved_diffusion." + name)  # noqa: E731
    return types.SimpleNamespace(su=mod("script_util"), iu=mod("inference_util"), respace=mod("respace"),
                                 tu=mod("test_util"))


def video_sample_full():
    """scripts/video_sample_full.py of the reference, loaded by path (it is a script, not a module of the package)."""
    load()
    spec = importlib.util.spec_from_file_location("ref_video_sample_full",
                                                  os.path.join(directory(), "scripts", "video_sample_full.py"))
    vsf = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vsf)
    return vsf


@contextlib.contextmanager
def cuda_is_identity():
    """The reference's hard-coded .cuda() / .to('cuda') (p_sample_loop) become no-ops inside the block; both methods are
    restored on exit, so a producer that runs afterwards in the same process sees the real ones."""
    orig_to, orig_cuda = torch.Tensor.to, torch.Tensor.cuda

    def _to(self, *a, **k):
        a = tuple(x for x in a if not (isinstance(x, str) and x.startswith("cuda")))
        if isinstance(k.get("device"), str) and k["device"].startswith("cuda"):
            k.pop("device")
        return orig_to(self, *a, **k) if (a or k) else self

    torch.Tensor.to = _to
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        yield
    finally:
        torch.Tensor.to, torch.Tensor.cuda = orig_to, orig_cuda
