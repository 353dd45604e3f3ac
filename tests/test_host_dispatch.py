"""The Python glue between the ops and the library, without a device: the ctypes signature table against the header's
declarations, and the one place that creates a plan (``functional._cached_plan``) seen from each of its five callers."""
import os
import re

import pytest
import torch

from fft_conv_pytorch_amd import _native
from fft_conv_pytorch_amd import functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ signatures
def _declarations():
    """name -> (return type, parameter count) of every ``fc_*`` function the header declares."""
    text = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    found = {}
    for ret, name, params in re.findall(r"^\s*([A-Za-z_][\w \*]*?)\s*\b(fc_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text, flags=re.M):
        params = params.strip()
        found[name] = (ret.strip(), 0 if params == "void" else len(params.split(",")))
    return found


def test_every_export_has_the_argument_count_and_return_kind_of_its_declaration():
    """ctypes reports neither a missing argument nor a restype set on a void function: the table is checked here."""
    declared = _declarations()
    assert set(declared) == set(_native.SIGNATURES) and _native.EXPORTS == tuple(_native.SIGNATURES)
    assert declared["fc_version"] == ("int", 0) and declared["fc_long_wgrad"][1] == 11      # (the parser reads the header)
    for name, (restype, argtypes) in _native.SIGNATURES.items():
        ret, count = declared[name]
        assert len(argtypes) == count, (name, len(argtypes), count)
        assert (restype is None) == (ret == "void"), (name, restype, ret)
    lib = _native.load_library()
    for name, (restype, argtypes) in _native.SIGNATURES.items():      # ... and it is what the loaded library carries
        fn = getattr(lib, name)
        assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes), name


# ------------------------------------------------------------------------------------------------ plan creation
class _FakeCudaTensor:
    """Just enough of a contiguous (B, C, L) device tensor for the host-side part of a plan lookup (no device is touched)."""

    def __init__(self, shape, index, dtype=torch.float32):
        self.shape, self.ndim, self.dtype = torch.Size(shape), len(shape), dtype
        self.is_cuda, self.device = True, torch.device("cuda", index)

    def detach(self):
        return self

    def contiguous(self):
        return self

    def is_contiguous(self):
        return True

    def is_complex(self):
        return False

    def element_size(self):
        return 4


class _ReachedLaunch(Exception):
    """Raised by the fake device guard where ``_long_wgrad_run`` enters its launch (the guard then gets a device, not the
    ordinal ``_cached_plan`` gives it): the plan lookup is over, the test stops the call there."""


X, W = _FakeCudaTensor((2, 4, 6000), 1), _FakeCudaTensor((6, 4, 5), 1)
DY = _FakeCudaTensor((2, 6, 5996), 1)
WKEY = F_._long_wgrad_key(2, 4, 6, 1, 6000, 5, 0, 0, 5996, False, 0, 1, 1)
CALLERS = {
    "_plan_for": (lambda: F_._plan_for(X, W, None, 1, 0, 1, 1, "constant"), None),
    "_long_plan": (lambda: F_._long_plan(X, 6, 1, 5, 0, 0, False, 0, True), "long"),
    "_long_decim_plan": (lambda: F_._long_decim_plan(X, 6, 1, 5, 2, 0, 0, 0, False, True), "long_decim"),
    "_long_phases_plan": (lambda: F_._long_phases_plan(X, 6, 1, 5, 2, 0, 0, True), "long_phases"),
    "_long_wgrad_run": (lambda: F_._long_wgrad_run(X, DY, (6, 4, 5), WKEY, torch.float32), "long_wgrad"),
}


@pytest.mark.parametrize("name", sorted(CALLERS))
def test_each_caller_creates_its_plan_on_the_tensors_device_and_switches_nothing_on_a_hit(name, monkeypatch):
    """Plans own device allocations: each of the five callers of ``_cached_plan`` builds its plan with the TENSORS' device
    current (cuda:1 here, whatever device is current) and caches it under that ordinal; a cached plan is returned without
    a device switch."""
    call, tag = CALLERS[name]
    seen = {"guards": []}

    class Guard:
        def __init__(self, index):
            self.index = index

        def __enter__(self):
            if not isinstance(self.index, int):
                raise _ReachedLaunch
            seen["guards"].append(self.index)
            seen["inside"] = True

        def __exit__(self, *a):
            seen["inside"] = False

    def fake_get_plan(index, key):
        seen["created"] = (index, key[0], seen.get("inside", False))
        return "plan"

    def run():
        if name != "_long_wgrad_run":
            return call()
        with pytest.raises(_ReachedLaunch):
            call()
        return seen.get("found", "plan")

    monkeypatch.setattr(F_.torch.cuda, "device", Guard)
    monkeypatch.setattr(_native, "lookup_plan", lambda index, key: None)
    monkeypatch.setattr(_native, "get_plan", fake_get_plan)
    assert run() == "plan"
    assert seen["guards"] == [1] and seen["created"][0] == 1 and seen["created"][2]
    assert tag is None or seen["created"][1] == tag
    # a cached plan: looked up under the tensors' ordinal, no device switch, nothing created
    seen.clear()
    seen["guards"] = []

    def hit(index, key):
        seen["found"] = ("cached", index)
        return seen["found"]
    monkeypatch.setattr(_native, "lookup_plan", hit)
    assert run() == ("cached", 1)
    assert seen["guards"] == [] and "created" not in seen
