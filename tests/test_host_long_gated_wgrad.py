"""``fc_long_wgrad_gated`` and the weight gradient of ``fft_long_conv_gated`` without a GPU: header, ctypes table and
library export of the new call, its null-argument answer, the table of ``_long_gated_dw_route``, and the plan lookup of
``_long_wgrad_run`` with gates (the fake tensors of tests/test_host_dispatch.py, which stop the call at its launch)."""
import ctypes
import os
import re

import pytest
import torch

from fft_conv_pytorch_amd import _native
from fft_conv_pytorch_amd import functional as F_
from tests.test_host_dispatch import _FakeCudaTensor, _ReachedLaunch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, BF16, C64 = torch.float32, torch.float16, torch.bfloat16, torch.complex64
KNOBS = ("FFTCONV_LONG_WGRAD", "FFTCONV_LONG_DECIM", "FFTCONV_LONG_NLC", "FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB",
         "FFTCONV_HALF_IO")


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------ header, table, library
PARAMS = ["const fc_long_wgrad_plan* plan", "const void* x", "const void* pregate", "int x_dtype", "int x_layout",
          "const void* dy", "const void* postgate", "int dy_dtype", "int dy_layout", "void* dw", "int dw_dtype",
          "void* workspace", "void* hip_stream"]


def test_header_table_and_library_carry_the_call():
    header = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    found = re.search(r"int fc_long_wgrad_gated\((.*?)\);", header, re.S)
    assert found, "include/fftconv_amd.h does not declare fc_long_wgrad_gated"
    params = [" ".join(p.split()) for p in found.group(1).split(",")]
    assert params == PARAMS and len(params) == 13
    # declared in the section of the weight-gradient plan, behind fc_long_wgrad
    section = header.index("Weight gradient of a long plan")
    assert section < header.index("int fc_long_wgrad(") < found.start() < header.index("Channels-last tensors of the 2-D / 3-D plans")
    # the table: right behind fc_long_wgrad, and the last export is still the gated forward
    at = _native.EXPORTS.index("fc_long_wgrad")
    assert _native.EXPORTS[at + 1] == "fc_long_wgrad_gated"
    assert _native.EXPORTS[-1] == "fc_long_forward_gated"
    assert set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", header)) == set(_native.EXPORTS)
    restype, argtypes = _native.SIGNATURES["fc_long_wgrad_gated"]
    assert restype is ctypes.c_int and len(argtypes) == len(params)
    for a, p in zip(argtypes, params):
        assert a is (ctypes.c_void_p if "*" in p else ctypes.c_int), p
    # nothing that existed moved: the ungated call keeps its eleven arguments
    assert len(_native.SIGNATURES["fc_long_wgrad"][1]) == 11
    lib = _native.load_library()
    assert hasattr(lib, "fc_long_wgrad_gated")
    fn = lib.fc_long_wgrad_gated
    assert fn.restype is restype and tuple(fn.argtypes) == tuple(argtypes)
    m = re.search(r"#define\s+FC_ABI_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == 7 == _native.ABI_VERSION == lib.fc_version()
    assert _native._PLAN_TAGS == {"long": _native.LongPlan, "long_phases": _native.LongPhasesPlan,
                                  "long_decim": _native.LongDecimPlan, "long_wgrad": _native.LongWgradPlan}
    assert "fc_long_wgrad_gated" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_null_arguments_are_refused_without_a_device(monkeypatch):
    import torch.cuda
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    lib = _native.load_library()
    assert lib.fc_long_wgrad_gated(None, None, None, 0, 0, None, None, 0, 0, None, 0, None, None) == _native.FC_ERR_INVALID
    assert b"null argument" in lib.fc_last_error()


# ------------------------------------------------------------------------------------------------ the route of dW
BASE = dict(signal_shape=(3, 5, 2500), kernel_shape=(5, 1, 2500), groups=5, causal=True)
CASE2B = dict(signal_shape=(2, 6, 4000), kernel_shape=(4, 3, 2401), padding=400, groups=2)
INELIGIBLE = {
    "complex64": dict(dtype=C64),
    "stride 2": dict(stride=2),
    "dilation 2": dict(dilation=2),
    "reflect": dict(causal=False, padding=1000, padding_mode="reflect"),
    "channels_last result": dict(channels_last=True),
    "channels-last signal": dict(x_layout="nlc"),
    "hand-off row": dict(signal_shape=(3, 5, 1000), kernel_shape=(5, 1, 1000)),
}
# 16 x 16 rows of 8192 points are 16 MiB of W2: above a budget of 1 MiB, so the library refuses the geometry
WIDE = dict(signal_shape=(2, 16, 5000), kernel_shape=(16, 16, 301), padding=150)


def _route(**kw):
    return F_._long_gated_dw_route(**{**BASE, **kw})


def test_the_route_of_the_weight_gradient(monkeypatch):
    import torch.cuda
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    fused = [dict(dtype=d) for d in (F32, F16, BF16)] + [dict(CASE2B, causal=False, dtype=d) for d in (F32, F16, BF16)]
    others = list(INELIGIBLE.values()) + [dict(WIDE, groups=1, causal=False)]
    for value in (None, "0", "", "yes"):      # the switch unset (or anything but "1"): the products, whatever the call
        if value is not None:
            monkeypatch.setenv("FFTCONV_LONG_WGRAD", value)
        for kw in fused + others:
            assert _route(**kw) == "products", (value, kw)
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    for kw in fused:
        assert F_._long_gated_route(**{**BASE, **kw}) == "fused"
        assert _route(**kw) == "gated-plan", kw
    for name, kw in INELIGIBLE.items():
        assert F_._long_gated_route(**{**BASE, **kw}) == "composed", name
        assert _route(**kw) == "products", name
    # a fused call whose weight-gradient geometry the library refuses
    wide = dict(WIDE, groups=1, causal=False)
    assert _route(**wide) == "gated-plan"
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "1")
    assert F_._long_gated_route(**{**BASE, **wide}) == "fused"
    with pytest.raises(NotImplementedError, match=r"16 x 16 rows of 8192 points \(16 MiB\).*budget of 1 MiB"):
        _native.wgrad_geometry(F_._long_wgrad_key(2, 16, 16, 1, 5000, 301, 150, 150, 5000, False, 0, 1, 1))
    assert _route(**wide) == "products"
    # the cast path of 16-bit tensors is no fused call
    monkeypatch.delenv("FFTCONV_LONG_WS_MB")
    monkeypatch.setenv("FFTCONV_HALF_IO", "0")
    assert _route(dtype=BF16) == "products" and _route(dtype=F32) == "gated-plan"


def test_the_route_asks_for_the_key_backward_runs(monkeypatch):
    """The key the route asks the library about is the one ``FFTLongConvGatedFunction.backward`` builds: the forward's
    paddings and output length, mode constant, stride 1, dilation 1."""
    asked = []
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    monkeypatch.setattr(_native, "wgrad_geometry", lambda key: asked.append(key) or {})
    assert _route() == "gated-plan" and F_._long_gated_dw_route(**CASE2B) == "gated-plan"
    assert asked == [F_._long_wgrad_key(3, 5, 5, 5, 2500, 2500, 2499, 0, 2500, True, 0, 1, 1),
                     F_._long_wgrad_key(2, 6, 4, 2, 4000, 2401, 400, 400, 2400, False, 0, 1, 1)]


# ------------------------------------------------------------------------------------------------ the plan lookup
X, DY = _FakeCudaTensor((2, 4, 6000), 1), _FakeCudaTensor((2, 6, 5996), 1)
WKEY = F_._long_wgrad_key(2, 4, 6, 1, 6000, 5, 0, 0, 5996, False, 0, 1, 1)


@pytest.mark.parametrize("gates", ["none", "both", "pregate", "postgate"])
def test_gates_do_not_change_the_plan_that_is_looked_up(gates, monkeypatch):
    class Guard:
        def __init__(self, index):
            self.index = index

        def __enter__(self):
            if not isinstance(self.index, int):
                raise _ReachedLaunch

        def __exit__(self, *a):
            pass

    seen = []
    monkeypatch.setattr(F_.torch.cuda, "device", Guard)
    monkeypatch.setattr(_native, "lookup_plan", lambda index, key: seen.append((index, key)) or "plan")
    monkeypatch.setattr(_native, "get_plan", lambda index, key: pytest.fail("a cached plan is not created again"))
    kw = {}
    if gates in ("both", "pregate"):
        kw["pregate"] = _FakeCudaTensor(X.shape, 1)
    if gates in ("both", "postgate"):
        kw["postgate"] = _FakeCudaTensor(DY.shape, 1)
    with pytest.raises(_ReachedLaunch):
        F_._long_wgrad_run(X, DY, (6, 4, 5), WKEY, F32, **kw)
    assert seen == [(1, ("long_wgrad",) + WKEY)]


def test_a_gate_that_does_not_match_its_tensor_is_refused_before_the_lookup(monkeypatch):
    monkeypatch.setattr(_native, "lookup_plan", lambda index, key: pytest.fail("looked up a plan"))
    for kw in (dict(pregate=_FakeCudaTensor(DY.shape, 1)), dict(postgate=_FakeCudaTensor(X.shape, 1)),
               dict(pregate=_FakeCudaTensor(X.shape, 1, BF16)), dict(postgate=_FakeCudaTensor(DY.shape, 0))):
        with pytest.raises(ValueError, match="a gate of the weight-gradient plan must match its tensor"):
            F_._long_wgrad_run(X, DY, (6, 4, 5), WKEY, F32, **kw)
