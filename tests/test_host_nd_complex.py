"""complex64 2-D / 3-D ``fft_conv`` without a GPU: the mathematics of the complex plan restated in complex128
(tests/nd_complex_util.py) against a direct complex128 convolution, the three gradient constructions of autograd.py
against complex128 autograd, the exactness of the integer inputs of every GPU case, argument checks, and the ABI.

The direct convolution is four real float64 convolutions (``accuracy_util.direct``); the bound is 1e-10 of the result's
maximum: a complex128 FFT of at most 256 points per axis errs by a few 1e-15 of it."""
import ctypes
import os

import pytest
import torch

from fft_conv_pytorch_amd import _native, autograd
from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests import nd_complex_util as ncu

C128 = torch.complex128
TOL = 1e-10


def _close(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype)
    err = (got - want).abs().max().item() / want.abs().max().item()
    assert err <= TOL, f"{what}: {err:.3e} of the maximum"
    return err


def _inputs(name, cls="centred"):
    c = ncu.CASES[name][0]
    return (c,) + tuple(t.to(C128) for t in au.inputs(c, cls, complex_=True))


@pytest.fixture
def backend(monkeypatch):
    autograd._BWD_PLANS.clear()
    yield ncu.Backend().install(monkeypatch)
    autograd._BWD_PLANS.clear()


@pytest.mark.parametrize("name", list(ncu.CASES))
def test_restated_row_passes_give_the_direct_convolution(name):
    c, x, w, b = _inputs(name, "offset")
    print(name, _close(ncu.restated(c, x, w, b), au.direct(c, x, w, b), name))


@pytest.mark.parametrize("taps,signal", [("imaginary", "real"), ("real", "imaginary")])
def test_restatement_keeps_the_sign_of_purely_imaginary_operands(taps, signal):
    """A wrong conjugation flips the sign of the whole result here."""
    c, x, w, b = _inputs("one-tile")
    part = lambda t, which: torch.complex(t.real, torch.zeros_like(t.real)) if which == "real" else torch.complex(torch.zeros_like(t.real), t.real)  # noqa: E731
    x, w = part(x, signal), part(w, taps)
    want = au.direct(c, x, w, None)
    assert want.real.abs().max() == 0 and want.imag.abs().max() > 0
    _close(ncu.restated(c, x, w, None), want, f"{taps} taps, {signal} signal")


@pytest.mark.parametrize("name", ncu.TRAINING)
def test_gradient_constructions_against_complex128_autograd(name, backend):
    """FFTConvFunction / FFTConvTransposeFunction as they are written, the library behind them replaced by the restatement:
    dX against conj(W) (through ``_pad_adjoint`` in the padding modes), dW from conj(x) in the permuted copy, db."""
    c, x, w, b = _inputs(name)
    gy = au.grad_output((c.B, c.cout) + au.out_spatial(c), C128)
    want = au.truth_grads(c, x, w, b, gy)
    xr, wr, br = (t.clone().requires_grad_() for t in (x, w, b))
    op = fft_conv_transpose if c.tr else fft_conv
    y = op(xr, wr, br, **ncu.kw(c))
    _close(y.detach(), au.direct(c, x, w, b), name + " y")
    y.backward(gy)
    for got, ref, what in zip((xr.grad, wr.grad, br.grad), want, ("dX", "dW", "db")):
        _close(got, ref, f"{name} {what}")
    # every plan asked for was a complex one of 2 or 3 axes: dX, dW and the forward
    assert len(backend.plans) == 3 and all(p.dtype == C128 for p in backend.plans)
    # a real loss: the gradient PyTorch's convention defines for it
    xr, wr, br = (t.clone().requires_grad_() for t in (x, w, b))
    op(xr, wr, br, **ncu.kw(c)).abs().square().sum().backward()
    xs, ws, bs = (t.clone().requires_grad_() for t in (x, w, b))
    au.direct(c, xs, ws, bs).abs().square().sum().backward()
    for got, ref, what in zip((xr.grad, wr.grad, br.grad), (xs.grad, ws.grad, bs.grad), ("dX", "dW", "db")):
        _close(got, ref, f"{name} real loss {what}")


@pytest.mark.parametrize("mode", ["reflect", "replicate", "circular"])
def test_pad_adjoint_on_complex_tensors(mode):
    gen = torch.Generator().manual_seed(3)
    x = au.integers((2, 3, 9, 11), gen, C128).requires_grad_()
    g = au.integers((2, 3, 13, 17), gen, C128)
    ncu._pad_planes(x, [3, 3, 2, 2], mode).backward(g)
    got = autograd._pad_adjoint(g, (9, 11), (2, 3), mode)
    assert got.dtype == C128 and torch.equal(got, x.grad)


def test_lazy_conjugates_are_resolved_inside_the_graph(backend):
    c, x, w, b = _inputs("one-tile")
    xr = x.clone().requires_grad_()
    y = fft_conv(xr.conj(), w.conj(), b.conj(), **ncu.kw(c))
    _close(y.detach(), au.direct(c, x.conj().resolve_conj(), w.conj().resolve_conj(), b.conj().resolve_conj()), "conj")
    gy = au.grad_output(y.shape, C128)
    y.backward(gy)
    xs = x.clone().requires_grad_()
    au.direct(c, xs.conj(), w.conj(), b.conj()).backward(gy)
    _close(xr.grad, xs.grad, "dX through the conjugate")


@pytest.mark.parametrize("name", list(ncu.CASES))
@pytest.mark.parametrize("cls", au.CLASSES)
def test_truth_of_every_gpu_case_is_exact(name, cls):
    c = ncu.CASES[name][0]
    assert au.assert_exact(c, cls, complex_=True) == au.exactness_bound(c, cls, complex_=True) < au.EXACT_LIMIT


def test_argument_errors_come_before_the_device_error():
    c, x, w, b = _inputs("one-tile")
    x, w, b = (t.to(torch.complex64) for t in (x, w, b))
    with pytest.raises(ValueError, match="channel mismatch"):
        fft_conv(x[:, :2], w, b, padding=(2, 3))
    with pytest.raises(ValueError, match="bias must have shape"):
        fft_conv(x, w, b[:2], padding=(2, 3))
    with pytest.raises(ValueError, match="padding_mode"):
        fft_conv(x, w, b, padding=(2, 3), padding_mode="mirror")
    with pytest.raises(ValueError, match="zero padding only|channel mismatch"):
        fft_conv_transpose(x, w, b)
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        fft_conv(x, w, b, padding=(2, 3))
    with pytest.raises(RuntimeError, match="ROCm devices only"):
        fft_conv_transpose(x, w.transpose(0, 1).contiguous(), b)
    # the plan key of a complex call carries the complex dtype code; a 1-D complex signal gets none
    assert F_._DTYPE_CODES[torch.complex64] == _native.FC_C64
    assert torch.complex64 in F_._CONV_ND_DTYPES and torch.complex64 not in F_._CONV_DTYPES


def test_library_refuses_what_has_no_complex_plan_before_it_touches_a_device():
    key = (1, 2, 2, 2, 1, (500,), (9,), (1,), (0,), (1,), 0, False, 0, False, (0,), _native.FC_C64)
    with pytest.raises(NotImplementedError, match="long-filter"):
        _native.Plan(key)
    desc = _native.conv_desc(2, 2, 2, 2, 1, (20, 30), (3, 3), (1, 1), (0, 0), (1, 1), 0, _native.FC_C64)
    with pytest.raises(NotImplementedError, match="complex64"):
        _native.WgradPlan(desc)


def test_abi_is_unchanged():
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "fftconv_amd.h")).read()
    assert "#define FC_ABI_VERSION 7\n" in header
    assert _native.ABI_VERSION == 7
    assert ctypes.sizeof(_native.FcDesc) == 8 + 4 * 8 + 5 * 24 + 16 + 24
    assert _native.FC_C64 == 4 and "FC_C64 = 4" in header
    assert _native.ROUTE_KINDS[:6] == ("f32_1d", "f32_nd", "f64_direct", "f64_fft_1d", "f64_fft_nd", "f64_fft_long")
    assert _native.ROUTE_KINDS[6] == "c64_nd" and _native.ROUTE_WORDS["c64_nd"] == _native.ROUTE_WORDS["f32_nd"]
