"""complex64 tensors through 2-D / 3-D ``fft_conv`` / ``fft_conv_transpose`` and their modules: the complex builds of the
two row passes (csrc/nd_passes.hpp, rows_c2c_fwd_kernel / rows_c2c_inv_kernel), complex plans (fc_debug_route kind
"c64_nd"), the gradients in PyTorch's convention.

Inputs are the integers of tests/accuracy_util.py in both classes, the truth is the exact complex128 direct convolution
(computed on the CPU and verified against explicit dot products), the baseline is ``accuracy_util.baseline`` in complex64
on the device (on the CPU where the device's FFT library fails it, ``_baseline``), and the bound is ``accuracy_util.check`` with the standard margins.  The cases (tests/nd_complex_util.py)
are the smallest shapes at which each mechanism can go wrong; each asserts its route."""
import functools

import pytest
import torch

from fft_conv_pytorch_amd import FFTConv2d, FFTConv3d, FFTConvTranspose2d, FFTConvTranspose3d, _native, autograd
from fft_conv_pytorch_amd import functional as F_
from fft_conv_pytorch_amd.functional import fft_conv, fft_conv_transpose
from tests import accuracy_util as au
from tests import guard_util as gu
from tests import nd_complex_util as ncu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
C64, C128 = torch.complex64, torch.complex128


def _clear():
    _native.clear_plan_cache()
    autograd._BWD_PLANS.clear()


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    """Knobs are read at plan creation and are not part of a cache key: none set on entry, no plan outlives the test."""
    for k in ncu.KNOBS:
        monkeypatch.delenv(k, raising=False)
    _clear()
    yield
    _clear()


def _set(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _clear()


def _op(c):
    op = fft_conv_transpose if c.tr else fft_conv
    return lambda x, w, b: op(x, w, b, **ncu.kw(c))


def _plan_of(c, x, w, b):
    k = ncu.kw(c)
    return F_._plan_for(x, w, b, k["stride"], k["padding"], k["dilation"], c.g, "constant" if c.tr else c.mode,
                        transposed=c.tr, output_padding=k.get("output_padding", 0))


def _assert_route(name, c, pred, x, w, b):
    r = _plan_of(c, x, w, b).route
    assert r["kind"] == "c64_nd" and r["planes"] == 0 and r["nseg0"] == r["nseg1"] == 1, f"{name}: {r}"
    assert pred is None or pred(r), f"{name}: case not on the route it was sized for: {r}"
    return r


@functools.lru_cache(maxsize=None)
def _cpu(name, cls):
    """(x, w, b) in complex64 on the CPU and the exact complex128 truth (shared, never written)."""
    c = ncu.CASES[name][0]
    au.assert_exact(c, cls, complex_=True)
    x, w, b = au.inputs(c, cls, complex_=True)
    return x, w, b, au.truth(c, x, w, b)


BASELINE_BROKEN = 1e-3      # e_rms no complex64 FFT formulation has: the device's FFT library returned something else


def _baseline(c, x, w, b, want):
    """``accuracy_util.baseline`` in complex64 on the tensors' device.  Where that result is not a convolution at all (the
    device FFT library's 3-D real transforms at some of these sizes: e_rms 0.5 and more against the truth, which would make
    the bound vacuous) the same formulation runs in complex64 on the CPU instead, as ``accuracy_util.truth`` replaces a device
    convolution that fails its check."""
    base = au.baseline(c, x, w, b)
    if not au.e_rms(base, want) <= BASELINE_BROKEN:      # (not `>`: such a result may hold NaN)
        print(f"    (device baseline off by e_rms {au.e_rms(base, want):.2e}: the CPU's complex64 baseline stands in)")
        base = au.baseline(c, x.cpu(), w.cpu(), None if b is None else b.cpu())
        assert au.e_rms(base, want) < BASELINE_BROKEN
    return base


def _baseline_grads(c, x, w, b, gy, want_y):
    out = au.baseline_grads(c, x, w, b, gy)
    if not au.e_rms(out[0], want_y) <= BASELINE_BROKEN:
        print(f"    (device baseline off by e_rms {au.e_rms(out[0], want_y):.2e}: the CPU's complex64 baseline stands in)")
        out = au.baseline_grads(c, x.cpu(), w.cpu(), b.cpu(), gy.cpu())
        assert au.e_rms(out[0], want_y) < BASELINE_BROKEN
    return out


# ------------------------------------------------------------------------------------------------ forward, transposed
@pytest.mark.parametrize("cls,name", [(cls, name) for name in ncu.CASES for cls in au.CLASSES
                                      if cls == "offset" or name not in ncu.ROW_LENGTHS])
def test_forward_against_exact_truth(name, cls, monkeypatch):
    c, pred = ncu.CASES[name]
    _set(monkeypatch, c.env)
    xc, wc, bc, want = _cpu(name, cls)
    x, w, b = (t.to(DEV) for t in (xc, wc, bc))
    r = _assert_route(name, c, pred, x, w, b)
    got = _op(c)(x, w, b)
    assert got.dtype == C64 and got.is_contiguous() and got.shape == want.shape
    print(f"\n{name} ({cls}) {r}")
    au.check(f"{name} y", got, want, _baseline(c, x, w, b, want), C64)
    # without a bias: another plan key, no bias read
    plain = want - bc.to(C128).reshape(1, -1, *([1] * c.nd))
    au.check(f"{name} y, no bias", _op(c)(x, w, None), plain, _baseline(c, x, w, None, plain), C64)


@pytest.mark.parametrize("taps,signal", [("imaginary", "real"), ("real", "imaginary")])
def test_purely_imaginary_operands_keep_their_sign(taps, signal):
    """Taps purely imaginary on a real-valued complex signal, and the reverse: a wrong conjugation shows as a sign error of
    the whole result."""
    c = ncu.CASES["one-tile"][0]
    xc, wc, _, _ = _cpu("one-tile", "centred")
    part = lambda t, which: torch.complex(t.real, torch.zeros_like(t.real)) if which == "real" else torch.complex(torch.zeros_like(t.real), t.real)  # noqa: E731
    xc, wc = part(xc, signal), part(wc, taps)
    want = au.direct(c, xc, wc, None)
    assert au.is_whole(want) and want.real.abs().max() == 0 and want.imag.abs().max() > 0
    x, w = xc.to(DEV), wc.to(DEV)
    au.check(f"{taps} taps on a {signal} signal", _op(c)(x, w, None), want, _baseline(c, x, w, None, want), C64)


# ------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("name", ncu.TRAINING)
def test_training_step_against_exact_autograd(name, monkeypatch):
    c, pred = ncu.CASES[name]
    _set(monkeypatch, c.env)
    xc, wc, bc, want = _cpu(name, "centred")
    gyc = au.grad_output(want.shape, C64)
    want_g = au.truth_grads(c, xc, wc, bc, gyc)
    x, w, b = (t.to(DEV).requires_grad_() for t in (xc, wc, bc))
    gy = gyc.to(DEV)
    y = _op(c)(x, w, b)
    y.backward(gy)
    by, bdx, bdw, bdb = _baseline_grads(c, x.detach(), w.detach(), b.detach(), gy, want)
    print()
    au.check(f"{name} y", y.detach(), want, by, C64)
    for what, got, ref, base in (("dX", x.grad, want_g[0], bdx), ("dW", w.grad, want_g[1], bdw), ("db", b.grad, want_g[2], bdb)):
        assert got.dtype == C64 and got.shape == ref.shape, what
        au.check(f"{name} {what}", got, ref, base, C64)
    # a real loss: against complex128 autograd on the CPU (abs() divides: that reference is not whole, it is exact to
    # complex128 rounding), the baseline differentiated the same way
    x2, w2, b2 = (t.to(DEV).requires_grad_() for t in (xc, wc, bc))
    _op(c)(x2, w2, b2).abs().square().sum().backward()
    xs, ws, bs = (t.to(C128).requires_grad_() for t in (xc, wc, bc))
    au.direct(c, xs, ws, bs).abs().square().sum().backward()
    dev = DEV if au.e_rms(au.baseline(c, x.detach(), w.detach(), b.detach()), want) < BASELINE_BROKEN else "cpu"
    xb, wb, bb = (t.to(dev).requires_grad_() for t in (xc, wc, bc))
    au.baseline(c, xb, wb, bb).abs().square().sum().backward()
    for what, got, ref, base in (("dX", x2.grad, xs.grad, xb.grad), ("dW", w2.grad, ws.grad, wb.grad), ("db", b2.grad, bs.grad, bb.grad)):
        au.check(f"{name} real loss {what}", got, ref, base, C64)


# ------------------------------------------------------------------------------------------------ bit-for-bit relations
def test_relations_that_hold_bit_for_bit():
    c = ncu.CASES["reflect"][0]
    xc, wc, bc, _ = _cpu("reflect", "centred")
    x, w, b = (t.to(DEV) for t in (xc, wc, bc))
    first = _op(c)(x, w, b)
    gu.same_bits(_op(c)(x, w, b), first, "two runs of the same call")
    lazy = x.conj()
    assert lazy.is_conj()
    gu.same_bits(_op(c)(lazy, w, b), _op(c)(lazy.resolve_conj(), w, b), "a lazy conjugate against its resolved copy")
    gu.same_bits(_op(c)(x, w.conj(), b.conj()), _op(c)(x, w.conj().resolve_conj(), b.conj().resolve_conj()),
                 "lazily conjugated taps and bias")
    assert not torch.equal(torch.view_as_real(_op(c)(lazy.resolve_conj(), w, b)), torch.view_as_real(first))


# ------------------------------------------------------------------------------------------------ modules
def _layer(cls, *args, **kw):
    torch.manual_seed(0)
    return cls(*args, **kw)


def test_module_against_the_functional_and_its_spectrum_cache():
    xc, _, _, _ = _cpu("one-tile", "centred")
    x = xc.to(DEV)
    layer = _layer(FFTConv2d, 3, 4, (5, 7), padding=(2, 3), dtype=C64).to(DEV).eval()
    assert layer.weight.dtype == C64 and layer.bias.dtype == C64
    want = fft_conv(x, layer.weight.detach(), layer.bias.detach(), padding=(2, 3))
    gu.same_bits(layer(x).detach(), want, "module against the functional")
    cached = layer.__dict__["_spectrum_cache"][1]
    gu.same_bits(layer(x).detach(), want, "cached-spectrum call")
    assert layer.__dict__["_spectrum_cache"][1] is cached and cached.plan.route["kind"] == "c64_nd"
    with torch.no_grad():
        layer.weight.mul_(2)                                  # a weight update: the version counter moves
    got = layer(x).detach()
    assert layer.__dict__["_spectrum_cache"][1] is not cached
    gu.same_bits(got, fft_conv(x, layer.weight.detach(), layer.bias.detach(), padding=(2, 3)), "after a weight update")
    # a training call transforms per call and trains
    layer.train()
    layer(x).abs().square().sum().backward()
    assert layer.weight.grad.dtype == C64 and layer.bias.grad.dtype == C64 and "_spectrum_cache" not in layer.__dict__
    # state_dict round-trips into a fresh complex module, and into torch's own
    other = FFTConv2d(3, 4, (5, 7), padding=(2, 3), dtype=C64).to(DEV).eval()
    other.load_state_dict(layer.state_dict())
    gu.same_bits(other(x).detach(), layer.eval()(x).detach(), "state_dict round trip")
    ref = torch.nn.Conv2d(3, 4, (5, 7), padding=(2, 3), dtype=C64)
    ref.load_state_dict({k: v.cpu() for k, v in layer.state_dict().items()})


def test_module_converted_with_to_complex64():
    xc, _, _, _ = _cpu("one-tile", "centred")
    x = xc.to(DEV)
    layer = _layer(FFTConv2d, 3, 4, (5, 7), padding=(2, 3)).to(DEV).eval()
    real = layer(x.real.contiguous())                          # a float32 call first: its plan and spectrum are dropped
    layer = layer.to(C64)
    assert layer.weight.dtype == C64 and "_spectrum_cache" not in layer.__dict__
    got = layer(x).detach()
    gu.same_bits(got, fft_conv(x, layer.weight.detach(), layer.bias.detach(), padding=(2, 3)), "after .to(complex64)")
    # real weights on a real-valued complex signal: the float32 layer's values
    zero_imag = torch.complex(x.real, torch.zeros_like(x.real))
    assert au.e_max(layer(zero_imag).detach().real, real.detach()) < 1e-5


@pytest.mark.parametrize("cls,args,kw,shape", [
    (FFTConv3d, (2, 3, (3, 5, 7)), dict(padding=1), (1, 2, 10, 20, 70)),
    (FFTConvTranspose2d, (4, 6, (4, 5)), dict(stride=(2, 3), padding=(1, 2), output_padding=(1, 0), dilation=(1, 2), groups=2), (2, 4, 19, 23)),
    (FFTConvTranspose3d, (2, 2, 3), dict(stride=2), (1, 2, 5, 7, 9)),
], ids=["conv3d", "transpose2d", "transpose3d"])
def test_other_modules_against_the_functional(cls, args, kw, shape):
    layer = _layer(cls, *args, dtype=C64, **kw).to(DEV).eval()
    x = au.integers(shape, torch.Generator().manual_seed(1), C64, DEV)
    op = fft_conv_transpose if "Transpose" in cls.__name__ else fft_conv
    want = op(x, layer.weight.detach(), layer.bias.detach(), **kw)
    gu.same_bits(layer(x).detach(), want, "module against the functional")
    gu.same_bits(layer(x).detach(), want, "cached-spectrum call")
    assert layer.__dict__["_spectrum_cache"][1].plan.route["kind"] == "c64_nd"


# ------------------------------------------------------------------------------------------------ memory discipline
RUNS = (0x00, 0xFF, 0x7F, 0x00)


def _runs(op, inputs, what):
    """``op(*inputs)`` once per pattern with the inputs in guarded blocks and every torch.empty of the call guarded and filled
    with the pattern: no guard byte and no input changes, every run has the bits of the first.  Returns the first run."""
    first = None
    for n, pattern in enumerate(RUNS):
        pairs = [gu.guarded(t, pattern) for t in inputs]
        with gu.guarded_empty(pattern) as ge:
            out = op(*(p[0] for p in pairs))
        out = tuple(out) if isinstance(out, (tuple, list)) else (out,)
        tag = f"{what}, run {n} ({pattern:#04x})"
        assert ge.served, f"{tag}: no buffer came from the guarded allocator"
        assert ge.violations() == [], f"{tag}: guard bytes of a library buffer changed: {ge.violations()}"
        for i, (_, check) in enumerate(pairs):
            assert check() == [], f"{tag}: input {i} or its guards changed: {check()}"
        if first is None:
            first = out
        else:
            for j, (a, b) in enumerate(zip(out, first)):
                gu.same_bits(a, b, f"{tag}, output {j} against the first run")
    return first


@pytest.mark.parametrize("name", ["one-tile", "x-tiles", "3d", "rows-1024", "rows-4096"])
def test_memory_discipline_forward(name, monkeypatch):
    c, pred = ncu.CASES[name]
    _set(monkeypatch, c.env)
    xc, wc, bc, want = _cpu(name, "centred")
    x, w, b = (t.to(DEV) for t in (xc, wc, bc))
    _assert_route(name, c, pred, x, w, b)
    (y,) = _runs(_op(c), (x, w, b), name)
    au.check(f"{name} first guarded run", y, want, _baseline(c, x, w, b, want), C64)


def test_memory_discipline_training_step():
    c = ncu.CASES["reflect"][0]
    xc, wc, bc, want = _cpu("reflect", "centred")
    gy = au.grad_output(want.shape, C64, DEV)

    def step(x, w, b, g):
        x, w, b = (t.detach().requires_grad_() for t in (x, w, b))
        y = _op(c)(x, w, b)
        y.backward(g)
        return y.detach(), x.grad, w.grad, b.grad
    y, dx, dw, db = _runs(step, tuple(t.to(DEV) for t in (xc, wc, bc)) + (gy,), "training step")
    ref = au.truth_grads(c, xc, wc, bc, gy.cpu())
    base = _baseline_grads(c, xc.to(DEV), wc.to(DEV), bc.to(DEV), gy, want)
    for what, got, r, bs in (("y", y, want, base[0]), ("dX", dx, ref[0], base[1]), ("dW", dw, ref[1], base[2]), ("db", db, ref[2], base[3])):
        au.check(f"guarded training step {what}", got, r, bs, C64)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(monkeypatch):
    xc, wc, bc, _ = _cpu("one-tile", "centred")
    x, w, b = (t.to(DEV) for t in (xc, wc, bc))
    wide = lambda t: t.to(C128)      # noqa: E731
    real = lambda t: t.real.contiguous()      # noqa: E731
    for args in ((wide(x), wide(w), wide(b)), (x, wide(w), b), (x, real(w), b), (real(x), w, b), (x, w, real(b)),
                 (real(x), real(w), b)):
        with pytest.raises(TypeError, match="must share"):
            fft_conv(*args, padding=(2, 3))
    wt = w.transpose(0, 1).contiguous()
    for args in ((wide(x), wide(wt), wide(b)), (x, real(wt), b), (real(x), wt, b)):
        with pytest.raises(TypeError, match="must share"):
            fft_conv_transpose(*args)
    with pytest.raises(TypeError, match="fft_long_conv"):     # 1-D complex rows have another home
        fft_conv(x[:, :, 0], w[:, :, 0], b, padding=3)
    with pytest.raises(ValueError, match="channel mismatch"):
        fft_conv(x[:, :2], w, b)
    # segments of taps: the accumulating store is float32-only
    _set(monkeypatch, {"FFTCONV_NDSEG": "4"})
    with pytest.raises(NotImplementedError, match="segments"):
        fft_conv(x, w, b, padding=(2, 3))
    gu.same_bits(fft_conv(real(x), real(w), real(b), padding=(2, 3)), fft_conv(real(x), real(w), real(b), padding=(2, 3)),
                 "the float32 call runs in segments as ever")
    monkeypatch.delenv("FFTCONV_NDSEG")
    _clear()
    # the C ABI: no 1-D complex descriptor, no complex fc_wgrad_nd
    key = (1, 2, 2, 2, 1, (500,), (9,), (1,), (0,), (1,), 0, False, 0, False, (0,), _native.FC_C64)
    with pytest.raises(NotImplementedError, match="long-filter"):
        _native.Plan(key)
    desc = _native.conv_desc(2, 2, 3, 4, 1, (37, 50), (5, 7), (1, 1), (2, 3), (1, 1), 0, _native.FC_C64)
    with pytest.raises(NotImplementedError, match="complex64"):
        _native.WgradPlan(desc)
