"""Channels-last tensors through the 2-D / 3-D ``fft_conv`` / ``fft_conv_transpose`` and their modules: a signal that lies
as ``torch.channels_last`` / ``channels_last_3d`` is read where it lies, ``channels_last=True`` has the last pass write y that
way, and backward reads a dY that lies so and writes dX in the signal's layout (csrc/nd_passes.hpp, rows_r2c_cl_kernel and
rows_c2r_cl_kernel).

The yardstick is bits.  The channels-last builds keep the pairing of rows and run the planar builds' register transforms on
the same samples, so every result must equal, bit for bit, the same call on ``.contiguous()`` tensors with
``channels_last=False`` -- the existing path, which has its own tests against the oracle.  A spy on ``Plan.forward_lay``
records the (x_layout, y_layout) of every launch: each case says whether the kernels or torch copies serve its layouts.

Which calls take layouts natively (``functional._nd_cl_native``): a call with ``channels_last=True``, for its signal, its
result and its backward; under FFTCONV_ND_CL=1 every call; under FFTCONV_ND_CL=0 none.  A call without the keyword and
without the knob copies a strided signal as it always did and returns a contiguous dX."""
import copy
import math
import os
import pickle

import pytest
import torch

from fft_conv_pytorch_amd import FFTConv2d, FFTConv3d, FFTConvTranspose2d, _native, autograd, fft_conv
from fft_conv_pytorch_amd import functional as F_
from fft_conv_pytorch_amd.functional import fft_conv_transpose
from tests import guard_util as gu

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF16, C64, F64 = torch.float32, torch.float16, torch.bfloat16, torch.complex64, torch.float64
KNOBS = ("FFTCONV_XTILE", "FFTCONV_YTILE", "FFTCONV_PLANES", "FFTCONV_NDSEG", "FFTCONV_ND_CL", "FFTCONV_HALF_IO", "FFTCONV_TILE")
PL, CL = _native.ND_PLANAR, _native.ND_CHANNELS_LAST
COMBOS = [(False, False), (True, False), (False, True), (True, True)]      # (strided signal, channels_last)
NCH = 4      # channels per workgroup of the channels-last builds (csrc/tile_inst.hip, nch_cl): 4, but 2 in the 16-bit builds
             # at T <= 128, which get a case with exactly two channels of their own (CHANNELS_16)


def _clear():
    _native.clear_plan_cache()
    F_._REFUSED_HALF.clear()
    autograd._BWD_PLANS.clear()


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    _clear()
    yield
    _clear()


@pytest.fixture
def lay(monkeypatch):
    """(x_layout, y_layout) of every ``Plan.forward_lay`` call."""
    calls = []
    real = _native.Plan.forward_lay

    def forward_lay(plan, x_ptr, w_hat_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_layout=PL, y_layout=PL):
        calls.append((x_layout, y_layout))
        return real(plan, x_ptr, w_hat_ptr, bias_ptr, y_ptr, workspace_ptr, stream, x_layout, y_layout)
    monkeypatch.setattr(_native.Plan, "forward_lay", forward_lay)
    return calls


def _randn(shape, dtype, gen):
    if dtype == C64:
        return torch.complex(torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)).to(DEV)
    return torch.randn(shape, generator=gen).to(DEV).to(dtype)


def _tensors(B, cin, cout, g, sp, k, bias, dtype, seed=0, transposed=False):
    """x (B, Cin, *sp) contiguous, weight scaled so that outputs are of order one, bias."""
    gen = torch.Generator().manual_seed(seed + sum(sp) + 3 * sum(k) + 7 * cin)
    x = _randn((B, cin) + tuple(sp), dtype, gen)
    wshape = (cin, cout // g) if transposed else (cout, cin // g)
    w = _randn(wshape + tuple(k), dtype, gen) * (1.0 / math.sqrt(cin // g * math.prod(k)))
    b = _randn((cout,), dtype, gen) if bias else None
    return x, w.to(dtype), b


def _as_cl(t):
    """The values of ``t`` lying channels-last (what ``t.to(memory_format=torch.channels_last)`` gives a 4-D tensor)."""
    out = F_._to_channels_last(t)
    assert F_._nd_layout(out) == "cl" and _lies_cl(out)
    return out


def _lies_cl(t):
    n = t.ndim - 2
    return t.permute((0,) + tuple(range(2, n + 2)) + (1,)).is_contiguous()


def _auto():
    return os.environ.get("FFTCONV_ND_CL") == "1"


def _check_combos(fn, x, what, lay_calls, native=True):
    """``fn(signal, channels_last)`` for the four layout combinations against the contiguous call; ``native``: the kernels
    serve the layouts (one ``forward_lay`` launch with them: the signal's where the call has the keyword or the knob is
    1), else torch copies do (no such launch)."""
    assert x.is_contiguous() and x.shape[1] > 1
    want = fn(x, False)
    assert want.is_contiguous()
    xs = _as_cl(x)
    for strided, cl in COMBOS:
        lay_calls.clear()
        got = fn(xs if strided else x, cl)
        tag = f"{what}: strided signal {strided}, channels_last {cl}"
        if cl:
            assert _lies_cl(got), (tag, got.stride())
        else:
            assert got.is_contiguous(), (tag, got.stride())
        gu.same_bits(got, want, tag)
        x_native = strided and (cl or _auto())
        if native:
            assert lay_calls == ([(CL if x_native else PL, CL if cl else PL)] if (x_native or cl) else []), (tag, lay_calls)
        else:
            assert lay_calls == [], (tag, lay_calls)
    return want


def _route(x, w, b, **kw):
    conf = dict(stride=1, padding=0, dilation=1, groups=1, padding_mode="constant")
    conf.update(kw)
    return F_._plan_for(x, w, b, conf["stride"], conf["padding"], conf["dilation"], conf["groups"], conf["padding_mode"]).route


# ------------------------------------------------------------------------------------------------ forward
# W -> the row transform the planner picks under FFTCONV_XTILE=0 (one tile, no padding: the smallest FFT that holds the row)
ROW_W = {64: 61, 128: 101, 256: 201, 512: 401, 1024: 1001, 2048: 2001, 4096: 4001}
# (Cin, Cout, groups): 3 and NCH + 1 leave a tail block of channels, NCH fills one; dense and depthwise
CHANNELS = [(3, 3, 3), (NCH, NCH, 1), (NCH + 1, NCH + 1, NCH + 1), (NCH + 1, 3, 1)]
# 16-bit: one full block of two (the NCH = 2 builds), a full block of four, five (a tail block for either count), 5 -> 3
CHANNELS_16 = [(2, 2, 1), (NCH, NCH, NCH)] + CHANNELS[2:]


@pytest.mark.parametrize("knob", (None, "1"), ids=("keyword", "FFTCONV_ND_CL=1"))
@pytest.mark.parametrize("dtype", (F32, F16, BF16), ids=str)
@pytest.mark.parametrize("Tx", sorted(ROW_W))
def test_every_row_transform(Tx, dtype, knob, monkeypatch, lay):
    """B 2, H 5 (three row pairs: a last pair without a partner; a partial block of rows), every row transform length.
    64 ... 1024 points are served by the kernels; 2048 and 4096 points have no channels-last build: torch copies.
    Under FFTCONV_ND_CL=1 the call without the keyword reads its strided signal where it lies too."""
    monkeypatch.setenv("FFTCONV_XTILE", "0")
    if knob:
        monkeypatch.setenv("FFTCONV_ND_CL", knob)
    _clear()
    for cin, cout, g in CHANNELS if dtype == F32 else CHANNELS_16:
        x, w, b = _tensors(2, cin, cout, g, (5, ROW_W[Tx]), (3, 3), True, dtype)
        route = _route(x, w, b, groups=g)
        assert (route["Tx"], route["nxt"], route["planes"]) == (Tx, 1, 0), route
        fn = lambda s, cl: fft_conv(s, w, b, groups=g, channels_last=cl)      # noqa: E731
        _check_combos(fn, x, f"Tx {Tx} {cin}->{cout} g{g} {dtype}", lay, native=Tx <= 1024)


@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
@pytest.mark.parametrize("Tx", (64, 128, 1024))
def test_row_major_pipeline(Tx, dtype, monkeypatch, lay):
    """``planes`` 2 (FFTCONV_PLANES=2): the row passes keep the rows as they are -- the other store / load mode."""
    monkeypatch.setenv("FFTCONV_XTILE", "0")
    monkeypatch.setenv("FFTCONV_PLANES", "2")
    _clear()
    for cin, cout in ((NCH + 1, NCH + 1), (8, 6)):
        x, w, b = _tensors(2, cin, cout, 1, (5, ROW_W[Tx]), (3, 3), True, dtype)
        route = _route(x, w, b)
        assert (route["Tx"], route["nxt"], route["planes"]) == (Tx, 1, 2), route
        fn = lambda s, cl: fft_conv(s, w, b, channels_last=cl)      # noqa: E731
        _check_combos(fn, x, f"planes 2, Tx {Tx} {cin}->{cout} {dtype}", lay)


@pytest.mark.parametrize("planes", (0, 2))
def test_three_tiles_along_the_rows(planes, monkeypatch, lay):
    monkeypatch.setenv("FFTCONV_XTILE", "64")
    monkeypatch.setenv("FFTCONV_PLANES", str(planes))
    _clear()
    for dtype in (F32, BF16):
        x, w, b = _tensors(2, NCH + 1, NCH + 1, 1, (5, 150), (3, 3), True, dtype)
        route = _route(x, w, b)
        assert (route["Tx"], route["nxt"], route["planes"]) == (64, 3, planes), route
        _check_combos(lambda s, cl: fft_conv(s, w, b, channels_last=cl), x, f"nxt 3 planes {planes} {dtype}", lay)


HYPER = [
    ("reflect", 5, 5, 5, dict(padding=(1, 2), padding_mode="reflect")),
    ("replicate", 5, 3, 1, dict(padding=(2, 1), padding_mode="replicate")),
    ("circular", 3, 3, 3, dict(padding=(1, 2), padding_mode="circular")),
    ("stride (2, 3)", 5, 5, 1, dict(stride=(2, 3), padding=1)),
    ("dilation (2, 1)", 5, 5, 5, dict(dilation=(2, 1), padding=(2, 1))),
    ("groups 2", 4, 6, 2, dict(padding=1)),
]


@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
@pytest.mark.parametrize("name,cin,cout,g,kw", HYPER, ids=[c[0] for c in HYPER])
def test_hyper_parameters(name, cin, cout, g, kw, dtype, monkeypatch, lay):
    monkeypatch.setenv("FFTCONV_XTILE", "0")
    _clear()
    x, w, b = _tensors(2, cin, cout, g, (7, 101), (3, 3), True, dtype)
    assert _route(x, w, b, groups=g, **kw)["Tx"] == 128
    _check_combos(lambda s, cl: fft_conv(s, w, b, groups=g, channels_last=cl, **kw), x, f"{name} {dtype}", lay)


@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
def test_same_padding_with_an_odd_total(dtype, monkeypatch, lay):
    """k = (2, 4): 'same' needs 1 and 3 padded samples, run with 1 and 2 on both sides and the leading output sample
    dropped -- one torch copy either way, which gives the result its layout; the signal is still read where it lies."""
    monkeypatch.setenv("FFTCONV_XTILE", "0")
    _clear()
    x, w, b = _tensors(2, 5, 5, 5, (6, 100), (2, 4), True, dtype)
    fn = lambda s, cl: fft_conv(s, w, b, padding="same", groups=5, channels_last=cl)      # noqa: E731
    want = fn(x, False)
    assert want.shape == x.shape
    xs = _as_cl(x)
    for strided, cl in COMBOS:
        lay.clear()
        got = fn(xs if strided else x, cl)
        assert _lies_cl(got) if cl else got.is_contiguous()
        gu.same_bits(got, want, f"'same' odd {dtype}: strided {strided}, channels_last {cl}")
        assert lay == ([(CL if strided else PL, CL)] if cl else []), lay


@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
def test_transposed_convolution(dtype, monkeypatch, lay):
    monkeypatch.setenv("FFTCONV_XTILE", "0")
    _clear()
    x, w, b = _tensors(2, 5, 6, 1, (4, 45), (3, 3), True, dtype, transposed=True)
    kw = dict(stride=2, padding=1, output_padding=1)
    plan = F_._plan_for(x, w, b, 2, 1, 1, 1, "constant", transposed=True, output_padding=1)
    assert plan.route["Tx"] == 128 and plan.out_spatial == (8, 90)
    _check_combos(lambda s, cl: fft_conv_transpose(s, w, b, channels_last=cl, **kw), x, f"transposed {dtype}", lay)


# ------------------------------------------------------------------------------------------------ 3-D
@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
def test_3d_separable_plan_is_native(dtype, monkeypatch, lay):
    monkeypatch.setenv("FFTCONV_PLANES", "0")
    _clear()
    x, w, b = _tensors(2, 5, 5, 1, (3, 5, 61), (2, 3, 3), True, dtype)
    route = _route(x, w, b)
    assert (route["planes"], route["Tx"]) == (0, 64), route
    _check_combos(lambda s, cl: fft_conv(s, w, b, channels_last=cl), x, f"3-D separable {dtype}", lay)


def test_3d_plane_major_plan_copies(lay):
    x, w, b = _tensors(2, 8, 8, 1, (3, 5, 61), (2, 3, 3), True, F32)
    plan = F_._plan_for(x, w, b, 1, 0, 1, 1, "constant")
    assert plan.route["planes"] == 1
    assert "plane-major" in plan.takes_layout(CL, PL) and "plane-major" in plan.takes_layout(PL, CL)
    _check_combos(lambda s, cl: fft_conv(s, w, b, channels_last=cl), x, "3-D plane-major", lay, native=False)


# ------------------------------------------------------------------------------------------------ expected copies
def test_layouts_the_library_does_not_take_keep_values_and_strides(monkeypatch, lay):
    fn = lambda x, w, b: (lambda s, cl: fft_conv(s, w, b, padding=1, channels_last=cl))      # noqa: E731
    # segments of taps
    monkeypatch.setenv("FFTCONV_NDSEG", "2")
    _clear()
    x, w, b = _tensors(2, 5, 5, 1, (5, 61), (3, 3), True, F32)
    plan = F_._plan_for(x, w, b, 1, 1, 1, 1, "constant")
    assert plan.route["nseg0"] == 2 and "segments of taps" in plan.takes_layout(CL, CL)
    _check_combos(fn(x, w, b), x, "segments of taps", lay, native=False)
    monkeypatch.delenv("FFTCONV_NDSEG")
    _clear()
    # complex64 and float64
    for dtype, word in ((C64, "complex64"), (F64, "float64")):
        x, w, b = _tensors(2, 5, 5, 1, (5, 61), (3, 3), True, dtype)
        plan = F_._plan_for(x, w, b, 1, 1, 1, 1, "constant")
        assert word in plan.takes_layout(CL, PL) and word in plan.takes_layout(PL, CL)
        _check_combos(fn(x, w, b), x, word, lay, native=False)
    # the knob
    for dtype in (F32, BF16):
        x, w, b = _tensors(2, 5, 5, 1, (5, 61), (3, 3), True, dtype)
        want = _check_combos(fn(x, w, b), x, f"native {dtype}", lay)
        monkeypatch.setenv("FFTCONV_ND_CL", "0")
        gu.same_bits(_check_combos(fn(x, w, b), x, f"FFTCONV_ND_CL=0 {dtype}", lay, native=False), want, "knob")
        monkeypatch.delenv("FFTCONV_ND_CL")


# ------------------------------------------------------------------------------------------------ storage offset
@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
def test_signal_at_a_storage_offset(dtype, monkeypatch, lay):
    B, C, H, W = 2, 5, 5, 101
    big, w, b = _tensors(B + 1, C, C, C, (H, W), (3, 3), True, dtype)
    bigs = _as_cl(big)
    x = bigs[1:]
    assert x.storage_offset() == C * H * W and F_._nd_layout(x) == "cl"
    want = fft_conv(x.contiguous(), w, b, groups=C)
    before = bigs.clone()
    got = fft_conv(x, w, b, groups=C, channels_last=True)
    assert lay == [(CL, CL)]
    gu.same_bits(got, want, f"storage offset {dtype}")
    gu.same_bits(bigs, before, "the buffer the signal is a view of")
    # an offset that is only element-aligned (a call without the keyword: read where it lies under the knob)
    monkeypatch.setenv("FFTCONV_ND_CL", "1")
    flat = torch.zeros(B * C * H * W + 1, dtype=dtype, device=DEV)
    flat[1:] = x.permute(0, 2, 3, 1).reshape(-1)
    odd = flat[1:].view(B, H, W, C).permute(0, 3, 1, 2)
    assert F_._nd_layout(odd) == "cl" and odd.data_ptr() % (2 * odd.element_size()) != 0
    gu.same_bits(fft_conv(odd, w, b, groups=C), want, f"odd storage offset {dtype}")
    assert lay[-1] == (CL, PL)


# ------------------------------------------------------------------------------------------------ gradients
def _step(fn, x, w, b, cl, gy=None, downstream=None):
    """One training step on leaves with the strides of ``x`` -> (y, dX, dW, db, the dY that reached the function)."""
    xs = x.detach().clone(memory_format=torch.preserve_format).requires_grad_()
    assert xs.stride() == x.stride()
    ws, bs = w.detach().clone().requires_grad_(), b.detach().clone().requires_grad_()
    y = fn(xs, ws, bs, cl)
    seen = []
    y.register_hook(seen.append)
    if downstream is not None:
        M, G = downstream
        n = y.ndim - 2
        (y.permute((0,) + tuple(range(2, n + 2)) + (1,)) @ M).backward(G)
    else:
        y.backward(gy)
    torch.cuda.synchronize()
    return y.detach(), xs.grad, ws.grad, bs.grad, seen[0]


GRAD = [
    ("conv zeros", False, dict(padding=1)),
    ("conv reflect", False, dict(padding=(1, 2), padding_mode="reflect")),
    ("conv strided", False, dict(stride=(2, 1), padding=1)),
    ("transposed", True, dict(stride=2, padding=1, output_padding=1)),
]


@pytest.mark.parametrize("knob", (None, "1"), ids=("keyword", "FFTCONV_ND_CL=1"))
@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
@pytest.mark.parametrize("name,transposed,kw", GRAD, ids=[c[0] for c in GRAD])
def test_gradient_bits_and_strides_with_dy_from_a_downstream_matmul(name, transposed, kw, dtype, knob, monkeypatch, lay):
    """y, dX, dW and db of a step whose dY is delivered channels-last by a matmul over the channels: the bits of the step on
    contiguous tensors with that dY's contiguous copy; dW and db are contiguous.  A call that takes layouts natively (the
    keyword, or the knob): dX has the signal's strides, and with zero padding the forward and the dX launch are the first
    two launches and both take the layouts as they lie.  A call without keyword and knob launches nothing by layout and
    returns a contiguous dX, as ever."""
    monkeypatch.setenv("FFTCONV_XTILE", "0")
    if knob:
        monkeypatch.setenv("FFTCONV_ND_CL", knob)
    _clear()
    B, cin, cout, g = 2, 5, 6, 1
    x, w, b = _tensors(B, cin, cout, g, (6, 45), (3, 3), True, dtype, transposed=transposed)
    op = fft_conv_transpose if transposed else fft_conv
    fn = lambda s, ww, bb, cl: op(s, ww, bb, groups=g, channels_last=cl, **kw)      # noqa: E731
    with torch.no_grad():
        shape = fn(x, w, b, False).shape
    gen = torch.Generator().manual_seed(2)
    M, G = _randn((cout, 7), dtype, gen), _randn((shape[0],) + tuple(shape[2:]) + (7,), dtype, gen)
    xs = _as_cl(x)
    zeros = kw.get("padding_mode", "constant") == "constant"
    for strided, cl in COMBOS:
        lay.clear()
        xin = xs if strided else x
        got = _step(fn, xin, w, b, cl, downstream=(M, G))
        dy = got[4]
        tag = f"{name} {dtype}: strided signal {strided}, channels_last {cl}"
        assert F_._nd_layout(dy) == "cl", f"{tag}: the matmul's gradient reaches the function channels-last"
        opted = cl or _auto()
        x_lay, y_lay = CL if (strided and opted) else PL, CL if cl else PL
        first = [(x_lay, y_lay)] if (x_lay, y_lay) != (PL, PL) else []
        if not opted:
            assert lay == [], (tag, lay)
        elif zeros:
            assert lay[:2] == first + [(CL, x_lay)], (tag, lay)
        else:      # (dX goes through _pad_adjoint: written planar, one torch copy restores the signal's layout)
            assert lay[:2] == first + [(CL, PL)], (tag, lay)
        lay.clear()
        want = _step(fn, x, w, b, False, gy=dy.contiguous())
        assert lay == []
        for what, a, r in zip(("y", "dX", "dW", "db"), got, want):
            gu.same_bits(a, r, f"{tag}: {what}")
        if opted:      # (otherwise autograd lays the leaf's .grad out as it sees fit: the function returned a contiguous dX)
            assert got[1].stride() == xin.stride(), (tag, got[1].stride())
        assert got[2].is_contiguous() and got[3].is_contiguous()
        assert _lies_cl(got[0]) if cl else got[0].is_contiguous()


def test_backward_under_create_graph_copies_dy_and_keeps_the_bits(lay):
    """A differentiable backward (create_graph with a dY that requires grad) of the transposed layer runs its dX as
    ``FFTConvFunction.apply``, which carries the keyword but not the decision to read dY where it lies: a channels-last dY
    of a planar signal is copied there -- no launch by layout -- and dX has the bits of the plain backward."""
    x, w, b = _tensors(2, 5, 6, 1, (4, 45), (3, 3), True, F32, transposed=True)
    kw = dict(stride=2, padding=1, output_padding=1)
    with torch.no_grad():
        shape = fft_conv_transpose(x, w, b, **kw).shape
    gy = _as_cl(_randn(tuple(shape), F32, torch.Generator().manual_seed(5)))

    def dx(create_graph, g):
        xs = x.clone().requires_grad_()
        y = fft_conv_transpose(xs, w, b, channels_last=True, **kw)
        return torch.autograd.grad(y, xs, g, create_graph=create_graph)[0]
    want = dx(False, gy)
    assert lay == [(PL, CL), (CL, PL)], lay
    lay.clear()
    g2 = gy.clone(memory_format=torch.preserve_format).requires_grad_()
    assert F_._nd_layout(g2) == "cl"
    got = dx(True, g2)
    assert got.requires_grad and lay == [(PL, CL)], lay
    gu.same_bits(got.detach(), want, "dX under create_graph")


# ------------------------------------------------------------------------------------------------ modules
@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
def test_module_cache_and_bits(dtype, monkeypatch, lay):
    torch.manual_seed(0)
    layers = [(FFTConv2d(5, 5, 3, padding=1, groups=5, channels_last=True), (5, 61)),
              (FFTConvTranspose2d(5, 6, 3, stride=2, padding=1, output_padding=1, channels_last=True), (4, 45)),
              (FFTConv3d(5, 5, (2, 3, 3), channels_last=True), (3, 5, 61))]
    monkeypatch.setenv("FFTCONV_PLANES", "0")
    _clear()
    for layer, sp in layers:
        layer = layer.to(DEV).to(dtype)
        assert "channels_last=True" in repr(layer) and "channels_last" not in layer.state_dict()
        x = torch.randn((2, 5) + sp, device=DEV).to(dtype)
        xs = _as_cl(x)
        plain = copy.deepcopy(layer)
        plain.channels_last = False
        with torch.no_grad():
            want = plain(x)
        assert want.is_contiguous()
        calls = []
        real = F_.transform_kernel
        monkeypatch.setattr(F_, "transform_kernel", lambda plan, kernel: calls.append(kernel.dtype) or real(plan, kernel))
        layer.eval()
        lay.clear()
        with torch.no_grad():
            y1, y2 = layer(xs), layer(xs)
        assert len(calls) == 1, calls                      # one kernel transform for two calls
        assert lay == [(CL, CL)] * 2, lay
        for y in (y1, y2):
            assert _lies_cl(y)
            gu.same_bits(y, want, f"module {type(layer).__name__} {dtype}")
        for other in (copy.deepcopy(layer), pickle.loads(pickle.dumps(layer))):
            assert other.channels_last is True
            with torch.no_grad():
                gu.same_bits(other(xs), want, "copied module")
        layer.train()
        y = layer(xs.detach().clone(memory_format=torch.preserve_format).requires_grad_())
        assert _lies_cl(y)
        gu.same_bits(y.detach(), want, "module in training")
        monkeypatch.setattr(F_, "transform_kernel", real)


# ------------------------------------------------------------------------------------------------ memory discipline
RUNS = (0x00, 0xFF, 0x7F, 0x00)


@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
@pytest.mark.parametrize("planes", (0, 2))
def test_strided_call_and_backward_between_guard_bands(planes, dtype, monkeypatch, lay):
    """Strided in, strided out, forward and backward, every torch.empty poisoned, the caller's tensors between guard bands:
    no byte outside a tensor changes and the runs agree bit for bit, so every sample of y and dX is written.  B 2, 5
    channels, 5 rows: the tail channel block and the row pair without a partner are the cases under guard."""
    monkeypatch.setenv("FFTCONV_XTILE", "0")
    monkeypatch.setenv("FFTCONV_PLANES", str(planes))
    _clear()
    B, C, H, W = 2, 5, 5, 101
    x, w, b = _tensors(B, C, C, 1, (H, W), (3, 3), True, dtype)
    assert _route(x, w, b)["planes"] == planes
    fn = lambda s, ww, bb, cl: fft_conv(s, ww, bb, channels_last=cl)      # noqa: E731
    gy = _randn((B, C, H - 2, W - 2), dtype, torch.Generator().manual_seed(4))
    want = _step(fn, x, w, b, False, gy=gy)[:4]
    u, gyu = x.permute(0, 2, 3, 1).contiguous(), gy.permute(0, 2, 3, 1).contiguous()
    first = None
    for n, pattern in enumerate(RUNS):
        pairs = [gu.guarded(t, pattern) for t in (u, w, b, gyu)]
        ug, wg, bg, gyg = (p[0] for p in pairs)
        lay.clear()
        with gu.guarded_empty(pattern) as ge:
            xs = ug.permute(0, 3, 1, 2).detach().requires_grad_()
            ws, bs = wg.detach().requires_grad_(), bg.detach().requires_grad_()
            y = fft_conv(xs, ws, bs, channels_last=True)
            y.backward(gyg.permute(0, 3, 1, 2))
            out = (y.detach(), xs.grad, ws.grad, bs.grad)
        tag = f"planes {planes} {dtype}, run {n} ({pattern:#04x})"
        assert lay[:2] == [(CL, CL), (CL, CL)], (tag, lay)
        assert ge.served and ge.violations() == [], f"{tag}: guard bytes of a library buffer changed: {ge.violations()}"
        for i, (_, check) in enumerate(pairs):
            assert check() == [], f"{tag}: input {i} or its guards changed: {check()}"
        assert _lies_cl(out[0]) and _lies_cl(out[1])
        for what, a, r in zip(("y", "dX", "dW", "db"), out, want):
            gu.same_bits(a, r, f"{tag}: {what} against the contiguous call")
        if first is None:
            first = out
        for what, a, r in zip(("y", "dX", "dW", "db"), out, first):
            gu.same_bits(a, r, f"{tag}: {what} against the first run")


def _added_peak(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def test_no_hidden_copy(monkeypatch, lay):
    """Derived, not measured: the copy path holds the signal's contiguous copy alive across the launches (and a second y
    while it rearranges the result), the native call allocates y, the workspace and the spectrum and nothing else."""
    B, C, H, W = 2, 32, 32, 64
    gen = torch.Generator(device=DEV).manual_seed(0)
    x = F_._to_channels_last(torch.randn(B, C, H, W, generator=gen, device=DEV))
    w = torch.randn(C, 1, 3, 3, generator=gen, device=DEV) / 3
    b = torch.randn(C, generator=gen, device=DEV)

    def forward():
        with torch.no_grad():
            return fft_conv(x, w, b, padding=1, groups=C, channels_last=True)
    want = forward()                                      # warm: plan and tables
    plan = F_._plan_for(x, w, b, 1, 1, 1, C, "constant")
    assert lay == [(CL, CL)]
    native = _added_peak(forward)
    monkeypatch.setenv("FFTCONV_ND_CL", "0")
    gu.same_bits(forward(), want, "copy path")
    copied = _added_peak(forward)
    monkeypatch.delenv("FFTCONV_ND_CL")
    nbytes = x.numel() * x.element_size()
    bound = want.numel() * want.element_size() + plan.workspace_bytes + plan.spectrum_bytes + 3 * 512
    print(f"B{B} C{C} {H}x{W}: added peak native {native / 2**20:.2f} MiB, copy path {copied / 2**20:.2f} MiB, "
          f"signal {nbytes / 2**20:.2f} MiB, y + workspace + spectrum {bound / 2**20:.2f} MiB")
    assert native <= copied - nbytes
    assert native <= bound


# ------------------------------------------------------------------------------------------------ library
def test_library_answers(monkeypatch):
    monkeypatch.setenv("FFTCONV_XTILE", "0")
    _clear()
    B, C, H, W = 2, 5, 5, 101
    x, w, b = _tensors(B, C, C, 1, (H, W), (3, 3), True, F32)
    plan = F_._plan_for(x, w, b, 1, 0, 1, 1, "constant")
    assert plan.takes_layout(PL, PL) is None and plan.takes_layout(CL, CL) is None
    spectrum = F_.transform_kernel(plan, w)
    ws = F_.new_workspace(plan, x.device)
    u = x.permute(0, 2, 3, 1).contiguous()
    out = torch.empty(B, H - 2, W - 2, C, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream
    args = (u.data_ptr(), spectrum.buf.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), stream)
    for bad in ((7, CL), (CL, -1)):
        with pytest.raises(ValueError, match=f"unknown layout code {[c for c in bad if c not in (PL, CL)][0]}"):
            plan.forward_lay(*args, *bad)
        with pytest.raises(ValueError, match="unknown layout code"):
            plan.takes_layout(*bad)
    plan.forward_lay(*args, CL, CL)
    torch.cuda.synchronize()
    want = fft_conv(x, w, b)
    gu.same_bits(out.permute(0, 3, 1, 2), want, "C level, both channels-last")
    out2 = torch.empty_like(want)
    plan.forward_lay(x.data_ptr(), *args[1:3], out2.data_ptr(), *args[4:], PL, PL)      # both planar: fc_forward
    torch.cuda.synchronize()
    gu.same_bits(out2, want, "C level, both planar")
    # refusals: each with its sentence, from fc_plan_takes_layout and from the launch call alike (nothing is launched)
    monkeypatch.setenv("FFTCONV_XTILE", "0")
    long_x, long_w, _ = _tensors(1, 2, 2, 1, (4, 2001), (3, 3), False, F32)
    p2048 = F_._plan_for(long_x, long_w, None, 1, 0, 1, 1, "constant")
    assert p2048.route["Tx"] == 2048
    assert "2048-point row transform has no channels-last build" in p2048.takes_layout(CL, PL)
    with pytest.raises(NotImplementedError, match="2048-point row transform"):
        p2048.forward_lay(*args, PL, CL)
    x1, w1, _ = _tensors(2, 4, 4, 1, (500,), (5,), False, F32)
    p1d = F_._plan_for(x1, w1, None, 1, 0, 1, 1, "constant")
    assert "1-D plan" in p1d.takes_layout(CL, PL) and "fc_long_forward_lay" in p1d.takes_layout(PL, CL)
    # a channels-last output whose block of rows would pass 2 GiB: refused from the descriptor (no tensor has that size)
    key = (2, 1, 32768, 32768, 32768, (2, 1000), (1, 1), (1, 1), (0, 0), (1, 1), 0, False, 0, False, (0, 0), 0)
    big = _native.get_plan(0, key)
    assert big.takes_layout(CL, PL) is None
    assert "exceed the 2 GiB a workgroup's block of rows may span" in big.takes_layout(PL, CL)
    with pytest.raises(NotImplementedError, match="2 GiB a workgroup's block of rows"):
        big.forward_lay(*args, PL, CL)
    # a channels-last signal is addressed with 32-bit byte offsets from its start: 2^32 - 1 bytes or more are refused, one
    # row less is taken (descriptors only: 1024 channels x 1023 / 1024 rows of 1024 float32 samples, the 4 GiB boundary)
    def plan_of(rows):
        return _native.get_plan(0, (2, 1, 1024, 1024, 1024, (rows, 1024), (1, 1), (1, 1), (0, 0), (1, 1), 0, False, 0, False, (0, 0), 0))
    under, at = plan_of(1023), plan_of(1024)
    assert under.route["Tx"] == at.route["Tx"] == 1024
    assert under.takes_layout(CL, PL) is None and under.takes_layout(CL, CL) is None
    assert 4 * 1024 * 1024 * 1024 == 1 << 32
    assert "a channels-last signal of 4294967296 bytes exceeds the 4 GiB its 32-bit offsets span" in at.takes_layout(CL, PL)
    assert at.takes_layout(PL, CL) is None       # (the guards of x and y are independent)
    with pytest.raises(NotImplementedError, match="exceeds the 4 GiB its 32-bit offsets span"):
        at.forward_lay(*args, CL, PL)
    half = _native.get_plan(0, (2, 1, 1024, 1024, 1024, (2048, 1024), (1, 1), (1, 1), (0, 0), (1, 1), 0, False, 0, False, (0, 0), 3))
    assert "4294967296 bytes" in half.takes_layout(CL, PL)       # bfloat16: twice the rows
    # a weight-gradient plan (fc_wgrad_nd_plan_create) is a plan handle too: refused with its own sentence
    wplan = _native.WgradPlan(_native.conv_desc(2, B, C, C, 1, (H, W), (3, 3), (1, 1), (0, 0), (1, 1), 0))
    lib = _native.load_library()
    for lays in ((CL, PL), (PL, CL)):
        assert lib.fc_plan_takes_layout(wplan._h, *lays) == _native.FC_ERR_UNSUPPORTED
        assert b"weight-gradient plan" in lib.fc_last_error()
    assert lib.fc_plan_takes_layout(wplan._h, PL, PL) == _native.FC_OK
    assert lib.fc_forward_lay(wplan._h, args[0], CL, args[1], None, args[3], PL, args[4], args[5]) == _native.FC_ERR_UNSUPPORTED
    assert b"weight-gradient plan" in lib.fc_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ capture
@pytest.mark.parametrize("dtype", (F32, BF16), ids=str)
def test_warm_strided_call_is_capturable_and_replays_bit_for_bit(dtype, monkeypatch):
    monkeypatch.setenv("FFTCONV_XTILE", "0")
    _clear()
    B, C, H, W = 2, 5, 5, 101
    x, w, b = _tensors(B, C, C, C, (H, W), (3, 3), True, dtype)
    plan = F_._plan_for(x, w, b, 1, 1, 1, C, "constant")
    spectrum = F_.transform_kernel(plan, w)
    static_x = _as_cl(x)
    F_._forward_native(static_x, spectrum, b, True)       # warm: plan and device tables exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = F_._forward_native(static_x, spectrum, b, True)
    assert static_y.dtype == dtype and _lies_cl(static_y)
    for seed in (1, 2, 3):
        fresh = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed)).to(DEV).to(dtype)
        static_x.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        gu.same_bits(static_y, F_._forward_native(fresh, spectrum, b), f"replay {seed} {dtype}")
