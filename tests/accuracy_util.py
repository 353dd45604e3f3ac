"""What tests/test_gpu_accuracy.py measures with: integer inputs whose float64 convolution is exact, the model project's
FFT formulation as a baseline in the case's own precision, two error measures relative to rms(want), and the bound that
ties a kernel's error to the baseline's.  Nothing here needs a GPU (tests/test_host_accuracy_util.py runs it on the CPU).

Exact truth.  Signal, weight, bias and dY are random integers in [-8, 8] stored in the case's dtype (class "offset": the
signal is 64 + [-8, 8], so that the DC and Nyquist bins of the packed real transforms carry energy).  Every product and
every partial sum of a convolution of them, and of its gradients, is an integer below 2**53 (``assert_exact`` checks the
case's shape first), so a float64 direct convolution and its float64 autograd are exact whatever the order of summation:
the error measured against them is the kernel's alone, in float64 plans too.  ``truth`` asserts that the values are whole
numbers and equal explicit float64 dot products at sampled positions; a device convolution that fails that is replaced
by the CPU's.

Measures.  e_rms = rms(got - want) / rms(want), e_max = max|got - want| / rms(want).

Baseline.  Pad in the case's mode, rfftn, multiply by the conjugate spectrum of the zero-stuffed kernel per group, irfftn,
crop, take every stride-th sample, add the bias (oracle.fft_conv_oracle.fft_conv_oracle_torch), on the same tensors and
device, with every spatial axis zero-extended on the right to a power of two so that the FFT library stays on its
radix-2 family plans.  Gradients of the baseline come from autograd through it.

Bound.  e_rms(kernel) <= max(2 e_rms(baseline), 4 eps), e_max(kernel) <= max(3 e_max(baseline), 16 eps), eps = 2**-23
for float32 / complex64 plans and 2**-52 for float64 ones.  2: the kernels' transforms are no longer than the baseline's
and their channel sums as long; an honest float32 FFT of another factorisation measures 0.9-1.0 x the baseline, a
two-ulp twiddle defect 2.2 x.  3 = 2 x 1.5 for the scatter of the largest of 1e4-1e7 samples between two implementations
of equal spread.  The floors cover cases both sides compute exactly."""
import math

import torch
import torch.nn.functional as F

from oracle.fft_conv_oracle import fft_conv_oracle_torch
from tests import route_util as ru

LO, HI, OFFSET = -8, 8, 64
CLASSES = ("centred", "offset")
EPS = {torch.float32: 2.0 ** -23, torch.complex64: 2.0 ** -23, torch.float64: 2.0 ** -52}
RMS_MARGIN, MAX_MARGIN = 2.0, 3.0
RMS_FLOOR, MAX_FLOOR = 4.0, 16.0          # in eps
RMS_MARGIN_CAP = 4.0                      # no route's own margin may exceed this
EXACT_LIMIT = 2 ** 53


class TruthNotExact(AssertionError):
    pass


# ------------------------------------------------------------------------------------------------ inputs
def integers(shape, gen, dtype, device="cpu", offset=0):
    """Uniform integers in [offset + LO, offset + HI] in ``dtype`` (complex: both parts), drawn on the CPU."""
    def draw():
        return torch.randint(LO, HI + 1, tuple(shape), generator=gen, dtype=torch.int64) + offset
    if dtype.is_complex:
        part = torch.float32 if dtype == torch.complex64 else torch.float64
        t = torch.complex(draw().to(part), draw().to(part))
    else:
        t = draw().to(dtype)
    return t.to(device)


def case_dtype(c, complex_=False):
    return torch.complex64 if complex_ else torch.float64 if c.f64 else torch.float32


def inputs(c, cls, device="cpu", complex_=False):
    """(x, w, b) of a route_util.Case in input class ``cls``."""
    assert cls in CLASSES, cls
    dtype = case_dtype(c, complex_)
    gen = torch.Generator().manual_seed(sum(c.size) + 7 * c.B + c.cin + 1000 * CLASSES.index(cls))
    x = integers((c.B, c.cin) + tuple(c.size), gen, dtype, device, OFFSET if cls == "offset" else 0)
    return x, integers(c.wshape, gen, dtype, device), integers((c.cout,), gen, dtype, device)


def grad_output(shape, dtype, device="cpu"):
    return integers(shape, torch.Generator().manual_seed(9), dtype, device)


def out_spatial(c):
    if c.tr:
        return tuple((S - 1) * s - 2 * p + d * (k - 1) + o + 1
                     for S, s, p, d, k, o in zip(c.size, c.tup(c.s), c.tup(c.p), c.tup(c.d), c.k, c.tup(c.op)))
    return tuple((S + 2 * p - d * (k - 1) - 1) // s + 1
                 for S, s, p, d, k in zip(c.size, c.tup(c.s), c.tup(c.p), c.tup(c.d), c.k))


def exactness_bound(c, cls, complex_=False):
    """The largest magnitude a partial sum of y, dX, dW or db of the case can reach: taps x channels per group terms for y
    and dX, batch x row terms for dW and db (K . Cin/g . B . Lout in one figure: the maximum of the four)."""
    xmax = HI + (OFFSET if cls == "offset" else 0)
    taps = math.prod(c.k)
    per_group = max(c.cin // c.g, c.cout // c.g)
    rows = c.B * max(math.prod(out_spatial(c)), math.prod(c.size))
    bound = max(xmax * HI * taps * per_group + HI, HI * HI * taps * per_group, xmax * HI * rows, HI * rows)
    return bound * (2 if complex_ else 1)


def assert_exact(c, cls, complex_=False):
    bound = exactness_bound(c, cls, complex_)
    if bound >= EXACT_LIMIT:
        raise ValueError(f"{c.ident()} ({cls}): partial sums reach {bound:.3e} >= 2**53, float64 is not exact for this shape")
    return bound


# ------------------------------------------------------------------------------------------------ measures
def _abs64(t):
    t = t.to(torch.complex128) if t.is_complex() else t.double()
    return t.abs()


def rms(t):
    return _abs64(t).pow(2).mean().sqrt().item()


def _diff(got, want):
    assert got.shape == want.shape, (tuple(got.shape), tuple(want.shape))
    wide = torch.complex128 if (got.is_complex() or want.is_complex()) else torch.float64
    return (got.to(wide) - want.to(wide).to(got.device)).abs()


def e_rms(got, want):
    return _diff(got, want).pow(2).mean().sqrt().item() / max(rms(want), 1e-300)


def e_max(got, want):
    return _diff(got, want).max().item() / max(rms(want), 1e-300)


def measure(got, want, base, dtype):
    """Both measures of kernel and baseline and their ratios.  A ratio divides by the larger of the baseline's error and
    the floor over the standard margin, so ``ratio <= margin`` is the bound itself."""
    eps = EPS[dtype]
    m = dict(e_rms=e_rms(got, want), base_e_rms=e_rms(base, want), e_max=e_max(got, want), base_e_max=e_max(base, want))
    m["rms_ratio"] = m["e_rms"] / max(m["base_e_rms"], RMS_FLOOR * eps / RMS_MARGIN)
    m["max_ratio"] = m["e_max"] / max(m["base_e_max"], MAX_FLOOR * eps / MAX_MARGIN)
    return m


def finite(t):
    return bool(torch.isfinite(torch.view_as_real(t) if t.is_complex() else t).all())


def assert_bound(what, m, rms_margin=RMS_MARGIN, exact=False):
    """The bound on a ``measure`` (``exact``: a plan that runs no transform must give the truth itself).  A route whose
    design performs more roundings than the baseline passes its own ``rms_margin`` (at most RMS_MARGIN_CAP); the margin of
    the maximum grows with it."""
    print(f"    {what}: e_rms {m['e_rms']:.2e} (baseline {m['base_e_rms']:.2e}, x{m['rms_ratio']:.2f})  "
          f"e_max {m['e_max']:.2e} (baseline {m['base_e_max']:.2e}, x{m['max_ratio']:.2f})")
    assert RMS_MARGIN <= rms_margin <= RMS_MARGIN_CAP, rms_margin
    if exact:
        assert m["e_max"] == 0.0, f"{what}: a plan without a transform is off the exact result by e_max {m['e_max']:.3e}"
    max_margin = MAX_MARGIN * rms_margin / RMS_MARGIN
    assert m["rms_ratio"] <= rms_margin, \
        f"{what}: e_rms {m['e_rms']:.3e} is {m['rms_ratio']:.2f} x the baseline's {m['base_e_rms']:.3e} (bound {rms_margin:g} x)"
    assert m["max_ratio"] <= max_margin, \
        f"{what}: e_max {m['e_max']:.3e} is {m['max_ratio']:.2f} x the baseline's {m['base_e_max']:.3e} (bound {max_margin:g} x)"


def check(what, got, want, base, dtype, rms_margin=RMS_MARGIN, exact=False):
    """Measure, print, assert the bound."""
    assert finite(got), f"{what}: result not finite"
    m = measure(got, want, base, dtype)
    assert_bound(what, m, rms_margin, exact)
    return m


# ------------------------------------------------------------------------------------------------ baseline
def _next_pow2(n):
    return 1 << max(0, int(n) - 1).bit_length()


def _via_real(fn, x, w, b):
    """A bilinear real op on complex operands: (xr + i xi)(wr + i wi) as four real calls, the bias added last."""
    if not x.is_complex():
        return fn(x, w, b)
    re = fn(x.real, w.real, None) - fn(x.imag, w.imag, None)
    im = fn(x.real, w.imag, None) + fn(x.imag, w.real, None)
    out = torch.complex(re, im)
    return out if b is None else out + b.reshape(1, -1, *([1] * (x.dim() - 2)))


def _baseline_real(x, w, b, stride, padding, dilation, groups, mode):
    nd = x.dim() - 2
    if any(padding):
        flat = [q for p in reversed(padding) for q in (p, p)]
        x = F.pad(x, flat, mode=mode)
    if any(d != 1 for d in dilation):
        wide = [(k - 1) * d + 1 for k, d in zip(w.shape[2:], dilation)]
        stuffed = w.new_zeros(tuple(w.shape[:2]) + tuple(wide))
        stuffed[(Ellipsis,) + tuple(slice(None, None, d) for d in dilation)] = w
        w = stuffed
    size, kd = tuple(x.shape[2:]), tuple(w.shape[2:])
    grow = [q for s in reversed(size) for q in (0, _next_pow2(s) - s)]
    full = fft_conv_oracle_torch(F.pad(x, grow), w, None, groups=groups)
    window = (slice(None), slice(None)) + tuple(slice(0, s - k + 1, t) for s, k, t in zip(size, kd, stride))
    out = full[window]
    if b is not None:
        out = out + b.reshape(1, -1, *([1] * nd))
    return out.contiguous()


def baseline_conv(x, w, b, stride, padding, dilation, groups, mode="constant"):
    """The model project's formulation in the tensors' own precision and on their device; differentiable."""
    nd = x.dim() - 2
    t = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * nd      # noqa: E731
    return _via_real(lambda x_, w_, b_: _baseline_real(x_, w_, b_, t(stride), t(padding), t(dilation), groups, mode), x, w, b)


def transposed_as_forward(x, w, stride, padding, output_padding, dilation, groups):
    """The forward convolution a transposed one is: (the signal spread over the stride's grid between zero paddings of
    kd - 1 - p, output_padding more on the right; the kernel flipped, in and out channels swapped inside every group).
    Stride 1, no padding, the same dilation."""
    nd = x.dim() - 2
    cin, cog = w.shape[:2]
    k = tuple(w.shape[2:])
    wf = torch.flip(w, dims=tuple(range(2, 2 + nd)))
    wf = wf.reshape((groups, cin // groups, cog) + k).transpose(1, 2).reshape((groups * cog, cin // groups) + k)
    spread = x.new_zeros(tuple(x.shape[:2]) + tuple((S - 1) * s + 1 for S, s in zip(x.shape[2:], stride)))
    spread[(Ellipsis,) + tuple(slice(None, None, s) for s in stride)] = x
    flat = []
    for ax in reversed(range(nd)):
        edge = (k[ax] - 1) * dilation[ax] - padding[ax]
        flat += [edge, edge + output_padding[ax]]
    return F.pad(spread, flat), wf


def baseline_conv_transpose(x, w, b, stride, padding, output_padding, dilation, groups):
    nd = x.dim() - 2
    t = lambda v: tuple(v) if isinstance(v, (tuple, list)) else (v,) * nd      # noqa: E731

    def real(x_, w_, b_):
        xs, wf = transposed_as_forward(x_, w_, t(stride), t(padding), t(output_padding), t(dilation), groups)
        return _baseline_real(xs, wf, b_, (1,) * nd, (0,) * nd, t(dilation), groups, "constant")
    return _via_real(real, x, w, b)


def baseline(c, x, w, b):
    if c.tr:
        return baseline_conv_transpose(x, w, b, c.tup(c.s), c.tup(c.p), c.tup(c.op), c.tup(c.d), c.g)
    return baseline_conv(x, w, b, c.tup(c.s), c.tup(c.p), c.tup(c.d), c.g, c.mode)


# ------------------------------------------------------------------------------------------------ truth
def _wide(t):
    return t.to(torch.complex128) if t.is_complex() else t.double()


def direct(c, x, w, b):
    """torch's float64 convolution of the case (complex operands: four real convolutions)."""
    from tests import test_gpu_routes as tr
    return _via_real(lambda x_, w_, b_: tr._reference(c, x_, w_, b_), _wide(x), _wide(w), None if b is None else _wide(b))


def _forward_view(c, x, w):
    """(case, x, w) of the forward convolution with the same outputs: the case itself, or the spread form of a transposed
    one, on which explicit dot products can be sampled."""
    if not c.tr:
        return c, x, w
    xs, wf = transposed_as_forward(x, w, c.tup(c.s), c.tup(c.p), c.tup(c.op), c.tup(c.d), c.g)
    return ru.Case(c.B, c.cin, c.cout, tuple(xs.shape[2:]), c.k, d=c.d, g=c.g, f64=c.f64), xs, wf


def sampled(c, x, w, b, idx):
    """Explicit float64 dot products at the output positions idx (test_gpu_routes._sampled; complex: four of them)."""
    from tests import test_gpu_routes as tr
    cf, xf, wf = _forward_view(c, _wide(x), _wide(w))
    b = None if b is None else _wide(b)
    if not xf.is_complex():
        return tr._sampled(cf, xf, wf, b, idx)
    re = tr._sampled(cf, xf.real, wf.real, None, idx) - tr._sampled(cf, xf.imag, wf.imag, None, idx)
    im = tr._sampled(cf, xf.real, wf.imag, None, idx) + tr._sampled(cf, xf.imag, wf.real, None, idx)
    out = torch.complex(re, im)
    return out if b is None else out + b[idx[:, 1].to(b.device)]


def is_whole(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return bool((t == t.round()).all())


def verify_truth(c, x, w, b, want, seams=None, n=200):
    """The truth holds whole numbers only and equals explicit dot products at the positions test_gpu_routes._sample_idx
    gives (random ones, the row ends, both sides of every seam)."""
    from tests import test_gpu_routes as tr
    if not is_whole(want):
        raise TruthNotExact(f"{c.ident()}: the float64 convolution of integers is not integer-valued")
    cf = _forward_view(c, x[:1, :, ...], w)[0] if c.tr else c
    idx = tr._sample_idx(cf, tuple(want.shape), seams if seams is not None else [[] for _ in range(c.nd)], n)
    dots = sampled(c, x, w, b, idx)
    at = want[tuple(idx.t().to(want.device))]
    if not torch.equal(at, dots.to(at.device)):
        raise TruthNotExact(f"{c.ident()}: the float64 convolution differs from explicit dot products "
                            f"(by up to {(at - dots.to(at.device)).abs().max().item():.3e})")


def truth(c, x, w, b, seams=None):
    """The exact result in float64 (complex128), on the tensors' device if its float64 convolution is a direct one (it
    passes ``verify_truth``), else on the CPU."""
    want = direct(c, x, w, b)
    try:
        verify_truth(c, x, w, b, want, seams)
    except TruthNotExact:
        if x.device.type == "cpu":
            raise
        want = direct(c, x.cpu(), w.cpu(), None if b is None else b.cpu())
        verify_truth(c, x.cpu(), w.cpu(), None if b is None else b.cpu(), want, seams)
        want = want.to(x.device)
    return want


def whole(t, what="value"):
    """A float64 result known to be a whole number up to its own rounding (a float64 FFT convolution of integers, its
    autograd): the nearest integers, after checking that none is further than 1/4 away."""
    r = torch.view_as_real(t) if t.is_complex() else t
    off = (r - r.round()).abs().max().item()
    if not off < 0.25:
        raise TruthNotExact(f"{what}: {off:.3f} from a whole number")
    r = r.round()
    return torch.view_as_complex(r.contiguous()) if t.is_complex() else r


def truth_by_fft(c, x, w, b, seams=None):
    """For filters too long for a direct convolution: the float64 FFT convolution of the integers, rounded to the nearest
    integers (its error is below 1e-6 of a unit for every shape ``assert_exact`` lets through) and verified like ``truth``."""
    want = whole(baseline(c, _wide(x), _wide(w), None if b is None else _wide(b)), c.ident())
    verify_truth(c, x, w, b, want, seams)
    return want


def truth_grads(c, x, w, b, gy, by_fft=False, only_dx=False):
    """(dX, dW, db) by float64 autograd of the exact convolution (dW and db None with ``only_dx``)."""
    xr = _wide(x).clone().requires_grad_()
    wr, br = (_wide(t).clone().requires_grad_(not only_dx) for t in (w, b))
    y = baseline(c, xr, wr, br) if by_fft else direct(c, xr, wr, br)
    y.backward(_wide(gy))
    grads = (xr.grad, wr.grad, br.grad)
    if by_fft:
        grads = tuple(None if g is None else whole(g, f"{c.ident()} {n}") for g, n in zip(grads, ("dX", "dW", "db")))
    for g, n in zip(grads, ("dX", "dW", "db")):
        if g is not None and not is_whole(g):
            raise TruthNotExact(f"{c.ident()}: float64 {n} of integers is not integer-valued")
    return grads


def baseline_grads(c, x, w, b, gy, only_dx=False):
    """(y, dX, dW, db) of the baseline in the tensors' own precision, by autograd through it."""
    xr = x.clone().requires_grad_()
    wr, br = (t.clone().requires_grad_(not only_dx) for t in (w, b))
    y = baseline(c, xr, wr, br)
    y.backward(gy)
    return y.detach(), xr.grad, wr.grad, br.grad
