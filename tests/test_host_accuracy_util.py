"""tests/accuracy_util.py on the CPU: the integer generators and the exactness precondition, the baseline wrapper against
the exact truth in float64 (formulation, crop and stride proven before it serves as a yardstick), and the bound's power
to tell a float32 FFT with correctly rounded twiddles from one with two-ulp phase noise or recurrence twiddles -- which
route_util.TOL32 lets through."""
import numpy as np
import pytest
import torch

from tests import accuracy_util as au
from tests import route_util as ru

C = ru.Case


# ------------------------------------------------------------------------------------------------ generators
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.complex64])
def test_integers_stay_within_their_bounds(dtype):
    gen = torch.Generator().manual_seed(1)
    for offset in (0, au.OFFSET):
        t = au.integers((3, 5, 4001), gen, dtype, offset=offset)
        assert t.dtype == dtype
        parts = torch.view_as_real(t) if t.is_complex() else t
        assert au.is_whole(t)
        assert parts.min().item() == offset + au.LO and parts.max().item() == offset + au.HI


def test_inputs_of_a_case():
    c = C(3, 4, 6, (50, 31), (3, 5), g=2, f64=True)
    x, w, b = au.inputs(c, "offset")
    assert x.shape == (3, 4, 50, 31) and w.shape == (6, 2, 3, 5) and b.shape == (6,) and x.dtype == torch.float64
    assert x.min().item() >= au.OFFSET + au.LO and x.max().item() <= au.OFFSET + au.HI
    assert w.abs().max().item() <= au.HI and b.abs().max().item() <= au.HI
    x0 = au.inputs(c, "centred")[0]
    assert x0.abs().max().item() <= au.HI and not torch.equal(x0 + au.OFFSET, x)
    ct = C(2, 4, 6, (20,), (5,), s=2, p=1, op=1, g=2, tr=True)
    assert au.inputs(ct, "centred")[1].shape == (4, 3, 5) and au.out_spatial(ct) == (42,)


def test_exactness_precondition():
    biggest = max((c for r in ru.ROUTES + ru.TRANSPOSED_ROUTES for c in r.cases),
                  key=lambda c: au.exactness_bound(c, "offset"))
    assert au.assert_exact(biggest, "offset") < 2 ** 53 / 1000          # the route tables are far inside
    assert au.assert_exact(C(1, 1, 1, (1 << 22,), (1 << 21,), p=(1 << 21) - 1), "offset") < 2 ** 53
    with pytest.raises(ValueError, match="2\\*\\*53"):
        au.assert_exact(C(1 << 20, 1, 1, (1 << 26,), (3,)), "offset")
    # (the same shape without the offset: 64 x 2**46 terms still fit)
    au.assert_exact(C(1 << 20, 1, 1, (1 << 26,), (3,)), "centred")


def test_measures():
    want = torch.tensor([3.0, -4.0, 0.0, 5.0], dtype=torch.float64)
    got = want + torch.tensor([0.0, 0.0, 0.1, 0.0], dtype=torch.float64)
    r = au.rms(want)
    assert abs(r - (50 / 4) ** 0.5) < 1e-15
    assert abs(au.e_rms(got, want) - 0.05 / r) < 1e-15 and abs(au.e_max(got, want) - 0.1 / r) < 1e-15
    z = torch.complex(want, want)
    assert abs(au.rms(z) - r * 2 ** 0.5) < 1e-14


def test_truth_check_rejects_a_wrong_or_inexact_convolution():
    c = C(2, 3, 4, (300,), (9,), p=4, mode="reflect")
    x, w, b = au.inputs(c, "centred")
    want = au.truth(c, x, w, b)
    assert want.dtype == torch.float64 and au.is_whole(want)
    off = want.clone()
    off[..., 0] += 1                         # (the row ends are among the sampled positions)
    with pytest.raises(au.TruthNotExact, match="dot products"):
        au.verify_truth(c, x, w, b, off)
    with pytest.raises(au.TruthNotExact, match="integer-valued"):
        au.verify_truth(c, x, w, b, want + 1e-9)
    with pytest.raises(au.TruthNotExact):
        au.whole(want + 0.3)
    assert torch.equal(au.whole(want + 1e-7), want)


# ------------------------------------------------------------------------------------------------ the baseline is right
KINDS = [
    C(2, 3, 4, (301,), (17,), p=8, note="1d"),
    C(2, 3, 4, (33, 45), (4, 3), p=(2, 1), note="2d"),
    C(1, 2, 3, (9, 12, 14), (3, 2, 3), p=(1, 0, 1), note="3d"),
    C(2, 4, 4, (200,), (9,), s=3, p=4, note="strided"),
    C(2, 2, 3, (31, 40), (3, 4), s=(2, 3), d=(3, 2), p=(3, 3), note="dilated"),
    C(2, 6, 4, (150,), (11,), g=2, p=5, note="grouped"),
    C(2, 2, 2, (120,), (9,), p=7, mode="reflect"),
    C(2, 2, 2, (20, 33), (3, 5), p=(2, 4), mode="replicate"),
    C(2, 2, 2, (120,), (9,), s=2, p=8, mode="circular"),
    C(2, 6, 4, (70,), (9,), s=2, p=5, d=3, op=1, g=2, tr=True, note="output-padding"),
    C(2, 2, 3, (11, 13), (3, 4), s=(2, 3), p=(1, 2), op=(1, 2), tr=True, note="2d-output-padding"),
    C(1, 2, 2, (40,), (5,), s=2, p=9, d=1, op=1, tr=True, note="padding-past-the-kernel"),
]


@pytest.mark.parametrize("cls", au.CLASSES)
@pytest.mark.parametrize("c", KINDS, ids=[c.ident() for c in KINDS])
def test_float64_baseline_reproduces_the_exact_truth(c, cls):
    c = C(**{**c.__dict__, "f64": True})
    au.assert_exact(c, cls)
    x, w, b = au.inputs(c, cls)
    want = au.truth(c, x, w, b)
    assert want.shape[2:] == au.out_spatial(c)
    got = au.baseline(c, x, w, b)
    assert got.dtype == torch.float64 and au.e_rms(got, want) <= 1e-13
    assert torch.equal(au.truth_by_fft(c, x, w, b), want)
    gy = au.grad_output(want.shape, torch.float64)
    exact = au.truth_grads(c, x, w, b, gy)
    by_fft = au.truth_grads(c, x, w, b, gy, by_fft=True)
    base = au.baseline_grads(c, x, w, b, gy)
    for name, e, f, g in zip(("dX", "dW", "db"), exact, by_fft, base[1:]):
        assert torch.equal(e, f), name
        assert au.e_rms(g, e) <= 1e-13, name


@pytest.mark.parametrize("cls", au.CLASSES)
def test_complex_baseline_reproduces_the_exact_truth(cls):
    c = C(2, 4, 4, (260,), (31,), s=2, p=6, d=2, g=2, mode="reflect")
    x, w, b = (t.to(torch.complex128) for t in au.inputs(c, cls, complex_=True))
    assert au.assert_exact(c, cls, complex_=True) == 2 * au.exactness_bound(c, cls)
    want = au.truth(c, x, w, b)
    assert want.dtype == torch.complex128 and au.is_whole(want)
    # four real convolutions are what torch's complex convolution computes
    pad = torch.nn.functional.pad
    ref = torch.nn.functional.conv1d(pad(x, (6, 6), mode="reflect"), w, b, stride=2, dilation=2, groups=2)
    assert (ref - want).abs().max().item() < 1e-9
    assert au.e_rms(au.baseline(c, x, w, b), want) <= 1e-13
    gy = au.grad_output(want.shape, torch.complex128)
    exact = au.truth_grads(c, x, w, b, gy)
    base = au.baseline_grads(c, x, w, b, gy)
    for name, e, g in zip(("dX", "dW", "db"), exact, base[1:]):
        assert au.e_rms(g, e) <= 1e-13, name


def test_float32_baseline_of_exact_cases_sits_on_the_floor():
    """K = 1 and tiny shapes: both sides may be exact, the floors keep the bound meaningful."""
    c = C(2, 1, 1, (64,), (1,))
    x, w, b = au.inputs(c, "centred")
    want = au.truth(c, x, w, b)
    m = au.check("k1", want.float(), want, au.baseline(c, x, w, b), torch.float32)
    assert m["e_rms"] == 0.0 and m["rms_ratio"] == 0.0


# ------------------------------------------------------------------------------------------------ the bound discriminates
def _bitrev(n):
    bits = n.bit_length() - 1
    idx = np.arange(n)
    rev = np.zeros(n, dtype=np.int64)
    for i in range(bits):
        rev |= ((idx >> i) & 1) << (bits - 1 - i)
    return rev


def _cmul(a, b):
    """(re, im) pairs of float32 arrays: four products, one difference and one sum, each rounded once (written out, so that
    no fused multiply-add of a complex64 loop decides the figures)."""
    return a[0] * b[0] - a[1] * b[1], a[0] * b[1] + a[1] * b[0]


def _fft_r2(a, tw, inverse=False):
    """Radix-2 decimation in time on the last axis of an (re, im) pair, every operation in float32; tw[k] =
    exp(-2 pi i k / n), k < n/2, as an (re, im) pair."""
    n = a[0].shape[-1]
    rev = _bitrev(n)
    re, im = (np.ascontiguousarray(v[..., rev], dtype=np.float32) for v in a)
    tw = (tw[0], -tw[1]) if inverse else tw
    m = 2
    while m <= n:
        half = m // 2
        t = tuple(v[::n // m][:half] for v in tw)
        re, im = (v.reshape(v.shape[:-1] + (n // m, m)) for v in (re, im))
        hr, hi = _cmul((re[..., half:], im[..., half:]), t)
        re, im = (np.concatenate([lo[..., :half] + h, lo[..., :half] - h], axis=-1).reshape(lo.shape[:-2] + (n,))
                  for lo, h in ((re, hr), (im, hi)))
        assert re.dtype == im.dtype == np.float32
        m *= 2
    return (re / np.float32(n), im / np.float32(n)) if inverse else (re, im)


def _twiddles(n, kind):
    ang = -2.0 * np.pi * np.arange(n // 2) / n
    if kind == "noise":
        # two float32 ulps of phase: every entry off by 2**-22 rad, the signs in Thue-Morse order (no seed, and no
        # stage's subset of the table carries a net turn).  Normal noise of that deviation measures 1.7-2.9 x the
        # baseline's e_rms from seed to seed, this table 2.4-2.5 x.
        ang = ang + np.array([1 - 2 * (bin(k).count("1") & 1) for k in range(n // 2)]) * 2.0 ** -22
    if kind == "recurrence":                     # w[i] = w[i-1] * w[1] in float32
        re, im = np.empty(n // 2, dtype=np.float32), np.empty(n // 2, dtype=np.float32)
        re[0], im[0] = 1, 0
        w1 = (np.float32(np.cos(ang[1])), np.float32(np.sin(ang[1])))
        for i in range(1, n // 2):
            re[i], im[i] = _cmul((re[i - 1], im[i - 1]), w1)
        return re, im
    return np.cos(ang).astype(np.float32), np.sin(ang).astype(np.float32)


def _model_conv(x, w, kind):
    """Cross-correlation of (B, 1, N) rows with one (1, 1, K) kernel through the float32 radix-2 transform of N points."""
    n = x.shape[-1]
    tw = _twiddles(n, kind)
    xr = x.numpy()[:, 0].astype(np.float32)
    xs = _fft_r2((xr, np.zeros_like(xr)), tw)
    wp = np.zeros(n, dtype=np.float32)
    wp[:w.shape[-1]] = w.numpy()[0, 0]
    ws = _fft_r2((wp, np.zeros_like(wp)), tw)
    y = _fft_r2(_cmul(xs, (ws[0], -ws[1])), tw, inverse=True)[0]
    return torch.from_numpy(np.ascontiguousarray(y[:, None, :n - w.shape[-1] + 1]))


def _model_case(n, cls):
    c = C(8, 1, 1, (n,), (n // 8 + 1,))
    x, w, _ = au.inputs(c, cls)
    want = au.truth(c, x, w, None)
    return c, x, w, want, au.baseline(c, x, w, None)


@pytest.mark.parametrize("cls", au.CLASSES)
@pytest.mark.parametrize("n", [1024, 4096])
def test_bound_passes_correctly_rounded_twiddles(n, cls):
    c, x, w, want, base = _model_case(n, cls)
    au.check(f"rounded twiddles N {n}", _model_conv(x, w, "rounded"), want, base, torch.float32)


@pytest.mark.parametrize("n", [1024, 4096])
def test_bound_fails_phase_noise_of_two_ulps(n):
    """(Centred inputs, here and below: a single-channel row of the offset class is mostly its mean, which every
    transform carries exactly in bin 0, so that both sides sit under the floor.)"""
    c, x, w, want, base = _model_case(n, "centred")
    with pytest.raises(AssertionError, match="x the baseline's"):
        au.check(f"2**-22 phase noise N {n}", _model_conv(x, w, "noise"), want, base, torch.float32)


@pytest.mark.parametrize("n", [1024, 4096])
def test_bound_fails_recurrence_twiddles_that_the_old_bound_passes(n):
    c, x, w, want, base = _model_case(n, "centred")
    got = _model_conv(x, w, "recurrence")
    with pytest.raises(AssertionError, match="x the baseline's"):
        au.check(f"recurrence twiddles N {n}", got, want, base, torch.float32)
    if n == 1024:
        old = (got.double() - want).abs().max().item() / want.abs().max().item()
        print(f"recurrence twiddles N 1024: max|got - want| / max|want| = {old:.2e}")
        assert old <= ru.TOL32, "the point of the accuracy suite: the project's old bound lets this through"
