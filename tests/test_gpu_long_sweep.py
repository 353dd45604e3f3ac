"""The cross-feature sweep of the long-filter family on the GPU: every case of the seeded table of
tests/long_sweep_util.py (tests/test_host_long_sweep.py holds the table to its conditions) runs under its switches and is
held to ``long_sweep_util.run_case``: (a) the plans that ran are the predicted ones, at the forced N1 x N2 and the expected
slab count; (b) y, dX, dW and db against the exact truth, within ``accuracy_util.check``'s default margins of the float32 /
complex64 FFT baseline; (c) shape, dtype and strides; (d) the bit relations the docstrings promise; (e) untouched inputs.
The id of a case is printed before it runs and stands in every assertion message.

Directed regression cases for what the sweep found follow the table."""
import pytest
import torch

from tests import long_sweep_util as su

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHUNK = 8
CHUNKS = [(kind, n) for kind, table in zip(("fwd", "tr"), su.tables()) for n in range(0, len(table), CHUNK)]


@pytest.fixture(autouse=True)
def _fresh(monkeypatch):
    for k in su.ALL_KNOBS:
        monkeypatch.delenv(k, raising=False)
    su.clear()
    yield
    su.clear()


def _setenv(monkeypatch):
    return lambda k, v: monkeypatch.delenv(k, raising=False) if v is None else monkeypatch.setenv(k, v)


@pytest.mark.parametrize("kind,first", CHUNKS, ids=[f"{k}{n:02d}" for k, n in CHUNKS])
def test_sweep(kind, first, monkeypatch):
    cases = su.tables()[0 if kind == "fwd" else 1][first:first + CHUNK]
    assert cases
    for c in cases:
        su.run_case(c, DEV, _setenv(monkeypatch), log=lambda s: print(s, flush=True))
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ what the sweep found
def test_dx_by_phases_has_the_signals_layout_under_nlc_0(monkeypatch):
    """Seed 1, case F26-bf16-B3g2i3o2-L2702K6180-p2702cons-s7d1-nlc0/ncl-lg-decim1-nlc0-longn64x128-ws1: under
    FFTCONV_LONG_NLC=0 a signal that lies as (B, L, C) is copied and so, with FFTCONV_LONG_DECIM=1, runs by phases; backward
    returned the phases plan's contiguous dX -- strides (16212, 2702, 1) for a signal of (16212, 1, 6) -- where the
    docstring promises dX in the signal's layout and strides that the switch leaves unchanged.  The smallest row past the
    hand-off shows it."""
    from fft_conv_pytorch_amd import fft_long_conv
    monkeypatch.setenv("FFTCONV_LONG_NLC", "0")
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    gen = torch.Generator().manual_seed(26)
    x = su.place(su.au.integers((1, 2, 4100), gen, torch.float32), "nlc0", DEV).requires_grad_()
    w = su.au.integers((2, 2, 5), gen, torch.float32).to(DEV).requires_grad_()
    seen = []
    x.register_hook(lambda g: seen.append(tuple(g.stride())))
    with su.Spy() as spy:
        y = fft_long_conv(x, w, stride=2)
        y.backward(torch.ones_like(y))
    assert spy.tokens() == ["decim", "phases", "long/3"], spy.tokens()
    assert seen == [tuple(x.stride())] == [(8200, 1, 2)], seen
    xc = x.detach().contiguous().requires_grad_()
    fft_long_conv(xc, w.detach(), stride=2).sum().backward()
    su.gu.same_bits(x.grad, xc.grad, "dX of the strided signal against the contiguous one")


@pytest.mark.parametrize("nlc_switch", [None, "0"])
def test_replicate_fold_of_a_strided_dx_has_the_bits_of_the_contiguous_call(nlc_switch, monkeypatch):
    """Seed 3, case F02-f32-B5g2i2o3-L6359K12-samerepl-s1d2-nlc0/ncl-blg-nlc0-longn64x256-ws1: dX of a signal that lies as
    (B, L, C) differed from the contiguous call's in the first sample of each of the 20 rows by two units in the last place
    (0x4363fffc against 0x4363fffa).  With replicate padding the adjoint of the padding sums the 11 border samples of the
    padded row's gradient onto the edge sample, and torch summed them in another order on the channels-last tensor than on
    the contiguous one; the docstring promises the bits of the contiguous call."""
    from fft_conv_pytorch_amd import fft_long_conv
    if nlc_switch is not None:
        monkeypatch.setenv("FFTCONV_LONG_NLC", nlc_switch)
    gen = torch.Generator().manual_seed(302)
    x0 = su.au.integers((2, 2, 4200), gen, torch.float32)
    w = su.au.integers((3, 2, 12), gen, torch.float32).to(DEV)
    gy = su.au.integers((2, 3, 4200), gen, torch.float32).to(DEV)
    grads = []
    for layout in ("ncl", "nlc0"):
        x = su.place(x0, layout, DEV).requires_grad_()
        y = fft_long_conv(x, w, padding="same", dilation=2, padding_mode="replicate")
        y.backward(gy)
        grads.append(x.grad)
    su.gu.same_bits(grads[1], grads[0], "dX of the strided signal against the contiguous one")


def test_replicate_padding_as_wide_as_the_row_keeps_dx_within_the_bound():
    """Seed 3, case F44-bf16-B2g3i1o5-L2427K10-p2427repl-s2d3-copy/nlc-g-decim1-wgrad1-nlc0-half0-longn128x64: in one run of
    three dX of the float32 twin had e_max 1.633e-05, 3.43 x the baseline's 4.762e-06 (bound 3 x).  With replicate padding
    p = L the edge sample of dX is the sum of p + 1 samples of the padded row's gradient, about sqrt(p) x rms(dX), so that
    one float32 unit of it is about 6e-06 of rms(dX) and e_max of the whole tensor is decided by the 2 B Cin edge samples.
    Two things were wrong.  The baseline went through torch's replication-pad backward, which accumulates with atomic adds:
    its own edge samples moved by units in the last place from run to run (4.8e-06 ... 9e-06), and the bound with them
    (``long_sweep_util.pad`` now writes the padding as slices).  And ``_pad_adjoint`` summed the border in float32; it
    accumulates in float64 now and rounds once.  This is that case's geometry in float32 (nothing smaller has an edge
    sample as large), held to the default margins on the whole of dX and on its edge samples alone."""
    c = su.Case("fwd", 44, 3, (), 2, 3, 1, 5, 2427, 10, 2427, "replicate", 2, 3, False, 0, False, False, "f32", "ncl", "ncl", True,
                False, "centred", (), 2427, 2427, 3 * 2427, (3 * 2427 - 27 - 1) // 2 + 1, "plain", None, 0, 0, 0, 9, 0, ())
    x0, w0, b0, gy0 = su.inputs(c)
    want = su.truth(c, x0, w0, b0, gy0)
    x, w, gy = x0.to(DEV), w0.to(DEV), gy0.to(DEV)
    with su.Spy() as spy:
        got = su.step(c, x, w, None, gy)
    assert spy.tokens() == su.predict(c)["tokens"] == ["long/0", f"long/{3 * c.L}", f"long/{c.K}"], spy.tokens()
    base = su.baseline(c, x, w, None, gy)
    su.check_values(c, got, want, base)
    edge = lambda t: t[..., [0, c.L - 1]].contiguous()      # noqa: E731
    assert su.au.rms(edge(want["dX"])) > 20 * su.au.rms(want["dX"])          # (4674 against 179)
    su.au.check(f"{c.id} edge samples of dX", edge(got["dX"]), edge(want["dX"]), edge(base["dX"]), torch.float32)
