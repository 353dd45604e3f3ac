"""The probes of tests/backward_util.py do not degenerate (no GPU: torch's float64 convolution on the CPU).

For every forward case of the backward tables, on a copy with the row geometry kept and batch and channels cut down: both
probes are non-empty and inside the row, and clearing one probed dY sample -- the first, one in the middle, the last --
moves the float64 dW by at least 100 x TOL32 of its maximum, so that a kernel dropping that sample cannot pass the
element-wise bound.  A condition on the probes, not a measurement of any kernel."""
import pytest
import torch

from tests import backward_util as bu

CASES = bu.forward_cases()


@pytest.mark.parametrize("family,c", CASES, ids=[f"{f}/{c.ident()}" for f, c in CASES])
def test_probe_sets_and_sensitivity(family, c):
    small = bu.cpu_sized(c)
    dy_axes, x_samples = bu.probe_sets(c)          # (placed for the case itself: channels decide which route runs)
    lout = bu.out_len(small)
    for ax, pos in enumerate(dy_axes):
        assert pos and all(0 <= v < lout[ax] for v in pos), (ax, pos, lout)
    gen = torch.Generator().manual_seed(11)
    if x_samples is not None:
        assert x_samples and all(0 <= v < small.size[0] for v in x_samples), x_samples
        xp = bu.impulses((small.B, small.cin) + tuple(small.size), [x_samples], gen, torch.float64, "cpu")
        assert int((xp != 0).sum()) == small.B * small.cin * len(x_samples)
    x = torch.randn((small.B, small.cin) + tuple(small.size), generator=gen, dtype=torch.float64)
    gy = bu.impulses((small.B, small.cout) + lout, dy_axes, gen, torch.float64, "cpu")
    dw, _ = bu.reference_dw(small, x, gy)
    top = dw.abs().max().item()
    assert top > 0
    n = len(dy_axes[0])
    worst = float("inf")
    for i in sorted({0, n // 2, n - 1}):
        at = (0, 0, dy_axes[0][i]) + tuple(a[len(a) // 2] for a in dy_axes[1:])
        cleared = gy.clone()
        assert cleared[at] != 0
        cleared[at] = 0
        moved = (bu.reference_dw(small, x, cleared)[0] - dw).abs().max().item() / top
        worst = min(worst, moved)
        assert moved >= bu.PROBE_MOVES, f"{family}: clearing dY{at} moves dW by {moved:.2e} of its maximum"
    print(f"\n{family} / {c.ident()}: a cleared probe sample moves dW by at least {worst:.1e} of its maximum")


def test_tables_are_sized_for_their_edges():
    """On a device of 256 compute units every case of the fc_wgrad1d families satisfies its family's predicate and its own
    (the GPU test repeats this with the device's count and the library's slices), every refusal lies outside the restated
    geometry, and its chunks are cut as its entry says."""
    for f in bu.WGRAD1D_FAMILIES:
        assert f.cases, f.name
        for c in f.cases:
            geo = bu.wgrad_geometry(c, 256)
            assert geo is not None and f.pred(geo) and (c.expect is None or c.expect(geo)), (f.name, c.ident(), geo)
    for name, c, chunked, sized in bu.REFUSALS:
        assert bu.wgrad_geometry(c, 256) is None, name
        is_chunked, c_taps, nchunk = bu.chunk_plan(c)
        assert is_chunked == chunked and (sized is None or sized(c_taps, nchunk, bu.out_len(c)[0])), (name, c_taps, nchunk)
    for name, _, c, _ in bu.WGRAD_ND:
        assert name not in bu.STRIDE_TAILS or all(t != 0 for t in bu.stride_tails(c)), (name, bu.stride_tails(c))
    assert all(any(n == name for n, _, _, _ in bu.WGRAD_ND) for name in bu.STRIDE_TAILS)
    for name, dtype, c in bu.HALF_CASES:
        geo = bu.wgrad_geometry(c, 256)
        assert geo is not None and geo["diag"] == (name == "depthwise-strided"), name
