"""Batch-pair rows of the 1-D batch-sharing kernel (conv1d_pers.hpp BPAIR).

In the dense builds without phases a complex sequence carries one channel of two slots of a work item (two batch items,
or with slot_tiles two tiles): real part slot 2j, imaginary part slot 2j+1.  What can go wrong there, and what the cases
below are sized for: an imaginary part that is empty (an odd number of slots, the last batch item), a remainder item of
one slot, a missing channel (a whole empty row), groups, no bias, border tiles in every padding mode, rows on and off
the cache-line grid, 16-bit rows, a segmented kernel that adds into y.

Every case asserts that the batch-sharing kernel ran (layout word 7 = its slots, word 6 = 0: neither the wide nor the
dense pipeline) and is held, on integer inputs whose float64 convolution is exact, to the bound of
tests/accuracy_util.py against torch's float64 convolution on the CPU."""
import pytest
import torch

from tests import accuracy_util as au
from tests import route_util as ru
from tests import test_gpu_routes as tr

pytestmark = pytest.mark.gpu
DEV = tr.DEV
C = ru.Case
KNOBS = tr.KNOBS


@pytest.fixture(autouse=True)
def _no_knob_plans_afterwards():
    yield
    from fft_conv_pytorch_amd import _native
    _native.clear_plan_cache()


def _knobs(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    tr._knobs(monkeypatch, env)


def _plan(c, x, w, b):
    from fft_conv_pytorch_amd import functional as fc
    kw = tr._kw(c)
    return fc._plan_for(x, w, b, kw["stride"], kw["padding"], kw["dilation"], c.g, c.mode)


def _forward(plan, x, w, b):
    """transform_kernel + Plan.forward into an output filled with NaN (a sample never stored stays NaN)."""
    from fft_conv_pytorch_amd import functional as fc
    spec = fc.transform_kernel(plan, w)
    out = torch.full((x.shape[0], plan.key[3]) + plan.out_spatial, float("nan"), dtype=x.dtype, device=DEV)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    plan.forward(x.data_ptr(), spec.buf.data_ptr(), None if b is None else b.data_ptr(), out.data_ptr(), None, stream)
    torch.cuda.synchronize()
    return out


def _seams(c, plan):
    r = plan.route
    kt = (plan.layout[3] - 1) * c.tup(c.d)[0] + 1 if r["nseg"] > 1 else (c.k[0] - 1) * c.tup(c.d)[0] + 1
    V = r["T"] - kt + 1
    return [[j * V for j in range(1, r["ntiles"])]]


def _run(c, nb, monkeypatch, cls="offset", bias=True, want_route=None):
    """One case on the batch-sharing kernel with nb slots: the plan's route, the result against float64 on the CPU."""
    _knobs(monkeypatch, {"FFTCONV_PERS": str(nb), **c.env})
    au.assert_exact(c, cls)
    x, w, b = au.inputs(c, cls, DEV)
    if not bias:
        b = None
    plan = _plan(c, x, w, b)
    r = plan.route
    assert plan.layout[7] == nb and plan.layout[6] == 0 and r["ph"] == 1 and r["diag"] == 0, (plan.layout, r)
    assert want_route is None or want_route(r), f"case not sized as intended: {r}"
    got = _forward(plan, x, w, b)
    assert au.finite(got), f"{int((~torch.isfinite(got)).sum())} output samples not written / not finite"
    want = au.truth(c, x.cpu(), w.cpu(), None if b is None else b.cpu(), _seams(c, plan))
    base = au.baseline(c, x, w, b)
    au.check(f"{c.ident()} nb{nb} [{cls}]", got, want.to(DEV), base, torch.float32)
    return plan, x, w, b, got


# B 1 .. 3 with four slots (and B 1 with two): the slots are tiles (5 of them: an item of four and one of a single tile);
# B 3 / nb 2 and B 5 / nb 4: a remainder item of one batch item; B 2, 8: full items only
@pytest.mark.parametrize("B,nb", [(1, 4), (2, 4), (3, 4), (5, 4), (8, 4), (1, 2), (2, 2), (3, 2), (5, 2)])
def test_batch_counts(B, nb, monkeypatch):
    c = C(B, 8, 8, (3000,), (512,))
    plan = _run(c, nb, monkeypatch, want_route=lambda r: r["T"] == 1024 and r["ntiles"] == 5)[0]
    assert plan.route["slot_tiles"] == (1 if B < nb else 0)


@pytest.mark.parametrize("K,T", [(33, 1024), (129, 1024)])
def test_short_kernels(K, T, monkeypatch):
    _run(C(4, 8, 8, (3000,), (K,)), 4, monkeypatch, cls="centred", want_route=lambda r: r["T"] == T)


def test_missing_channels(monkeypatch):
    _run(C(4, 5, 8, (3000,), (512,)), 4, monkeypatch)
    _run(C(3, 5, 8, (3000,), (129,)), 2, monkeypatch)


def test_groups(monkeypatch):
    _run(C(4, 16, 16, (3000,), (512,), g=2), 4, monkeypatch, want_route=lambda r: r["n_ochunks"] == 1)
    _run(C(3, 8, 16, (3000,), (129,)), 4, monkeypatch, want_route=lambda r: r["n_ochunks"] == 2)


def test_no_bias(monkeypatch):
    _run(C(5, 8, 8, (3000,), (512,)), 4, monkeypatch, bias=False)


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate", "circular"])
def test_odd_padding(mode, monkeypatch):
    _run(C(5, 8, 8, (3008,), (129,), p=37, mode=mode), 4, monkeypatch, want_route=lambda r: r["ntiles"] == 4)
    _run(C(3, 8, 8, (3008,), (129,), p=37, mode=mode), 2, monkeypatch, want_route=lambda r: r["ntiles"] == 4)


@pytest.mark.parametrize("nb", [4, 2])
def test_rows_on_and_off_the_line_grid(nb, monkeypatch):
    """Rows of 4096 samples start on 128-byte lines, rows of 4100 do not; both run 7 tiles of 513 valid samples."""
    _run(C(4, 8, 8, (4096,), (512,)), nb, monkeypatch, want_route=lambda r: r["ntiles"] == 7 and r["pers_items"] == 7 * 4 // nb)
    _run(C(4, 8, 8, (4100,), (512,)), nb, monkeypatch, want_route=lambda r: r["ntiles"] == 7)


def test_bench_shape_keeps_full_tiles(monkeypatch):
    """B 32, 8 -> 8 channels, 32768 samples, 512 taps (the bench shape), planner's own choice: the 1024-point tile with four
    slots and V = T - K + 1 = 513 valid samples per tile, 63 tiles, 504 work items.  Tiles of 512 samples on the
    cache-line grid (64 tiles, 512 items) measured slower, profiles/batch_pairs_bench.jsonl: the planner does not round V."""
    _knobs(monkeypatch, {})
    c = C(32, 8, 8, (32768,), (512,))
    x = torch.empty(32, 8, 32768, device=DEV)
    plan = _plan(c, x, torch.empty(8, 8, 512, device=DEV), torch.empty(8, device=DEV))
    r = plan.route
    assert plan.layout[7] == 4 and plan.layout[6] == 0, plan.layout
    assert (r["T"], r["ntiles"], r["pers_items"], r["slot_tiles"]) == (1024, 63, 504, 0), r
    assert r["ntiles"] == -(-(32768 - 511) // 513)


@pytest.mark.parametrize("dtype", [torch.float16])
def test_half_rows(dtype, monkeypatch):
    """16-bit x and y: the bits of widening x, running the float32 plan and rounding y once; against float64 that is one
    rounding of the store (half an ulp, 2**-11 of the value) on top of the float32 plans' bound (route_util.TOL32 of
    max|want|)."""
    from fft_conv_pytorch_amd import functional as fc
    c = C(5, 8, 8, (3000,), (129,), p=64)
    _knobs(monkeypatch, {"FFTCONV_PERS": "4"})
    x, w, b = au.inputs(c, "centred", DEV)
    # (a 16-bit plan is made for 16-bit x, w and bias tensors, but its forward reads the bias as Cout float32 values --
    # functional._forward_native converts it -- so the plan sees bh and the launch gets b, which holds the same integers)
    xh, wh, bh = x.to(dtype), w.to(dtype), b.to(dtype)
    assert torch.equal(bh.float(), b)
    plan = _plan(c, xh, wh, bh)
    assert plan.layout[7] == 4 and plan.layout[6] == 0 and plan.dtype == dtype, (plan.layout, plan.dtype)
    spec = fc.transform_kernel(plan, wh)
    out = torch.full((c.B, c.cout) + plan.out_spatial, float("nan"), dtype=dtype, device=DEV)
    plan.forward(xh.data_ptr(), spec.buf.data_ptr(), b.data_ptr(), out.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert au.finite(out)
    wide = _forward(_plan(c, x, w, b), x, w, b)
    assert torch.equal(out, wide.to(dtype)), "not the rounded float32 result"
    want = au.truth(c, x.cpu(), w.cpu(), b.cpu()).to(DEV)
    err = (out.double() - want).abs()
    assert bool((err <= 2.0 ** -11 * want.abs() + ru.TOL32 * want.abs().max()).all()), err.max().item()


def test_segments_accumulate(monkeypatch):
    """4100 taps run as segments of 1025 on the 2048-point tile: the later segments add into y."""
    c = C(3, 8, 8, (6000,), (4100,), p=50)
    plan = _run(c, 2, monkeypatch, cls="centred", want_route=lambda r: r["T"] == 2048 and r["nseg"] == 4)[0]
    assert plan.layout[3] == 1025


def test_forward_twice_same_bits(monkeypatch):
    c = C(5, 8, 8, (3000,), (512,), p=3, mode="reflect")
    plan, x, w, b, got = _run(c, 4, monkeypatch)
    assert torch.equal(got, _forward(plan, x, w, b))
