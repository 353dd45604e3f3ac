"""The four-slot dense builds of the 1-D batch-sharing kernel with their pass-A twiddles in registers (conv1d_pers.hpp REGTW).

Those builds have no twiddle table in LDS and no barrier in front of their first work item, and a workgroup that runs two
items starts the second item's first transform between the first item's output stores.  A launch hands a workgroup a
second item only when it has more items than the device has CUs, so two cases are sized for that (B 209 and B 261: 269
and 268 items on 256 CUs, second items that are half items, remainder items of one batch item and border tiles).  The
small cases (all 8 -> 8 channels unless noted, 512 taps on 3000 samples: five 1024-point tiles; one item per workgroup):

    B 8    10 full items (run twice: equal bits; and between guard bands);
    B 4    5 items;
    B 5    remainder items of one batch item;
    odd padding in every mode at 129 taps on 3008 samples: border tiles (per-sample loads);
    5 input channels (an empty row), no bias, float16 rows;
    a segmented kernel of 4100 taps on the 2048-point tile and two slots on the 1024-point tile: builds that keep the
    table in LDS and their code.

Every case asserts its route as tests/test_gpu_pers_batch_pairs.py does, runs into an output filled with NaN and is held
to the bound of tests/accuracy_util.py against torch's float64 convolution."""
import pytest
import torch

from tests import accuracy_util as au
from tests import guard_util as gu
from tests import route_util as ru
from tests import test_gpu_pers_batch_pairs as bp

pytestmark = pytest.mark.gpu
DEV = bp.DEV
C = ru.Case


@pytest.fixture(autouse=True)
def _no_knob_plans_afterwards():
    yield
    from fft_conv_pytorch_amd import _native
    _native.clear_plan_cache()


def _five_tiles(r):
    return r["T"] == 1024 and r["ntiles"] == 5


def _run_many_items(c, monkeypatch, cls="offset"):
    """bp._run for a case with more work items than CUs -- only then does the launch hand a workgroup a second item (item
    i + grid, host_1d.cpp build_work_list) -- with the truth from the float64 FFT convolution (exact integers, verified at
    explicit dot products: a direct float64 convolution of this many rows takes the CPU a minute)."""
    bp._knobs(monkeypatch, {"FFTCONV_PERS": "4", **c.env})
    au.assert_exact(c, cls)
    x, w, b = au.inputs(c, cls, DEV)
    plan = bp._plan(c, x, w, b)
    r = plan.route
    cus = torch.cuda.get_device_properties(DEV).multi_processor_count
    assert plan.layout[7] == 4 and plan.layout[6] == 0 and r["ph"] == 1 and r["diag"] == 0, (plan.layout, r)
    assert r["T"] == 1024 and cus < r["pers_items"] <= 2 * cus, f"case not sized for second items on {cus} CUs: {r}"
    got = bp._forward(plan, x, w, b)
    assert au.finite(got), f"{int((~torch.isfinite(got)).sum())} output samples not written / not finite"
    want = au.truth_by_fft(c, x, w, b, bp._seams(c, plan))
    au.check(f"{c.ident()} nb4 [{cls}]", got, want, au.baseline(c, x, w, b), torch.float32)
    return plan, x, w, b, got


def test_second_items_full_and_remainder(monkeypatch):
    """B 209 on five tiles: 260 full items, the last four of them split into halves of two slots for the tail of the launch
    (256 CUs), and 5 remainder items of one batch item: 269 items.  Thirteen workgroups run two items, and the second
    items are the eight halves and the five remainders.  Twice: equal bits; and again between guard bands, because the
    output stores of a first item and the LDS stores of a second one interleave."""
    c = C(209, 8, 8, (3000,), (512,))
    plan, x, w, b, got = _run_many_items(c, monkeypatch)
    assert plan.route["pers_items"] in (265, 269)          # (269 where the tail is split: 256 CUs)
    gu.same_bits(got, bp._forward(plan, x, w, b), "second forward against the first")
    _guarded_forward(plan, c, x, w, b, got)


def test_second_items_on_border_tiles(monkeypatch):
    """B 261 on four tiles with odd reflected padding: 260 full items, border tiles first, and 4 remainder items, two of
    them border tiles, all four as second items (behind the halves of the last four full items, split as above)."""
    plan = _run_many_items(C(261, 8, 8, (3008,), (129,), p=37, mode="reflect"), monkeypatch)[0]
    assert plan.route["pers_items"] in (264, 268) and plan.route["ntiles"] == 4


def test_full_items_same_bits_twice(monkeypatch):
    c = C(8, 8, 8, (3000,), (512,))
    plan, x, w, b, got = bp._run(c, 4, monkeypatch, want_route=lambda r: _five_tiles(r) and r["pers_items"] == 10)
    gu.same_bits(got, bp._forward(plan, x, w, b), "second forward against the first")


def test_one_batch_group(monkeypatch):
    bp._run(C(4, 8, 8, (3000,), (512,)), 4, monkeypatch, want_route=lambda r: _five_tiles(r) and r["pers_items"] == 5)


def test_remainder_items(monkeypatch):
    bp._run(C(5, 8, 8, (3000,), (512,)), 4, monkeypatch, want_route=lambda r: _five_tiles(r) and r["pers_items"] == 10)


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate", "circular"])
def test_border_tiles(mode, monkeypatch):
    bp._run(C(8, 8, 8, (3008,), (129,), p=37, mode=mode), 4, monkeypatch, want_route=lambda r: r["T"] == 1024 and r["ntiles"] == 4)


def test_empty_row(monkeypatch):
    bp._run(C(8, 5, 8, (3000,), (512,)), 4, monkeypatch, want_route=_five_tiles)


def test_no_bias(monkeypatch):
    bp._run(C(8, 8, 8, (3000,), (512,)), 4, monkeypatch, bias=False, want_route=_five_tiles)


def test_half_rows(monkeypatch):
    """float16 x and y: the bits of the float32 plan's result rounded once (as test_gpu_pers_batch_pairs states it), and
    against float64 one rounding of the store on top of the float32 plans' bound."""
    from fft_conv_pytorch_amd import functional as fc
    dtype = torch.float16
    c = C(8, 8, 8, (3000,), (129,), p=64)
    bp._knobs(monkeypatch, {"FFTCONV_PERS": "4"})
    x, w, b = au.inputs(c, "centred", DEV)
    xh, wh, bh = x.to(dtype), w.to(dtype), b.to(dtype)
    assert torch.equal(bh.float(), b)
    plan = bp._plan(c, xh, wh, bh)
    assert plan.layout[7] == 4 and plan.layout[6] == 0 and plan.dtype == dtype, (plan.layout, plan.dtype)
    spec = fc.transform_kernel(plan, wh)
    out = torch.full((c.B, c.cout) + plan.out_spatial, float("nan"), dtype=dtype, device=DEV)
    plan.forward(xh.data_ptr(), spec.buf.data_ptr(), b.data_ptr(), out.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert au.finite(out)
    wide = bp._forward(bp._plan(c, x, w, b), x, w, b)
    assert torch.equal(out, wide.to(dtype)), "not the rounded float32 result"
    want = au.truth(c, x.cpu(), w.cpu(), b.cpu()).to(DEV)
    err = (out.double() - want).abs()
    assert bool((err <= 2.0 ** -11 * want.abs() + ru.TOL32 * want.abs().max()).all()), err.max().item()


def test_segments_on_the_2048_tile(monkeypatch):
    """4100 taps at B 3 with two slots: segments of 1025 taps on the 2048-point tile (the lane split), later ones add into y."""
    c = C(3, 8, 8, (6000,), (4100,), p=50)
    plan = bp._run(c, 2, monkeypatch, cls="centred", want_route=lambda r: r["T"] == 2048 and r["nseg"] == 4)[0]
    assert plan.layout[3] == 1025


def test_two_slots_keep_the_table(monkeypatch):
    """Two slots on the 1024-point tile: two workgroups per CU, the twiddle table in LDS, the code as it was."""
    plan = bp._run(C(8, 8, 8, (3000,), (512,)), 2, monkeypatch, want_route=_five_tiles)[0]
    assert plan.layout[7] == 2


def _guarded_forward(plan, c, x, w, b, got):
    """The forward again with x, w and the bias between guard bands at addresses that are only element-aligned and y from
    a guarded, NaN-filled block.  No guard may change, no input may change, y is fully written and has the bits of
    ``got``, the plain run."""
    from fft_conv_pytorch_amd import functional as fc
    held = [gu.guarded(t, 0xFF, offset=1) for t in (x, w, b)]
    xg, wg, bg = (h[0] for h in held)
    with gu.guarded_empty(0xFF) as ge:
        spec = fc.transform_kernel(plan, wg)
        out = torch.empty((c.B, c.cout) + plan.out_spatial, dtype=x.dtype, device=DEV)
        plan.forward(xg.data_ptr(), spec.buf.data_ptr(), bg.data_ptr(), out.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert ge.violations() == [], ge.violations()
    for _, check in held:
        assert check() == [], check()
    assert au.finite(out)
    gu.same_bits(out, got, "guarded run against the plain run")


def test_guard_bands(monkeypatch):
    c = C(8, 8, 8, (3000,), (512,))
    plan, x, w, b, got = bp._run(c, 4, monkeypatch, want_route=_five_tiles)
    _guarded_forward(plan, c, x, w, b, got)
