"""The second item's sample requests in front of the mix's last barrier (conv1d_pers.hpp, pers::early_fetch).

The four-slot dense builds on the 1024-point tile take the feature; only a workgroup that runs TWO items executes the
moved code (the first item requests the second one's samples).  The planner launches max(ceil(items / 2), min(items, CUs))
workgroups, so a workgroup gets a second item only where the launch has more items than the device has CUs.

The cases of 8 -> 8 channels, 512 taps and L = 2048 (1537 outputs in three tiles of V = 513) at batch 2 .. 8 have 2 .. 6
items: on a device of more than 6 CUs every workgroup runs ONE item, `two` is false everywhere and the moved fetch is never
executed.  They are kept -- they hold the build to torch's float64 convolution on its one-item path, with a remainder item
of two slots in four (batch 6), slots that are tiles (batch 2), reflected borders, 16-bit rows and both sides of the
lower_rows threshold (481 / 480 taps) -- and each asserts the item count and that no workgroup has a second item, so that
nobody reads them as covering more.

What runs the moved fetch are the two launches below them, sized by the item count (a 256-CU device is asserted):
  * batch 512, reflect padding 3: four tiles (1543 outputs), 512 full items in 256 workgroups, EVERY workgroup two items;
    the second items are the 128 items of tile 3 (border branch of fetch) and the 128 of tile 1 (interior branch);
  * batch 344: 258 full items, of which the planner splits the last two into four items of two slots: 260 items in 256
    workgroups -- four workgroups whose second item has nbc = 2 in four slots (slot pair B reads zeros, its stores are
    dropped), 252 workgroups with `two` false.
A float64 convolution of 512 batch items costs 12 s on the host, so these two are checked in two steps that together cover
every output sample: every 32nd batch item against torch's float64 convolution to the bound of tests/accuracy_util.py, and
the whole output bit for bit against the same rows run in launches of 64 batch items, whose workgroups run one item each
(the arithmetic of a slot pair does not depend on what else the launch holds).  Both launches run twice and must give the
same bits: the samples are requested earlier now, and a race would show as a difference between runs."""
import pytest
import torch

from tests import accuracy_util as au
from tests import route_util as ru
from tests import test_gpu_routes as tr

pytestmark = pytest.mark.gpu
DEV = tr.DEV
C = ru.Case
LOWER_ROWS_MAX_V = 17 * 32       # pers::lower_rows_max_v(32)
NB = 4
# four slots on the 1024-point tile: FFTCONV_PERS as the other tests of the kernel set it, and the tile named too (left to the
# planner, two batch items of 2048 samples run the 2048-point tile without slots)
KNOBS = {"FFTCONV_PERS": "4", "FFTCONV_TILE": "1024"}


@pytest.fixture(autouse=True)
def _no_knob_plans_afterwards():
    yield
    from fft_conv_pytorch_amd import _native
    _native.clear_plan_cache()


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
    plan.forward(x.data_ptr(), spec.buf.data_ptr(), b.data_ptr(), out.data_ptr(), None, stream)
    torch.cuda.synchronize()
    return out


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _assert_plan(c, plan, items, second_items, lower=True, slot_tiles=0):
    """The early_fetch build (four slots on the 1024-point tile, dense, no phases, no segments: what pers_build gives the
    feature to), with or without the lower rows, and the item split the case is sized for."""
    r = plan.route
    assert plan.layout[7] == NB and plan.layout[6] == 0, plan.layout
    assert r["T"] == 1024 and r["ph"] == 1 and r["diag"] == 0 and r["nseg"] == 1 and r["slot_tiles"] == slot_tiles, r
    V = 1024 - c.k[0] + 1
    assert (V <= LOWER_ROWS_MAX_V) == lower, f"case not sized as intended: V = {V}"
    assert r["pers_items"] == items, r
    grid = max((items + 1) // 2, min(items, _cus()))           # the planner's launch (host_1d.cpp)
    assert items - grid == second_items, f"{items} items in {grid} workgroups on {_cus()} CUs"
    return V


def _items(B, ntiles, slot_tiles=0):
    """full items and one remainder item per tile; or, where the plan's slots are tiles, groups of four tiles of a batch item"""
    return B * -(-ntiles // NB) if slot_tiles else ntiles * (B // NB + (1 if B % NB else 0))


def _small(c, monkeypatch, ntiles, lower=True, cls="offset", twice=True):
    tr._knobs(monkeypatch, KNOBS)
    au.assert_exact(c, cls)
    x, w, b = au.inputs(c, cls, DEV)
    plan = _plan(c, x, w, b)
    st = plan.route["slot_tiles"]
    V = _assert_plan(c, plan, _items(c.B, ntiles, st), 0, lower, slot_tiles=st)
    assert plan.route["ntiles"] == ntiles, plan.route
    got = _forward(plan, x, w, b)
    assert au.finite(got), f"{int((~torch.isfinite(got)).sum())} output samples not written / not finite"
    want = au.truth(c, x.cpu(), w.cpu(), b.cpu(), [[j * V for j in range(1, ntiles)]])
    au.check(f"{c.ident()} V{V} [{cls}]", got, want.to(DEV), au.baseline(c, x, w, b), torch.float32)
    if twice:
        assert torch.equal(got, _forward(plan, x, w, b)), "two runs of one plan differ"


@pytest.mark.parametrize("B", [2, 4, 6, 8])
def test_one_item_per_workgroup(B, monkeypatch):
    """Up to 6 items (batch 2: two slots in four, or tiles as slots; batch 6: three full items and three of two slots in
    four), each alone in its workgroup."""
    _small(C(B, 8, 8, (2048,), (512,)), monkeypatch, ntiles=3)


def test_reflected_borders(monkeypatch):
    """padding 3: 1543 outputs in four tiles, the first and the last two on the border branch of fetch."""
    _small(C(6, 8, 8, (2048,), (512,), p=3, mode="reflect"), monkeypatch, ntiles=4)


@pytest.mark.parametrize("K,lower", [(481, True), (480, False)])
def test_both_sides_of_the_lower_rows_threshold(K, lower, monkeypatch):
    """481 taps (V = 544) is the smallest kernel of early_fetch | lower_rows, 480 (V = 545) runs early_fetch alone."""
    _small(C(8, 8, 8, (2048,), (K,)), monkeypatch, ntiles=3, lower=lower)


def test_16_bit_rows(monkeypatch):
    """early_fetch | lower_rows | half_io: the bits of widening x, running the float32 plan and rounding y once; against
    float64 one rounding of the store (2**-11 of the value) on top of the float32 plans' bound."""
    from fft_conv_pytorch_amd import functional as fc
    c = C(8, 8, 8, (2048,), (512,))
    tr._knobs(monkeypatch, KNOBS)
    x, w, b = au.inputs(c, "centred", DEV)
    xh, wh, bh = x.half(), w.half(), b.half()
    assert torch.equal(xh.float(), x) and torch.equal(wh.float(), w) and torch.equal(bh.float(), b)
    plan = _plan(c, xh, wh, bh)
    assert plan.dtype == torch.float16, plan.dtype
    _assert_plan(c, plan, 6, 0)
    spec = fc.transform_kernel(plan, wh)
    out = torch.full((c.B, c.cout) + plan.out_spatial, float("nan"), dtype=torch.float16, device=DEV)
    plan.forward(xh.data_ptr(), spec.buf.data_ptr(), b.data_ptr(), out.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert au.finite(out)
    wide_plan = _plan(c, x, w, b)
    _assert_plan(c, wide_plan, 6, 0)
    assert torch.equal(out, _forward(wide_plan, x, w, b).half()), "not the rounded float32 result"
    want = au.truth(c, x.cpu(), w.cpu(), b.cpu()).to(DEV)
    err = (out.double() - want).abs()
    assert bool((err <= 2.0 ** -11 * want.abs() + ru.TOL32 * want.abs().max()).all()), err.max().item()


def _two_items(c, monkeypatch, ntiles, items, second_items, cls="offset"):
    """A launch whose workgroups run second items: see the module docstring for the two steps of the check."""
    tr._knobs(monkeypatch, KNOBS)
    assert _cus() == 256, f"sized for the 256 CUs of an MI355X, not {_cus()}"
    au.assert_exact(c, cls)
    x, w, b = au.inputs(c, cls, DEV)
    plan = _plan(c, x, w, b)
    V = _assert_plan(c, plan, items, second_items)
    assert plan.route["ntiles"] == ntiles, plan.route
    got = _forward(plan, x, w, b)
    assert au.finite(got), f"{int((~torch.isfinite(got)).sum())} output samples not written / not finite"
    assert torch.equal(got, _forward(plan, x, w, b)), "two runs of one plan differ"
    # every 32nd batch item against float64 (an item holds batch items 4i .. 4i + 3: items of every tile, first and second)
    sel = torch.arange(0, c.B, 32)
    cs = C(len(sel), c.cin, c.cout, c.size, c.k, p=c.p, mode=c.mode)
    xs = x[sel].contiguous()
    want = au.truth(cs, xs.cpu(), w.cpu(), b.cpu(), [[j * V for j in range(1, ntiles)]])
    au.check(f"{c.ident()} V{V} [{cls}], every 32nd batch item", got[sel], want.to(DEV), au.baseline(cs, xs, w, b), torch.float32)
    # the whole output against launches of 64 batch items: at most 64 items each, one per workgroup
    for b0 in range(0, c.B, 64):
        xc = x[b0:b0 + 64].contiguous()
        cc = C(xc.shape[0], c.cin, c.cout, c.size, c.k, p=c.p, mode=c.mode)
        pc = _plan(cc, xc, w, b)
        _assert_plan(cc, pc, _items(cc.B, ntiles), 0)
        assert torch.equal(got[b0:b0 + 64], _forward(pc, xc, w, b)), f"batch items {b0} .. differ from their one-item launch"


def test_every_workgroup_runs_two_items(monkeypatch):
    """512 items in 256 workgroups; second items on both branches of fetch (tile 3 on the border, tile 1 interior)."""
    _two_items(C(512, 8, 8, (2048,), (512,), p=3, mode="reflect"), monkeypatch, ntiles=4, items=512, second_items=256)


def test_second_items_of_two_slots_and_workgroups_without_one(monkeypatch):
    """258 full items, the last two split into four of two slots: 260 items, 256 workgroups, four second items with
    nbc = 2 in four slots; the other 252 workgroups have `two` false."""
    _two_items(C(344, 8, 8, (2048,), (512,)), monkeypatch, ntiles=3, items=260, second_items=4)
