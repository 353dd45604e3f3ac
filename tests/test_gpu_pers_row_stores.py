"""The last inverse pass of the four-slot batch-sharing kernel on the 1024-point tile (conv1d_pers.hpp, pers::lower_rows).

A tile keeps its first V = 1024 - K_d + 1 outputs; in the last pass lane o holds the outputs o + 32 k, k = 0 .. 31.  Where
V <= 17 * 32 = 544 (K_d >= 481) no row past k = 16 is stored, and the plan runs a build whose last radix-2 stage computes
the sums of its butterflies and the one difference that is row 16 (fft_regs<.., LOWER>), and whose store code ends at row
16.  What can go wrong, and what the cases are sized for: row 16 partly valid (V = 513: lane 0 alone; V = 525: 13 lanes),
fully valid (V = 544, the largest V of the build), V = 545 (one sample in row 17: the full build must run), a last tile
shorter than V, slots without an imaginary part (odd batch counts, slots that are tiles), missing input channels, every
padding mode, 16-bit rows, the transposed plan that computes dX, and a kernel short enough that the build is not taken.

Every case asserts the 1024-point tile with four slots from the plan (layout word 7 = 4 slots, word 6 = 0, route T) and
which of the two builds the plan's V selects, and is held on integer inputs, whose float64 convolution is exact, to the
bound of tests/accuracy_util.py against torch's float64 convolution.  The segmented plan of the last test runs 1025-tap
segments, which never fit the 1024-point tile: it runs the two-slot segments build on the 2048-point tile, whose code did
not change, and is here because its store loop shares the source lines."""
import pytest
import torch

from tests import accuracy_util as au
from tests import route_util as ru
from tests import test_gpu_routes as tr

pytestmark = pytest.mark.gpu
DEV = tr.DEV
C = ru.Case
LOWER_ROWS_MAX_V = 17 * 32       # pers::lower_rows_max_v(32)


@pytest.fixture(autouse=True)
def _no_knob_plans_afterwards():
    yield
    from fft_conv_pytorch_amd import _native
    _native.clear_plan_cache()


def _plan(c, x, w, b):
    from fft_conv_pytorch_amd import functional as fc
    kw = tr._kw(c)
    return fc._plan_for(x, w, b, kw["stride"], kw["padding"], kw["dilation"], c.g, "constant" if c.tr else c.mode,
                        transposed=c.tr, output_padding=kw.get("output_padding", 0))


def _forward(plan, x, w, b):
    """transform_kernel + Plan.forward into an output filled with NaN (a sample never stored stays NaN)."""
    from fft_conv_pytorch_amd import functional as fc
    spec = fc.transform_kernel(plan, w)
    out = torch.full((x.shape[0], plan.key[3]) + plan.out_spatial, float("nan"), dtype=x.dtype, device=DEV)
    stream = torch.cuda.current_stream(x.device).cuda_stream
    plan.forward(x.data_ptr(), spec.buf.data_ptr(), None if b is None else b.data_ptr(), out.data_ptr(), None, stream)
    torch.cuda.synchronize()
    return out


def _assert_build(c, plan, lower, ntiles=None, slot_tiles=0):
    """Four slots on the 1024-point tile, and the build the plan's V selects (lower: pers::lower_rows)."""
    r = plan.route
    assert plan.layout[7] == 4 and plan.layout[6] == 0, plan.layout
    assert r["T"] == 1024 and r["ph"] == 1 and r["diag"] == 0 and r["nseg"] == 1 and r["slot_tiles"] == slot_tiles, r
    V = 1024 - ((c.k[0] - 1) * c.tup(c.d)[0] + 1) + 1
    assert (V <= LOWER_ROWS_MAX_V) == lower, f"case not sized as intended: V = {V}"
    assert ntiles is None or r["ntiles"] == ntiles, r
    return V


def _run(c, monkeypatch, lower, cls="offset", ntiles=None, slot_tiles=0):
    tr._knobs(monkeypatch, {"FFTCONV_PERS": "4"})
    au.assert_exact(c, cls)
    x, w, b = au.inputs(c, cls, DEV)
    plan = _plan(c, x, w, b)
    V = _assert_build(c, plan, lower, ntiles, slot_tiles)
    got = _forward(plan, x, w, b)
    assert au.finite(got), f"{int((~torch.isfinite(got)).sum())} output samples not written / not finite"
    want = au.truth(c, x.cpu(), w.cpu(), b.cpu(), [[j * V for j in range(1, plan.route["ntiles"])]])
    au.check(f"{c.ident()} V{V} [{cls}]", got, want.to(DEV), au.baseline(c, x, w, b), torch.float32)
    return plan, x, w, b, got


def test_border_tiles_and_a_short_last_tile(monkeypatch):
    """V = 513: rows 0 .. 15 and lane 0 of row 16; three tiles, the last one of 511 outputs."""
    _run(C(4, 8, 8, (2048,), (512,)), monkeypatch, lower=True, ntiles=3)


@pytest.mark.parametrize("K,lower", [(500, True), (481, True), (480, False)])
def test_around_the_largest_window_of_the_build(K, lower, monkeypatch):
    """V = 525: 13 lanes of row 16; V = 544: all of row 16, the largest V of the build; V = 545: lane 0 of row 17 --
    the full build."""
    _run(C(4, 8, 8, (2048,), (K,)), monkeypatch, lower=lower)


def test_odd_slot_counts(monkeypatch):
    """B 5: a remainder item of one slot (no imaginary part); B 3: the slots are tiles, 7 of them in items of 4 and 3."""
    _run(C(5, 8, 8, (4096,), (512,)), monkeypatch, lower=True, ntiles=7)
    _run(C(3, 8, 8, (4096,), (512,)), monkeypatch, lower=True, ntiles=7, slot_tiles=1)


def test_missing_input_channels(monkeypatch):
    """Cin 6: two empty sequences per slot pair.  K 400 (V = 625) runs the full build, K 512 the lower rows."""
    _run(C(4, 6, 8, (2048,), (400,)), monkeypatch, lower=False)
    _run(C(4, 6, 8, (2048,), (512,)), monkeypatch, lower=True)


def test_window_past_row_16_keeps_the_full_build(monkeypatch):
    """K 300: V = 725, rows 0 .. 22 are stored."""
    _run(C(4, 8, 8, (2048,), (300,)), monkeypatch, lower=False, ntiles=3)


@pytest.mark.parametrize("mode", ["constant", "reflect", "replicate", "circular"])
def test_same_padding(mode, monkeypatch):
    """K 512 padded to the length of the row: 256 samples on both sides (an even kernel has no symmetric 'same' padding;
    this is one output more), 2049 outputs in four tiles, the first and the last on the padding."""
    _run(C(4, 8, 8, (2048,), (512,), p=256, mode=mode), monkeypatch, lower=True, ntiles=4)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16])
def test_16_bit_rows(dtype, monkeypatch):
    """The half_io build: the bits of widening x, running the float32 plan and rounding y once.  Against float64 that is one
    rounding of the store (half an ulp: 2**-11 of the value in float16, 2**-8 in bfloat16) on top of the float32 plans'
    bound (route_util.TOL32 of max|want|)."""
    from fft_conv_pytorch_amd import functional as fc
    c = C(4, 8, 8, (2048,), (512,))
    tr._knobs(monkeypatch, {"FFTCONV_PERS": "4"})
    x, w, b = au.inputs(c, "centred", DEV)
    xh, wh, bh = x.to(dtype), w.to(dtype), b.to(dtype)
    assert torch.equal(xh.float(), x) and torch.equal(wh.float(), w) and torch.equal(bh.float(), b)
    plan = _plan(c, xh, wh, bh)
    assert plan.dtype == dtype, plan.dtype
    _assert_build(c, plan, True, 3)
    spec = fc.transform_kernel(plan, wh)
    out = torch.full((c.B, c.cout) + plan.out_spatial, float("nan"), dtype=dtype, device=DEV)
    plan.forward(xh.data_ptr(), spec.buf.data_ptr(), b.data_ptr(), out.data_ptr(), None, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert au.finite(out)
    wide_plan = _plan(c, x, w, b)
    _assert_build(c, wide_plan, True, 3)
    wide = _forward(wide_plan, x, w, b)
    assert torch.equal(out, wide.to(dtype)), "not the rounded float32 result"
    want = au.truth(c, x.cpu(), w.cpu(), b.cpu()).to(DEV)
    half_ulp = 2.0 ** -11 if dtype == torch.float16 else 2.0 ** -8
    err = (out.double() - want).abs()
    assert bool((err <= half_ulp * want.abs() + ru.TOL32 * want.abs().max()).all()), err.max().item()


def test_input_gradient_plan(monkeypatch):
    """dX of B 4, L 2048, K 512 is the transposed plan of dY (1537 samples): padding 511 on both sides, the same tile,
    slots and build."""
    _run(C(4, 8, 8, (1537,), (512,), tr=True), monkeypatch, lower=True, ntiles=4)


def test_forward_twice_same_bits(monkeypatch):
    plan, x, w, b, got = _run(C(5, 8, 8, (2048,), (512,), p=3, mode="reflect"), monkeypatch, lower=True)
    assert torch.equal(got, _forward(plan, x, w, b))


def test_segments_add_into_y(monkeypatch):
    """K 2048 runs as two segments of 1025 and 1023 taps on the 2048-point tile with two slots (see above): the second
    segment adds into y."""
    tr._knobs(monkeypatch, {"FFTCONV_PERS": "2"})
    c = C(4, 8, 8, (4096,), (2048,))
    au.assert_exact(c, "centred")
    x, w, b = au.inputs(c, "centred", DEV)
    plan = _plan(c, x, w, b)
    r = plan.route
    assert r["nseg"] == 2 and plan.layout[3] == 1025 and r["T"] == 2048 and plan.layout[7] == 2 and plan.layout[6] == 0, (r, plan.layout)
    got = _forward(plan, x, w, b)
    assert au.finite(got)
    V = 2048 - 1025 + 1
    want = au.truth(c, x.cpu(), w.cpu(), b.cpu(), [[j * V for j in range(1, r["ntiles"])]])
    au.check(f"{c.ident()} segments", got, want.to(DEV), au.baseline(c, x, w, b), torch.float32)
