"""The 2 GiB and 4 GiB addressing thresholds of the float32 1-D kernels and of the 2-D / 3-D passes, each pinned from both
sides (the audit table: one entry of THRESHOLDS per guard that stands between a shape and a 32-bit
buffer offset).

A side is a route_util.Case just below or at / above the threshold of its guard, with what must happen there: the route
words of its plan (fc_debug_route), or the refusal's class and text, raised by the planner before anything is launched.  A
side that runs is checked in FULL against the exact sparse truth of tests/big_util.py: inputs that are zero but for windows
of small integers around every multiple of 2**30 bytes and at the ends of the rows, held in guarded blocks; the output
allocated under guard_util.guarded_empty(0xFF), so that a sample never stored is a NaN and a store past the end lands in a
guard; max|got - want| <= TOL32 max|want| over every sample.  The bias is a different integer per channel: a dead store that
lands in another row of y carries the wrong one even where the sparse convolution is zero.  Plan-only sides create the plan
and launch nothing (their smallest running shapes need thousands of channels, or rows of 16 GiB).

Memory: a side plans its peak of allocated bytes (``_planned``), is skipped when the device has less free, may not plan more
than CAP, and torch.cuda.max_memory_allocated() must stay within 10 % of the plan.  The last test fails unless both sides of
every entry ran in this run of the file (or were skipped for memory, which it lists)."""
import math
import time
from dataclasses import dataclass
from typing import Callable, Optional

import numpy as np
import pytest
import torch

from tests import accuracy_util as au
from tests import big_util as bu
from tests import guard_util as gu
from tests import route_util as ru
from tests.test_gpu_routes import _knobs, _kw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GIB = 1 << 30
CAP = 32 * GIB
C = ru.Case
_1d, _nd = ru._1d, ru._nd
GENERAL = _1d(pers_nb=0, wide=0, dense=0, diag=0, bd_gs=0)
ROWS = []          # one dict per side that ran: scripts/threshold_report.py writes them out
DONE = {}          # (entry, side) -> "ran" | "plan-only" | "refused" | "skipped: ..."


@dataclass
class Side:
    case: ru.Case
    pred: Optional[Callable] = None          # route predicate of the plan
    raises: Optional[tuple] = None           # (exception class, text) of the refusal
    plan_only: bool = False
    dtype: torch.dtype = torch.float32
    kind: str = "forward"                    # "forward" | "wgrad" (1-D: dW, db, dX) | "wgrad_nd" (dW by fc_wgrad_nd)
    extra: Optional[Callable] = None         # (plan, case): asserts, or returns whether the case is sized as intended
    long: Optional[str] = None               # long filters: "causal" | "causal-nlc" | "decim" | "transpose" | "index" | "geom"


@dataclass
class Threshold:
    name: str
    site: str
    guard: str
    env: dict
    below: Side
    above: Side


def _x_bytes(c):
    return 4 * c.B * c.cin * math.prod(c.size)


def _dy_bytes(c):
    return 4 * c.B * c.cout * math.prod(au.out_spatial(c))


def _c2c_span(plan, c):
    """bytes the 16 sequences of a c2c_fwd workgroup reach along the middle axis of a 3-D plan"""
    r = plan.route
    return (15 * (r["Tx"] // 2 * r["nxt"]) * c.size[1] + c.size[1]) * 8


def _f64_fused_items(c):
    """work-items of the fused pass of a float64 2-D plan with 2048-point tiles on both axes: tiles x columns x T / 2"""
    lf = c.size[0] - c.k[0] + 1
    return -(-lf // (2048 - c.k[0] + 1)) * 1025 * 1024


def _weight_bytes(c):
    return 4 * math.prod(c.wshape)


def _buffer_path(plan, c):
    assert _weight_bytes(c) < 0x7F000000, _weight_bytes(c)


def _pointer_path(plan, c):
    assert _weight_bytes(c) >= 0x7F000000, _weight_bytes(c)


def _spectrum_below_4gib(plan, c):
    assert (1 << 32) - (1 << 27) <= plan.spectrum_bytes < 1 << 32, plan.spectrum_bytes


def _slab_128(plan, c):
    # workspace = one slab of X and Y rows: 128 rows of G * NF * (Cig_pad + Cog_pad) complex values
    nf = plan.route["T"] // 2 + 1
    row = nf * (c.cin + c.cout) * 8
    assert plan.workspace_bytes == 128 * row and nf * 128 * max(c.cin, c.cout) * 8 < 1 << 32, plan.workspace_bytes


L25, L24 = 1 << 25, 1 << 24
THRESHOLDS = [
    Threshold("1d-row-4gib", "conv1d_fused.hpp:147", "host_1d.cpp:224", {},
              Side(C(1, 1, 1, ((1 << 30) - 64,), (33,)), pred=GENERAL),
              Side(C(1, 1, 1, (1 << 30,), (33,)), raises=(NotImplementedError, "32-bit buffer offsets"))),
    Threshold("1d-sharing-x", "conv1d_pers.hpp:144,173", "host_1d.cpp:18", {"FFTCONV_PERS": "4"},
              Side(C(4, 8, 8, (L25 - 2048,), (129,)), pred=_1d(pers_nb=4)),
              Side(C(4, 8, 8, (L25,), (129,)), pred=GENERAL)),
    # ES = 2 against a guard that counts 4-byte samples
    Threshold("1d-sharing-x-float16", "conv1d_pers.hpp:144,173", "host_1d.cpp:18", {"FFTCONV_PERS": "4"},
              Side(C(4, 8, 8, (L25 - 2048,), (129,)), pred=_1d(pers_nb=4), dtype=torch.float16),
              Side(C(4, 8, 8, (L25,), (129,)), pred=GENERAL, dtype=torch.float16)),
    # zero padding makes Lout long while L stays short: the y resource of an out-chunk (8 rows of Lout samples) must end
    # below bit 31, the mark of a dead store.  Past the guard the general kernel (plain pointers) takes the shape.
    Threshold("1d-sharing-y", "conv1d_pers.hpp:749-767,801-824,842-897", "host_1d.cpp:22", {"FFTCONV_PERS": "2"},
              Side(C(2, 8, 8, (L25 - 4096,), (129,), p=1 << 23), pred=_1d(pers_nb=2)),
              Side(C(2, 8, 8, (L25 - 4096,), (129,), p=L24 + 4096), pred=GENERAL)),
    # the same guard from just below (the 8 rows end 32 KiB under 0x7F000000 bytes) and from where the kernel would go wrong
    # without it: from 7 Lout samples = 2 GiB on, the offset of a dead store of row 6 has bit 31 set before the mark is
    # ORed in, and the store lands at the start of row 7
    Threshold("1d-sharing-y-row7", "conv1d_pers.hpp:749-767,801-824,842-897", "host_1d.cpp:22", {"FFTCONV_PERS": "2"},
              Side(C(2, 8, 8, (L25 - 4096,), (129,), p=16516672), pred=_1d(pers_nb=2)),
              Side(C(2, 8, 8, (L25 - 4096,), (129,), p=21700000), pred=GENERAL)),
    Threshold("1d-wide-x", "conv1d_wide.hpp:49", "host_1d.cpp:278", {},
              Side(C(4, 16, 8, (L24 - 2048,), (100,)), pred=_1d(wide=1)),
              Side(C(4, 16, 8, (L24,), (100,)), pred=_1d(wide=0, dense=0, pers_nb=0))),
    # (Lout = L - 64: the below side's group of 16 output rows ends 1 KiB under 2 GiB)
    Threshold("1d-dense-y", "dense1d.hpp:185-200", "host_1d.cpp:262", {"FFTCONV_DENSE": "2"},
              Side(C(1, 16, 16, (L25 + 48,), (65,)), pred=_1d(dense=1)),
              Side(C(1, 16, 16, (L25 + 64,), (65,)), pred=_1d(dense=0))),
    Threshold("1d-spectrum-weight", "spectrum1d.hpp:65", "host_1d.cpp:424", {},
              Side(C(1, 1024, 1024, (4096,), (1000,), g=2), pred=_1d(), extra=_buffer_path),
              Side(C(1, 1024, 1024, (4096,), (1024,), g=2), pred=_1d(), extra=_pointer_path)),
    Threshold("wgrad1d-tensor", "wgrad1d.hpp:107-108,359-360", "host_1d.cpp:541", {},
              # (two output channels: the forward-plan dW that takes over past the guard holds a padded and a gathered copy
              #  of x and of dY and a spectrum the size of dY, 33 GiB with eight)
              Side(C(8, 8, 2, (L24 - 64,), (33,)), kind="wgrad", pred=lambda slices: slices > 0),
              Side(C(8, 8, 2, (L24,), (33,)), kind="wgrad", pred=lambda slices: slices == 0)),
    # eight output channels: dY lies 2 KiB under 4 GiB as well (host_1d.cpp:542); past the guard only the geometry is asked
    Threshold("wgrad1d-tensor-dy", "wgrad1d.hpp:107-108,359-360", "host_1d.cpp:541-542", {},
              Side(C(8, 8, 8, (L24 - 64,), (33,)), kind="wgrad", pred=lambda slices: slices > 0),
              Side(C(8, 8, 8, (L24,), (33,)), kind="wgrad", plan_only=True, pred=lambda slices: slices == 0)),
    # plan-only: the smallest running shapes hold 512 x 512 channels at the 4096-point tile, or 8192 channels
    Threshold("1d-spectrum-4gib", "conv1d_fused.hpp:149", "host_1d.cpp:337", {},
              Side(C(1, 504, 516, (8192,), (2049,)), plan_only=True, pred=_1d(T=4096, chunk_launches=1),
                   extra=_spectrum_below_4gib),
              Side(C(1, 512, 516, (8192,), (2049,)), raises=(NotImplementedError, "exceeds 4 GiB"))),
    Threshold("1d-dense-slab", "dense1d.hpp:153,277", "host_1d.cpp:263", {"FFTCONV_DENSE": "2"},
              Side(C(1, 8168, 16, (125000,), (65,)), plan_only=True, pred=_1d(dense=1, T=1024), extra=_slab_128),
              Side(C(1, 8192, 16, (125000,), (65,)), plan_only=True, pred=_1d(dense=0))),
    # padded extents and stride-1 output counts are ints in the plan and in every kernel's arguments (plan-only: a row of
    # 2**31 output samples is 8 GiB)
    Threshold("axis-extent-int", "fc_api.cpp:223-244", "fc_api.cpp:205-212", {},
              Side(C(1, 1, 1, (1 << 20,), (33,), p=(1 << 30) - (1 << 19) - 1), plan_only=True, pred=GENERAL),
              Side(C(1, 1, 1, (1 << 20,), (33,), p=(1 << 30) - (1 << 19)), raises=(NotImplementedError, "32-bit positions"))),
    # ------------------------------------------------------------------------------------------------ float32 2-D / 3-D
    # rows_r2c reads a zero-padded signal through one resource over the whole tensor while it is below 4 GiB, through
    # row pointers staged in LDS from there on.  (17 x tiles of 1024 bin columns: the column pass takes its pointer path,
    # nd_passes.hpp:704, on both sides.)
    Threshold("nd-src-4gib", "nd_passes.hpp:181", "host_nd.cpp:475", {},
              Side(C(1, 1, 1, (32767, 32768), (3, 3), p=1), pred=_nd(planes=0), extra=lambda plan, c: _x_bytes(c) < 0xFFFFFFFF),
              Side(C(1, 1, 1, (32768, 32768), (3, 3), p=1), pred=_nd(planes=0),
                   extra=lambda plan, c: _x_bytes(c) >= 0xFFFFFFFF)),
    # the same guard on the dY of a weight-gradient plan (host_nd.cpp:391), which fc_wgrad_nd reads as the kernel of the
    # swapped convolution: 64 images of 8192 x 2047 / 2048 samples, the first axis in segments of taps
    Threshold("nd-src-4gib-dy", "nd_passes.hpp:181", "host_nd.cpp:391", {},
              Side(C(8, 1, 8, (8194, 2049), (3, 3)), kind="wgrad_nd", pred=lambda c: _dy_bytes(c) < 0xFFFFFFFF),
              Side(C(8, 1, 8, (8194, 2050), (3, 3)), kind="wgrad_nd", pred=lambda c: _dy_bytes(c) >= 0xFFFFFFFF)),
    # a block of Tx/2 = 512 bin columns over all rows: 0.92 of the 2 GiB it may span (rows % 16 = 5: the last block of rows
    # marks its missing rows dead), refused past it
    Threshold("nd-bin-columns", "nd_passes.hpp:262,485", "host_nd.cpp:187", {"FFTCONV_XTILE": "0", "FFTCONV_PLANES": "0"},
              Side(C(1, 1, 1, (480005, 600), (3, 3)), pred=_nd(planes=0, Tx=1024, nxt=1),
                   extra=lambda plan, c: 0.9 * 2 ** 31 < 512 * c.size[0] * 8 < 2 ** 31),
              Side(C(1, 1, 1, (540000, 600), (3, 3)), raises=(NotImplementedError, "2 GiB"))),
    # the column pass reads the 8 channel rows of a chunk (7 ncol + 1) NLEN complex values apart through one resource
    # while that is below 2 GiB, through pointers past it; likewise its stores of the 8 output rows of a chunk
    Threshold("nd-span-fusedc-load", "nd_passes.hpp:704", "nd_passes.hpp:704", {"FFTCONV_XTILE": "0", "FFTCONV_PLANES": "0"},
              Side(C(1, 8, 1, (74800, 600), (3, 3)), pred=_nd(planes=0, Tx=1024, nxt=1),
                   extra=lambda plan, c: (7 * 512 + 1) * c.size[0] * 8 < 0x7fffffff),
              Side(C(1, 8, 1, (75000, 600), (3, 3)), pred=_nd(planes=0, Tx=1024, nxt=1),
                   extra=lambda plan, c: (7 * 512 + 1) * c.size[0] * 8 >= 0x7fffffff)),
    Threshold("nd-span-fusedc-store", "nd_passes.hpp:820", "nd_passes.hpp:820", {"FFTCONV_XTILE": "0", "FFTCONV_PLANES": "0"},
              Side(C(1, 1, 8, (74800, 600), (3, 3)), pred=_nd(planes=0, Tx=1024, nxt=1, cob=8),
                   extra=lambda plan, c: (7 * 512 + 1) * (c.size[0] - 2) * 8 < 0x7fffffff),
              Side(C(1, 1, 8, (75000, 600), (3, 3)), pred=_nd(planes=0, Tx=1024, nxt=1, cob=8),
                   extra=lambda plan, c: (7 * 512 + 1) * (c.size[0] - 2) * 8 >= 0x7fffffff)),
    # the middle-axis pass of a 3-D plan reads the 16 sequences of a workgroup 15 Fxt Sp1 complex values apart (512-point
    # transforms: 16 sequences per workgroup; 35 x tiles of 1024 bin columns)
    Threshold("nd-span-c2c-fwd", "nd_passes.hpp:328", "nd_passes.hpp:328", {"FFTCONV_PLANES": "0"},
              Side(C(1, 1, 1, (16, 480, 70000), (3, 3, 3)), pred=_nd(planes=0, Tm=512, nyt=1),
                   extra=lambda plan, c: _c2c_span(plan, c) < 0x7fffffff),
              Side(C(1, 1, 1, (16, 500, 70000), (3, 3, 3)), pred=_nd(planes=0, Tm=512, nyt=1),
                   extra=lambda plan, c: _c2c_span(plan, c) >= 0x7fffffff)),
    # 4 C rows Fxt 8 < 2**31 with C = 8 and Fxt = 10 tiles of 32 bin columns: 26214 rows
    Threshold("nd-colz-guard", "planes3d.hpp:385-530", "host_nd.cpp:255", {},
              Side(C(1, 8, 8, (26000, 600), (3, 3)), pred=_nd(planes=2, Tx=64, nxt=10)),
              Side(C(1, 8, 8, (26300, 600), (3, 3)), pred=_nd(planes=0, Tx=64, nxt=10))),
    # 2 C Sp0 tiles < 65536 with C = 32 and 18 tiles: 56 padded planes (the shapes of route_util's two guard routes)
    Threshold("nd-planes-guard", "planes3d.hpp:385-530", "host_nd.cpp:241", {},
              Side(C(1, 8, 32, (54, 500, 64), (3, 3, 3), p=1), pred=_nd(planes=1, Tx=64, Tm=64)),
              Side(C(1, 8, 32, (56, 500, 64), (3, 3, 3), p=1), pred=_nd(planes=0, Tx=64, Tm=64))),
    # ------------------------------------------------------------------------------------------------ long filters
    # depthwise, K = L, causal: every row is 2 MiB, the tensor passes 4 GiB between 15 and 16 batch items (row bases past
    # an int).  (B4 C256 K = L = 2**20 + 4096 is the same tensor, but one pair of batch items holds a workspace of 512 rows
    # x 2**22 points x 8 bytes = 16 GiB and the spectrum 8 GiB: 36 GiB with x and y, over CAP; 128 channels of half the
    # length need 4 + 2 GiB.)
    Threshold("long-row-bases", "long1d.hpp:199-228,542-552", "host_long.cpp:79-82", {},
              Side(C(15, 128, 128, ((1 << 19) + 2048,), ((1 << 19) + 2048,), g=128), long="causal",
                   pred=lambda c: _x_bytes(c) < 1 << 32),
              Side(C(16, 128, 128, ((1 << 19) + 2048,), ((1 << 19) + 2048,), g=128), long="causal",
                   pred=lambda c: _x_bytes(c) >= 1 << 32)),
    # (batch, length, channels) tensors read and written where they lie: one batch item's block 2 MiB under 2**31 bytes;
    # from 2**31 bytes on the library refuses the layout before it uses a pointer (functional._long_run takes torch copies)
    Threshold("long-nlc-block", "long1d.hpp:210-228,277,544-567", "host_long.cpp:399", {},
              Side(C(1, 128, 128, ((1 << 22) - 4096,), (2048,), g=128), long="causal-nlc",
                   pred=lambda c: c.cin * c.size[0] * 4 == (1 << 31) - (1 << 21)),
              Side(C(1, 128, 128, (1 << 22,), (2048,), g=128), long="causal-nlc",
                   raises=(NotImplementedError, "x in the channels-last layout.*2147483648 bytes"))),
    # a float32 row lies behind one resource of at most 2**31 bytes: descriptor only (a row of 2**29 samples, 1000 outputs kept)
    Threshold("long-row-limit", "long1d.hpp:226-253", "host_long.cpp:79-82", {},
              Side(C(1, 1, 1, (1 << 29,), (1,)), long="geom", plan_only=True, pred=lambda n: n == 4096),
              Side(C(1, 1, 1, ((1 << 29) + 1,), (1,)), long="geom",
                   raises=(NotImplementedError, "more than 2.29 samples"))),
    # stride x transform points <= 2**30, an index of 32 bits: plan-only at the limit (64 x 2**24 is taken, 96 x 2**24
    # refused; an output row stays below 2**29 samples, so only a stride that is no power of two gets there), and running
    # at 64 x 2**23 = 2**29 on the decimated rows of a strided fft_long_conv and by the phases of fft_long_conv_transpose.
    # (A decimation plan has stride <= 64 and at most 2**24 points: host_long.cpp:261 cannot refuse.)
    Threshold("long-phases-index", "long1d.hpp:240,563", "host_long.cpp:209", {},
              Side(C(1, 1, 1, (1 << 22,), (3 << 26,), s=64, tr=True), long="index", plan_only=True,
                   pred=lambda n: 64 * n == 1 << 30),
              Side(C(1, 1, 1, (2708000,), (275000000,), s=96, tr=True), long="index",
                   raises=(NotImplementedError, "exceeds the 2.30 samples the phases plan indexes"))),
    Threshold("long-phases-run", "long1d.hpp:240,563", "host_long.cpp:209,261", {"FFTCONV_LONG_DECIM": "1"},
              Side(C(1, 1, 1, (64 * ((1 << 22) + 64),), (512,), s=64), long="decim", pred=lambda n: 64 * n == 1 << 29),
              Side(C(1, 1, 1, ((1 << 22) + 100,), (512,), s=64, tr=True), long="transpose",
                   pred=lambda n: 64 * n == 1 << 29)),
    # ------------------------------------------------------------------------------------------------ float64
    # plan-only: a row of 2**31 - 2**22 float64 samples is 16 GiB
    Threshold("f64-positions", "long_f64.hip", "host_f64.cpp:135", {},
              Side(C(1, 1, 1, ((1 << 31) - (1 << 22) - 1,), (2049,), f64=True), plan_only=True, dtype=torch.float64,
                   pred=ru._f64("f64_fft_long", N1=2048, N2=2048)),
              Side(C(1, 1, 1, ((1 << 31) - (1 << 22),), (2049,), f64=True), plan_only=True, dtype=torch.float64,
                   pred=ru._f64("f64_direct"))),
    # every launch of a float64 N-d plan within 2**32 work-items: plan-only (the signal is 128 GiB)
    Threshold("f64-grid", "nd_f64.hip", "host_f64.cpp:77", {},
              Side(C(1, 1, 1, (8343597, 2048), (10, 10), f64=True), plan_only=True, dtype=torch.float64,
                   pred=ru._f64("f64_fft_nd", t0=2048, t1=2048), extra=lambda plan, c: _f64_fused_items(c) < 1 << 32),
              Side(C(1, 1, 1, (8343598, 2048), (10, 10), f64=True), plan_only=True, dtype=torch.float64,
                   pred=ru._f64("f64_direct"), extra=lambda plan, c: _f64_fused_items(c) >= 1 << 32)),
]
SIDES = [(th, name) for th in THRESHOLDS for name in ("below", "above")]


@pytest.fixture(autouse=True)
def _no_knob_plans_afterwards():
    yield
    from fft_conv_pytorch_amd import _native, autograd
    _native.clear_plan_cache()
    autograd._BWD_PLANS.clear()
    torch.cuda.empty_cache()


def _shapes(c):
    return (c.B, c.cin) + tuple(c.size), (c.B, c.cout) + au.out_spatial(c)


def _planned(c, side, plan=None):
    """Peak of allocated bytes of a side: x twice (the guarded copy and the one its checker compares it with), the weight
    likewise, y once, the plan's kernel spectrum and workspace, and 1.5 GiB for the check (four float64 chunks of
    big_util.CHUNK_BYTES and their index lists).  The weight-gradient sides hold x and dY twice and dX once; the one past the
    guard (forward plans over strided copies of both operands) holds a padded and a gathered copy of each and a spectrum
    the size of dY besides."""
    item = torch.zeros(0, dtype=side.dtype).element_size()
    xs, ys = _shapes(c)
    xb, yb = math.prod(xs) * item, math.prod(ys) * item
    wb = math.prod(c.wshape) * item
    if side.kind == "wgrad":
        if plan == 0:        # (x and dY as they are: the kernels read torch's copies of them, not the tensors)
            return 3 * xb + 4 * yb + 3 * GIB // 2
        return 2 * xb + 2 * yb + xb + 3 * GIB // 2
    return 2 * xb + 2 * wb + yb + (plan.spectrum_bytes + plan.workspace_bytes if plan is not None else 0) + 3 * GIB // 2


def _placeholder(shape, dtype):
    """a tensor of this shape that owns one element: the planner reads shapes only"""
    return torch.zeros(1, dtype=dtype, device=DEV).expand(shape)


def _plan(c, side):
    from fft_conv_pytorch_amd import functional as fc
    kw = _kw(c)
    x, w, b = _placeholder(_shapes(c)[0], side.dtype), _placeholder(c.wshape, side.dtype), _placeholder((c.cout,), side.dtype)
    return fc._plan_for(x, w, b, kw["stride"], kw["padding"], kw["dilation"], c.g, "constant" if c.tr else c.mode,
                        transposed=c.tr, output_padding=kw.get("output_padding", 0))


def _weights(c, dtype, seed):
    """(weight, bias) as numpy float64 and on the device: integers in [-8, 8]; the bias counts the channels"""
    gen = torch.Generator().manual_seed(seed)
    w = torch.randint(au.LO, au.HI + 1, c.wshape, generator=gen, dtype=torch.int8).float()
    b = torch.arange(1, c.cout + 1, dtype=torch.float32) % 61
    return w.numpy(), b.numpy().astype(np.float64), w.to(dtype).to(DEV), b.to(dtype).to(DEV)


def _free_or_skip(key, planned):
    assert planned <= CAP, f"{key}: plans {planned / GIB:.1f} GiB, more than the cap of {CAP // GIB} GiB"
    free = torch.cuda.mem_get_info()[0]
    if free < planned:
        DONE[key] = f"skipped: plans {planned} bytes, {free} free"
        pytest.skip(f"plans {planned} bytes of device memory, {free} are free")


def _record(th, name, side, route, planned, t0, errs):
    peak = torch.cuda.max_memory_allocated()
    row = dict(entry=th.name, side=name, site=th.site, guard=th.guard, case=side.case.ident(), padding=side.case.p,
               dtype=str(side.dtype), route=route, planned_bytes=planned, peak_bytes=peak, seconds=round(time.time() - t0, 2),
               worst_error_over_tol=max(errs) if errs else None)
    ROWS.append(row)
    print(f"\n{th.name} / {name}: {row}")
    assert peak <= 1.1 * planned, f"peak of {peak} bytes allocated, planned {planned}"


def _forward(th, name, side):
    from fft_conv_pytorch_amd import functional as fc
    c, key = side.case, (th.name, name)
    plan = _plan(c, side)
    r = plan.route

    def on_route():
        assert side.pred(r), f"plan is on another route: {r}"
        if side.extra:
            held = side.extra(plan, c)
            assert held is None or held, f"case not sized as intended: {c.ident()}, {r}"
    if side.plan_only:
        on_route()
        DONE[key] = "plan-only"
        return
    planned = _planned(c, side, plan)
    _free_or_skip(key, planned)
    t0 = time.time()
    item = torch.zeros(0, dtype=side.dtype).element_size()
    kd = (c.k[-1] - 1) * c.tup(c.d)[-1] + 1            # windows lie along the last axis: its tile and its taps
    tile = r.get("Tx", r["T"]) - kd + 1
    xs = bu.sparse_input(_shapes(c)[0], item, seed=len(th.name) + c.B, groups=c.g, tile=tile, reach=kd)
    wn, bn, w, b = _weights(c, side.dtype, 3)
    x, x_check = gu.guarded(xs.dense(side.dtype, DEV), 0xFF)
    w, w_check = gu.guarded(w, 0xFF)
    spec = fc.transform_kernel(plan, w)
    with gu.guarded_empty(0xFF) as ge:
        y = fc._forward_native(x, spec, b)
    assert not ge.violations(), f"stores outside y: {ge.violations()}"
    assert not x_check() and not w_check(), "an input was written or its guards were"
    del spec
    flat, val = bu.conv_truth(c, xs, wn)
    worst, wmax = bu.check_full(y, flat, val, bn, tol=ru.TOL32, what=f"{th.name} / {name}")
    on_route()            # (after the values: whatever route a library takes, its output is checked first)
    DONE[key] = "ran"
    _record(th, name, side, {k: v for k, v in r.items() if v}, planned, t0, [worst / (ru.TOL32 * wmax)])


def _wgrad(th, name, side):
    """dW and db (fc_wgrad1d below the guard, forward plans past it) and dX of the case, from a sparse x and a sparse dY"""
    from fft_conv_pytorch_amd import _native, autograd
    c, key = side.case, (th.name, name)
    kw = _kw(c)
    desc = _native.conv_desc(1, c.B, c.cin, c.cout, c.g, c.size, c.k, kw["stride"], kw["padding"], kw["dilation"],
                             _native.PAD_MODES[c.mode], 0)
    slices = _native.wgrad1d_slices(desc)
    assert side.pred(slices), f"fc_wgrad1d_slices = {slices}"
    if side.plan_only:
        DONE[key] = "plan-only"
        return
    planned = _planned(c, side, slices)
    _free_or_skip(key, planned)
    t0 = time.time()
    xshape, yshape = _shapes(c)
    xs = bu.sparse_input(xshape, 4, seed=11, groups=c.g, tile=1024 - c.k[0] + 1, reach=c.k[0])
    dys = bu.sparse_input(yshape, 4, seed=12, groups=c.g, tile=1024 - c.k[0] + 1, reach=c.k[0])
    wn, _, w, _ = _weights(c, side.dtype, 3)
    x, dy = xs.dense(side.dtype, DEV), dys.dense(side.dtype, DEV)
    x_check = dy_check = list
    if slices:               # fc_wgrad1d reads the tensors themselves
        x, x_check = gu.guarded(x, 0xFF)
        dy, dy_check = gu.guarded(dy, 0xFF)
    args = (kw["stride"], kw["padding"], kw["dilation"], c.g, c.mode)
    with gu.guarded_empty(0xFF) as ge:
        dw, db = autograd._grad_weight_db(x, dy, c.wshape, *args, want_db=True)
        if db is None:
            db = autograd._grad_bias(dy)
    assert not ge.violations(), f"stores outside dW's buffers: {ge.violations()}"
    flat, val = bu.wgrad_truth(c, xs, dys)
    e_dw = bu.check_full(dw.contiguous()[None], flat, val, tol=ru.TOL32, what="dW")
    dbn = bu.bias_grad_truth(dys)
    e_db = bu.check_full(db.contiguous()[None, :, None], np.arange(c.cout), dbn, tol=ru.TOL32, what="db")
    del dw, db
    torch.cuda.empty_cache()
    with gu.guarded_empty(0xFF) as ge:
        dx = autograd._grad_input(dy, w, c.size, *args)
    assert not ge.violations(), f"stores outside dX: {ge.violations()}"
    assert not x_check() and not dy_check(), "an input was written or its guards were"
    ct = C(c.B, c.cout, c.cin, au.out_spatial(c), c.k, s=c.s, p=c.p, d=c.d, g=c.g, tr=True)
    assert au.out_spatial(ct) == tuple(c.size)
    flat, val = bu.conv_truth(ct, dys, wn)
    e_dx = bu.check_full(dx, flat, val, tol=ru.TOL32, what="dX")
    DONE[key] = "ran"
    _record(th, name, side, {"fc_wgrad1d_slices": slices}, planned, t0, [e / (ru.TOL32 * m) for e, m in (e_dw, e_db, e_dx)])


def _wgrad_nd(th, name, side):
    """dW of a 2-D / 3-D case by fc_wgrad_nd (the batch / channel-swapped convolution on x and dY as they lie)"""
    from fft_conv_pytorch_amd import autograd
    c, key = side.case, (th.name, name)
    # (the guard is a byte count with no route word: the predicate is the case's own arithmetic, not a route assertion)
    assert side.pred(c), f"case not sized as intended: {c.ident()}"
    xshape, yshape = _shapes(c)
    # x and dY twice (guarded copy and original), the spectra of up to 8 segments of taps and the workspace
    planned = 2 * 4 * (math.prod(xshape) + math.prod(yshape)) + 31 * GIB // 2
    _free_or_skip(key, planned)
    t0 = time.time()
    kw = _kw(c)
    xs = bu.sparse_input(xshape, 4, seed=21, groups=c.g, tile=c.size[-1], reach=c.k[-1])
    dys = bu.sparse_input(yshape, 4, seed=22, groups=c.g, tile=yshape[-1], reach=c.k[-1])
    x, x_check = gu.guarded(xs.dense(side.dtype, DEV), 0xFF)
    dy, dy_check = gu.guarded(dys.dense(side.dtype, DEV), 0xFF)
    with gu.guarded_empty(0xFF) as ge:
        dw = autograd._grad_weight_nd_native(x, dy, c.wshape, kw["stride"], kw["padding"], kw["dilation"], c.g, c.mode)
    assert dw is not None, "fc_wgrad_nd refused the shape"
    assert not ge.violations(), f"stores outside dW's buffers: {ge.violations()}"
    assert not x_check() and not dy_check(), "an input was written or its guards were"
    flat, val = bu.wgrad_truth(c, xs, dys)
    worst, wmax = bu.check_full(dw.contiguous()[None], flat, val, tol=ru.TOL32, what="dW")
    assert wmax > 0
    DONE[key] = "ran"
    _record(th, name, side, {"dy_bytes": _dy_bytes(c)}, planned, t0, [worst / (ru.TOL32 * wmax)])


def _long_points(c, side):
    """N = N1 x N2 of the long plan of a side, from the descriptor alone"""
    from fft_conv_pytorch_amd import _native
    L, K, s = c.size[0], c.k[0], c.tup(c.s)[0]
    if side.long == "geom":      # the plain plan of a row of which 1000 outputs are kept
        g = _native.long_geometry((c.B, c.cin, c.cout, c.g, L, K, 0, 0, 1000, 0, 1))
    elif side.long in ("transpose", "index"):
        g = _native.phases_geometry((c.B, c.cin, c.cout, c.g, L, K, s, 0, 0, 1))
    elif side.long == "decim":
        g = _native.decim_geometry((c.B, c.cin, c.cout, c.g, L, K, s, 0, 0, 0, 0, 1))
    else:        # causal: K - 1 zeros in front, L outputs kept, taps flipped
        g = _native.long_geometry((c.B, c.cin, c.cout, c.g, L, K, K - 1, 0, L, 1, 1))
    return g


def _long_refusal(c, side):
    """What must refuse a long-filter side: the geometry of its descriptor, or (channels-last) fc_long_forward_lay, which
    checks the layouts before it uses a pointer -- none of the pointers handed over has the tensors' size."""
    from fft_conv_pytorch_amd import _native
    if side.long != "causal-nlc":
        return _long_points(c, side)
    L, K = c.size[0], c.k[0]
    plan = _native.get_plan(0, ("long", c.B, c.cin, c.cout, c.g, L, K, K - 1, 0, L, 1, 1))
    assert plan.out_len * c.cout * 4 >= _native.LONG_NLC_MAX_BYTES
    p = torch.zeros(16, device=DEV).data_ptr()
    plan.forward_lay(p, p, p, p, p, torch.cuda.current_stream().cuda_stream, 0, 0, _native.LONG_NLC, _native.LONG_NCL)


def _long(th, name, side):
    """A long-filter side: fft_long_conv (causal depthwise, plain or channels-last; strided by decimated rows) or
    fft_long_conv_transpose (by phases) against the sparse truth.  The depthwise filters are sparse too (windows at both ends
    and in the middle of the tap range): the truth of K = L taps stays a short list."""
    from fft_conv_pytorch_amd import functional as F_
    from fft_conv_pytorch_amd.functional import fft_long_conv, fft_long_conv_transpose
    c, key = side.case, (th.name, name)
    L, K = c.size[0], c.k[0]
    if side.long in ("index", "geom"):
        assert side.pred(_long_points(c, side)["N1"] * _long_points(c, side)["N2"])
        DONE[key] = "plan-only"
        return
    causal = side.long.startswith("causal")
    # (causal sides: thresholds in bytes with no route word -- the predicate is the case's own arithmetic; the others: N)
    assert side.pred(c) if causal else side.pred(_long_points(c, side)["N1"] * _long_points(c, side)["N2"]), c.ident()
    if side.plan_only:
        DONE[key] = "plan-only"
        return
    geo = _long_points(c, side)
    xshape = (c.B, c.cin, L)
    if side.long == "decim":
        assert F_._long_route(xshape, c.wshape, stride=c.tup(c.s)[0]) == "phases"
    elif side.long == "transpose":
        assert F_._long_transpose_route(xshape, c.wshape, stride=c.tup(c.s)[0]) == "phases"
    nout = L if causal else au.out_spatial(c)[0]
    xb, yb = 4 * math.prod(xshape), 4 * c.B * c.cout * nout
    # x twice (guarded copy and original), y (twice where a channels-last result is copied for the check), the spectrum, and
    # the workspace twice (the kernel transform's and the forward's: measured, the first is still held when the second comes)
    planned = (2 * xb + (2 if side.long == "causal-nlc" else 1) * yb + geo["spectrum_bytes"] + 2 * geo["workspace_bytes"]
               + 3 * GIB // 2)
    _free_or_skip(key, planned)
    t0 = time.time()
    xs = bu.sparse_input(xshape, 4, seed=31 + c.B, groups=1, tile=4096, reach=min(K, L))
    gen = torch.Generator().manual_seed(32)
    if causal:
        taps = np.unique(np.clip(np.concatenate([np.arange(4), K // 2 + np.arange(4), K - 4 + np.arange(4)]), 0, K - 1))
        wv = au.integers((c.cout, taps.size), gen, torch.float64).numpy()
        w = torch.zeros(c.wshape, device=DEV)
        w[:, 0, torch.from_numpy(taps).to(DEV)] = torch.from_numpy(wv).float().to(DEV)
    else:
        wn = au.integers(c.wshape, gen, torch.float64).numpy()
        w = torch.from_numpy(wn).float().to(DEV)
    bn = (np.arange(1, c.cout + 1) % 61).astype(np.float64)
    b = torch.from_numpy(bn).float().to(DEV)
    x = xs.dense(torch.float32, DEV)
    if side.long == "causal-nlc":
        u, x_check = gu.guarded(x.transpose(1, 2).contiguous(), 0xFF)
        del x
        x = u.transpose(1, 2)
    else:
        x, x_check = gu.guarded(x, 0xFF)
    with gu.guarded_empty(0xFF) as ge:
        if causal:
            y = fft_long_conv(x, w, b, groups=c.g, causal=True, channels_last=side.long == "causal-nlc")
        elif side.long == "decim":
            y = fft_long_conv(x, w, b, stride=c.tup(c.s)[0])
        else:
            y = fft_long_conv_transpose(x, w, b, stride=c.tup(c.s)[0])
    assert not ge.violations(), f"stores outside the buffers of the call: {ge.violations()}"
    assert not x_check(), "the signal was written or its guards were"
    assert tuple(y.shape) == (c.B, c.cout, nout), tuple(y.shape)
    if side.long == "causal-nlc":
        assert tuple(y.stride()) == (nout * c.cout, 1, c.cout)
        y = y.contiguous()
    if causal:      # y[b, ch, j] = sum_k w[ch, k] x[b, ch, j - k]
        co = xs.coords()
        j = co[:, 2][:, None] + taps[None]
        ok = j < L
        flat = ((co[:, 0] * c.cout + co[:, 1])[:, None] * L + j)[ok]
        val = (xs.val[:, None] * wv[co[:, 1]])[ok]
        flat, val = bu._coalesce(flat, val)
    else:
        flat, val = bu.conv_truth(c, xs, wn)
    worst, wmax = bu.check_full(y, flat, val, bn, tol=ru.TOL32, what=f"{th.name} / {name}")
    DONE[key] = "ran"
    _record(th, name, side, {k: geo[k] for k in ("N1", "N2", "slabs")}, planned, t0, [worst / (ru.TOL32 * wmax)])


@pytest.mark.parametrize("th,name", SIDES, ids=[f"{th.name}-{name}" for th, name in SIDES])
def test_threshold(th, name, monkeypatch):
    side = getattr(th, name)
    _knobs(monkeypatch, th.env)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    if side.raises:
        cls, text = side.raises
        with pytest.raises(cls, match=text):          # raised by the planner: nothing was launched
            _long_refusal(side.case, side) if side.long else _plan(side.case, side)
        DONE[(th.name, name)] = "refused"
    elif side.long:
        _long(th, name, side)
    elif side.kind == "wgrad":
        _wgrad(th, name, side)
    elif side.kind == "wgrad_nd":
        _wgrad_nd(th, name, side)
    else:
        _forward(th, name, side)


def test_every_threshold_ran_on_both_sides():
    """Both sides of every entry passed in this run of the file: one that failed or was deselected is missing here.  Sides
    skipped for want of device memory are listed; on an idle MI355X there are none."""
    missing = [f"{th.name}-{name}" for th, name in SIDES if (th.name, name) not in DONE]
    skipped = {f"{k[0]}-{k[1]}": v for k, v in DONE.items() if v.startswith("skipped")}
    print(f"\nthresholds: {len(DONE) - len(skipped)} sides done, skipped for memory: {skipped or 'none'}")
    assert not missing, f"not exercised: {missing}; skipped for memory: {skipped}"
    if torch.cuda.get_device_properties(0).total_memory >= 200 * GIB and torch.cuda.mem_get_info()[0] >= 100 * GIB:
        assert not skipped, f"skipped for memory on an idle device: {skipped}"
