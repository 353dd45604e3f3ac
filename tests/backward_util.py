"""Backward route table of tests/test_gpu_backward_routes.py: the families of fc_wgrad1d cases sized for the edges of
``wgrad_geometry`` (csrc/host_1d.cpp), the shapes one step past its limits (the forward-plan dW of
``autograd._grad_weight_plans``), the fc_wgrad_nd cases, and the two probes that make a wrong boundary sample visible
whatever the row length.

``wgrad_geometry`` restates the library's launch geometry in Python.  It places the probes and is what the ``expect``
lambdas of the cases test (every case also asserts its ``slices`` against ``_native.wgrad1d_slices``); it is never the source
of an expected value -- those come from torch's float64 convolution autograd.

A family is (name, knobs, predicate on the geometry, cases) in the style of ``route_util.Route``; the cases are
``route_util.Case``s whose ``expect`` takes the restated geometry."""
from dataclasses import dataclass
from typing import Callable

import torch
import torch.nn.functional as F

from tests import route_util as ru

T_WGRAD = 1024          # the tile of fc_wgrad1d
NB_DENSE = 2            # (batch item, tile) items per iteration of wgrad1d_kernel; the depthwise kernel takes one
PROBE_MOVES = 100 * ru.TOL32     # clearing one probed dY sample moves dW by at least this share of its maximum


@dataclass
class Family:
    name: str
    env: dict
    pred: Callable      # on the restated geometry of a case
    cases: list


def _cdiv(a, b):
    return -(-a // b)


def wgrad_geometry(c, cus, diag_on=True):
    """The launch geometry of fc_wgrad1d for a case (None: the library refuses the shape and the forward-plan route runs),
    as ``wgrad_geometry`` of csrc/host_1d.cpp decides it on a device of ``cus`` compute units."""
    if c.nd != 1 or c.tr or c.f64:
        return None
    L, k, s, p, d, g = c.size[0], c.k[0], c.tup(c.s)[0], c.tup(c.p)[0], c.tup(c.d)[0], c.g
    if s < 1 or s > 64 or g < 1 or c.B < 1 or c.cin % g or c.cout % g:
        return None
    cig, cog = c.cin // g, c.cout // g
    if cig > 64 or cog > 64 or p < 0 or d > 512:
        return None
    kd = (k - 1) * d + 1
    if L + 2 * p - kd < 0:
        return None
    lout = (L + 2 * p - kd) // s + 1
    lext = (lout - 1) * s + 1
    if (c.mode == "reflect" and p >= L) or (c.mode == "circular" and p > L):
        return None
    if c.B * c.cin * L * 4 >= 1 << 32 or c.B * c.cout * lout * 4 >= 1 << 32:
        return None
    ks = min(k, k if kd <= 768 else 512 // d + 1)
    kd_seg = (ks - 1) * d + 1
    nseg = _cdiv(k, ks)
    if nseg > 64:
        return None
    V = (T_WGRAD - kd_seg + 1) // s * s
    if V < 1:
        return None
    ntiles = _cdiv(lext, V)
    n_items = c.B * ntiles
    diag = bool(diag_on and g == c.cin and g == c.cout and g % 8 == 0)
    nb = 1 if diag else NB_DENSE
    nob, nib = _cdiv(cog, 4), _cdiv(cig, 4)
    types = g // 8 if diag else g * nob * nib
    slices = max(1, _cdiv(2 * cus, types))
    slices = min(slices, max(1, n_items // (4 * nb)))
    ipw = _cdiv(_cdiv(n_items, slices), nb) * nb
    return dict(ks=ks, kd_seg=kd_seg, nseg=nseg, V=V, ntiles=ntiles, n_items=n_items, ipw=ipw, slices=_cdiv(n_items, ipw),
                diag=diag, nob=nob, nib=nib, lout=lout, lext=lext, last=n_items - (_cdiv(n_items, ipw) - 1) * ipw)


def chunk_plan(c):
    """(chunked, c_taps, nchunk) of ``autograd._grad_weight_plans`` for a 1-D case: whether dY is longer than one tile of the
    role-swapped plan takes, and the chunks it is then cut into."""
    from fft_conv_pytorch_amd import autograd as A
    L, k, s, p, d = c.size[0], c.k[0], c.tup(c.s)[0], c.tup(c.p)[0], c.tup(c.d)[0]
    kd0 = (k - 1) * d + 1
    lout = (L + 2 * p - kd0) // s + 1
    max_ext = max(A._DW_TILE - kd0 + 1, A._DW_TILE // 4)
    chunked = (lout - 1) * s + 1 > max_ext
    c_taps = max(1, (max_ext - 1) // s + 1)
    return chunked, c_taps, _cdiv(lout, c_taps)


# ------------------------------------------------------------------------------------------------ probes
def out_len(c):
    return tuple((S + 2 * p - d * (k - 1) - 1) // s + 1
                 for S, p, d, k, s in zip(c.size, c.tup(c.p), c.tup(c.d), c.k, c.tup(c.s)))


def dy_probe_outputs(lout, starts):
    """Outputs of a dY probe: the row ends and the outputs just before, at and after every start in ``starts`` (the first
    output of a tile, a chunk or a segment), inside the row."""
    pos = {0, 1, lout - 2, lout - 1}
    for q in starts:
        pos.update((q - 1, q, q + 1))
    return sorted(v for v in pos if 0 <= v < lout)


def wgrad1d_dy_outputs(c, geo):
    s = c.tup(c.s)[0]
    return dy_probe_outputs(geo["lout"], [j * geo["V"] // s for j in range(geo["ntiles"])])


def wgrad1d_x_samples(c, geo):
    """Samples of an x probe: the row ends, the padding boundary and its mirror, and the first and last sample of every
    tile's window (``j * V - p + pos_shift`` and that plus T - 1, for every tap segment's ``pos_shift``)."""
    L, p, d = c.size[0], c.tup(c.p)[0], c.tup(c.d)[0]
    pos = {0, 1, L - 2, L - 1, p - 1, p, p + 1, L - 1 - (p - 1), L - 1 - p, L - 1 - (p + 1)}
    for j in range(geo["ntiles"]):
        for sg in range(geo["nseg"]):
            first = j * geo["V"] - p + sg * geo["ks"] * d
            pos.update((first, first + T_WGRAD - 1))
    return sorted(v for v in pos if 0 <= v < L)


def _amplitudes(shape, gen, dtype, device):
    """Random amplitudes of either sign, between 0.5 and 1.5 in size (an amplitude near zero would hide its sample)."""
    a = torch.rand(shape, generator=gen, device=device, dtype=dtype) + 0.5
    sign = torch.randint(0, 2, shape, generator=gen, device=device).to(dtype) * 2 - 1
    return a * sign


def impulses(shape, per_axis, gen, dtype, device):
    """Zeros plus random amplitudes where every spatial axis sits on one of its positions (``per_axis``: a list per axis),
    on every batch item and channel."""
    t = torch.zeros(shape, dtype=dtype, device=device)
    mask = None
    for ax, pos in enumerate(per_axis):
        m = torch.zeros(shape[2 + ax], dtype=torch.bool)
        m[list(pos)] = True
        view = [1] * len(per_axis)
        view[ax] = shape[2 + ax]
        m = m.view(view)
        mask = m if mask is None else mask & m
    mask = mask.to(device)
    return torch.where(mask, _amplitudes(shape, gen, dtype, device), t)


def reference_dw(c, x, gy):
    """(dW, db) of the forward convolution of a case by torch's float64 convolution autograd, on float64 copies."""
    nd = c.nd
    conv = (F.conv1d, F.conv2d, F.conv3d)[nd - 1]
    x, gy = x.double(), gy.double()
    w = torch.zeros((c.cout, c.cin // c.g) + tuple(c.k), dtype=torch.float64, device=x.device, requires_grad=True)
    b = torch.zeros(c.cout, dtype=torch.float64, device=x.device, requires_grad=True)
    pads = c.tup(c.p)
    if c.mode == "constant":
        y = conv(x, w, b, stride=c.tup(c.s), padding=pads, dilation=c.tup(c.d), groups=c.g)
    else:
        flat = [q for p in reversed(pads) for q in (p, p)]
        y = conv(F.pad(x, flat, mode=c.mode), w, b, stride=c.tup(c.s), dilation=c.tup(c.d), groups=c.g)
    assert y.shape == gy.shape, (y.shape, gy.shape)
    y.backward(gy)
    return w.grad, b.grad


def cpu_sized(c):
    """The case with its row geometry (length, taps, stride, dilation, padding) kept and batch and channels cut down to what
    a CPU convolution in float64 takes in a moment: the probes sit where they sit on the device."""
    g = min(c.g, 2)
    cig, cog = min(c.cin // c.g, 3), min(c.cout // c.g, 3)
    if c.g == c.cin == c.cout:
        g, cig, cog = 8, 1, 1            # (still depthwise: the geometry keeps its kernel)
    return ru.Case(**{**c.__dict__, "B": min(c.B, 2), "cin": g * cig, "cout": g * cog, "g": g, "env": dict(c.env)})


# ------------------------------------------------------------------------------------------------ 1. fc_wgrad1d
C = ru.Case
_V65 = T_WGRAD - 65 + 1          # 960: tile step of a 65-tap kernel at stride 1


def _dense(geo):
    return geo is not None and not geo["diag"]


WGRAD1D_FAMILIES = [
    # 7 -> 9 channels: nib 2, nob 3, both last 4 x 4 blocks ragged.  35 (batch item, tile) items in 4 slices of 10: the last
    # slice holds 5, so one item slot of its last iteration idles.  db rides both launches.
    Family("blocks-remainders-short-last-slice", {}, lambda g: _dense(g) and (g["nib"], g["nob"]) == (2, 3), [
        C(5, 7, 9, (6700,), (65,), p=8, mode="reflect", note="odd-last-slice",
          expect=lambda g: (g["V"], g["ntiles"], g["n_items"]) == (960, 7, 35) and g["slices"] > 1 and g["last"] % 2 == 1),
        C(4, 7, 9, (3848,), (65,), p=8, mode="reflect", note="exact-slices",
          expect=lambda g: g["ntiles"] == 4 and g["slices"] > 1 and g["n_items"] == g["slices"] * g["ipw"]),
    ]),
    Family("one-slice-one-tile", {}, lambda g: _dense(g) and g["slices"] == 1 and g["ntiles"] == 1 and g["n_items"] == 1, [
        C(1, 1, 1, (900,), (33,), p=16),
        C(1, 4, 4, (900,), (33,), p=16, mode="replicate"),
    ]),
    Family("stride-64", {}, _dense, [
        # 19967 = 311 * 64 + 63: the last 63 samples of the row are never reached
        C(2, 6, 5, (20000,), (33,), s=64, expect=lambda g: (g["V"], g["ntiles"]) == (960, 21)),
        C(2, 6, 5, (20000,), (33,), s=64, p=16, mode="circular", expect=lambda g: (g["V"], g["ntiles"]) == (960, 21)),
        C(2, 4, 4, (20011,), (33,), s=63, p=5, note="s63", expect=lambda g: g["V"] == 945 and g["lext"] % g["V"] != 0),
        C(2, 4, 4, (20011,), (33,), s=63, p=5, mode="circular", note="s63",
          expect=lambda g: g["V"] == 945 and g["lext"] % g["V"] != 0),
    ]),
    Family("dilation-512", {}, lambda g: _dense(g) and g["V"] == 512 and g["kd_seg"] == 513, [
        C(2, 5, 6, (5000,), (2,), d=512, p=3, mode="replicate", note="one-segment", expect=lambda g: g["nseg"] == 1),
        C(2, 5, 6, (5000,), (3,), d=512, p=3, mode="replicate", note="segments-2+1",
          expect=lambda g: g["nseg"] == 2 and g["ks"] == 2),
    ]),
    Family("tap-segments-64", {}, lambda g: _dense(g) and g["nseg"] == 64 and g["ks"] == 3, [
        C(1, 4, 4, (50000,), (192,), d=256),
        C(1, 4, 4, (50000,), (190,), d=256, p=100, mode="reflect", note="ragged-last-segment"),
    ]),
    Family("channels-64", {}, lambda g: _dense(g) and (g["nib"], g["nob"]) == (16, 16), [
        C(2, 64, 61, (3000,), (17,), p=8),
        C(2, 128, 122, (3000,), (17,), g=2, p=3, mode="reflect"),
    ]),
    Family("depthwise-strided", {}, lambda g: g is not None and g["diag"] and g["slices"] > 1, [
        C(3, 8, 8, (9000,), (33,), g=8, s=2, d=3, p=20, mode="circular"),
        C(3, 24, 24, (9000,), (33,), g=24, s=2, d=3, p=20, mode="circular"),
        C(3, 8, 8, (9001,), (65,), g=8, s=3, p=7, mode="reflect", note="s3"),
        C(2, 24, 24, (9001,), (65,), g=24, s=3, p=7, mode="reflect", note="s3"),
        C(3, 8, 8, (9000,), (300,), g=8, s=2, d=3, p=5, note="segments", expect=lambda g: g["nseg"] == 2),
    ]),
    # p 0 and L = 2 V + T: tile 0 starts at sample 0 and the window of tile 2 ends at L, the bounds of the loaders' interior
    # path (tile_pos >= 0, tile_pos + T <= L); then one sample to either side of them
    Family("interior-fast-path-bounds", {}, lambda g: _dense(g) and g["V"] == _V65 and g["ntiles"] in (3, 4), [
        C(2, 4, 4, (2 * _V65 + T_WGRAD,), (65,), note="exact", expect=lambda g: g["ntiles"] == 3),
        C(2, 4, 4, (2 * _V65 + T_WGRAD - 1,), (65,), note="L-1", expect=lambda g: g["ntiles"] == 3),
        C(2, 4, 4, (2 * _V65 + T_WGRAD + 1,), (65,), note="L+1", expect=lambda g: g["ntiles"] == 4),
        C(2, 4, 4, (2 * _V65 + T_WGRAD - 2,), (65,), p=1, note="tile0-at--1", expect=lambda g: g["ntiles"] == 3),
        C(2, 3, 4, (2 * _V65 + T_WGRAD,), (65,), note="odd-cig"),
        C(2, 7, 4, (2 * _V65 + T_WGRAD,), (65,), mode="reflect", note="odd-cig-2-blocks"),
    ]),
]

# float16 / bfloat16: bits equal to the FFTCONV_HALF_IO=0 path
HALF_CASES = [
    ("stride-64", torch.float16, C(2, 6, 5, (20000,), (33,), s=64, p=16)),
    ("stride-64", torch.bfloat16, C(2, 6, 5, (20000,), (33,), s=64, p=16)),
    ("depthwise-strided", torch.float16, C(3, 8, 8, (9000,), (33,), g=8, s=2, d=3, p=20)),
    ("depthwise-strided", torch.bfloat16, C(3, 8, 8, (9000,), (33,), g=8, s=2, d=3, p=20)),
]

# ------------------------------------------------------------------------------------------------ 2. refusals
# One step past a limit of the geometry above: the forward-plan dW runs, through the chunked gather where dY is longer than
# one tile of the role-swapped plan takes ((name, case, chunked, predicate on (c_taps, nchunk, lout))).
_K33 = 2048 - 33 + 1            # 2016: taps of dY one chunk holds at k 33, stride 1
REFUSALS = [
    ("cig-65-chunked", C(2, 65, 8, (9000,), (33,), p=5, mode="reflect"), True, lambda ct, n, lo: n > 2),
    ("cig-65-groups-stride", C(2, 130, 16, (9000,), (33,), g=2, s=3, p=7, mode="circular"), True, lambda ct, n, lo: n > 2),
    ("cig-65-exact-chunks", C(2, 65, 8, (2 * _K33 + 32,), (33,)), True, lambda ct, n, lo: n == 2 and n * ct == lo),
    ("cig-65-one-tap-chunk", C(2, 65, 8, (2 * _K33 + 33,), (33,)), True, lambda ct, n, lo: n == 3 and (n - 1) * ct + 1 == lo),
    ("cig-65-single-plan", C(2, 65, 8, (1500,), (33,), p=5, mode="reflect"), False, None),
    ("cig-65-groups-single-plan", C(2, 130, 16, (1500,), (33,), g=2, s=3, p=7, mode="circular"), False, None),
    ("stride-65", C(2, 4, 4, (9000,), (33,), s=65, p=4), True, lambda ct, n, lo: n > 2),
    ("dilation-513", C(2, 4, 4, (5000,), (2,), d=513, p=3, mode="replicate"), True, lambda ct, n, lo: n > 2),
    ("taps-193-at-256", C(1, 4, 4, (52000,), (193,), d=256), True, lambda ct, n, lo: n > 2),
]
# fft_conv_transpose with output_padding >= stride (possible under a dilation): backward zero-extends x to the extent of
# conv(dY, W) before the weight gradient, on a row of several tiles
TRANSPOSED_DW = [
    ("transposed-dw-f32", C(4, 6, 4, (3000,), (9,), s=2, d=3, p=4, op=2, tr=True)),
    ("transposed-dw-f64", C(4, 6, 4, (3000,), (9,), s=2, d=3, p=4, op=2, tr=True, f64=True)),
]

# ------------------------------------------------------------------------------------------------ 4. fc_wgrad_nd
# (name, knobs, case, predicate on the weight-gradient plan's route)
WGRAD_ND = [
    ("nd-batch-9", {}, C(9, 3, 5, (33, 40), (5, 5), p=(2, 0), mode="circular"), None),
    ("nd-batch-17-3d", {}, C(17, 2, 3, (9, 12, 14), (3, 2, 3), p=(1, 0, 1)), None),
    # a tail the stride never reaches on every axis (STRIDE_TAILS): (50 + 4 - 10) % 3 = 2, (64 + 4 - 7) % 2 = 1;
    # 3-D: (19 - 2) % 2 = 1, (32 + 2 - 3) % 3 = 1, (22 + 2 - 3) % 2 = 1
    ("nd-stride-tails-2d", {}, C(2, 4, 4, (50, 64), (4, 3), s=(3, 2), p=2, d=(3, 3), mode="reflect", note="tails"), None),
    ("nd-stride-tails-3d", {}, C(3, 4, 6, (19, 32, 22), (2, 3, 3), s=(2, 3, 2), p=(0, 1, 1), g=2, mode="replicate", note="tails"), None),
    ("nd-segments-last-axis", {}, C(2, 3, 4, (16, 8192), (3, 3), p=1), lambda r: r["nseg1"] > 1 and r["nseg0"] == 1),
    ("nd-segments-outer-axis", {}, C(1, 2, 3, (4500, 4, 5), (3, 3, 3), p=1),
     lambda r: r["nseg0"] > 1 and r["nseg1"] == r["nseg2"] == 1),
    ("nd-ragged-groups", {}, C(3, 15, 21, (41, 37), (3, 5), s=(2, 1), p=(1, 2), g=3), None),
]


STRIDE_TAILS = ("nd-stride-tails-2d", "nd-stride-tails-3d")     # cases that must leave a tail on every axis


def stride_tails(c):
    """Per axis, the samples at the end of the padded row that no window of the strided convolution reaches."""
    return tuple((S + 2 * p - ((k - 1) * d + 1)) % s
                 for S, p, d, k, s in zip(c.size, c.tup(c.p), c.tup(c.d), c.k, c.tup(c.s)))


def wgrad_nd_dy_axes(c, route):
    """Per axis, the dY outputs of a probe: the row ends and both sides of every segment boundary of that axis (the
    segments of fc_wgrad_nd cut dY, the kernel of the role-swapped convolution: ``seg_taps`` outputs each)."""
    axes = []
    for ax, lo in enumerate(out_len(c)):
        nseg, taps = route.get(f"nseg{ax}", 1), route.get(f"seg_taps{ax}", 0)
        assert nseg <= 1 or 0 < taps < lo, f"axis {ax}: {nseg} segments of {taps} outputs on a row of {lo}"
        axes.append(dy_probe_outputs(lo, [j * taps for j in range(1, nseg)] if nseg > 1 else []))
    return axes


def probe_sets(c, cus=256, route=None):
    """(dY outputs per axis, x samples or None) of the probes of a forward case of the tables above.  1-D inside the
    geometry: tiles and tap segments; 1-D refused: the chunks of the forward-plan dW (first output of every chunk, first
    and last sample of its window); 2-D / 3-D: the segments of ``route``, the weight-gradient plan's (without one, as on a
    host without a device, a stand-in boundary in the middle of every axis of more than 2048 outputs)."""
    if c.nd > 1:
        if route is None:
            route = {}
            for ax, lo in enumerate(out_len(c)):
                route[f"nseg{ax}"], route[f"seg_taps{ax}"] = (2, lo // 2) if lo > 2048 else (1, 0)
        return wgrad_nd_dy_axes(c, route), None
    geo = wgrad_geometry(c, cus)
    if geo is not None:
        return [wgrad1d_dy_outputs(c, geo)], wgrad1d_x_samples(c, geo)
    L, k, s, p, d = c.size[0], c.k[0], c.tup(c.s)[0], c.tup(c.p)[0], c.tup(c.d)[0]
    _, c_taps, nchunk = chunk_plan(c)
    lout = out_len(c)[0]
    seg = (c_taps - 1) * s + (k - 1) * d + 1
    pos = {0, 1, L - 2, L - 1, p - 1, p, p + 1, L - 1 - (p - 1), L - 1 - p, L - 1 - (p + 1)}
    for j in range(nchunk):
        pos.update((j * c_taps * s - p, j * c_taps * s - p + seg - 1))
    return [dy_probe_outputs(lout, [j * c_taps for j in range(nchunk)])], sorted(v for v in pos if 0 <= v < L)


def forward_cases():
    """(family, case) of every forward case of the tables: what the host test of the probes walks."""
    out = [(f.name, c) for f in WGRAD1D_FAMILIES for c in f.cases]
    out += [(name, c) for name, c, _, _ in REFUSALS]
    out += [(name, c) for name, _, c, _ in WGRAD_ND]
    return out
