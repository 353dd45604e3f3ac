"""Shared by tests/test_host_nd_complex.py and tests/test_gpu_nd_complex.py: the case table of the complex64 2-D / 3-D
plans, and a complex128 restatement of what those plans compute that needs no GPU.

The restatement follows the kernels' own steps (csrc/nd_passes.hpp, rows_c2c_fwd_kernel / rows_c2c_inv_kernel): the signal
padded by the axis maps, ONE row per transform of the last axis with all T bins kept and no odd-frequency turn, the taps
dilated and conjugated as they are loaded, torch.fft for the middle passes, the spectrum stored as conj(.) * scale, the
plain product summed over the input channels of a group, the unnormalised inverse, then the valid window, the stride and
a complex bias.  ``Backend`` puts it behind the three functions of ``functional`` through which ``autograd`` reaches the
library, so the gradient constructions of autograd.py run on the CPU exactly as they are written."""
import math
import types

import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests import route_util as ru

C = ru.Case
REFLECT = C(3, 4, 6, (40, 61), (3, 5), s=(2, 3), d=(2, 1), p=(2, 4), g=2, mode="reflect", grads=True)

# name -> (case, predicate on Plan.route beyond kind == "c64_nd" and planes == 0)
FORWARD = {
    # one 64-point tile per axis; 41 padded rows: the last block of rows is partial, and no row has a partner
    "one-tile": (C(2, 3, 4, (37, 50), (5, 7), p=(2, 3)),
                 lambda r: (r["T"], r["ntiles"], r["Tx"], r["nxt"]) == (64, 1, 64, 1)),
    "reflect": (REFLECT, None),
    "replicate": (C(3, 4, 6, (40, 61), (3, 5), s=(2, 3), d=(2, 1), p=(2, 4), g=2, mode="replicate", grads=True), None),
    "circular": (C(3, 4, 6, (40, 61), (3, 5), s=(2, 3), d=(2, 1), p=(2, 4), g=2, mode="circular", grads=True), None),
    "x-tiles": (C(1, 2, 2, (20, 150), (3, 9), env={"FFTCONV_XTILE": "64"}), lambda r: r["Tx"] == 64 and r["nxt"] > 1),
    "outer-tiles": (C(1, 2, 2, (150, 40), (9, 3), env={"FFTCONV_TILE": "64"}), lambda r: r["T"] == 64 and r["ntiles"] > 1),
    "3d": (C(1, 2, 3, (10, 20, 70), (3, 5, 7), p=1, grads=True), lambda r: r["Tm"] > 0),
    "middle-tiles": (C(2, 2, 2, (6, 100, 40), (3, 9, 3), env={"FFTCONV_YTILE": "64"}), lambda r: r["Tm"] == 64 and r["nyt"] > 1),
}
TRANSPOSED = {
    "t2d": (C(2, 4, 6, (19, 23), (4, 5), s=(2, 3), p=(1, 2), op=(1, 0), d=(1, 2), g=2, tr=True, grads=True), None),
    "t3d": (C(1, 2, 2, (5, 7, 9), (3, 3, 3), s=2, tr=True), lambda r: r["Tm"] > 0),
}
# every build of the two row kernels (one per transform length; 8, 4, 2 and 1 rows per workgroup): five rows of L samples,
# so the last block of rows is partial wherever a workgroup holds more than one
ROW_LENGTHS = {f"rows-{T}": (C(1, 2, 2, (5, L), (3, 9)), (lambda r, T=T: r["Tx"] == T and r["nxt"] == 1))
               for T, L in ((256, 250), (512, 500), (1024, 1000), (2048, 2000), (4096, 4000))}
CASES = {**FORWARD, **TRANSPOSED, **ROW_LENGTHS}
TRAINING = ("reflect", "replicate", "circular", "3d", "t2d")
KNOBS = ("FFTCONV_TILE", "FFTCONV_XTILE", "FFTCONV_YTILE", "FFTCONV_PLANES", "FFTCONV_NDSEG", "FFTCONV_ZEROWRAP")


def kw(c):
    if c.tr:
        return dict(stride=c.tup(c.s), padding=c.tup(c.p), output_padding=c.tup(c.op), dilation=c.tup(c.d), groups=c.g)
    return dict(stride=c.tup(c.s), padding=c.tup(c.p), dilation=c.tup(c.d), groups=c.g, padding_mode=c.mode)


def _pad_planes(x, flat, mode):
    if mode == "constant":
        return F.pad(x, flat)
    return torch.complex(F.pad(x.real, flat, mode=mode), F.pad(x.imag, flat, mode=mode))


def restated_forward(x, w, b, stride, padding, dilation, groups, mode="constant"):
    """The complex plan's passes in the tensors' own (complex128) precision; forward convolution, (Cout, Cin/g, *k) taps."""
    nd = x.dim() - 2
    xp = _pad_planes(x, [q for p in reversed(padding) for q in (p, p)], mode) if any(padding) else x
    sp = tuple(xp.shape[2:])
    kd = tuple((k - 1) * d + 1 for k, d in zip(w.shape[2:], dilation))
    T = tuple(max(64, 1 << (s - 1).bit_length()) for s in sp)          # one transform per axis holds the padded axis
    # the taps as the kernel pass loads them: spread by the dilation, conjugated
    taps = w.new_zeros(tuple(w.shape[:2]) + kd)
    taps[(Ellipsis,) + tuple(slice(None, None, d) for d in dilation)] = w.conj()
    # row passes: one row per sequence, all T bins
    xs = torch.fft.fft(xp, n=T[-1], dim=-1)
    ws = torch.fft.fft(taps, n=T[-1], dim=-1)
    # the middle passes
    other = tuple(range(2, 1 + nd))
    xs = torch.fft.fftn(xs, s=T[:-1], dim=other)
    ws = torch.fft.fftn(ws, s=T[:-1], dim=other)
    h = ws.conj() / math.prod(T)                                       # the spectrum layout stores conj(.) * scale
    B, cin, cout = x.shape[0], x.shape[1], w.shape[0]
    xg = xs.reshape((B, groups, cin // groups) + T)
    hg = h.reshape((groups, cout // groups, cin // groups) + T)
    ys = torch.einsum("bgi...,goi...->bgo...", xg, hg).reshape((B, cout) + T)      # plain product: nothing conjugated
    ys = torch.fft.ifftn(ys, dim=other, norm="forward")                # (unnormalised inverses: the scale is in h)
    y = torch.fft.ifft(ys, dim=-1, norm="forward")
    # valid window, stride, complex bias
    y = y[(Ellipsis,) + tuple(slice(0, s - k + 1, t) for s, k, t in zip(sp, kd, stride))]
    if b is not None:
        y = y + b.reshape(1, -1, *([1] * nd))
    return y.contiguous()


def restated(c, x, w, b):
    """``restated_forward`` of a case; a transposed one through the forward convolution it is (spread signal, flipped and
    exchanged taps -- the index maps the kernels apply as they load)."""
    if c.tr:
        xs, wf = au.transposed_as_forward(x, w, c.tup(c.s), c.tup(c.p), c.tup(c.op), c.tup(c.d), c.g)
        return restated_forward(xs, wf, b, (1,) * c.nd, (0,) * c.nd, c.tup(c.d), c.g)
    return restated_forward(x, w, b, c.tup(c.s), c.tup(c.p), c.tup(c.d), c.g, c.mode)


class Backend:
    """``functional._plan_for`` / ``transform_kernel`` / ``_forward_native`` on CPU tensors: a plan is its arguments, a
    spectrum the resolved weight, and the forward the restatement above.  ``install(monkeypatch)`` puts them in place."""

    def __init__(self):
        self.plans = []

    def plan_for(self, signal, kernel, bias, stride, padding, dilation, groups, padding_mode, tile_hint=None,
                 transposed=False, output_padding=0):
        n = signal.ndim - 2
        t = lambda v: tuple(int(q) for q in v) if isinstance(v, (tuple, list)) else (int(v),) * n      # noqa: E731
        plan = types.SimpleNamespace(stride=t(stride), padding=t(padding), dilation=t(dilation), groups=groups,
                                     mode=padding_mode, transposed=bool(transposed), output_padding=t(output_padding),
                                     dtype=signal.dtype, signal_shape=tuple(signal.shape), kernel_shape=tuple(kernel.shape))
        self.plans.append(plan)
        return plan

    @staticmethod
    def transform_kernel(plan, kernel):
        assert tuple(kernel.shape) == plan.kernel_shape
        return types.SimpleNamespace(plan=plan, weight=F_._resolved(kernel.detach()).contiguous())

    @staticmethod
    def forward_native(signal, spectrum, bias):
        p = spectrum.plan
        assert tuple(signal.shape) == p.signal_shape and not signal.is_conj()
        x, w = signal.detach(), spectrum.weight
        b = None if bias is None else F_._resolved(bias.detach())
        if p.transposed:
            xs, wf = au.transposed_as_forward(x, w, p.stride, p.padding, p.output_padding, p.dilation, p.groups)
            n = x.dim() - 2
            return restated_forward(xs, wf, b, (1,) * n, (0,) * n, p.dilation, p.groups)
        return restated_forward(x, w, b, p.stride, p.padding, p.dilation, p.groups, p.mode)

    def install(self, monkeypatch):
        monkeypatch.setattr(F_, "_plan_for", self.plan_for)
        monkeypatch.setattr(F_, "transform_kernel", self.transform_kernel)
        monkeypatch.setattr(F_, "_forward_native", self.forward_native)
        return self
