"""Backward of ``fft_conv`` built from the same HIP kernels.

The reference has no custom backward: autograd differentiates its rfftn/einsum/irfftn graph
(/root/reference/tests/test_functional.py:111-117 pins dW and db).  A C-ABI forward is opaque to
autograd, so the three gradients are expressed as convolutions the native library already runs:

    dX = conv_transpose(dY, W)             -> ``fc_forward`` on a transposed plan
    dW = correlate(X, dY) over the batch   -> 1-D, <= 64 channels per group: ``fc_wgrad1d`` (cross-spectra
                                              accumulated on chip); 2-D / 3-D: ``fc_wgrad_nd`` (the role-swapped
                                              convolution below, run by the library on the tensors as they lie);
                                              otherwise ``fc_forward`` with the roles of
                                              batch and channels swapped: signal' = X^T (Cin/g, B, *S), kernel' =
                                              dY^T (Cout/g, B, *Lout), dilation' = stride, stride' = dilation;
                                              all channel groups ride the group axis of that one call, long 1-D
                                              rows are cut into chunks that ride it too
    db = sum of dY over batch and space    -> a plain reduction

torch is used for data movement only (transposes, unfold views, the final chunk sum and db).

float16 / bfloat16 calls save their 16-bit signal and weight.  Backward gives each gradient the bits of the float32 cast
path (widen, run the float32 function, round): the kernels read 16-bit dY and x and compute what the float32 plan of the
same route computes; dX is written in 16 bits by its transposed plan, dW and db are summed in float32 and rounded once.
Where no 16-bit route exists (a refused dX plan, non-constant padding, the forward-plan dW, a library that predates 16-bit
weight gradients) dY and x are widened for that gradient only.

complex64 calls (2-D / 3-D) return gradients in PyTorch's convention for complex tensors, each one complex plan of the same
library: dX runs dY against conj(W) (a conjugated copy of the small weight), dW is the role-swapped forward plan of
``_grad_weight_plans`` on conj(x) and dY (the conjugate is written by the permuted copy that function builds anyway; no
conjugation flag exists in the C ABI), db is dY summed.  ``fc_wgrad_nd`` takes no complex tensors.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F
from torch import Tensor

from . import functional as F_

_DW_TILE = 2048      # FFT tile the dW correlation is sized for: the largest one that also fits the
                     # accumulating (> 8 channels', i.e. batch > 8) mode of the fused kernel in LDS


# fc_dtype code of the x / dY a weight-gradient launch reads (dW is float32 for all of them)
_WGRAD_IO = {torch.float32: 0, torch.float16: 2, torch.bfloat16: 3}

_BWD_PLANS: dict = {}      # (shapes, hyper-parameters, device) -> (transposed plan of dX, ...): skips the argument
                           # normalisation and descriptor lookup of the functional on every backward call


def _pad_adjoint(dxp: Tensor, in_spatial, padding, mode: str) -> Tensor:
    """Adjoint of ``F.pad(x, padding, mode)`` for reflect / replicate / circular: fold the border samples of the
    gradient w.r.t. the padded signal back onto their sources, one axis after the other (the padding is separable).
    A handful of slice-adds on border planes; the round-2 version back-propagated through torch's own pad with a
    zeros probe per call."""
    t = dxp
    for i, (n, p) in enumerate(zip(in_spatial, padding)):
        ax = 2 + i
        if p == 0:
            continue
        core = t.narrow(ax, p, n).clone()
        left, right = t.narrow(ax, 0, p), t.narrow(ax, n + p, p)
        if mode == "reflect":          # padded j < p reads source p - j; padded n + p + j reads source n - 2 - j
            core.narrow(ax, 1, p).add_(left.flip(ax))
            core.narrow(ax, n - 1 - p, p).add_(right.flip(ax))
        elif mode == "replicate":
            # (accumulated in float64 and rounded once: the edge sample takes up to n border samples.  A tensor that does
            # not lie contiguous is summed on compact copies of its borders, in the order of the contiguous one, whose
            # bits a channels-last gradient must have)
            wide = torch.complex128 if t.is_complex() else torch.float64
            if not t.is_contiguous():
                left, right = left.contiguous(), right.contiguous()
            core.narrow(ax, 0, 1).add_(left.sum(dim=ax, keepdim=True, dtype=wide).to(core.dtype))
            core.narrow(ax, n - 1, 1).add_(right.sum(dim=ax, keepdim=True, dtype=wide).to(core.dtype))
        elif mode == "circular":       # padded j < p reads source n - p + j; padded n + p + j reads source j
            core.narrow(ax, n - p, p).add_(left)
            core.narrow(ax, 0, p).add_(right)
        else:
            raise ValueError(f"no adjoint for padding mode {mode!r}")
        t = core
    return t.contiguous()


def _grad_input(grad: Tensor, weight: Tensor, in_spatial, stride, padding, dilation, groups, padding_mode,
                channels_last: bool = False, native: bool = False) -> Tensor:
    """dX of ``fft_conv``.  ``native``: a ``grad`` that lies channels-last is read where it lies
    (``F_._forward_native``); ``channels_last``: dX lies that way (the layout of the signal) -- written so by the
    transposed plan's last pass where the padding is zeros, one torch copy behind ``_pad_adjoint`` otherwise."""
    lay = (channels_last, native)
    if grad.dtype in F_._LOW_PRECISION:
        if padding_mode == "constant":
            try:
                return _grad_input_plan(grad, weight, in_spatial, stride, padding, dilation, groups, padding_mode, *lay)
            except NotImplementedError:
                pass      # a route the 16-bit transposed plan refuses (it would round dX between launches)
        # float32 dX (and the padding adjoint in float32), rounded once; the widened dY lives for this call only
        return _grad_input_plan(grad.float(), weight.float(), in_spatial, stride, padding, dilation, groups,
                                padding_mode, *lay).to(grad.dtype)
    return _grad_input_plan(grad, weight, in_spatial, stride, padding, dilation, groups, padding_mode, *lay)


def _grad_input_plan(grad: Tensor, weight: Tensor, in_spatial, stride, padding, dilation, groups, padding_mode,
                     channels_last: bool = False, native: bool = False) -> Tensor:
    n = grad.ndim - 2
    key = ("dx", tuple(grad.shape), tuple(weight.shape), tuple(in_spatial), stride, padding, dilation, groups, padding_mode,
           grad.device, grad.dtype)
    plan = _BWD_PLANS.get(key)
    if plan is None:
        pad_t = padding if padding_mode == "constant" else (0,) * n
        full = tuple(s + 2 * (p if padding_mode != "constant" else 0) for s, p in zip(in_spatial, padding))
        out_pad = []
        for i in range(n):
            base = (grad.shape[2 + i] - 1) * stride[i] - 2 * pad_t[i] + dilation[i] * (weight.shape[2 + i] - 1) + 1
            out_pad.append(full[i] - base)
        # conv weight (Cout, Cin/g, *k) is exactly the transposed-conv layout (Cin_t = Cout, Cout_t/g = Cin/g)
        plan = F_._plan_for(grad, weight, None, stride, pad_t, dilation, groups, "constant", transposed=True,
                            output_padding=tuple(out_pad))
        if len(_BWD_PLANS) > 256:
            _BWD_PLANS.clear()
        _BWD_PLANS[key] = plan
    if padding_mode == "constant":
        return F_._forward_lay(grad, F_.transform_kernel(plan, weight), None, channels_last, native)
    dx = _pad_adjoint(F_._forward_lay(grad, F_.transform_kernel(plan, weight), None, False, native), in_spatial, padding,
                      padding_mode)
    return F_._to_channels_last(dx) if channels_last else dx


def _permuted_copy(view: Tensor, shape, conj: bool) -> Tensor:
    """A contiguous copy of a permuted view, reshaped; ``conj``: the copy holds the conjugate (one pass either way)."""
    if not conj:
        return view.reshape(shape).contiguous()
    out = torch.empty(tuple(view.shape), dtype=view.dtype, device=view.device)
    torch.conj_physical(view, out=out)
    return out.view(shape)


def _grad_weight_plans(x: Tensor, grad: Tensor, wshape, stride, padding, dilation, groups, padding_mode,
                       conj: str = "") -> Tensor:
    """dW through forward plans with the roles of batch and channels swapped, ALL channel groups in one call
    (they ride the group axis of the swapped convolution).  x: (B, Cin, *S), grad: (B, Cout, *Lout) -> (Cout, Cin/g, *k).
    16-bit x and dY are widened here (the float32 plans; dW comes back float32).  complex64 operands (2-D / 3-D) run a
    complex plan; ``conj`` = "x" or "grad" has the permuted copy of that operand hold its conjugate (the gradient of a
    bilinear product in PyTorch's convention conjugates the operand that is not dY)."""
    if x.dtype in F_._LOW_PRECISION:
        x, grad = x.float(), grad.float()
    n = x.ndim - 2
    b, g = x.shape[0], groups
    cog, cig, ksize = wshape[0] // groups, wshape[1], tuple(wshape[2:])
    sp, lo = tuple(x.shape[2:]), tuple(grad.shape[2:])
    kext = [(lo[i] - 1) * stride[i] + 1 for i in range(n)]
    kd0 = (ksize[0] - 1) * dilation[0] + 1
    # one overlap-save tile must hold kernel' (extent kext) plus the kd - 1 further samples that give the
    # k taps of dW; a longer gradient would leave the tile (almost) no valid window (V = T - kext + 1)
    max_ext = max(_DW_TILE - kd0 + 1, _DW_TILE // 4)
    if n == 1 and kext[0] > max_ext:
        # Long rows: kernel' (the gradient) is cut into chunks of C taps; chunk j only meets the signal
        # window [j*C*s - p, j*C*s - p + (C-1)*s + 1 + Kd - 1).  Chunks (and channel groups) ride the group axis.
        s, p, d = stride[0], padding[0], dilation[0]
        kd = kd0
        c_taps = max(1, (max_ext - 1) // s + 1)
        lout = lo[0]
        nchunk = (lout + c_taps - 1) // c_taps
        seg = (c_taps - 1) * s + kd                                  # signal samples one chunk needs
        # one padded copy of each operand, then one gather through an overlapping strided view
        need = (nchunk - 1) * c_taps * s + seg
        if padding_mode == "constant" or p == 0:
            xp = F.pad(x, [p, max(0, need - x.shape[-1] - p)])       # (B, Cin, >= need)
        else:
            xp = F.pad(x, [p, p], mode=padding_mode)
            if xp.shape[-1] < need:
                xp = F.pad(xp, [0, need - xp.shape[-1]])
        xp = xp.contiguous()
        sb, sc, sl = xp.stride()
        # signal' (Cig, [g, chunk, b], seg): batch' = the input channel inside its group, channels' = (group, chunk, batch)
        sig = xp.as_strided((cig, g, nchunk, b, seg), (sc, cig * sc, c_taps * s * sl, sb, sl)).reshape(cig, g * nchunk * b, seg)
        gp = F.pad(grad, [0, nchunk * c_taps - lout]).contiguous()   # (B, Cout, nchunk*C)
        gb, gc, gl = gp.stride()
        # kernel' ([g, chunk, o], b, C): out' = (group, chunk, output channel inside the group), in' = batch
        ker = gp.as_strided((g, nchunk, cog, b, c_taps), (cog * gc, c_taps * gl, gc, gb, gl)).reshape(g * nchunk * cog, b, c_taps)
        part = F_.fft_conv(sig, ker.contiguous(), None, stride=d, padding=0, dilation=s, groups=g * nchunk)
        part = part.reshape(cig, g, nchunk, cog, -1).sum(dim=2)      # (Cig, g, Cog, >= k)
        return part[..., : ksize[0]].permute(1, 2, 0, 3).reshape(g * cog, cig, ksize[0]).contiguous()
    # signal' (Cig, [g, b], *S), kernel' ([g, o], b, *Lout), groups' = g
    xt = _permuted_copy(x.reshape((b, g, cig) + sp).permute((2, 1, 0) + tuple(range(3, 3 + n))), (cig, g * b) + sp, conj == "x")
    gt = _permuted_copy(grad.reshape((b, g, cog) + lo).permute((1, 2, 0) + tuple(range(3, 3 + n))), (g * cog, b) + lo,
                        conj == "grad")
    key = ("dwp", tuple(xt.shape), tuple(gt.shape), stride, padding, dilation, g, padding_mode, xt.device, xt.dtype)
    plan = _BWD_PLANS.get(key)
    if plan is None:
        plan = F_._plan_for(xt, gt, None, dilation, padding, stride, g, padding_mode)
        if len(_BWD_PLANS) > 256:
            _BWD_PLANS.clear()
        _BWD_PLANS[key] = plan
    out = F_._forward_native(xt, F_.transform_kernel(plan, gt), None)      # (Cig, g*Cog, >= k per axis)
    index = (slice(None), slice(None)) + tuple(slice(0, k) for k in ksize)
    return out[index].transpose(0, 1).contiguous()                  # (g*Cog, Cig, *k)


def _grad_weight_native(x: Tensor, grad: Tensor, wshape, stride, padding, dilation, groups, padding_mode,
                        want_db: bool = False):
    """dW by ``fc_wgrad1d`` (cross-spectra accumulated on chip over batch and row); None when not covered.  With
    ``want_db`` the bias gradient rides the same launch where the kernel offers it (bin 0 of the gradient spectra):
    the slices come as rows [dW | db] and ONE reduction sums both.  Returns (dW, db or None), float32 also for 16-bit
    x and dY (read as they are: a descriptor of their dtype)."""
    if x.ndim != 3 or x.dtype not in _WGRAD_IO:      # (float64 runs the direct kernel: dW through forward plans)
        return None
    from . import _native
    if grad.device != x.device:
        raise ValueError(f"gradient is on {grad.device} but the signal is on {x.device}")
    if grad.dtype != x.dtype:
        raise TypeError(f"gradient is {grad.dtype} but the signal is {x.dtype}")
    key = ("dw", tuple(x.shape), tuple(wshape), stride, padding, dilation, groups, padding_mode, x.device, x.dtype)
    hit = _BWD_PLANS.get(key)
    if hit is None:
        desc = _native.conv_desc(1, x.shape[0], x.shape[1], wshape[0], groups, (x.shape[2],), (wshape[2],), stride, padding,
                                 dilation, F_._native.PAD_MODES[padding_mode], _WGRAD_IO[x.dtype])
        # the library sizes the launch for, and keeps its twiddle tables on, the CURRENT device
        with torch.cuda.device(x.device):
            slices = _native.wgrad1d_slices(desc)
            db_ok = bool(slices) and _native.wgrad1d_db_supported(desc)
        hit = (desc, slices, db_ok)
        if len(_BWD_PLANS) > 256:
            _BWD_PLANS.clear()
        _BWD_PLANS[key] = hit
    desc, slices, db_ok = hit
    if slices == 0:
        return None
    with_db = want_db and db_ok
    n_w = wshape[0] * wshape[1] * wshape[2]
    row = n_w + (wshape[0] if with_db else 0)
    x = x.contiguous()
    grad = grad.contiguous()
    with torch.cuda.device(x.device):
        part = torch.empty((slices, row), device=x.device, dtype=torch.float32)
        _native.wgrad1d_db(desc, x.data_ptr(), grad.data_ptr(), part.data_ptr(),
                           part.data_ptr() + 4 * n_w if with_db else None, row, slices,
                           torch.cuda.current_stream(x.device).cuda_stream)
    total = part[0] if slices == 1 else part.sum(dim=0)
    return total[:n_w].view(wshape), (total[n_w:] if with_db else None)


def _grad_weight_nd_native(x: Tensor, grad: Tensor, wshape, stride, padding, dilation, groups, padding_mode):
    """2-D / 3-D dW by ``fc_wgrad_nd``: the role-swapped convolution run by the library on the tensors as they are
    (x (B, Cin, *S) and dY (B, Cout, *Lout) are read, dW (Cout, Cin/g, *k) is written, in these layouts) -- no transposed
    copies, no crop, no reduction on the torch side.  None when not covered (1-D, float64, a shape the plan refuses).
    16-bit x and dY are read as they are; dW is float32."""
    n = x.ndim - 2
    if n < 2 or x.dtype not in _WGRAD_IO:
        return None
    from . import _native
    if grad.device != x.device:
        raise ValueError(f"gradient is on {grad.device} but the signal is on {x.device}")
    if grad.dtype != x.dtype:
        raise TypeError(f"gradient is {grad.dtype} but the signal is {x.dtype}")
    key = ("dwn", tuple(x.shape), tuple(wshape), stride, padding, dilation, groups, padding_mode, x.device, x.dtype)
    plan = _BWD_PLANS.get(key)
    if plan is None:
        desc = _native.conv_desc(n, x.shape[0], x.shape[1], wshape[0], groups, tuple(x.shape[2:]), tuple(wshape[2:]), stride,
                                 padding, dilation, F_._native.PAD_MODES[padding_mode], _WGRAD_IO[x.dtype])
        try:
            with torch.cuda.device(x.device):
                plan = _native.WgradPlan(desc)
        except NotImplementedError:
            plan = False                      # (remembered: the forward-plan route below takes this shape)
        if len(_BWD_PLANS) > 256:
            _BWD_PLANS.clear()
        _BWD_PLANS[key] = plan
    if plan is False:
        return None
    x = x.contiguous()
    grad = grad.contiguous()
    with torch.cuda.device(x.device):
        dw = torch.empty(tuple(wshape), device=x.device, dtype=torch.float32)
        spec = torch.empty(plan.spectrum_bytes, device=x.device, dtype=torch.uint8)
        ws = torch.empty(max(plan.workspace_bytes, 1), device=x.device, dtype=torch.uint8)
        plan.run(x.data_ptr(), grad.data_ptr(), dw.data_ptr(), spec.data_ptr(), ws.data_ptr(),
                 torch.cuda.current_stream(x.device).cuda_stream)
    return dw


def _grad_weight_db(x: Tensor, grad: Tensor, wshape, stride, padding, dilation, groups, padding_mode,
                    want_db: bool = False, conj: str = ""):
    """(dW, db or None) in float32 by the first route that covers the shape: fc_wgrad1d (db riding it where offered),
    fc_wgrad_nd, forward plans.  16-bit x and dY that no 16-bit launch takes (a library without 16-bit weight gradients)
    are widened for this gradient, and the float32 routes decide -- the bits of the cast path either way."""
    if x.is_complex():      # (no complex weight-gradient launch: the role-swapped forward plan)
        return _grad_weight_plans(x, grad, wshape, stride, padding, dilation, groups, padding_mode, conj), None
    native = _grad_weight_native(x, grad, wshape, stride, padding, dilation, groups, padding_mode, want_db)
    if native is not None:
        return native
    nd = _grad_weight_nd_native(x, grad, wshape, stride, padding, dilation, groups, padding_mode)
    if nd is not None:
        return nd, None
    if x.dtype in F_._LOW_PRECISION:
        return _grad_weight_db(x.float(), grad.float(), wshape, stride, padding, dilation, groups, padding_mode, want_db)
    return _grad_weight_plans(x, grad, wshape, stride, padding, dilation, groups, padding_mode, conj), None


def _grad_weight(x: Tensor, grad: Tensor, wshape, stride, padding, dilation, groups, padding_mode, conj: str = "") -> Tensor:
    return _grad_weight_db(x, grad, wshape, stride, padding, dilation, groups, padding_mode, conj=conj)[0]


def _backward_operands(signal: Tensor, grad: Tensor, need_contiguous: bool, channels_last: bool):
    """What both N-d backward functions start from.  ``channels_last``: the keyword of the forward call.  -> (dY as the
    dX launch takes it: where it lies if it lies channels-last and the call takes layouts natively
    (``F_._nd_cl_native``), a contiguous copy otherwise; the contiguous dY that dW and db read -- one copy serves both,
    None when neither is wanted; whether dX gets the channels-last layout of the signal: in a call with the keyword, or
    under FFTCONV_ND_CL=1; whether the call takes layouts natively).  A call without the keyword and without the knob
    gets what it always got: one contiguous dY for all three gradients, a contiguous dX."""
    grad = F_._resolved(grad)
    nd = grad.ndim >= 4
    native = nd and F_._nd_cl_native(channels_last)
    follows = nd and (channels_last or native)
    lies_cl = native and F_._nd_layout(grad) == "cl"
    gradc = grad.contiguous() if (need_contiguous or not lies_cl) else None
    return (grad if lies_cl else gradc), gradc, follows and F_._nd_layout(signal) == "cl", native


def _grad_bias(grad: Tensor) -> Tensor:
    """Sum of dY over batch and space; a 16-bit dY is summed as the float32 cast path sums it (widened first)."""
    if grad.dtype in F_._LOW_PRECISION:
        grad = grad.float()
    return grad.sum(dim=[0] + list(range(2, grad.ndim)))


class FFTConvFunction(torch.autograd.Function):
    """``fft_conv`` with gradients; ``spectrum`` is an optional pre-transformed kernel (module cache)."""

    @staticmethod
    def forward(ctx, signal: Tensor, kernel: Tensor, bias: Optional[Tensor], stride: Tuple[int, ...],
                padding: Tuple[int, ...], dilation: Tuple[int, ...], groups: int, padding_mode: str, spectrum,
                channels_last: bool = False):
        plan = F_._plan_for(signal, kernel, bias, stride, padding, dilation, groups, padding_mode)
        if spectrum is None or spectrum.plan is not plan:
            spectrum = F_.transform_kernel(plan, kernel)
        ctx.save_for_backward(signal, kernel)
        ctx.conf = (stride, padding, dilation, groups, padding_mode, bias is not None)
        ctx.channels_last = bool(channels_last)
        return F_._forward_lay(signal, spectrum, bias, channels_last)

    @staticmethod
    def backward(ctx, grad: Tensor):
        signal, kernel = ctx.saved_tensors
        stride, padding, dilation, groups, padding_mode, has_bias = ctx.conf
        want_db = has_bias and ctx.needs_input_grad[2]
        # (dW and db keep contiguous operands -- their bits stay; dX reads a channels-last dY where it lies)
        grad_x, grad, dx_cl, native = _backward_operands(signal, grad, ctx.needs_input_grad[1] or want_db, ctx.channels_last)
        cx = signal.is_complex()      # PyTorch's convention: dW from conj(x), dX against conj(W)
        d_signal = d_kernel = d_bias = None
        if ctx.needs_input_grad[1]:
            # (db rides the weight-gradient launch where the kernel offers it; dW goes first: widened 16-bit operands of a
            # weight-gradient route are freed before dX is allocated)
            d_kernel, d_bias = _grad_weight_db(signal.detach(), grad, tuple(kernel.shape), stride, padding, dilation,
                                               groups, padding_mode, want_db, conj="x" if cx else "")
            d_kernel = d_kernel.to(kernel.dtype)     # (16-bit: the float32 sum rounded once)
        if ctx.needs_input_grad[0]:
            d_signal = _grad_input(grad_x, kernel.detach().conj() if cx else kernel.detach(), tuple(signal.shape[2:]), stride,
                                   padding, dilation, groups, padding_mode, dx_cl, native)
        if want_db and d_bias is None:
            d_bias = _grad_bias(grad)
        if d_bias is not None:
            d_bias = d_bias.to(kernel.dtype)
        return d_signal, d_kernel, d_bias, None, None, None, None, None, None, None


class FFTConvTransposeFunction(torch.autograd.Function):
    """``fft_conv_transpose`` with gradients (the reference's transposed op is
    differentiable through its rfftn/einsum/irfftn graph and its tests pin dW and db:
    /root/reference/tests/test_functional_transpose.py:73-124).  With y = convT(x, W), W of shape
    (Cin, Cout/g, *k):

        dX = conv(dY, W)                  the ordinary convolution with the same hyper-parameters: a forward plan
                                          (W read as a conv weight with Cin outputs and Cout/g inputs per group)
        dW = the weight gradient of that  convolution, with dY as its signal and x as its output gradient
        db = sum of dY over batch and space
    """

    @staticmethod
    def forward(ctx, signal: Tensor, kernel: Tensor, bias: Optional[Tensor], stride: Tuple[int, ...],
                padding: Tuple[int, ...], output_padding: Tuple[int, ...], dilation: Tuple[int, ...], groups: int,
                spectrum, channels_last: bool = False):
        plan = F_._plan_for(signal, kernel, bias, stride, padding, dilation, groups, "constant",
                            transposed=True, output_padding=output_padding)
        if spectrum is None or spectrum.plan is not plan:
            spectrum = F_.transform_kernel(plan, kernel)
        ctx.save_for_backward(signal, kernel)
        ctx.conf = (stride, padding, dilation, groups, bias is not None)
        ctx.channels_last = bool(channels_last)
        return F_._forward_lay(signal, spectrum, bias, channels_last)

    @staticmethod
    def backward(ctx, grad: Tensor):
        signal, kernel = ctx.saved_tensors
        stride, padding, dilation, groups, has_bias = ctx.conf
        want_db = has_bias and ctx.needs_input_grad[2]
        grad_x, grad, dx_cl, native = _backward_operands(signal, grad, ctx.needs_input_grad[1] or want_db, ctx.channels_last)
        cx = signal.is_complex()      # (as in FFTConvFunction: x is the "output gradient" operand of dW here)
        n = grad_x.ndim - 2      # (``grad``, the contiguous dY of dW and db, is None when neither is wanted)
        in_spatial = tuple(signal.shape[2:])
        # extent of conv(dY, W) per axis: >= the input extent; larger only when output_padding >= stride
        conv_sp = tuple((grad_x.shape[2 + i] + 2 * padding[i] - dilation[i] * (kernel.shape[2 + i] - 1) - 1) // stride[i] + 1
                        for i in range(n))
        d_signal = d_kernel = d_bias = None
        if ctx.needs_input_grad[0]:
            # (under create_graph this call becomes FFTConvFunction.apply, which carries the keyword but not ``native``: a
            #  channels-last dY of a planar signal is then copied -- the same values)
            dx = F_._fft_conv_impl(grad_x, kernel.detach().conj() if cx else kernel.detach(), None, stride, padding, dilation,
                                   groups, "constant", None, channels_last=dx_cl, native=native)
            if conv_sp != in_spatial:
                dx = dx[(slice(None), slice(None)) + tuple(slice(0, s) for s in in_spatial)]
                dx = F_._to_channels_last(dx) if dx_cl else dx.contiguous()
            d_signal = dx
        if ctx.needs_input_grad[1]:
            xg = signal.detach()
            if conv_sp != in_spatial:     # rows past the input contribute nothing: zero-extend (data movement)
                flat = []
                for i in reversed(range(n)):
                    flat += [0, conv_sp[i] - in_spatial[i]]
                xg = F.pad(xg, flat)
            d_kernel = _grad_weight(grad, xg, tuple(kernel.shape), stride, padding, dilation, groups, "constant",
                                    conj="grad" if cx else "")
            d_kernel = d_kernel.to(kernel.dtype)
        if want_db:
            d_bias = _grad_bias(grad).to(kernel.dtype)
        return d_signal, d_kernel, d_bias, None, None, None, None, None, None, None


def _phase_rows(t: Tensor, front: int, stride: int, rows: int, groups: int) -> Tensor:
    """The ``stride`` decimated rows of a (B, C, n) tensor read with ``front`` zeros in front, with batch and channels
    exchanged: (C/g * stride, g*B, rows), element [(c, p), (g, b), r] = trow[b, (g, c), stride*r + p] (zero past the data).
    The operand of a weight gradient by phases: the phase is a batch-like index of that run.  torch builds it."""
    B, C, n = t.shape
    row = F.pad(t, (front, stride * rows - front - n))          # (a negative count crops what no kept lag reaches)
    return row.view(B, groups, C // groups, rows, stride).permute(2, 4, 1, 0, 3).reshape(C // groups * stride, groups * B, rows).contiguous()


def _interleave_lags(du: Tensor, stride: int, taps: int) -> Tensor:
    """(C' * stride, O, Kp) lags of ``_phase_rows`` operands -> (O, C', K): lag stride*m + p from [(c, p), o, m]."""
    cs, o, kp = du.shape
    return du.view(cs // stride, stride, o, kp).permute(2, 0, 3, 1).reshape(o, cs // stride, kp * stride)[..., :taps]


def _long_backward_operands(signal: Tensor, grad: Tensor):
    """What both long backward functions start from -> (dY with a lazy conjugate resolved, read where it lies if the
    kernels read it channels-last (``F_._long_reads_nlc``) and contiguous otherwise; whether dX is written as a
    channels-last signal lies; whether the call is complex)."""
    grad = F_._resolved(grad.detach())
    if not F_._long_reads_nlc(grad):
        grad = grad.contiguous()
    return grad, F_._long_layout(signal) == "nlc", signal.dtype == torch.complex64


def _long_grad_bias(grad: Tensor, dtype: torch.dtype) -> Tensor:
    """db of the long functions: ``_grad_bias`` sums a contiguous dY, so a strided dY is copied for it."""
    return _grad_bias(grad.contiguous()).to(dtype)


def _long_dw_exchanged(rows: Tensor, taps: Tensor, groups: int, pad_left: int, pad_right: int, lags: int, **run) -> Tensor:
    """The weight gradient as the long primitive with batch and channels exchanged (the docstrings of the two functions
    below): signal' = ``rows`` (B, C, n) as (C/g, g*B, n), filter' = ``taps`` (B, O, m) as (O, B, m), the first ``lags`` lags
    kept -> float32 (O, C/g, lags).  ``run``: further keywords of ``F_._long_run``.  torch builds the transposed copies."""
    B, C, n = rows.shape
    sig = rows.reshape(B, groups, C // groups, n).permute(2, 1, 0, 3).reshape(C // groups, groups * B, n).contiguous()
    du = F_._long_run(sig, taps.permute(1, 0, 2).contiguous(), None, pad_left, pad_right, False, lags, groups,
                      out_dtype=torch.float32, **run)
    return du.permute(1, 0, 2)


def _long_dw_by_phases(rows: Tensor, taps: Tensor, groups: int, front: int, stride: int, lags: int) -> Tensor:
    """The weight gradient with the phase as a batch-like index: signal' = the ``stride`` decimated rows of ``rows``
    (B, C, n) read with ``front`` zeros in front (``_phase_rows``), filter' = ``taps`` (B, O, m) as (O, B, m) at tap_dil 1,
    ceil(lags / stride) lags kept and interleaved into ``lags`` by the permute copy -> float32 (O, C/g, lags)."""
    kp = -(-lags // stride)
    sig = _phase_rows(rows, front, stride, taps.shape[2] + kp - 1, groups)
    du = F_._long_run(sig, taps.permute(1, 0, 2).contiguous(), None, 0, 0, False, kp, groups, out_dtype=torch.float32)
    return _interleave_lags(du, stride, lags).contiguous()


def _fits_plain(key) -> bool:
    """Whether the long plan of this key (``_native.long_desc`` words) fits the 2**24 points of the path: its geometry, asked
    of the library from the descriptor alone (no device)."""
    try:
        F_._native.long_geometry(tuple(int(v) for v in key))
    except NotImplementedError:
        return False
    return True


class FFTLongConvFunction(torch.autograd.Function):
    """``fft_long_conv`` with its three gradients, each through the same three kernels (``F_._long_run``, the primitive
    y[j] = sum_k u[k] * xrow[out_step*j + tap_dil*k] with separate left / right padding in a padding mode, a tap order, a
    count of kept samples and a row that may be spread over a grid of src_up).  With stride s, dilation d, Lp the padded
    length and nout the output length:

        dX = the primitive on dY spread by s (src_up), the opposite tap order at tap_dil = d, left padding
             d*(K - 1) - pad_left, out_step 1 and in / out channels exchanged; L samples kept with zero padding, else the
             Lp samples of the gradient of the padded row, folded onto their sources by ``_pad_adjoint``;
        dW = the primitive with batch and channels exchanged, signal' = x as (Cin/g, g*B, L) read with the forward's
             padding and mode, kernel' = dY as (Cout, B, nout) at tap_dil = s, out_step = d, the first K lags kept --
             flipped afterwards when the forward read the taps flipped (causal);
        db = dY summed over batch and row.

    torch builds the transposed copies of the operands.

    FFTCONV_LONG_WGRAD=1 (read per call; ``F_._long_wgrad_route`` names the route) takes dW on this branch from a
    weight-gradient plan instead (``F_._long_wgrad_run``, float32 / float16 / bfloat16): x and dY are read where they lie,
    contiguous or channels-last, the correlation is summed over the batch pairs in registers, and dW is stored in the
    weight's own order and dtype (16-bit: the float32 result rounded once) -- no ``xt``, ``dyt`` or flipped copy exists.
    Its bits differ from the exchanged route's.  dX and db are unchanged.

    A non-causal forward that ran by phases (``decim``: ``F_._long_route`` "phases", a decimation plan) has the gradients of
    the same length: dX is the transposed convolution of dY run by PHASES (``F_._long_transpose_run``: stride s, padding p,
    output_padding (L + 2p - K) mod s, the (Cout, Cin/g, K) weight read where it lies), and dW the primitive with the phase
    as a batch-like index: signal' = the s decimated rows of x as (Cin/g * s, g*B, nout + Kp - 1), kernel' = dY as
    (Cout, B, nout) at tap_dil 1, Kp = ceil(K / s) lags kept, interleaved into K by the permute copy.  A CAUSAL forward
    keeps the constructions above whatever its route: a causal row past 2**24 points runs forward and cannot be trained.

    float16 / bfloat16 calls run on their 16-bit tensors (autograd saves 16-bit signal and weight): dX reads 16-bit dY
    and the 16-bit transposed weight and is written in 16 bits (with a padding mode to fold: in float32, folded, rounded
    once); dW reads the 16-bit transposed copies of x and dY, comes back float32 and is rounded once; db is summed in
    float32.  Each gradient has the bits of the float32 cast path.

    complex64 calls follow PyTorch's convention for complex gradients with the same three constructions, each one run of
    the primitive on a complex plan: dX runs dY against conj(weight), dW runs conj(x) as the signal against dY as the
    filter (K complex lags kept), db is dY summed.  The conjugates are not copies: the plan carries a flag
    (``conj_kernel`` / ``conj_signal`` of ``F_._long_run``) and ``long_cols_fwd`` flips the sign of the imaginary part as it
    loads.  A lazily conjugated dY is resolved first.

    Layouts (``F_._long_layout``): the forward reads a signal that lies as a contiguous (B, L, C) tensor where it lies and
    writes y that way with ``channels_last``.  dX is the same primitive, so a dY that lies that way is read where it lies,
    and dX is written in the signal's layout (after a padding-mode fold, which torch runs on whatever layout dX has, one
    torch copy restores it; so does one after the dX by phases, whose plan writes contiguous rows: a signal that lies
    that way runs by phases under FFTCONV_LONG_NLC=0 only).  dW's operands are transposed copies anyway and torch builds
    them from whichever layout the tensors have; db sums a contiguous dY, so a strided dY is copied for it.

    ``blocks`` = (the ``blocks`` keyword of the call, the block_points its forward runs by or None;
    ``F_._long_blocks_route_of``).  A forward by blocks runs the blocks plan.  dX is the same primitive on dY with the
    opposite tap order and runs by blocks under the keyword's own rule (``F_._long_blocks_choice`` on dX's numbers: with an
    int N by blocks of N wherever its row needs more, with True only where its row does not fit 2**24 points).  dW of a
    forward that ran by blocks comes from the weight-gradient plan by blocks whatever FFTCONV_LONG_WGRAD says (the
    exchanged route would need dY as a filter of nout taps); db is as ever."""

    @staticmethod
    def forward(ctx, signal, kernel, bias, pad_left, pad_right, causal, groups, spectrum, stride=1, dilation=1,
                padding_mode="constant", channels_last=False, decim=False, blocks=(False, None)):
        ctx.save_for_backward(signal, kernel)
        ctx.cfg = (int(pad_left), int(pad_right), bool(causal), int(groups), bias is not None, int(stride), int(dilation),
                   padding_mode)
        ctx.decim = bool(decim)
        ctx.blocks = blocks
        route = "blocks" if blocks[1] is not None else "phases" if decim else "plain"
        run = F_._long_forward_plan(signal, kernel.shape, bias is not None, pad_left, pad_right, causal, groups, stride,
                                    dilation, F_._native.PAD_MODES[padding_mode], route, block_points=blocks[1])[1]
        return F_._long_run(signal, kernel, bias, pad_left, pad_right, causal, groups=groups, spectrum=spectrum,
                            channels_last=channels_last, **run)

    @staticmethod
    def backward(ctx, grad):
        signal, kernel = ctx.saved_tensors
        pad_left, pad_right, flip, g, has_bias, s, d, padding_mode = ctx.cfg
        mode = F_._native.PAD_MODES[padding_mode]
        grad, x_nlc, cx = _long_backward_operands(signal, grad)
        B, cin, L = signal.shape
        cout, cig, K = kernel.shape
        cog = cout // g
        dx = dw = None
        want_db = has_bias and ctx.needs_input_grad[2]
        if ctx.decim and not flip:
            # (non-causal: pad_left == pad_right; the transposed convolution of dY by phases, and dW with the phase as batch)
            if ctx.needs_input_grad[0]:
                dx = F_._long_transpose_run(grad, kernel.detach().contiguous(), None, s, pad_left,
                                            (L + 2 * pad_left - K) % s, 1, g, "phases")
                if x_nlc:       # (FFTCONV_LONG_NLC=0 only: otherwise such a signal does not run by phases)
                    dx = F_._as_channels_last(dx)
            if ctx.needs_input_grad[1]:
                dw = _long_dw_by_phases(signal.detach(), grad, g, pad_left, s, K).to(kernel.dtype)
            return (dx, dw, _long_grad_bias(grad, kernel.dtype) if want_db else None) + (None,) * 11
        if ctx.needs_input_grad[0]:
            wt = kernel.detach().view(g, cog, cig, K).transpose(1, 2).reshape(cin, cog, K).contiguous()
            # zero padding: the gradient of the row itself; another mode: of the padded row, folded below
            keep, lead, dy = (L, d * (K - 1) - pad_left, grad) if mode == 0 else (L + pad_left + pad_right, d * (K - 1), grad)
            if lead < 0:        # padding wider than the filter: those leading output samples never met the data
                drop = -(lead // s)
                dy, lead = dy[..., drop:], lead + drop * s
            tail = keep + d * (K - 1) - lead - (s * (dy.shape[2] - 1) + 1)
            if tail < 0 and dy.shape[2]:
                dy, tail = dy[..., :max(0, dy.shape[2] - (-tail) // s)], 0
            if dy.shape[2] == 0:
                dx = torch.zeros_like(signal)          # (keeps the signal's strides)
            else:
                fold32 = mode != 0 and grad.dtype in F_._LOW_PRECISION
                tail = max(tail, 0)
                # (the keyword's rule on dX's own row: cout -> cin channels, dY's length, the row of lead + dY + tail samples)
                points = F_._long_blocks_choice(ctx.blocks[0], B, cout, cin, g, dy.shape[2], K, lead, tail, keep, not flip,
                                                lead + dy.shape[2] + tail, s, d, mode, dy.dtype, F_._long_route_layout(dy), x_nlc)
                if points is not None:
                    plan = F_._long_blocks_plan(dy, cin, g, K, lead, tail, not flip, keep, False, points)
                    dx = F_._long_run(dy, wt, None, lead, tail, not flip, keep, g, plan=plan)
                else:
                    dx = F_._long_run(dy, wt, None, lead, tail, not flip, keep, g,
                                      out_dtype=torch.float32 if fold32 else None, src_up=s, tap_dil=d, conj_kernel=cx,
                                      channels_last=x_nlc)
                if mode != 0:
                    # (_pad_adjoint folds equal paddings: a row padded by the larger one has zero gradient at the rest)
                    p = max(pad_left, pad_right)
                    if p:
                        dx = _pad_adjoint(F.pad(dx, (p - pad_left, p - pad_right)), (L,), (p,), padding_mode)
                    dx = dx.to(grad.dtype)
                    if x_nlc:
                        dx = F_._as_channels_last(dx)
        if ctx.needs_input_grad[1] and ctx.blocks[1] is not None:
            wkey = F_._long_wgrad_key(B, cin, cout, g, L, K, pad_left, pad_right, grad.shape[2], flip, 0, 1, 1)
            dw = F_._long_wgrad_run(signal, grad, tuple(kernel.shape), wkey, kernel.dtype, block_points=ctx.blocks[1])
        elif ctx.needs_input_grad[1]:
            dw = _long_grad_weight(signal, grad, kernel, g, pad_left, pad_right, flip, mode, s, d, cx)
        return (dx, dw, _long_grad_bias(grad, kernel.dtype) if want_db else None) + (None,) * 11


def _long_grad_weight(signal: Tensor, grad: Tensor, kernel: Tensor, g: int, pad_left: int, pad_right: int, flip: bool,
                      mode: int, s: int, d: int, cx: bool) -> Tensor:
    """dW of the plain branch of ``FFTLongConvFunction.backward`` (its docstring): the weight-gradient plan under
    FFTCONV_LONG_WGRAD=1, else the primitive with batch and channels exchanged; ``kernel`` gives shape and dtype."""
    B, cin, L = signal.shape
    cout, _, K = kernel.shape
    wkey = F_._long_wgrad_key(B, cin, cout, g, L, K, pad_left, pad_right, grad.shape[2], flip, mode, s, d)
    if F_._long_wgrad_eligible(wkey, signal.dtype):
        # FFTCONV_LONG_WGRAD=1: x and dY where they lie, dW in the weight's own order and dtype
        return F_._long_wgrad_run(signal, grad, tuple(kernel.shape), wkey, kernel.dtype)
    du = _long_dw_exchanged(signal.detach(), grad, g, pad_left, pad_right, K, pad_mode=mode, tap_dil=s, out_step=d,
                            conj_signal=cx)
    return (du.flip(-1) if flip else du).contiguous().to(kernel.dtype)


class FFTLongConvGatedFunction(torch.autograd.Function):
    """The fused route of ``fft_long_conv_gated`` (``F_._long_gated_route`` "fused": real tensors, the plain primitive at
    stride 1, dilation 1, zero padding, contiguous rows) with its five gradients.  With z = pregate * x, c = conv(z) + bias,
    y = postgate * c and g = postgate * dY (an absent gate: all ones):

        forward      one ``F_._long_run_gated``.  Saved: x, kernel, bias, the gates -- never z or y -- and c only where
                     ``postgate`` needs a gradient: the same launch stores it as its second result (float32 for 16-bit
                     tensors, so that d(postgate) is rounded once);
        dX, dPre     ONE run of the dX construction of ``FFTLongConvFunction`` (the same plan on the same transposed
                     weight, dY and ``postgate`` trimmed alike): ``postgate`` gates dY as the first pass loads it, the last
                     pass stores dX = pregate * dZ and d(pregate) = x * dZ, or the one of them that is wanted;
        dPost        dY * c, one torch multiply (in float32, rounded once);
        dW, db       with FFTCONV_LONG_WGRAD unset (or a layer the weight-gradient plan refuses; ``F_._long_gated_dw_route``
                     "products") the routes of ``FFTLongConvFunction`` on the products z and g, which torch forms in
                     float32: transient tensors.  Under FFTCONV_LONG_WGRAD=1 ("gated-plan") dW is ONE run of the
                     weight-gradient plan on the saved x, dY and the gates in their own dtype, each gate multiplied in as
                     the plan's column pass loads its sample (``F_._long_wgrad_run`` with gates): z is never formed, and g
                     only where db is wanted, as above, dropped before the plan runs.  dW then has the bits of that plan on
                     the float32 products, which is what the composed line computes under the same switch.

    Each gradient has the bits of autograd through ``postgate * fft_long_conv(pregate * x, ...)`` on float32 tensors,
    rounded once.  A backward that itself records a graph (``create_graph=True``) differentiates that composed line."""

    @staticmethod
    def forward(ctx, signal, kernel, bias, pregate, postgate, pad_left, pad_right, causal, groups, spectrum):
        keep_c = postgate is not None and ctx.needs_input_grad[4]
        plan, run = F_._long_forward_plan(signal, kernel.shape, bias is not None, pad_left, pad_right, causal, groups, 1, 1, 0,
                                          "plain")
        y, c = F_._long_run_gated(signal, kernel, bias, pad_left, pad_right, causal, run["out_keep"], groups, spectrum,
                                  pregate=pregate, gate=postgate, second=keep_c, second_dtype=torch.float32, plan=plan)
        ctx.save_for_backward(signal, kernel, bias, pregate, postgate, c)
        ctx.cfg = (int(pad_left), int(pad_right), bool(causal), int(groups))
        return y

    @staticmethod
    def backward(ctx, grad):
        signal, kernel, bias, pregate, postgate, c = ctx.saved_tensors
        pad_left, pad_right, flip, g = ctx.cfg
        need = ctx.needs_input_grad
        if torch.is_grad_enabled():      # a backward that records a graph: the composed line, which torch differentiates
            with torch.enable_grad():
                z = signal if pregate is None else pregate * signal
                out = FFTLongConvFunction.apply(z, kernel, bias, pad_left, pad_right, flip, g, None)
                out = out if postgate is None else postgate * out
            inputs = [t for t, n in zip((signal, kernel, bias, pregate, postgate), need) if n]
            grads = iter(torch.autograd.grad(out, inputs, grad, create_graph=True, allow_unused=True))
            return tuple(next(grads) if n else None for n in need[:5]) + (None,) * 5
        grad = grad.detach().contiguous()
        B, cin, L = signal.shape
        cout, cig, K = kernel.shape
        cog = cout // g
        low = signal.dtype in F_._LOW_PRECISION
        dx = dw = db = dpre = dpost = None
        want_dpre = pregate is not None and need[3]
        if postgate is not None and need[4]:
            dpost = grad.float().mul_(c).to(grad.dtype) if low else grad * c
        if need[0] or want_dpre:
            wt = kernel.detach().view(g, cog, cig, K).transpose(1, 2).reshape(cin, cog, K).contiguous()
            lead, dy, pg = K - 1 - pad_left, grad, postgate
            if lead < 0:        # padding wider than the filter: those leading output samples never met the data
                dy, pg, lead = dy[..., -lead:], None if pg is None else pg[..., -lead:], 0
            tail = L + K - 1 - lead - dy.shape[2]
            if tail < 0 and dy.shape[2]:
                keep = max(0, dy.shape[2] + tail)
                dy, pg, tail = dy[..., :keep], None if pg is None else pg[..., :keep], 0
            if dy.shape[2] == 0:
                dx = torch.zeros_like(signal) if need[0] else None
                dpre = torch.zeros_like(signal) if want_dpre else None
            else:
                # the results of the last pass: dX = pregate * dZ where wanted, then d(pregate) = x * dZ where wanted
                gates = ([pregate] if need[0] else []) + ([signal] if want_dpre else [])
                res = F_._long_run_gated(dy, wt, None, lead, max(tail, 0), not flip, L, g, pregate=pg, gate=gates[0],
                                         gate2=gates[1] if len(gates) > 1 else None)
                dx = res[0] if need[0] else None
                dpre = res[len(gates) - 1] if want_dpre else None
        wkey = F_._long_wgrad_key(B, cin, cout, g, L, K, pad_left, pad_right, grad.shape[2], flip, 0, 1, 1)
        if need[1] and F_._long_wgrad_eligible(wkey, signal.dtype):
            # FFTCONV_LONG_WGRAD=1 (``F_._long_gated_dw_route`` "gated-plan"): the gates ride the plan's two column reads, so
            # z never exists, and g only for db -- formed as below, and gone before the plan runs
            if bias is not None and need[2]:
                gq = grad if postgate is None else (grad.float().mul_(postgate.detach()) if low else grad * postgate.detach())
                db = _long_grad_bias(gq, kernel.dtype)
                del gq
            dw = F_._long_wgrad_run(signal, grad, tuple(kernel.shape), wkey, kernel.dtype, pregate=pregate, postgate=postgate)
        elif need[1] or (bias is not None and need[2]):
            # (the float32 products torch forms; an absent gate leaves the tensor as it is)
            # (16-bit: a float32 copy times the 16-bit tensor, widened as mul_ reads it: two passes, one float32 tensor)
            wide = (lambda a, b: a.float().mul_(b)) if low else torch.mul
            gq = grad if postgate is None else wide(grad, postgate.detach())
            if need[1]:
                z = signal.detach() if pregate is None else wide(signal.detach(), pregate.detach())
                dw = _long_grad_weight(z, gq, kernel, g, pad_left, pad_right, flip, 0, 1, 1, False)
            if bias is not None and need[2]:
                db = _long_grad_bias(gq, kernel.dtype)
        return (dx, dw, db, dpre, dpost) + (None,) * 5


class FFTLongConvTransposeFunction(torch.autograd.Function):
    """``fft_long_conv_transpose`` with its three gradients.  The forward runs on the route the functional picked
    (``F_._long_transpose_run``: by phases, or on the zero-spread row); the gradients are runs of the long primitive
    (``F_._long_run``) whatever the route, with the roles of ``FFTConvTransposeFunction``.  With y = convT(x, W), W of shape
    (Cin, Cout/g, K), stride s, dilation d, padding p and Lout the output length:

        dX = the FORWARD strided primitive on dY: tap_dil = d, out_step = s, the taps in tensor order, p zeros on both
             sides, L samples kept.  W (Cin, Cout/g, K) already is the (out, in/g, K) weight of that convolution: no copy;
        dW = the primitive with batch and channels exchanged: signal' = dY as (Cout/g, g*B, Lout) read with p zeros in
             front, filter' = x as (Cin, B, L) at tap_dil = s, out_step = d, the first K lags kept, permuted to
             (Cin, Cout/g, K).  torch builds the two transposed copies;
        db = dY summed over batch and row.

    float16 / bfloat16 and complex64 calls follow the rules of ``FFTLongConvFunction``: autograd saves the 16-bit tensors, dX
    is written in 16 bits, dW comes back float32 and is rounded once, db is summed in float32 -- each gradient has the bits
    of the float32 cast path; complex gradients follow PyTorch's convention, dX runs dY against conj(W) (``conj_kernel``) and
    dW runs dY against conj(x), which here is the FILTER of the run (``conj_kernel`` again), without conjugated copies.  A dY
    that lies as a contiguous (B, L, C) tensor is read where it lies for dX, and dX is written as the signal lies.

    With dilation 1, stride 2 ... 64 and real tensors both gradients also run on rows s times shorter, where
    FFTCONV_LONG_DECIM selects it ("1": wherever eligible; unset: only where the construction above does not fit 2**24
    points; "0": never):

        dX = the same strided primitive on a DECIMATION plan (``F_._long_run(decim=s)``): the s decimated rows of dY against
             the phases of W, a transform of about L + ceil(K/s) points.  dY is read contiguous;
        dW = the primitive with the phase as a batch-like index: signal' = the s decimated rows of dY read with p zeros in
             front as (Cout/g * s, g*B, L + Kp - 1), filter' = x as (Cin, B, L) at tap_dil 1, Kp = ceil(K/s) lags kept,
             interleaved into K by the permute copy.  One copy of dY, as above."""

    @staticmethod
    def forward(ctx, signal, kernel, bias, stride, padding, output_padding, dilation, groups, spectrum, channels_last, route):
        ctx.save_for_backward(signal, kernel)
        ctx.cfg = (int(stride), int(padding), int(output_padding), int(dilation), int(groups), bias is not None)
        return F_._long_transpose_run(signal, kernel, bias, stride, padding, output_padding, dilation, groups, route, spectrum,
                                      channels_last)

    @staticmethod
    def backward(ctx, grad):
        signal, kernel = ctx.saved_tensors
        s, p, op, d, g, has_bias = ctx.cfg
        grad, x_nlc, cx = _long_backward_operands(signal, grad)
        B, cin, L = signal.shape
        cog, K = kernel.shape[1], kernel.shape[2]
        lout = grad.shape[2]
        dx = dw = db = None
        mode = F_._long_decim_mode()
        kp = -(-K // s)
        eligible = mode is not False and F_._long_decim_eligible(lout, K, s, p, p, L, d, 0, signal.dtype)
        # (unset: only where the plan of the construction above does not fit)
        dx_decim = eligible and (mode or not _fits_plain((B, cog * g, cin, g, lout, K, p, p, L, 0, 0, 0, 1, d, s)))
        dw_decim = eligible and L + kp - 1 <= F_.LONG_MAX_POINTS and (
            mode or not _fits_plain((cog, g * B, cin, g, lout, L, p, max(0, p - op), K, 0, 0, 0, 1, s, d)))
        if ctx.needs_input_grad[0] and dx_decim:
            dx = F_._long_run(grad, kernel.detach().contiguous(), None, p, p, False, L, g, channels_last=x_nlc, decim=s)
        elif ctx.needs_input_grad[0]:
            dx = F_._long_run(grad, kernel.detach().contiguous(), None, p, p, False, L, g, tap_dil=d, out_step=s,
                              conj_kernel=cx, channels_last=x_nlc)
        if ctx.needs_input_grad[1] and dw_decim:
            dw = _long_dw_by_phases(grad, signal.detach(), g, p, s, K).to(kernel.dtype)
        elif ctx.needs_input_grad[1]:
            # (the row must reach lag K - 1 of the last signal sample: max(0, p - op) zeros behind it)
            dw = _long_dw_exchanged(grad, signal.detach(), g, p, max(0, p - op), K, tap_dil=s, out_step=d,
                                    conj_kernel=cx).contiguous().to(kernel.dtype)
        if has_bias and ctx.needs_input_grad[2]:
            db = _long_grad_bias(grad, kernel.dtype)
        return (dx, dw, db) + (None,) * 8
