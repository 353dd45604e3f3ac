"""``fft_conv`` for MI355X: same call signature as the reference, HIP kernels underneath.

Mirrors /root/reference/fft_conv_pytorch/functional.py (fft_conv :19-89,
complex_matmul :11-16, to_ntuple re-export :8).  The Python layer only
normalises arguments, checks shapes, allocates the output and hands raw device
pointers + the current HIP stream to libfftconv_amd.so.  There is no CPU path
and no torch.fft / rocFFT / hipFFT call anywhere in this package.
"""
from __future__ import annotations

import collections
import os
from typing import Iterable, Optional, Union

import torch
from torch import Tensor

from . import _native
from .utils import to_ntuple

__all__ = ["fft_conv", "fft_long_conv", "fft_long_conv_gated", "fft_long_conv_transpose", "fft_conv_transpose", "complex_matmul", "to_ntuple", "transform_kernel", "KernelSpectrum", "FFTLongConvStream"]


_DTYPE_CODES = {torch.float32: 0, torch.float64: 1, torch.float16: 2, torch.bfloat16: 3, torch.complex64: 4}      # enum fc_dtype
_CONV_DTYPES = (torch.float32, torch.float64, torch.float16, torch.bfloat16)      # of fft_conv / fft_conv_transpose plans
_CONV_ND_DTYPES = _CONV_DTYPES + (torch.complex64,)                               # ... of their 2-D and 3-D plans


def _require_gpu(name: str, t: Tensor, dtype: torch.dtype, gate: tuple):
    """Device + dtype gate of everything handed to the library: ``t`` on a ROCm device and of ``dtype`` (the signal's).
    ``gate``: (the dtypes the op takes, what its TypeError says it takes) -- _CONV_GATE or _LONG_GATE."""
    allowed, takes = gate
    if not t.is_cuda:
        raise RuntimeError(
            f"fft_conv_pytorch_amd: `{name}` is on {t.device}; this implementation runs on ROCm devices only "
            f"(no CPU fallback). Move the tensor to 'cuda'.")
    if t.dtype != dtype or dtype not in allowed:
        raise TypeError(f"fft_conv_pytorch_amd: `{name}` has dtype {t.dtype}; {takes}")


_CONV_GATE = (_CONV_ND_DTYPES,
              "signal, kernel and bias must share one of "
              "float32 (the FFT kernels), float64 (double-precision FFT kernels; a direct float64 kernel below "
              "their crossover), float16 / bfloat16 (read and written as 16-bit by the float32 FFT "
              "kernels, which widen the signal as they load it and round the output once as they store it) or, "
              "for 4-D and 5-D tensors, complex64 (1-D complex rows: fft_long_conv; complex128, complex32 and "
              "mixes of real and complex tensors are not taken: convert with .to(torch.complex64))")


class KernelSpectrum:
    """A weight tensor transformed for one plan (rows a2 + a6); reusable while the weight is unchanged.

    Read-only once built: the scratch area of the N-d passes is NOT part of it -- every forward call takes
    its own workspace from torch's (stream-ordered) allocator, so one spectrum can serve several streams."""

    __slots__ = ("plan", "buf")

    def __init__(self, plan, buf):
        self.plan, self.buf = plan, buf


def _same_device(**tensors) -> torch.device:
    """All tensors of one call must live on one device (else the kernels would be handed foreign pointers)."""
    dev = None
    for name, t in tensors.items():
        if t is None:
            continue
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"fft_conv_pytorch_amd: `{name}` is on {t.device} but the signal is on {dev}; "
                             f"all tensors of one call must be on the same device")
    return dev


def _device_index(dev: torch.device) -> int:
    return dev.index if dev.index is not None else torch.cuda.current_device()


def new_workspace(plan, device) -> Optional[Tensor]:
    """Scratch area of one forward / transform call of an N-d plan (None for 1-D plans)."""
    if not plan.workspace_bytes:
        return None
    return torch.empty(plan.workspace_bytes // 4, dtype=torch.float32, device=device)


def _scratch_and_stream(plan, device):
    """What every launch on ``plan`` takes last: (the workspace tensor, to be held until the launch is queued; its pointer
    or None; the handle of the current stream of ``device``)."""
    ws = new_workspace(plan, device)
    return ws, ws.data_ptr() if ws is not None else None, torch.cuda.current_stream(device).cuda_stream


def _cached_plan(index: int, key: tuple):
    """The cached plan of (device, key); on a miss it is created with that device current: the library allocates twiddle
    tables and work lists on the CURRENT HIP device and sizes the work list for its CU count."""
    plan = _native.lookup_plan(index, key)
    if plan is None:
        with torch.cuda.device(index):
            plan = _native.get_plan(index, key)
    return plan


def _plan_for(signal: Tensor, kernel: Tensor, bias, stride, padding, dilation, groups, padding_mode, tile_hint=None,
              transposed=False, output_padding=0):
    if tile_hint is None:   # debugging / tuning knob: force the FFT tile length
        tile_hint = int(os.environ.get("FFTCONV_TILE", "0"))
    n = signal.ndim - 2
    if n < 1 or n > 3:
        raise ValueError(f"fft_conv expects (batch, channels, *spatial) with 1-3 spatial dims, got shape {tuple(signal.shape)}")
    if kernel.ndim != signal.ndim:
        raise ValueError(f"kernel has {kernel.ndim} dims but signal has {signal.ndim}")
    padding_ = to_ntuple(padding, n=n)
    stride_ = to_ntuple(stride, n=n)
    dilation_ = to_ntuple(dilation, n=n)
    if padding_mode not in _native.PAD_MODES:
        raise ValueError(f"unknown padding_mode {padding_mode!r}; expected one of constant/zeros/reflect/replicate/circular")
    if not isinstance(groups, int) or groups < 1:
        raise ValueError(f"groups must be a positive int, got {groups!r}")
    output_padding_ = to_ntuple(output_padding, n=n)
    cin = int(signal.shape[1])
    if transposed:
        # kernel is (Cin, Cout/groups, *k) as in torch.nn.ConvTranspose{N}d (functional.py:109-114)
        cout = int(kernel.shape[1]) * groups
        if cin % groups or int(kernel.shape[0]) != cin:
            raise ValueError(
                f"channel mismatch: signal has {cin} channels, transposed kernel is {tuple(kernel.shape)} with "
                f"groups={groups} (need kernel.shape[0] == in_channels and in_channels % groups == 0)")
        if padding_mode not in ("constant", "zeros"):
            raise ValueError("fft_conv_transpose supports zero padding only")
    else:
        cout = int(kernel.shape[0])
        if cin % groups or cout % groups or int(kernel.shape[1]) * groups != cin:
            raise ValueError(
                f"channel mismatch: signal has {cin} channels, kernel is {tuple(kernel.shape)} with groups={groups} "
                f"(need kernel.shape[1] * groups == in_channels and out_channels % groups == 0)")
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f"bias must have shape ({cout},), got {tuple(bias.shape)}")
    # (complex64: 2-D and 3-D plans only; a 1-D complex signal fails the dtype gate below)
    dtype = signal.dtype if signal.dtype in (_CONV_DTYPES if n == 1 else _CONV_ND_DTYPES) else torch.float32
    key = (n, int(signal.shape[0]), cin, cout, groups,
           tuple(int(s) for s in signal.shape[2:]), tuple(int(k) for k in kernel.shape[2:]),
           tuple(int(s) for s in stride_), tuple(int(p) for p in padding_), tuple(int(d) for d in dilation_),
           _native.PAD_MODES[padding_mode], bias is not None, int(tile_hint), bool(transposed),
           tuple(int(o) for o in output_padding_), _DTYPE_CODES[dtype])
    # host-side validation is complete; only now touch the device library
    _require_gpu("signal", signal, dtype, _CONV_GATE)
    _require_gpu("kernel", kernel, dtype, _CONV_GATE)
    if bias is not None:
        _require_gpu("bias", bias, dtype, _CONV_GATE)
    dev = _same_device(signal=signal, kernel=kernel, bias=bias)
    index = _device_index(dev)
    if dtype in _LOW_PRECISION and (index,) + key in _REFUSED_HALF:      # (a refused key has no cached plan)
        raise NotImplementedError(_REFUSED_HALF[(index,) + key])
    try:
        return _cached_plan(index, key)
    except NotImplementedError as e:
        if dtype in _LOW_PRECISION:      # a route that reads y back: remembered, the caller takes the cast path
            _REFUSED_HALF[(index,) + key] = str(e)
            while len(_REFUSED_HALF) > 256:
                _REFUSED_HALF.popitem(last=False)
        raise


def transform_kernel(plan, kernel: Tensor) -> KernelSpectrum:
    """Kernel transform (dilate, zero-pad, FFT, conjugate) on the device; rows a2 + a6.  A float16 / bfloat16 plan takes
    a weight of its own dtype (widened to a float32 copy that lives for this call only) or a float32 one.  A long-filter
    plan reads a float16 / bfloat16 weight where it lies (no copy); its spectrum is float32, the bytes of the widened
    weight's.  A complex long plan takes a complex64 weight (a lazy conjugate is resolved first)."""
    io = ()
    if isinstance(plan, _native.LongPlan) and plan.complex:
        if kernel.dtype != torch.complex64:
            raise TypeError(f"kernel is {kernel.dtype} but the plan is a complex64 long plan")
        _require_gpu("kernel", kernel, kernel.dtype, _LONG_GATE)
        kernel = _resolved(kernel.detach()).contiguous()
        io = (_DTYPE_CODES[kernel.dtype],)
    elif isinstance(plan, _native.LongPlan) and kernel.dtype in _LOW_PRECISION:
        _require_gpu("kernel", kernel, kernel.dtype, _CONV_GATE)
        kernel = kernel.detach().contiguous()
        io = (_DTYPE_CODES[kernel.dtype],)
    else:
        _require_gpu("kernel", kernel, plan.weight_dtype if kernel.dtype == plan.weight_dtype else plan.dtype, _CONV_GATE)
        # (a complex64 plan: the library reads data_ptr(), a lazy conjugate is resolved first)
        kernel = _resolved(kernel.detach()).to(plan.weight_dtype).contiguous()
    if _device_index(kernel.device) != plan.device_index:
        raise ValueError(f"kernel is on {kernel.device} but the plan was made for cuda:{plan.device_index}")
    with torch.cuda.device(kernel.device):
        buf = torch.empty(max(plan.spectrum_bytes, 16) // 4, dtype=torch.float32, device=kernel.device)
        ws, ws_ptr, stream = _scratch_and_stream(plan, kernel.device)      # scratch of this call only
        plan.transform_kernel(kernel.data_ptr(), buf.data_ptr(), ws_ptr, stream, *io)
    return KernelSpectrum(plan, buf)


def _nd_layout(t: Tensor) -> str:
    """How the 2-D / 3-D kernels take a (B, C, *spatial) tensor (pure: sizes and strides only, any device):
    ``"planar"`` contiguous -- read where it lies, as ever (a tensor with one channel lies both ways and counts here);
    ``"cl"``     4-D and ``torch.channels_last`` / 5-D and ``torch.channels_last_3d`` contiguous, at any storage offset:
                 a contiguous (B, *spatial, C) tensor seen through ``permute`` -- read where it lies by the channels-last
                 build of the first pass;
    ``"copy"``   anything else (a channel slice, an expanded or spatially strided view, a 3-D tensor that is not
                 contiguous): ``.contiguous()`` first."""
    if t.is_contiguous():
        return "planar"
    if (t.ndim == 4 and t.is_contiguous(memory_format=torch.channels_last)) or (
            t.ndim == 5 and t.is_contiguous(memory_format=torch.channels_last_3d)):
        return "cl"
    return "copy"


def _nd_cl_native(channels_last: bool) -> bool:
    """Whether a 2-D / 3-D call has the kernels take channels-last tensors where they lie (FFTCONV_ND_CL, read per call):
    unset -- a call that asks for a channels-last result (``channels_last=True``) does, for its signal, its result and in
    its backward; a call that does not is the call it always was, copies included (measured: the training step of such a
    call lost to the copy, whose contiguous dY the weight gradient needs anyway -- DESIGN.md 4.3g);
    ``1`` -- every call does, whatever its keyword; ``0`` -- none does."""
    knob = os.environ.get("FFTCONV_ND_CL", "")
    return knob != "0" and (bool(channels_last) or knob == "1")


def _empty_channels_last(shape, dtype, device) -> Tensor:
    """An uninitialised (B, C, *spatial) tensor that lies as a contiguous (B, *spatial, C)."""
    n = len(shape) - 2
    return torch.empty((shape[0],) + tuple(shape[2:]) + (shape[1],), dtype=dtype, device=device).permute(
        (0, n + 1) + tuple(range(1, n + 1)))


def _to_channels_last(t: Tensor) -> Tensor:
    """The values of a (B, C, *spatial) tensor with the strides of ``_empty_channels_last``: one torch copy."""
    out = _empty_channels_last(tuple(t.shape), t.dtype, t.device)
    out.copy_(t)
    return out


def _check_channels_last(channels_last, signal: Tensor):
    """The ``channels_last`` keyword of ``fft_conv`` / ``fft_conv_transpose`` (ValueError, before any device call)."""
    if not isinstance(channels_last, bool):
        raise ValueError(f"channels_last must be a bool, got {channels_last!r}")
    if channels_last and signal.ndim == 3:
        raise ValueError("channels_last=True goes with 4-D and 5-D tensors; a (batch, channels, length) signal has no "
                         "channels-last result here: fft_long_conv(..., channels_last=True) returns one")


def _launch_forward(signal: Tensor, spectrum: KernelSpectrum, bias_c: Optional[Tensor], x_cl: bool = False,
                    y_cl: bool = False) -> Tensor:
    plan = spectrum.plan
    shape = (signal.shape[0], plan.key[3]) + plan.out_spatial
    if y_cl:
        out = _empty_channels_last(shape, plan.dtype, signal.device)
    else:
        out = torch.empty(shape, dtype=plan.dtype, device=signal.device)
    ws, ws_ptr, stream = _scratch_and_stream(plan, signal.device)
    args = (signal.data_ptr(), spectrum.buf.data_ptr(), bias_c.data_ptr() if bias_c is not None else None,
            out.data_ptr(), ws_ptr, stream)
    if x_cl or y_cl:
        plan.forward_lay(*args, _native.ND_CHANNELS_LAST if x_cl else _native.ND_PLANAR,
                         _native.ND_CHANNELS_LAST if y_cl else _native.ND_PLANAR)
    else:
        plan.forward(*args)
    return out


def _forward_native(signal: Tensor, spectrum: KernelSpectrum, bias: Optional[Tensor], channels_last: bool = False,
                    native: bool = False) -> Tensor:
    """One forward launch of ``spectrum.plan``.  ``channels_last=True`` returns the result lying channels-last.  Where the
    call takes layouts natively (``_nd_cl_native``; ``native``: the caller has decided so, a backward of such a call) a
    signal that lies channels-last (``_nd_layout`` "cl") is read where it lies and the last pass writes the channels-last
    result, if the plan takes the layout (``Plan.takes_layout``); otherwise one torch copy each keeps values and strides."""
    signal = _resolved(signal.detach())
    # (``native`` comes from ``_nd_cl_native`` too, in the backward that passes it: FFTCONV_ND_CL=0 is honoured there)
    nd_cl = signal.ndim >= 4 and (native or _nd_cl_native(channels_last))
    x_cl = (nd_cl and _nd_layout(signal) == "cl"
            and spectrum.plan.takes_layout(_native.ND_CHANNELS_LAST, _native.ND_PLANAR) is None)
    y_cl = (channels_last and nd_cl
            and spectrum.plan.takes_layout(_native.ND_PLANAR, _native.ND_CHANNELS_LAST) is None)
    if not x_cl:
        signal = signal.contiguous()
    # (a float16 / bfloat16 plan reads a float32 bias: Cout values; a complex64 plan Cout (re, im) pairs)
    bias_c = _resolved(bias.detach()).to(spectrum.plan.weight_dtype).contiguous() if bias is not None else None
    index = _device_index(signal.device)
    if signal.dtype != spectrum.plan.dtype:
        raise TypeError(f"signal is {signal.dtype} but the plan was made for {spectrum.plan.dtype}")
    if spectrum.plan.device_index != index or spectrum.buf.device != signal.device:
        raise ValueError(f"signal is on {signal.device} but the kernel spectrum / plan belong to "
                         f"cuda:{spectrum.plan.device_index}")
    if torch.cuda.current_device() == index:      # the common case: no device switch to pay for
        out = _launch_forward(signal, spectrum, bias_c, x_cl, y_cl)
    else:
        with torch.cuda.device(signal.device):
            out = _launch_forward(signal, spectrum, bias_c, x_cl, y_cl)
    return _to_channels_last(out) if channels_last and not y_cl else out


def _forward_lay(signal: Tensor, spectrum: KernelSpectrum, bias: Optional[Tensor], channels_last: bool,
                 native: bool = False) -> Tensor:
    """``_forward_native``; a call that asks for no channels-last result is the three-argument call it always was."""
    if channels_last or native:
        return _forward_native(signal, spectrum, bias, channels_last, native)
    return _forward_native(signal, spectrum, bias)


def fft_conv(
    signal: Tensor,
    kernel: Tensor,
    bias: Tensor = None,
    stride: Union[int, Iterable[int]] = 1,
    padding: Union[int, Iterable[int]] = 0,
    dilation: Union[int, Iterable[int]] = 1,
    groups: int = 1,
    padding_mode: str = "constant",
    *,
    channels_last: bool = False,
) -> Tensor:
    """N-d (1/2/3) cross-correlation through FFTs, equal to ``torch.nn.functional.conv{N}d``.

    Args and result as in the reference (functional.py:19-42): ``signal`` is
    (B, Cin, *spatial), ``kernel`` is (Cout, Cin/groups, *k), ``bias`` is (Cout,)
    or None; ``stride``/``padding``/``dilation`` are ints or per-axis iterables;
    ``padding_mode`` is one of constant | reflect | replicate | circular.
    The result is a fresh contiguous (B, Cout, *out) float32 tensor on the
    input's device.  Unlike the reference, a kernel larger than the padded
    input raises ``ValueError`` (torch's behaviour) instead of returning a
    wrongly shaped tensor.

    4-D and 5-D complex64 ``signal``, ``kernel`` and ``bias`` (all three) run a complex plan: plain bilinear product,
    nothing conjugated (``torch.nn.functional.conv2d`` / ``conv3d`` on complex tensors), every argument with its meaning,
    a complex64 result, gradients in PyTorch's convention for complex tensors; lazy conjugates and negations are resolved
    on entry.  complex128, complex32, mixes of real and complex tensors and 3-D (one spatial axis) complex tensors raise
    ``TypeError`` (complex rows: ``fft_long_conv``); a kernel that would run in segments of taps (a dilated extent past 4096
    on an axis) raises ``NotImplementedError``.

    Channels-last tensors (4-D and 5-D).  ``channels_last=True`` (keyword-only) returns the (B, Cout, *out) result with
    the strides of a contiguous (B, *out, Cout) tensor, written that way by the last pass; such a call also reads a
    ``signal`` that lies as ``torch.channels_last`` / ``channels_last_3d`` (``_nd_layout`` "cl") where it lies, and its
    backward reads a channels-last dY where it lies and returns dX in the signal's layout.  Every value has the bits of
    the call on contiguous copies.  Where the library does not take the layout (float64, complex64, the plane-major 3-D
    pipeline, segments of taps, 2048- / 4096-point row transforms, tensors past its 32-bit guards, FFTCONV_ND_CL=0) one
    torch copy per tensor keeps values and strides.  A call without the keyword is the call it always was (a strided
    signal is copied); FFTCONV_ND_CL=1 has every call read a channels-last signal and dY where they lie.  A non-bool
    raises ``ValueError``, and so does ``True`` with a 3-D signal (``fft_long_conv`` has the keyword for rows).
    """
    _check_channels_last(channels_last, signal)
    return _fft_conv_impl(signal, kernel, bias, stride, padding, dilation, groups, padding_mode, None,
                          channels_last=channels_last)


_LOW_PRECISION = (torch.float16, torch.bfloat16)
# (device, plan key) of float16 / bfloat16 descriptors whose route the library refuses (it would round y between
# launches) -> its message: such calls take the cast path without asking the library again
_REFUSED_HALF: "collections.OrderedDict[tuple, str]" = collections.OrderedDict()


def _half_native(signal: Tensor, kernel: Tensor, bias) -> bool:
    """A float16 / bfloat16 call the kernels read and write in its own dtype: the three tensors agree and FFTCONV_HALF_IO
    is not 0.  A call that needs gradients then runs the autograd function on the 16-bit tensors (autograd.py)."""
    return (signal.dtype in _LOW_PRECISION and kernel.dtype == signal.dtype
            and (bias is None or bias.dtype == signal.dtype)
            and os.environ.get("FFTCONV_HALF_IO", "1") != "0")


def _string_padding(padding: str, kernel: Tensor, stride, dilation, n: int):
    """``padding='valid' | 'same'`` as in torch.nn.functional.conv{N}d (the reference rejects strings: a str is
    Iterable for its to_ntuple).  Returns (symmetric padding per axis, leading output samples to
    drop per axis): 'same' needs d*(k-1) padded samples per axis, split floor/ceil like torch; an odd total is
    run with the larger half on both sides and the surplus leading output sample dropped."""
    if padding == "valid":
        return (0,) * n, (0,) * n
    if padding != "same":
        raise ValueError(f"invalid padding string {padding!r}; expected 'same' or 'valid'")
    if any(s != 1 for s in to_ntuple(stride, n)):
        raise ValueError("padding='same' is not supported for strided convolutions")
    total = [d * (int(k) - 1) for d, k in zip(to_ntuple(dilation, n), kernel.shape[2:])]
    return tuple(t - t // 2 for t in total), tuple(t % 2 for t in total)


def _needs_grad(*tensors) -> bool:
    return torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors)


def _conv_impl(transposed: bool, signal, kernel, bias, stride, padding, output_padding, dilation, groups, padding_mode,
               spectrum, plan, channels_last: bool = False, native: bool = False):
    """The body of ``_fft_conv_impl`` and ``_fft_conv_transpose_impl`` (``native``: see ``_forward_native``)."""
    if isinstance(padding, str) and signal.ndim >= 3 and not transposed:
        n = signal.ndim - 2
        pads, drop = _string_padding(padding, kernel, stride, dilation, n)
        out = _fft_conv_impl(signal, kernel, bias, stride, pads, dilation, groups, padding_mode, spectrum, plan,
                             channels_last=channels_last, native=native)
        if any(drop):
            # (a fresh contiguous tensor, as documented and as torch's convolutions return: a view would pin the
            # larger buffer and break downstream .view() calls; channels_last: a fresh tensor that lies that way)
            out = out[(slice(None), slice(None)) + tuple(slice(d, None) for d in drop)]
            out = _to_channels_last(out) if channels_last else out.contiguous()
        return out
    if signal.is_complex():
        # (the library reads data_ptr(): a conj or neg bit is resolved here, inside the autograd graph)
        signal, kernel, bias = _resolved(signal), _resolved(kernel), None if bias is None else _resolved(bias)
    conf = (stride, padding, dilation, groups, padding_mode, None, transposed, output_padding)      # of _plan_for
    # float16 / bfloat16: the kernels read x and write y in the tensors' dtype (float32 arithmetic, the bits of the cast
    # path below) -- unless the library refuses the route (it reads y back between launches): then the cast path
    native16 = _half_native(signal, kernel, bias)
    if native16 and plan is None:
        try:
            plan = _plan_for(signal, kernel, bias, *conf)
        except NotImplementedError:
            native16 = False
    if (not native16 and signal.dtype in _LOW_PRECISION and kernel.dtype == signal.dtype
            and (bias is None or bias.dtype == signal.dtype)):
        # half-precision tensors in, half-precision tensor out; the arithmetic is the fp32 path (one cast pass each way)
        out = _conv_impl(transposed, signal.float(), kernel.float(), None if bias is None else bias.float(), stride, padding,
                         output_padding, dilation, groups, padding_mode, None, None, channels_last, native)
        return out.to(signal.dtype)      # (.float() and .to() keep the strides of a channels-last tensor)
    if _needs_grad(signal, kernel, bias):
        # backward built from the same kernels (row N1; transposed: differentiable like the reference's op graph); native
        # 16-bit tensors are saved for backward, whose kernels read 16-bit dY and x (autograd.py)
        from . import autograd
        n = signal.ndim - 2
        if transposed:
            return autograd.FFTConvTransposeFunction.apply(signal, kernel, bias, to_ntuple(stride, n), to_ntuple(padding, n),
                                                           to_ntuple(output_padding, n), to_ntuple(dilation, n), groups,
                                                           spectrum, channels_last)
        return autograd.FFTConvFunction.apply(signal, kernel, bias, to_ntuple(stride, n), to_ntuple(padding, n),
                                              to_ntuple(dilation, n), groups, padding_mode, spectrum, channels_last)
    if plan is None:
        plan = _plan_for(signal, kernel, bias, *conf)
    if spectrum is None or spectrum.plan is not plan:
        spectrum = transform_kernel(plan, kernel)   # the reference also re-transforms per call (functional.py:71)
    return _forward_lay(signal, spectrum, bias, channels_last, native)


def _fft_conv_impl(signal, kernel, bias, stride, padding, dilation, groups, padding_mode, spectrum, plan=None, *,
                   channels_last: bool = False, native: bool = False):
    """Shared by the functional and the modules; ``spectrum`` is an optional cached kernel transform and
    ``plan`` the plan the caller already looked up (and validated) for exactly these arguments."""
    return _conv_impl(False, signal, kernel, bias, stride, padding, 0, dilation, groups, padding_mode, spectrum, plan,
                      channels_last, native)


def fft_conv_transpose(
    signal: Tensor,
    kernel: Tensor,
    bias: Tensor = None,
    stride: Union[int, Iterable[int]] = 1,
    padding: Union[int, Iterable[int]] = 0,
    output_padding: Union[int, Iterable[int]] = 0,
    dilation: Union[int, Iterable[int]] = 1,
    groups: int = 1,
    *,
    channels_last: bool = False,
) -> Tensor:
    """N-d transposed convolution through FFTs, equal to ``torch.nn.functional.conv_transpose{N}d``
    (reference: functional.py:92-176).

    ``kernel`` is (Cin, Cout/groups, *k).  The same HIP kernels as ``fft_conv`` run it: the stride
    becomes a zero-spread of the input folded into the load index map, the kernel flip and the
    in/out channel swap are folded into the kernel transform, padding / output_padding only move
    the window of kept samples -- no intermediate tensor is materialised.  4-D and 5-D complex64 tensors (all three)
    are taken as ``fft_conv`` takes them, and so are channels-last tensors (``channels_last``, keyword-only: see there).
    """
    _check_channels_last(channels_last, signal)
    return _fft_conv_transpose_impl(signal, kernel, bias, stride, padding, output_padding, dilation, groups, None,
                                    channels_last=channels_last)


def _fft_conv_transpose_impl(signal, kernel, bias, stride, padding, output_padding, dilation, groups, spectrum,
                             plan=None, *, channels_last: bool = False):
    """Shared by the functional and the transposed modules (``spectrum`` / ``plan``: see ``_fft_conv_impl``)."""
    return _conv_impl(True, signal, kernel, bias, stride, padding, output_padding, dilation, groups, "constant", spectrum,
                      plan, channels_last)


def complex_matmul(a: Tensor, b: Tensor, groups: int = 1) -> Tensor:
    """Grouped per-bin channel contraction ``einsum('bgi...,goi...->bgo...')`` (functional.py:11-16).

    In this implementation the contraction is fused into the convolution kernels
    (the "mix" step), so ``fft_conv`` never calls this function; it is kept for
    API compatibility and evaluates the same contraction on the tensors' device.
    """
    a_g = a.unflatten(1, [groups, a.size(1) // groups])
    b_g = b.unflatten(0, [groups, b.size(0) // groups])
    return torch.einsum("bgi...,goi...->bgo...", a_g, b_g).flatten(1, 2)


# ---------------------------------------------------------------------------------------------- long filters
LONG_HANDOFF_POINTS = 4096        # a padded row this short is one tile of the fft_conv path
LONG_MAX_POINTS = 1 << 24         # longest transform of the long-filter path (4096 x 4096)


def _long_plan(signal: Tensor, cout: int, groups: int, taps: int, pad_left: int, pad_right: int, flip: bool,
               out_keep: int, has_bias: bool, *, pad_mode: int = 0, src_up: int = 1, tap_dil: int = 1, out_step: int = 1,
               conj_signal: bool = False, conj_kernel: bool = False):
    """Cached long-filter plan (``fc_long_plan``) for a signal (B, Cin, L) against ``taps`` taps per filter row.  The four
    keywords are the words of ``fc_long_ext``; a plan that leaves them at their defaults keeps the 12-field key.  A
    complex64 signal gets a complex plan (one batch item per row of the transform), whose key always has 17 fields: the
    extension and the ``fc_long_kind`` bits, with ``conj_signal`` / ``conj_kernel`` (the plan reads that operand conjugated)."""
    key = ("long", int(signal.shape[0]), int(signal.shape[1]), int(cout), int(groups), int(signal.shape[2]), int(taps),
           int(pad_left), int(pad_right), int(out_keep), int(bool(flip)), int(bool(has_bias)))
    ext = (int(pad_mode), int(src_up), int(tap_dil), int(out_step))
    if signal.dtype == torch.complex64:
        key += ext + (_native.LONG_COMPLEX | (_native.LONG_CONJ_SIGNAL if conj_signal else 0)
                      | (_native.LONG_CONJ_TAPS if conj_kernel else 0),)
    elif conj_signal or conj_kernel:
        raise ValueError("conjugated reads go with complex64 tensors only")
    elif ext != _native.LONG_EXT_DEFAULT:
        key += ext
    return _cached_plan(_device_index(signal.device), key)


def _long_decim_plan(signal: Tensor, cout: int, groups: int, taps: int, stride: int, pad_left: int, pad_right: int,
                     out_keep: int, flip: bool, has_bias: bool):
    """Cached decimation plan (``fc_long_decim_plan_create``) of a (B, Cin, L) signal: the strided primitive of dilation 1
    on the ``stride`` decimated rows.  Its cache key carries a tag of its own."""
    key = ("long_decim", int(signal.shape[0]), int(signal.shape[1]), int(cout), int(groups), int(signal.shape[2]), int(taps),
           int(stride), int(pad_left), int(pad_right), int(out_keep), int(bool(flip)), int(bool(has_bias)))
    return _cached_plan(_device_index(signal.device), key)


def _long_blocks_plan(signal: Tensor, cout: int, groups: int, taps: int, pad_left: int, pad_right: int, flip: bool,
                      out_keep: int, has_bias: bool, block_points: int):
    """Cached blocks plan (``fc_long_blocks_plan_create``) of a (B, Cin, L) signal: the plain real primitive in overlap-save
    blocks of ``block_points`` points (0: the planner's choice).  Its cache key carries a tag of its own."""
    key = ("long_blocks", int(signal.shape[0]), int(signal.shape[1]), int(cout), int(groups), int(signal.shape[2]), int(taps),
           int(pad_left), int(pad_right), int(out_keep), int(bool(flip)), int(bool(has_bias)), int(block_points))
    return _cached_plan(_device_index(signal.device), key)


def _resolved(t: Tensor) -> Tensor:
    """A complex tensor with its lazy conjugate / negation materialised: the library reads ``data_ptr()``, which knows of
    neither bit.  Real tensors pass through."""
    return t.resolve_conj().resolve_neg() if t.is_complex() else t


def _long_layout(t: Tensor) -> str:
    """How the long-path kernels take a (B, C, L) tensor (pure: strides and sizes only, any device):
    ``"ncl"``  contiguous -- read where it lies, as ever;
    ``"nlc"``  strides exactly (L*C, 1, C) and not contiguous: ``u.transpose(1, 2)`` of a contiguous (B, L, C) tensor, at
               any storage offset -- read where it lies by the channels-last builds of the column kernels;
    ``"copy"`` anything else (a slice, an expanded or time-strided view): ``.contiguous()`` first."""
    if t.is_contiguous():
        return "ncl"
    if t.ndim == 3 and tuple(t.stride()) == (t.shape[2] * t.shape[1], 1, t.shape[1]):
        return "nlc"
    return "copy"


def _long_nlc_enabled() -> bool:
    """FFTCONV_LONG_NLC=0 (read per call): every strided tensor is copied and a channels-last result is one torch copy."""
    return os.environ.get("FFTCONV_LONG_NLC", "1") != "0"


def _long_reads_nlc(t: Tensor) -> bool:
    """Whether the long-path kernels read this (B, C, L) tensor channels-last where it lies: FFTCONV_LONG_NLC is not 0, it
    lies that way (``_long_layout`` "nlc") and one batch item's (L, C) block stays below LONG_NLC_MAX_BYTES.  Otherwise
    the caller takes ``.contiguous()``."""
    return (_long_layout(t) == "nlc" and _long_nlc_enabled()
            and t.shape[1] * t.shape[2] * t.element_size() < _native.LONG_NLC_MAX_BYTES)


def _as_channels_last(t: Tensor) -> Tensor:
    """(B, C, L) values with strides (L*C, 1, C): one torch copy, none if ``t`` already lies so."""
    return t.transpose(1, 2).contiguous().transpose(1, 2)


def _long_run(signal: Tensor, kernel: Tensor, bias: Optional[Tensor], pad_left: int, pad_right: int, flip: bool,
              out_keep: int, groups: int, spectrum: Optional[KernelSpectrum] = None,
              out_dtype: Optional[torch.dtype] = None, *, pad_mode: int = 0, src_up: int = 1, tap_dil: int = 1,
              out_step: int = 1, conj_signal: bool = False, conj_kernel: bool = False,
              channels_last: bool = False, weight_shape: Optional[tuple] = None, decim: int = 0, plan=None) -> Tensor:
    """The primitive every role of the long-filter path runs (include/fftconv_amd.h "Long filters"), no autograd:
    y[b, o, j] = bias[o] + sum_i sum_k u[o, i, k] * xrow[b, (g, i), out_step*j + tap_dil*k] for j < out_keep (0: all),
    u = the taps in tensor order or flipped, xrow = the signal padded in ``pad_mode`` (a PadMode code), or spread over a
    grid of ``src_up`` between zero paddings.

    ``signal`` and ``kernel`` are float32, float16 or bfloat16, each on its own: the kernels read them where they lie and
    widen as they load.  The result has ``out_dtype`` (default: the signal's; the weight gradient asks for float32 from
    16-bit operands) and is rounded once, at the store.  The plan, its cache key, the spectrum and the workspace are the
    float32 ones whatever the dtypes; the bias (Cout values) is widened to float32.

    complex64 ``signal``, ``kernel`` and ``bias`` (all three) run a complex plan: plain bilinear product, complex64 result,
    the bias read as Cout (re, im) pairs.  ``conj_signal`` / ``conj_kernel`` make that plan read conj(signal) / conj(kernel)
    (a sign flip as the kernels load; the gradients use it).  Lazy conjugates are resolved here.

    A signal that lies as a contiguous (B, L, C) tensor (``_long_layout`` "nlc") is read where it lies, and
    ``channels_last=True`` has the kernels write the result with strides (nout*Cout, 1, Cout); the two are independent.
    Either falls back to a torch copy under FFTCONV_LONG_NLC=0 and where one batch item's block reaches 2**31 bytes.

    ``weight_shape`` = (Cout, taps) lets a caller that holds this plan's ``spectrum`` pass ``kernel=None``.

    ``decim`` = s >= 2 runs the primitive with out_step = s on a decimation plan (``_long_decim_plan``: real tensors, zero
    padding, dilation 1): the s decimated rows of every input channel against the s phases of the taps, a transform of
    about nout + ceil(taps / s) points.  The signal is read contiguous; a channels-last result is written as ever.

    ``plan``: the plan of these arguments where the caller holds it already (``_long_forward_plan``,
    ``_long_transpose_plan``); a phases plan runs here too, on a contiguous signal."""
    signal = _resolved(signal.detach())
    cout, taps = (int(kernel.shape[0]), int(kernel.shape[2])) if weight_shape is None else weight_shape
    x_nlc = not decim and _long_reads_nlc(signal)
    if not x_nlc:
        signal = signal.contiguous()
    cx = signal.dtype == torch.complex64
    out_dtype = signal.dtype if out_dtype is None or cx else out_dtype
    if plan is None and decim:
        assert (pad_mode, src_up, tap_dil, out_step) == (0, 1, 1, 1) and not cx, "a decimation plan: zero padding, dilation 1, real rows"
        plan = _long_decim_plan(signal, cout, groups, taps, decim, pad_left, pad_right, out_keep, flip, bias is not None)
    elif plan is None:
        plan = _long_plan(signal, cout, groups, taps, pad_left, pad_right, flip, out_keep,
                          bias is not None, pad_mode=pad_mode, src_up=src_up, tap_dil=tap_dil, out_step=out_step,
                          conj_signal=conj_signal, conj_kernel=conj_kernel)
    if spectrum is None or spectrum.plan is not plan:
        spectrum = transform_kernel(plan, kernel)
    if bias is None:
        bias_c = None
    elif cx:
        bias_c = _resolved(bias.detach()).contiguous()
    else:
        bias_c = bias.detach().float().contiguous()
    batch, nout = int(signal.shape[0]), plan.out_len
    with torch.cuda.device(signal.device):
        y_nlc = bool(channels_last) and _long_nlc_enabled()
        if y_nlc:
            out = torch.empty((batch, nout, cout), dtype=out_dtype, device=signal.device)
            y_nlc = nout * cout * out.element_size() < _native.LONG_NLC_MAX_BYTES
            out = out.transpose(1, 2) if y_nlc else out.view(batch, cout, nout)
        else:
            out = torch.empty((batch, cout, nout), dtype=out_dtype, device=signal.device)
        ws, ws_ptr, stream = _scratch_and_stream(plan, signal.device)
        args = (signal.data_ptr(), spectrum.buf.data_ptr(), bias_c.data_ptr() if bias_c is not None else None,
                out.data_ptr(), ws_ptr, stream, _DTYPE_CODES[signal.dtype], _DTYPE_CODES[out_dtype])
        if x_nlc or y_nlc:
            plan.forward_lay(*args, _native.LONG_NLC if x_nlc else _native.LONG_NCL,
                             _native.LONG_NLC if y_nlc else _native.LONG_NCL)
        else:
            plan.forward(*args)
    return _as_channels_last(out) if channels_last and not y_nlc else out


def _long_int(name: str, value) -> int:
    """``stride`` / ``dilation`` of the 1-D long path: an int or a 1-tuple, at least 1."""
    if isinstance(value, (tuple, list)) and len(value) == 1:
        value = value[0]
    if isinstance(value, bool) or not isinstance(value, int) or value < 1:
        raise ValueError(f"{name} must be an int >= 1, got {value!r}")
    return int(value)


def _long_geometry(signal: Tensor, kernel: Tensor, bias, padding, groups, causal, stride=1, dilation=1,
                   padding_mode: str = "constant"):
    """Argument checks of ``fft_long_conv`` (ValueError, before any device call) -> (pad_left, pad_right, points the row
    needs)."""
    if signal.ndim != 3 or kernel.ndim != 3:
        raise ValueError(f"fft_long_conv expects a (batch, channels, length) signal and an (out, in/groups, taps) kernel, "
                         f"got shapes {tuple(signal.shape)} and {tuple(kernel.shape)}")
    if not isinstance(groups, int) or groups < 1:
        raise ValueError(f"groups must be a positive int, got {groups!r}")
    stride, dilation = _long_int("stride", stride), _long_int("dilation", dilation)
    if padding_mode not in _native.PAD_MODES:
        raise ValueError(f"unknown padding_mode {padding_mode!r}; expected one of constant/zeros/reflect/replicate/circular")
    mode = _native.PAD_MODES[padding_mode]
    cin, cout, taps, length = int(signal.shape[1]), int(kernel.shape[0]), int(kernel.shape[2]), int(signal.shape[2])
    if cin % groups or cout % groups or int(kernel.shape[1]) * groups != cin:
        raise ValueError(f"channel mismatch: signal has {cin} channels, kernel is {tuple(kernel.shape)} with groups={groups} "
                         f"(need kernel.shape[1] * groups == in_channels and out_channels % groups == 0)")
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f"bias must have shape ({cout},), got {tuple(bias.shape)}")
    if length < 1 or taps < 1 or signal.shape[0] < 1:
        raise ValueError("batch, length and taps must be positive")
    extent = dilation * (taps - 1) + 1
    if causal:
        if not (isinstance(padding, int) and padding == 0):
            raise ValueError(f"causal=True pads the row itself (taps - 1 zeros in front): padding must be 0, got {padding!r}")
        if mode != 0:
            raise ValueError(f"causal=True pads the row itself with zeros: padding_mode must be 'constant', got {padding_mode!r}")
        met = min(taps, (length - 1) // dilation + 1)      # taps at a lag of L or more never reach the output
        return extent - 1, 0, length + dilation * (met - 1)
    if isinstance(padding, str):
        if padding == "valid":
            pad_left = pad_right = 0
        elif padding == "same":
            if stride != 1:
                raise ValueError("padding='same' is not supported for strided convolutions")
            pad_left = (extent - 1) // 2
            pad_right = extent - 1 - pad_left
        else:
            raise ValueError(f"invalid padding string {padding!r}; expected 'same' or 'valid'")
    else:
        if isinstance(padding, (tuple, list)) and len(padding) == 1:
            padding = padding[0]
        if not isinstance(padding, int) or padding < 0:
            raise ValueError(f"padding must be a non-negative int, 'same' or 'valid', got {padding!r}")
        pad_left = pad_right = int(padding)
    if extent > length + pad_left + pad_right:
        at = "" if dilation == 1 else f", {extent} samples at dilation {dilation}"
        raise ValueError(f"kernel ({taps} taps{at}) is longer than the padded row ({length + pad_left + pad_right} samples)")
    if mode == 1 and max(pad_left, pad_right) >= length:
        raise ValueError(f"reflect padding ({max(pad_left, pad_right)}) must be smaller than the input size ({length})")
    if mode == 3 and max(pad_left, pad_right) > length:
        raise ValueError(f"circular padding ({max(pad_left, pad_right)}) must not exceed the input size ({length})")
    return pad_left, pad_right, length + pad_left + pad_right


LONG_DECIM_MAX_STRIDE = 64        # (stride x transform points stays below 2**30 up to the 2**24-point limit)
LONG_DECIM_MAX_LEN = 1 << 29      # a row of the signal lies behind one buffer resource (include/fftconv_amd.h)


def _long_decim_mode() -> Optional[bool]:
    """FFTCONV_LONG_DECIM (read per call): ``False`` for "0" (never), ``True`` for "1" (wherever eligible), ``None`` when
    unset or anything else: only where the construction the call takes otherwise does not fit 2**24 points."""
    return {"0": False, "1": True}.get(os.environ.get("FFTCONV_LONG_DECIM", ""))


def _long_decim_points(length: int, taps: int, stride: int, pad_left: int, pad_right: int, out_keep: int = 0) -> int:
    """Points a decimated row needs: the kept outputs and the ceil(taps / stride) - 1 positions behind the last."""
    nout = out_keep or (length + pad_left + pad_right - taps) // stride + 1
    return nout + -(-taps // stride) - 1


def _long_decim_eligible(length: int, taps: int, stride: int, pad_left: int, pad_right: int, out_keep: int, dilation: int = 1,
                         pad_mode: int = 0, dtype=torch.float32, x_layout: str = "ncl") -> bool:
    """Whether a decimation plan takes the strided primitive (pure): stride 2 ... 64, dilation 1, zero padding, float32 /
    float16 / bfloat16, a signal that is not read as channels-last, L < 2**29, decimated points <= 2**24."""
    return (2 <= stride <= LONG_DECIM_MAX_STRIDE and dilation == 1 and pad_mode == 0
            and dtype in (torch.float32,) + _LOW_PRECISION and x_layout != "nlc" and length < LONG_DECIM_MAX_LEN
            and _long_decim_points(length, taps, stride, pad_left, pad_right, out_keep) <= LONG_MAX_POINTS)


def _long_route_of(length: int, taps: int, pad_left: int, pad_right: int, need: int, causal: bool, stride: int, dilation: int,
                   pad_mode: int, dtype, x_layout: str) -> str:
    """``_long_route`` from the numbers ``_long_geometry`` returns."""
    if need <= LONG_HANDOFF_POINTS and dtype != torch.complex64:
        return "handoff"
    mode = _long_decim_mode()
    if (mode is True or (mode is None and need > LONG_MAX_POINTS)) and _long_decim_eligible(
            length, taps, stride, pad_left, pad_right, _long_keep(length, causal, stride), dilation, pad_mode, dtype, x_layout):
        return "phases"
    if need > LONG_MAX_POINTS:
        raise NotImplementedError(f"fft_long_conv: the row needs a transform of {need} points; the long-filter path stops at "
                                  f"2**24 = {LONG_MAX_POINTS} (blocks=True runs a stride-1, zero-padded row past it in "
                                  f"overlap-save blocks)")
    return "plain"


def _long_blocks_arg(blocks):
    """The ``blocks`` keyword of ``fft_long_conv`` checked (ValueError, before any device call) -> False, True or the int."""
    if isinstance(blocks, bool):
        return blocks
    if (not isinstance(blocks, int) or not _native.LONG_BLOCK_MIN <= blocks <= _native.LONG_BLOCK_MAX
            or blocks & (blocks - 1)):
        raise ValueError(f"blocks must be a bool or a power of two from {_native.LONG_BLOCK_MIN} to 2**24 = "
                         f"{_native.LONG_BLOCK_MAX} (the points of one block), got {blocks!r}")
    return int(blocks)


def _long_blocks_choice(blocks, batch: int, cin: int, cout: int, groups: int, length: int, taps: int, pad_left: int,
                        pad_right: int, out_keep: int, flip: bool, need: int, stride: int = 1, dilation: int = 1,
                        pad_mode: int = 0, dtype=torch.float32, x_layout: str = "ncl", channels_last: bool = False):
    """Whether the primitive of these numbers runs by blocks under ``blocks`` (pure: numbers and the library's geometry call,
    which touches no device) -> the block_points of its plan (0: the planner's choice, for ``True``), or None where it runs
    as without the keyword.  By blocks: float32 / float16 / bfloat16, stride 1, dilation 1, zero padding, a signal that is
    not read as channels-last and a contiguous result, a row that is no hand-off (``need`` > 4096 points) and needs more
    points than fit -- 2**24 for ``True``, N for an int N -- and taps read <= N / 2 (the library's refusal)."""
    if blocks is False or dtype not in (torch.float32,) + _LOW_PRECISION:
        return None
    if stride != 1 or dilation != 1 or pad_mode != 0 or x_layout == "nlc" or channels_last:
        return None
    if need <= LONG_HANDOFF_POINTS or need <= (LONG_MAX_POINTS if blocks is True else blocks):
        return None
    points = 0 if blocks is True else int(blocks)
    try:
        _native.blocks_geometry((int(batch), int(cin), int(cout), int(groups), int(length), int(taps), int(pad_left),
                                 int(pad_right), int(out_keep), int(bool(flip)), 0, points))
    except NotImplementedError:
        return None
    return points


def _long_blocks_route_of(blocks, batch: int, cin: int, cout: int, groups: int, length: int, taps: int, pad_left: int,
                          pad_right: int, need: int, causal: bool, stride: int, dilation: int, pad_mode: int, dtype,
                          x_layout: str, channels_last: bool):
    """``_long_blocks_route`` from the numbers ``_long_geometry`` returns -> (route, block_points of a "blocks" route)."""
    points = _long_blocks_choice(blocks, batch, cin, cout, groups, length, taps, pad_left, pad_right,
                                 _long_keep(length, causal, stride), causal, need, stride, dilation, pad_mode, dtype, x_layout,
                                 channels_last)
    if points is not None:
        return "blocks", points
    return _long_route_of(length, taps, pad_left, pad_right, need, causal, stride, dilation, pad_mode, dtype, x_layout), None


def _long_blocks_route(signal_shape, kernel_shape, stride=1, padding=0, dilation=1, groups=1, causal=False,
                       padding_mode="constant", dtype=torch.float32, x_layout="ncl", channels_last=False, blocks=False) -> str:
    """Which route a ``fft_long_conv(..., blocks=blocks)`` call takes (pure: shapes, numbers, the switches ``_long_route``
    reads and the library's geometry call):

    ``"blocks"``   ``blocks`` is True or an int N, float32 / float16 / bfloat16, stride 1, dilation 1, ``padding_mode``
                   constant, a signal that is not read as channels-last, ``channels_last=False``, a row that is no hand-off
                   and needs more points than 2**24 (True) or than N (int), taps read <= N / 2: overlap-save blocks of N
                   points against one filter spectrum of N bins (True: the planner's N);
    otherwise      whatever ``_long_route`` answers for the call without the keyword, its error included."""
    blocks = _long_blocks_arg(blocks)
    meta = dict(device="meta")
    signal, kernel = torch.empty(tuple(signal_shape), **meta), torch.empty(tuple(kernel_shape), **meta)
    pad_left, pad_right, need = _long_geometry(signal, kernel, None, padding, groups, causal, stride, dilation, padding_mode)
    stride, dilation, mode = _long_int("stride", stride), _long_int("dilation", dilation), _native.PAD_MODES[padding_mode]
    if not isinstance(channels_last, bool):
        raise ValueError(f"channels_last must be a bool, got {channels_last!r}")
    return _long_blocks_route_of(blocks, int(signal_shape[0]), int(signal_shape[1]), int(kernel_shape[0]), groups,
                                 int(signal_shape[2]), int(kernel_shape[2]), pad_left, pad_right, need, bool(causal), stride,
                                 dilation, mode, dtype, x_layout, channels_last)[0]


def _long_route(signal_shape, kernel_shape, stride=1, padding=0, dilation=1, groups=1, causal=False,
                padding_mode="constant", dtype=torch.float32, x_layout="ncl") -> str:
    """Which route a ``fft_long_conv`` call takes (pure: shapes, numbers and FFTCONV_LONG_DECIM only):

    ``"handoff"``  a real row whose padded length fits LONG_HANDOFF_POINTS: the ``fft_conv`` kernels;
    ``"phases"``   stride 2 ... 64, dilation 1, ``padding_mode`` constant, float32 / float16 / bfloat16, a signal that is not
                   read as channels-last, L < 2**29 and a decimated row of at most 2**24 points, causal or not:
                   y[j] = sum_p (u_p * x_p)[j] on the ``stride`` decimated rows x_p[t] = xrow[stride*t + p] against the
                   phases u_p[m] = u[stride*m + p] of the taps, a transform of about nout + ceil(K / stride) points.  Taken
                   wherever eligible under FFTCONV_LONG_DECIM=1, never under =0 and, with the variable unset, only where
                   the plain row does not fit 2**24 points;
    ``"plain"``    everything else: the long primitive on the whole padded row, its stride skipping outputs.

    ``x_layout``: ``_long_layout`` of the signal.  A row that fits no long route raises ``NotImplementedError`` with the count."""
    return _long_route_numbers(signal_shape, kernel_shape, stride, padding, dilation, groups, causal, padding_mode, dtype,
                               x_layout)[0]


def _long_route_numbers(signal_shape, kernel_shape, stride, padding, dilation, groups, causal, padding_mode, dtype, x_layout):
    """``_long_route`` of a call from its shapes -> (route, pad_left, pad_right, stride, dilation, PadMode code)."""
    meta = dict(device="meta")
    signal, kernel = torch.empty(tuple(signal_shape), **meta), torch.empty(tuple(kernel_shape), **meta)
    pad_left, pad_right, need = _long_geometry(signal, kernel, None, padding, groups, causal, stride, dilation, padding_mode)
    stride, dilation, mode = _long_int("stride", stride), _long_int("dilation", dilation), _native.PAD_MODES[padding_mode]
    route = _long_route_of(int(signal_shape[2]), int(kernel_shape[2]), pad_left, pad_right, need, bool(causal), stride, dilation,
                           mode, dtype, x_layout)
    return route, pad_left, pad_right, stride, dilation, mode


def _long_wgrad_mode() -> bool:
    """FFTCONV_LONG_WGRAD (read per call): "1" takes the weight-gradient plan wherever eligible; unset or anything else never."""
    return os.environ.get("FFTCONV_LONG_WGRAD", "0") == "1"


def _long_wgrad_key(batch: int, cin: int, cout: int, groups: int, length: int, taps: int, pad_left: int, pad_right: int,
                    nout: int, flip: bool, pad_mode: int, stride: int, dilation: int) -> tuple:
    """The words of ``_native.wgrad_desc`` for the layer of a forward long plan."""
    return (int(batch), int(cin), int(cout), int(groups), int(length), int(taps), int(pad_left), int(pad_right), int(nout),
            int(bool(flip)), int(pad_mode), int(stride), int(dilation))


def _long_wgrad_eligible(key: tuple, dtype) -> bool:
    """Whether dW of this layer takes the weight-gradient plan (pure: the switch, the dtype, and the library's geometry call
    on the descriptor, which touches no device): FFTCONV_LONG_WGRAD=1, float32 / float16 / bfloat16, and a geometry the
    library does not refuse (2**24 points, the rows of W2 inside the workspace budget, 32-bit grids)."""
    if not _long_wgrad_mode() or dtype not in (torch.float32,) + _LOW_PRECISION:
        return False
    try:
        _native.wgrad_geometry(key)
    except NotImplementedError:
        return False
    return True


def _long_wgrad_route(signal_shape, kernel_shape, stride=1, padding=0, dilation=1, groups=1, causal=False,
                      padding_mode="constant", dtype=torch.float32, x_layout="ncl") -> str:
    """Which route the weight gradient of a ``fft_long_conv`` call takes in ``FFTLongConvFunction.backward`` (pure: shapes,
    numbers, FFTCONV_LONG_WGRAD and FFTCONV_LONG_DECIM, and the library's geometry call):

    ``"plan"``       FFTCONV_LONG_WGRAD=1 on the plain branch of backward (a forward on the plain route, or a causal one
                     whatever its route), float32 / float16 / bfloat16: ``_long_wgrad_run``, x and dY read where they lie;
    ``"exchanged"``  everything else: the route of a call with the switch unset (the forward primitive with batch and
                     channels exchanged on transposed copies; by phases where the forward ran so; ``fft_conv``'s own
                     gradient for a row that hands off)."""
    route, pad_left, pad_right, stride, dilation, mode = _long_route_numbers(
        signal_shape, kernel_shape, stride, padding, dilation, groups, causal, padding_mode, dtype, x_layout)
    length, taps = int(signal_shape[2]), int(kernel_shape[2])
    if route == "handoff" or (route == "phases" and not causal):
        return "exchanged"
    nout = _long_keep(length, causal, stride) or (length + pad_left + pad_right - dilation * (taps - 1) - 1) // stride + 1
    key = _long_wgrad_key(signal_shape[0], signal_shape[1], kernel_shape[0], groups, length, taps, pad_left, pad_right, nout,
                          causal, mode, stride, dilation)
    return "plan" if _long_wgrad_eligible(key, dtype) else "exchanged"


def _long_wgrad_run(signal: Tensor, grad: Tensor, wshape, key: tuple, out_dtype: torch.dtype, *,
                    pregate: Optional[Tensor] = None, postgate: Optional[Tensor] = None,
                    block_points: Optional[int] = None) -> Tensor:
    """dW (``wshape``, ``out_dtype``) of the layer ``key`` describes (``_long_wgrad_key``) on its weight-gradient plan, no
    autograd.  ``signal`` (B, Cin, L) and ``grad`` (B, Cout, nout) are float32, float16 or bfloat16, each on its own, and
    each is read where it lies: contiguous, or as the channels-last view ``_long_layout`` recognises (another layout, a
    block of 2**31 bytes or more, FFTCONV_LONG_NLC=0: one torch copy of that tensor).  No transposed operand and no
    flipped copy of the result exists; the float32 result is rounded once as it is stored.

    ``pregate`` (like ``signal``) and ``postgate`` (like ``grad``), each in its tensor's dtype: dW of the rows
    pregate * signal and the gradient postgate * grad, multiplied as the column passes load them
    (``LongWgradPlan.run_gated``: neither product exists, the bits are those of this call on the float32 products).  A
    gated side and its gate are read as contiguous (B, C, L) tensors.  The plan is the one of the call without gates; what
    it refuses under a gate (a padding mode under ``pregate``, a stride under ``postgate``) raises ``NotImplementedError``.

    ``block_points`` (not None): the weight-gradient plan BY BLOCKS of that many points (0: the planner's choice), for a
    layer whose forward ran by blocks (``fc_long_wgrad_blocks_plan_create``): both tensors are read contiguous, no gates."""
    gates = (pregate, postgate)
    tensors, layouts = [], []
    for t, gate in zip((signal.detach(), grad.detach()), gates):
        # (the kernel reads the gate at the offsets of its tensor: same shape, element size and device, or it reads elsewhere)
        if gate is not None and (tuple(gate.shape) != tuple(t.shape) or gate.dtype != t.dtype or gate.device != t.device):
            raise ValueError(f"a gate of the weight-gradient plan must match its tensor {tuple(t.shape)} {t.dtype} on "
                             f"{t.device}, got {tuple(gate.shape)} {gate.dtype} on {gate.device}")
        nlc = gate is None and block_points is None and _long_reads_nlc(t)
        tensors.append(t if nlc else t.contiguous())
        layouts.append(_native.LONG_NLC if nlc else _native.LONG_NCL)
    x, dy = tensors
    pregate, postgate = (None if t is None else t.detach().contiguous() for t in gates)
    if block_points is None:
        plan = _cached_plan(_device_index(x.device), ("long_wgrad",) + tuple(key))
    else:
        plan = _cached_plan(_device_index(x.device), ("long_wgrad_blocks",) + tuple(key) + (int(block_points),))
    with torch.cuda.device(x.device):
        dw = torch.empty(tuple(wshape), dtype=out_dtype, device=x.device)
        ws, ws_ptr, stream = _scratch_and_stream(plan, x.device)
        codes = (_DTYPE_CODES[x.dtype], _DTYPE_CODES[dy.dtype], _DTYPE_CODES[out_dtype], layouts[0], layouts[1])
        if pregate is None and postgate is None:
            plan.run(x.data_ptr(), dy.data_ptr(), dw.data_ptr(), ws_ptr, stream, *codes)
        else:
            ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
            plan.run_gated(x.data_ptr(), ptr(pregate), dy.data_ptr(), ptr(postgate), dw.data_ptr(), ws_ptr, stream, *codes)
    return dw


def fft_long_conv(signal: Tensor, kernel: Tensor, bias: Tensor = None, padding: Union[int, str] = 0, groups: int = 1,
                  causal: bool = False, *, stride: int = 1, dilation: int = 1, padding_mode: str = "constant",
                  channels_last: bool = False, blocks: Union[bool, int] = False) -> Tensor:
    """1-D convolution with a filter as long as the row: ONE transform over the whole padded row (as the reference does,
    functional.py:66-75) instead of overlap-save tiles, so the work does not grow with the number of taps.

    ``signal`` (B, Cin, L), ``kernel`` (Cout, Cin/groups, K), ``bias`` (Cout,) or None, on a ROCm device, all three float32,
    float16, bfloat16 or complex64.  ``causal=False``: equal to ``fft_conv(signal, kernel, bias, stride, padding, dilation, groups,
    padding_mode)`` (cross-correlation; ``padding`` an int, 'same' or 'valid'; ``padding_mode`` constant | reflect |
    replicate | circular), output length (L + 2*padding - dilation*(K-1) - 1) // stride + 1.  ``causal=True`` (``padding``
    must be 0 and ``padding_mode`` constant):
    y[b, o, j] = bias[o] + sum_i sum_k kernel[o, i, k] * signal[b, (g, i), stride*j - dilation*k] over the taps with
    dilation*k <= stride*j, output length ceil(L / stride); K may exceed L.  The stride only skips outputs, the dilation
    only spreads the taps inside the one transform: neither a zero-stuffed kernel nor a padded copy of the row exists.
    Differentiable in signal, kernel and bias.

    float16 / bfloat16 tensors are read and written by the kernels themselves: float32 arithmetic, the signal and the
    taps widened as they are loaded, the output rounded once as it is stored, so the result (and, in training, each
    gradient) has the bits of widening the tensors, running the float32 function and rounding with ``.to(dtype)``.
    Autograd saves the 16-bit tensors.  ``FFTCONV_HALF_IO=0`` takes that cast path instead.

    complex64 tensors (all three) run the same transform with one batch item per row of it instead of a packed pair: the
    product is plain bilinear, nothing is conjugated (as ``torch.nn.functional.conv1d`` on complex tensors), every
    argument keeps its meaning, the output is complex64 of the same length, arithmetic and spectra are float32.  The
    gradients follow PyTorch's convention for complex tensors.  Lazy conjugates (``x.conj()``) are resolved on entry.

    Sequence models keep (batch, length, channels) activations.  A ``signal`` that is ``u.transpose(1, 2)`` of a contiguous
    (B, L, C) tensor ``u`` (strides exactly (L*C, 1, C), any storage offset) is read where it lies, with no copy, and
    ``channels_last=True`` returns the (B, Cout, nout) result with strides (nout*Cout, 1, Cout), so that
    ``y.transpose(1, 2)`` is a contiguous (B, nout, Cout) tensor; input and output layout are independent.  The values
    have the bits of the call on contiguous tensors.  In backward a dY that lies that way is read where it lies and dX
    gets the signal's layout; the weight gradient's transposed operands are torch copies as ever, unless FFTCONV_LONG_WGRAD=1
    (read per call; opt-in, the bits of dW change) selects the weight-gradient plan, which reads x and dY where they lie in
    either layout (``_long_wgrad_route`` names the route; ``FFTLongConvFunction``).  Other non-contiguous
    tensors are copied.  ``FFTCONV_LONG_NLC=0`` (read per call) takes torch copies everywhere, as do rows that hand off
    to ``fft_conv``, the ``FFTCONV_HALF_IO=0`` path and tensors whose (L, C) block of one batch item reaches 2**31 bytes.

    With stride s = 2 ... 64, dilation 1 and ``padding_mode`` constant on float32 / float16 / bfloat16 tensors (a signal
    that is not read as channels-last; causal or not) the call can run BY PHASES instead: y[j] = sum_p (u_p * x_p)[j] on the
    s decimated rows x_p[t] = xrow[s*t + p] against the phases u_p[m] = u[s*m + p] of the taps, one transform of about
    nout + ceil(K/s) points per decimated row where the plain row needs L + 2*padding; signal and weight are read where
    they lie.  ``FFTCONV_LONG_DECIM`` (read per call) selects it: "0" never, "1" wherever eligible, unset only where the
    plain row does not fit 2**24 points (``_long_route`` names the route of a call).  A non-causal forward that ran by
    phases has gradients of the same length (dX the transposed convolution of dY by phases, dW with the phases of x as a
    batch-like index); a causal one keeps the plain gradients, so a causal row past 2**24 points cannot be trained.

    ``blocks`` (keyword-only) runs a row IN OVERLAP-SAVE BLOCKS over the long transform: the padded row is cut into blocks
    of N points that overlap by (taps read) - 1, each block is one cyclic transform against ONE filter spectrum of N bins,
    and the block index rides where the batch index does, so a row may be longer than 2**24 points and the spectrum and the
    workspace grow with the filter, not with the row.  ``False``: the call it always was.  ``True``: by blocks where the
    whole row does not fit 2**24 points (N: the planner's choice, the smallest power of two >= 4 * taps, at least 2**18).
    An int N (a power of two 4096 ... 2**24, else ``ValueError``): by blocks of N points wherever the row needs more than N.
    Either only where the call is eligible -- float32 / float16 / bfloat16, stride 1, dilation 1, ``padding_mode`` constant, a
    signal that is not read as channels-last, ``channels_last=False``, taps read <= N / 2, a row that is no hand-off; causal
    or not, any groups -- and otherwise the call is that of ``blocks=False`` (``_long_blocks_route`` names the route).  In
    backward dX is the same primitive on dY and runs by blocks under the same rule, and dW of a forward that ran by blocks
    comes from the weight-gradient plan by blocks (x and dY read where they lie, the unit pairs summed as batch pairs are).

    Real rows whose padded length is at most 4096 run the ``fft_conv`` kernels (complex rows stay here, at 64 x 64 points);
    a row that fits no route inside 2**24 points raises ``NotImplementedError`` (``blocks=True`` is the way past it).  float64 and complex128 tensors, tensors of
    different dtypes and mixes of real and complex tensors are not taken by this path (``TypeError``)."""
    return _fft_long_conv_impl(signal, kernel, bias, padding, groups, causal, None, stride, dilation, padding_mode,
                               channels_last, blocks)


def _fft_long_conv_impl(signal, kernel, bias, padding, groups, causal, spectrum, stride=1, dilation=1,
                        padding_mode="constant", channels_last=False, blocks=False):
    blocks = _long_blocks_arg(blocks)
    pad_left, pad_right, need = _long_geometry(signal, kernel, bias, padding, groups, causal, stride, dilation, padding_mode)
    stride, dilation, mode = _long_int("stride", stride), _long_int("dilation", dilation), _native.PAD_MODES[padding_mode]
    layout = _long_call_layout(signal, channels_last)
    if blocks is False:      # (the call it always was)
        route, points = _long_route_of(int(signal.shape[2]), int(kernel.shape[2]), pad_left, pad_right, need, bool(causal),
                                       stride, dilation, mode, signal.dtype, layout), None
    else:
        route, points = _long_blocks_route_of(blocks, int(signal.shape[0]), int(signal.shape[1]), int(kernel.shape[0]), groups,
                                              int(signal.shape[2]), int(kernel.shape[2]), pad_left, pad_right, need,
                                              bool(causal), stride, dilation, mode, signal.dtype, layout, channels_last)
    signal, kernel, bias, cast = _long_operands(signal, kernel, bias)
    if cast:      # FFTCONV_HALF_IO=0
        out = _fft_long_conv_impl(signal.float(), kernel.float(), None if bias is None else bias.float(), padding, groups,
                                  causal, None, stride, dilation, padding_mode, channels_last, blocks)
        return out.to(signal.dtype)          # (keeps the strides)
    if route == "handoff":      # (fft_conv has no complex route: a complex row never gets here)
        if not causal:
            out = _fft_conv_impl(signal, kernel, bias, stride, padding, dilation, groups, padding_mode, None)
        else:
            # taps at a lag of L or more never reach the output
            taps = min(int(kernel.shape[2]), (int(signal.shape[2]) - 1) // dilation + 1)
            padded = torch.nn.functional.pad(signal, (dilation * (taps - 1), 0))
            out = _fft_conv_impl(padded, kernel[..., :taps].flip(-1), bias, stride, 0, dilation, groups, "constant", None)
        return _as_channels_last(out) if channels_last else out
    if _needs_grad(signal, kernel, bias):
        from .autograd import FFTLongConvFunction
        return FFTLongConvFunction.apply(signal, kernel, bias, pad_left, pad_right, bool(causal), groups, spectrum,
                                         stride, dilation, padding_mode, channels_last, route == "phases",
                                         (blocks, points))
    run = _long_forward_plan(signal, kernel.shape, bias is not None, pad_left, pad_right, causal, groups, stride, dilation,
                             mode, route, block_points=points)[1]
    return _long_run(signal, kernel, bias, pad_left, pad_right, causal, groups=groups, spectrum=spectrum,
                     channels_last=channels_last, **run)


def _long_keep(length: int, causal: bool, stride: int) -> int:
    """``out_keep`` of the forward plan: ceil(L / stride) outputs of the causal form, all of them (0) otherwise."""
    return -(-int(length) // stride) if causal else 0


def _long_forward_plan(signal: Tensor, wshape, has_bias: bool, pad_left: int, pad_right: int, causal: bool, groups: int,
                       stride: int, dilation: int, pad_mode: int, route: str, *, block_points: Optional[int] = None):
    """(plan, the keyword arguments ``_long_run`` takes for it) of a ``fft_long_conv`` call on ``route`` ("plain" |
    "phases" | "blocks", the last with the ``block_points`` ``_long_blocks_route_of`` returns), from the numbers ``_long_geometry`` returns: the one place that maps a forward route to its plan (the
    functional, ``FFTLongConvFunction.forward`` and ``FFTLongConv1d``, which caches the spectrum of this plan).  Both plans
    transform the (Cout, Cin/groups, K) weight ``wshape`` itself."""
    cout, taps, keep = int(wshape[0]), int(wshape[2]), _long_keep(signal.shape[2], causal, stride)
    if route == "blocks":
        assert block_points is not None and (stride, dilation, pad_mode) == (1, 1, 0), "by blocks: the plain zero-padded primitive"
        run = dict(out_keep=keep)
        plan = _long_blocks_plan(signal, cout, groups, taps, pad_left, pad_right, causal, keep, has_bias, block_points)
    elif route == "phases":
        run = dict(out_keep=keep, decim=stride)
        plan = _long_decim_plan(signal, cout, groups, taps, stride, pad_left, pad_right, keep, causal, has_bias)
    else:
        assert route == "plain", route
        run = dict(out_keep=keep, pad_mode=pad_mode, tap_dil=dilation, out_step=stride)
        plan = _long_plan(signal, cout, groups, taps, pad_left, pad_right, causal, has_bias=has_bias, **run)
    run["plan"] = plan
    return plan, run


_LONG_DTYPES = (torch.float32,) + _LOW_PRECISION + (torch.complex64,)
_LONG_GATE = (_LONG_DTYPES,
              "fft_long_conv takes signal, kernel and bias "
              "that share one of float32, float16, bfloat16 or complex64 (float64 runs through fft_conv only; "
              "complex128, complex32 and mixes of real and complex tensors are not taken: convert with "
              ".to(torch.complex64))")


def _long_call_layout(signal: Tensor, channels_last) -> str:
    """The layout a long op routes its signal by: ``_long_layout``, "ncl" for every tensor under FFTCONV_LONG_NLC=0.  (The
    ``channels_last`` argument is checked here: after the geometry, before the route.)"""
    if not isinstance(channels_last, bool):
        raise ValueError(f"channels_last must be a bool, got {channels_last!r}")
    return _long_route_layout(signal)


def _long_route_layout(t: Tensor) -> str:
    """``_long_layout``, "ncl" for every tensor under FFTCONV_LONG_NLC=0: the layout a signal is routed by, in the forward
    and (dY as the signal of dX) in backward."""
    layout = _long_layout(t)
    return layout if layout == "ncl" or _long_nlc_enabled() else "ncl"


def _long_operands(signal: Tensor, kernel: Tensor, bias: Optional[Tensor]):
    """What the two long ops do between their route and their launch: the device and dtype gate, one device, complex
    tensors resolved (the library reads data_ptr(): a conj or neg bit is resolved first, inside the autograd graph) ->
    (signal, kernel, bias, whether the call takes the cast path).  The cast path is FFTCONV_HALF_IO=0: float32 copies in,
    one rounding pass out (what a caller would write by hand)."""
    for name, t in (("signal", signal), ("kernel", kernel), ("bias", bias)):
        if t is not None:
            _require_gpu(name, t, signal.dtype, _LONG_GATE)
    _same_device(signal=signal, kernel=kernel, bias=bias)
    if signal.dtype == torch.complex64:
        signal, kernel, bias = _resolved(signal), _resolved(kernel), None if bias is None else _resolved(bias)
    return signal, kernel, bias, signal.dtype in _LOW_PRECISION and not _half_native(signal, kernel, bias)


# ---------------------------------------------------------------------------------- gated long filters
def _long_out_len(length: int, taps: int, pad_left: int, pad_right: int, causal: bool, stride: int, dilation: int) -> int:
    """Output length of a ``fft_long_conv`` call from the numbers ``_long_geometry`` returns."""
    return _long_keep(length, causal, stride) or (length + pad_left + pad_right - dilation * (taps - 1) - 1) // stride + 1


def _long_gates(signal: Tensor, pregate: Optional[Tensor], postgate: Optional[Tensor], out_shape: tuple):
    """Argument checks of the gates of ``fft_long_conv_gated`` (before any device call): ``pregate`` has the signal's shape
    and ``postgate`` the result's (ValueError), each the signal's dtype (TypeError) and device (ValueError)."""
    for name, t, shape, of in (("pregate", pregate, tuple(signal.shape), "signal"), ("postgate", postgate, tuple(out_shape), "result")):
        if t is None:
            continue
        if not isinstance(t, Tensor):
            raise TypeError(f"`{name}` must be a tensor or None, got {type(t).__name__}")
        if tuple(t.shape) != shape:
            raise ValueError(f"`{name}` must have the {of}'s shape {shape}, got {tuple(t.shape)}")
        if t.dtype != signal.dtype:
            raise TypeError(f"`{name}` has dtype {t.dtype} but the signal is {signal.dtype}; the gates share the signal's dtype")
        if t.device != signal.device:
            raise ValueError(f"`{name}` is on {t.device} but the signal is on {signal.device}; all tensors of one call must be "
                             f"on the same device")


def _long_gated_route_of(route: str, stride: int, dilation: int, pad_mode: int, dtype, x_layout: str, channels_last: bool) -> str:
    """``_long_gated_route`` from the route ``_long_route_of`` names and the numbers of the call."""
    fused = (dtype in (torch.float32,) + _LOW_PRECISION and route == "plain" and stride == 1 and dilation == 1
             and pad_mode == 0 and not channels_last and x_layout != "nlc"
             and not (dtype in _LOW_PRECISION and os.environ.get("FFTCONV_HALF_IO", "1") == "0"))
    return "fused" if fused else "composed"


def _long_gated_route(signal_shape, kernel_shape, stride=1, padding=0, dilation=1, groups=1, causal=False,
                      padding_mode="constant", dtype=torch.float32, x_layout="ncl", channels_last=False) -> str:
    """Which route a ``fft_long_conv_gated`` call with a gate takes (pure: shapes, dtypes, strides and numbers only; no
    switch selects between the two):

    ``"fused"``     float32 / float16 / bfloat16 tensors, ``_long_route`` "plain", stride 1, dilation 1, ``padding_mode``
                    constant (the unmapped builds of the column kernels), neither a signal read channels-last
                    (``x_layout``: ``_long_layout`` of the signal) nor a channels-last result: the gates ride the column
                    passes of the one call (``fc_long_forward_gated``);
    ``"composed"``  everything else -- complex64, the phases route, a stride, a dilation, a padding mode, channels-last
                    signal or result, a row that hands off to ``fft_conv``, the FFTCONV_HALF_IO=0 cast path: the line
                    ``postgate * fft_long_conv(pregate * signal, ...)`` with torch multiplies."""
    route, _, _, stride, dilation, mode = _long_route_numbers(signal_shape, kernel_shape, stride, padding, dilation, groups,
                                                              causal, padding_mode, dtype, x_layout)
    return _long_gated_route_of(route, stride, dilation, mode, dtype, x_layout, bool(channels_last))


def _long_gated_dw_route(signal_shape, kernel_shape, padding=0, groups=1, causal=False, dtype=torch.float32, *, stride=1,
                         dilation=1, padding_mode="constant", x_layout="ncl", channels_last=False) -> str:
    """Where the weight gradient of a ``fft_long_conv_gated`` call with a gate comes from in
    ``FFTLongConvGatedFunction.backward`` (pure: shapes, numbers, FFTCONV_LONG_WGRAD read per call, and the library's
    geometry call, which touches no device):

    ``"gated-plan"``  ``_long_gated_route`` "fused" and a layer the weight-gradient plan takes (``_long_wgrad_eligible``:
                      FFTCONV_LONG_WGRAD=1 and a geometry the library does not refuse): ``_long_wgrad_run`` with the gates,
                      x, dY and the gates read where they lie in their own dtype, no product tensor;
    ``"products"``    everything else: the route of ``fft_long_conv``'s weight gradient on the float32 products
                      pregate * x and postgate * dY that torch forms (and, off the fused route, whatever the composed line's
                      autograd does)."""
    route, pad_left, pad_right, stride, dilation, mode = _long_route_numbers(
        signal_shape, kernel_shape, stride, padding, dilation, groups, causal, padding_mode, dtype, x_layout)
    if _long_gated_route_of(route, stride, dilation, mode, dtype, x_layout, bool(channels_last)) != "fused":
        return "products"
    length, taps = int(signal_shape[2]), int(kernel_shape[2])
    nout = _long_out_len(length, taps, pad_left, pad_right, bool(causal), 1, 1)
    key = _long_wgrad_key(signal_shape[0], signal_shape[1], kernel_shape[0], groups, length, taps, pad_left, pad_right, nout,
                          causal, 0, 1, 1)
    return "gated-plan" if _long_wgrad_eligible(key, dtype) else "products"


def _long_run_gated(signal: Tensor, kernel: Optional[Tensor], bias: Optional[Tensor], pad_left: int, pad_right: int,
                    flip: bool, out_keep: int, groups: int, spectrum: Optional[KernelSpectrum] = None, *,
                    pregate: Optional[Tensor] = None, gate: Optional[Tensor] = None, gate2: Optional[Tensor] = None,
                    second: bool = False, second_dtype: Optional[torch.dtype] = None, weight_shape: Optional[tuple] = None,
                    plan=None):
    """The plain primitive of ``_long_run`` (zero padding, no spread, dilation 1, every output kept; float32 / float16 /
    bfloat16, contiguous (B, C, L) tensors) with gates in its column passes, no autograd -> (y, y2):
    rows = pregate * signal, c = conv(rows) + bias, y = gate * c and, with ``second`` or a ``gate2``, y2 = gate2 * c from
    the same launch; an absent gate is all ones and y2 is None where not asked for.  ``second_dtype`` float32 on 16-bit
    tensors (no ``gate2``) stores c unrounded.  Tensors that do not lie contiguous are copied first."""
    signal = signal.detach().contiguous()
    pregate, gate, gate2 = (None if t is None else t.detach().contiguous() for t in (pregate, gate, gate2))
    cout, taps = (int(kernel.shape[0]), int(kernel.shape[2])) if weight_shape is None else weight_shape
    if plan is None:
        plan = _long_plan(signal, cout, groups, taps, pad_left, pad_right, flip, out_keep, bias is not None)
    if spectrum is None or spectrum.plan is not plan:
        spectrum = transform_kernel(plan, kernel)
    bias_c = None if bias is None else bias.detach().float().contiguous()
    shape = (int(signal.shape[0]), cout, plan.out_len)
    second = second or gate2 is not None
    with torch.cuda.device(signal.device):
        out = torch.empty(shape, dtype=signal.dtype, device=signal.device)
        out2 = torch.empty(shape, dtype=second_dtype or signal.dtype, device=signal.device) if second else None
        ws, ws_ptr, stream = _scratch_and_stream(plan, signal.device)
        ptr = lambda t: None if t is None else t.data_ptr()      # noqa: E731
        plan.forward_gated(signal.data_ptr(), spectrum.buf.data_ptr(), ptr(bias_c), out.data_ptr(), ws_ptr, stream,
                           _DTYPE_CODES[signal.dtype], _DTYPE_CODES[out.dtype], pregate_ptr=ptr(pregate), gate_ptr=ptr(gate),
                           y2_ptr=ptr(out2), gate2_ptr=ptr(gate2),
                           y2_dtype=None if out2 is None else _DTYPE_CODES[out2.dtype])
    return out, out2


def fft_long_conv_gated(signal: Tensor, kernel: Tensor, bias: Tensor = None, padding: Union[int, str] = 0, groups: int = 1,
                        causal: bool = False, *, pregate: Tensor = None, postgate: Tensor = None, stride: int = 1,
                        dilation: int = 1, padding_mode: str = "constant", channels_last: bool = False) -> Tensor:
    """The gated long convolution of Hyena / H3 / M2 layers, defined for every call ``fft_long_conv`` accepts:

        postgate * fft_long_conv(pregate * signal, kernel, bias, padding, groups, causal, stride=..., dilation=...,
                                 padding_mode=..., channels_last=...)

    ``pregate`` has the signal's shape and ``postgate`` the result's, each the signal's dtype and device; either may be
    None, and with both None the call IS ``fft_long_conv``, bit for bit.  A wrong shape or device raises ``ValueError``, a
    wrong dtype ``TypeError``, before any device call.

    On float32 / float16 / bfloat16 tensors, where ``fft_long_conv`` takes its plain route with stride 1, dilation 1 and
    ``padding_mode`` constant and neither the signal is read channels-last nor the result asked for that way, the gates
    are FUSED into the two column passes of the one call: each sample of the signal is multiplied by its pregate as it is
    loaded, each sample of the result by its postgate as it is stored -- no product tensor exists.  Signal and gates are
    read as contiguous (B, C, L) tensors (anything else is copied first).  The products are float32 multiplies and the
    result is rounded once, so it has the bits of: widen every tensor to float32, run the line above, round with
    ``.to(dtype)`` (float32 tensors: the bits of the line itself).  Every other call -- complex64, the phases route, a
    stride, a dilation, a padding mode, channels-last signal or result, rows that hand off to ``fft_conv``,
    FFTCONV_HALF_IO=0 -- runs the line above with torch multiplies.  ``_long_gated_route`` names the route; no switch
    selects it.

    Differentiable in signal, kernel, bias and both gates.  On the fused route autograd saves signal, kernel and the gates
    -- never ``pregate * signal`` nor the gated result -- and the ungated c = conv + bias only when ``postgate`` needs a
    gradient (stored by the same launch; float32 for 16-bit tensors, so that d(postgate) is rounded once).  dX and
    d(pregate) come from ONE run of the dX primitive: ``postgate`` gates dY as it is loaded and the last pass stores
    pregate * dZ and signal * dZ.  d(postgate) = dY * c is one torch multiply; dW and db take the routes of
    ``fft_long_conv`` on the float32 products torch forms -- except under FFTCONV_LONG_WGRAD=1 (read per call;
    ``_long_gated_dw_route`` "gated-plan"), where dW comes from the weight-gradient plan with both gates inside its column
    reads: the saved tensors are read in their own dtype and neither product exists (the bits of dW are those of that plan
    on the products).  Each gradient has the bits of autograd through the line above
    on float32 tensors, rounded once.  Double backward goes through the composed line.

    A skip term needs no argument: for a causal depthwise layer ``kernel[..., 0] += D`` adds ``D * (pregate * signal)``."""
    return _fft_long_conv_gated_impl(signal, kernel, bias, padding, groups, causal, None, pregate, postgate, stride, dilation,
                                     padding_mode, channels_last)


def _fft_long_conv_gated_impl(signal, kernel, bias, padding, groups, causal, spectrum, pregate, postgate, stride=1, dilation=1,
                              padding_mode="constant", channels_last=False):
    if pregate is None and postgate is None:
        return _fft_long_conv_impl(signal, kernel, bias, padding, groups, causal, spectrum, stride, dilation, padding_mode,
                                   channels_last)
    pad_left, pad_right, need = _long_geometry(signal, kernel, bias, padding, groups, causal, stride, dilation, padding_mode)
    s, d, mode = _long_int("stride", stride), _long_int("dilation", dilation), _native.PAD_MODES[padding_mode]
    length, taps = int(signal.shape[2]), int(kernel.shape[2])
    _long_gates(signal, pregate, postgate,
                (int(signal.shape[0]), int(kernel.shape[0]), _long_out_len(length, taps, pad_left, pad_right, bool(causal), s, d)))
    layout = _long_call_layout(signal, channels_last)
    route = _long_gated_route_of(_long_route_of(length, taps, pad_left, pad_right, need, bool(causal), s, d, mode, signal.dtype,
                                                layout), s, d, mode, signal.dtype, layout, channels_last)
    if route == "composed":
        out = _fft_long_conv_impl(signal if pregate is None else pregate * signal, kernel, bias, padding, groups, causal,
                                  spectrum, stride, dilation, padding_mode, channels_last)
        return out if postgate is None else postgate * out
    signal, kernel, bias, _ = _long_operands(signal, kernel, bias)
    if _needs_grad(signal, kernel, bias, pregate, postgate):
        from .autograd import FFTLongConvGatedFunction
        return FFTLongConvGatedFunction.apply(signal, kernel, bias, pregate, postgate, pad_left, pad_right, bool(causal), groups,
                                              spectrum)
    plan, run = _long_forward_plan(signal, kernel.shape, bias is not None, pad_left, pad_right, causal, groups, 1, 1, 0, "plain")
    return _long_run_gated(signal, kernel, bias, pad_left, pad_right, causal, run["out_keep"], groups, spectrum,
                           pregate=pregate, gate=postgate, plan=plan)[0]


# ---------------------------------------------------------------------------------- decoding: one token at a time
LONG_STREAM_HEAD = 64             # taps a step applies itself when ``head`` is None (DESIGN 4.7 has the sweep behind it)
_STREAM_DTYPES = (torch.float32,) + _LOW_PRECISION


def _long_stream_blocks(i: int, head: int, taps: int, first: int) -> list:
    """The blocks that fall due once ``i`` samples of the row are known (after the step at position i - 1), pure:
    a list of (n, lo, tap0, tap1, out0).  Level n = head, 2*head, 4*head, ... (while n < taps) is due when n divides i: the
    samples [lo, i), lo = max(i - n, first), against the taps [tap0, tap1) = [n, min(2n, taps)) form a full linear
    convolution whose first sample lands on position out0 = lo + n >= i.  Every pair (sample t >= first, tap k >= head)
    is in exactly one block, and that block is due before output t + k is emitted; taps below ``head`` are the step's own,
    samples below ``first`` the prefill's.  The only place the schedule lives."""
    due, n = [], int(head)
    while n < taps and i % n == 0:
        lo = max(i - n, first)
        if lo < i:
            due.append((n, lo, n, min(2 * n, taps), lo + n))
        n *= 2
    return due


def _long_push_bulk_enabled() -> bool:
    """FFTCONV_LONG_PUSH_BULK=0 (read per call): a push runs by windows and the step's own blocks only."""
    return os.environ.get("FFTCONV_LONG_PUSH_BULK", "1") != "0"


def _long_push_plan(p: int, T: int, head: int, taps: int, first: int, bulk: bool = True) -> list:
    """The ops of a push of ``T`` tokens at position ``p``, in order, pure; the only place the push's schedule lives:

      ("window", t, m)                         one ``fc_long_push`` launch over the columns [t, t + m);
      ("block", i, n, lo, tap0, tap1, out0)    one entry of ``_long_stream_blocks(i, ...)``, run as a step runs it;
      ("bulk", i, n, head, min(2n, taps))      the samples [i, i + n) of the chunk against the taps [head, min(2n, taps)),
                                               ONE full linear convolution that lands on the positions from i + head on.

    A bulk is emitted where i is a multiple of ``head`` and ``head < taps``: n is the largest power of two >= 2 head that
    divides i and fits the chunk (it stops doubling once it reaches ``taps``).  Because n divides i, every level <= n was
    due at i for the samples before i, and every block of a higher level that is still open lands at or after i + n: after
    the bulk, ``acc`` is complete on [i, i + n), so ONE window over all n columns follows, and at i + n only the due
    blocks of the levels > n run (the bulk has covered every (sample, tap) pair of the levels <= n).  Everywhere else a
    window runs up to the next multiple of ``head`` (or the end of the chunk), followed by all blocks due there.
    ``bulk=False``: windows and blocks only.  ``first`` is the prefill's and is not moved by a push."""
    ops, i, end = [], int(p), int(p) + int(T)

    def due(at, above):
        return [("block", at) + b for b in _long_stream_blocks(at, head, taps, first) if b[0] > above]

    while i < end:
        if bulk and head < taps and i % (2 * head) == 0 and i + 2 * head <= end:
            n = 2 * head
            while n < taps and i % (2 * n) == 0 and i + 2 * n <= end:
                n *= 2
            ops += [("bulk", i, n, head, min(2 * n, taps)), ("window", i, n)]
            i += n
            ops += due(i, n)
            continue
        m = min(head - i % head, end - i)
        ops.append(("window", i, m))
        i += m
        if i % head == 0:
            ops += due(i, 0)
    return ops


def _long_spec_multiple(p: int, head: int) -> int:
    """M = (p // head + 1) * head: the one multiple of ``head`` that a draft of at most ``head`` tokens at ``p`` can pass."""
    return (int(p) // head + 1) * head


def _long_spec_plan(p: int, T: int, head: int, taps: int, first: int, max_len: int):
    """What a draft of ``T`` <= head tokens at position ``p`` must add to its columns because the blocks inside it have
    not been run, pure -> (M or None, [(n, lo, tap0, tap1), ...]); the only place the draft's schedule lives.

    M = ``_long_spec_multiple(p, head)`` is the one multiple of ``head`` that can lie inside (p, p + T).  If it does not, or if
    M >= max_len (nothing is due there), the answer is (None, []): every column is ``acc`` + the head taps.  Otherwise the
    list holds the entries of ``_long_stream_blocks(M, ...)`` without their out0, and a column t >= M needs

        late(t) = sum over (n, lo, tap0, tap1) and the samples s = lo ... t - n with t - s < tap1 of  w[t - s] * hist[s]

    -- at most t - M + 1 <= T - 1 pairs per level, every s below p (t - n < p because t - p < head <= n): old samples.
    ``fc_long_spec`` derives the same M and levels from (t0, head, kernel, max_len); ``accept`` runs the blocks."""
    M = _long_spec_multiple(p, head)
    if M >= p + T or M >= max_len:
        return None, []
    return M, [(n, lo, tap0, tap1) for n, lo, tap0, tap1, _ in _long_stream_blocks(M, head, taps, first)]


def _long_stream_args(kernel, bias, groups, batch, max_len, head):
    """Argument checks of ``FFTLongConvStream`` (ValueError for shapes, counts and devices, TypeError for dtypes; before any
    device call) -> (cin, cout, taps, head)."""
    if not isinstance(kernel, Tensor):
        raise TypeError(f"`kernel` must be a tensor, got {type(kernel).__name__}")
    if kernel.ndim != 3:
        raise ValueError(f"FFTLongConvStream expects an (out, in/groups, taps) kernel, got shape {tuple(kernel.shape)}")
    if isinstance(groups, bool) or not isinstance(groups, int) or groups < 1:
        raise ValueError(f"groups must be a positive int, got {groups!r}")
    for name, value in (("batch", batch), ("max_len", max_len)):
        if isinstance(value, bool) or not isinstance(value, int) or value < 1:
            raise ValueError(f"{name} must be a positive int, got {value!r}")
    head = LONG_STREAM_HEAD if head is None else head
    if (isinstance(head, bool) or not isinstance(head, int) or head & (head - 1)
            or not _native.LONG_STEP_HEAD_MIN <= head <= _native.LONG_STEP_HEAD_MAX):
        raise ValueError(f"head must be a power of two from {_native.LONG_STEP_HEAD_MIN} to {_native.LONG_STEP_HEAD_MAX}, "
                         f"got {head!r}")
    cout, cig, taps = (int(s) for s in kernel.shape)
    if cout < 1 or cig < 1 or taps < 1 or cout % groups:
        raise ValueError(f"channel mismatch: kernel is {tuple(kernel.shape)} with groups={groups} (need positive sizes and "
                         f"out_channels % groups == 0)")
    if bias is not None and not isinstance(bias, Tensor):
        raise TypeError(f"`bias` must be a tensor or None, got {type(bias).__name__}")
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f"bias must have shape ({cout},), got {tuple(bias.shape)}")
    if kernel.dtype not in _STREAM_DTYPES:
        raise TypeError(f"`kernel` has dtype {kernel.dtype}; a stream takes float32, float16 or bfloat16 tensors")
    if bias is not None and bias.dtype != kernel.dtype:
        raise TypeError(f"`bias` has dtype {bias.dtype} but the kernel is {kernel.dtype}")
    if not kernel.is_cuda:
        raise ValueError(f"`kernel` is on {kernel.device}; a stream lives on a ROCm device (no CPU fallback)")
    if bias is not None and bias.device != kernel.device:
        raise ValueError(f"`bias` is on {bias.device} but the kernel is on {kernel.device}")
    if cig * max_len >= 1 << 29:
        raise NotImplementedError(f"a group's history of {cig} channels x {max_len} positions: the step kernel addresses "
                                  f"fewer than 2**29 samples per group")
    return cig * groups, cout, taps, head


def _long_stream_tensors(xname: str, x, pregate, postgate, xshape: tuple, yshape: tuple, dtype, device):
    """The checks that a step and a chunk share, on the samples ``x`` (called ``xname``) and the optional gates."""
    for name, t, shape in ((xname, x, xshape), ("pregate", pregate, xshape), ("postgate", postgate, yshape)):
        if t is None and name != xname:
            continue
        if not isinstance(t, Tensor):
            raise TypeError(f"`{name}` must be a tensor{'' if name == xname else ' or None'}, got {type(t).__name__}")
        if tuple(t.shape) != shape:
            raise ValueError(f"`{name}` must have shape {shape}, got {tuple(t.shape)}")
        if t.dtype != dtype:
            raise TypeError(f"`{name}` has dtype {t.dtype} but the stream was made for {dtype}")
        if t.device != device:
            raise ValueError(f"`{name}` is on {t.device} but the stream is on {device}")


def _long_step_args(x_t, pregate, postgate, batch: int, cin: int, cout: int, dtype, device):
    """Argument checks of ``FFTLongConvStream.step`` (before any device call), as ``_long_gates`` checks gates: a wrong
    shape or device raises ValueError, a wrong dtype TypeError."""
    _long_stream_tensors("x_t", x_t, pregate, postgate, (batch, cin), (batch, cout), dtype, device)


def _long_push_args(x, pregate, postgate, batch: int, cin: int, cout: int, dtype, device) -> int:
    """Argument checks of ``FFTLongConvStream.push`` (before any device call), as ``_long_step_args`` does it -> T."""
    if not isinstance(x, Tensor):
        raise TypeError(f"`x` must be a tensor, got {type(x).__name__}")
    if x.ndim != 3 or tuple(x.shape[:2]) != (batch, cin) or x.shape[2] < 1:
        raise ValueError(f"`x` must have shape ({batch}, {cin}, T >= 1), got {tuple(x.shape)}")
    count = int(x.shape[2])
    _long_stream_tensors("x", x, pregate, postgate, (batch, cin, count), (batch, cout, count), dtype, device)
    return count


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    """The address of an optional tensor (None: a null pointer)."""
    return None if t is None else t.data_ptr()


class FFTLongConvStream:
    """Token-by-token decoding of a causal long filter: after ``prefill`` and ``step`` calls the outputs, in order, are the
    columns of ``fft_long_conv(z, kernel, bias, groups=groups, causal=True)`` on the row z = pregate * x seen so far, each
    multiplied by its postgate:  y[t] = postgate[t] * (bias + sum_k kernel[k] * z[t - k]).

    ``kernel`` (Cout, Cin/groups, K) and ``bias`` (Cout,) or None are float32, float16 or bfloat16 tensors on a ROCm
    device; the stream keeps float32 copies made at construction (a snapshot: later changes of the weight do not reach
    it).  ``batch`` and ``max_len`` size the state, ``head`` (a power of two 8 ... 1024; None: LONG_STREAM_HEAD) is the
    number of taps a step applies itself.  Inference only: nothing is differentiable, outputs are detached.

    Only the kernel is known in advance, so the convolution is cut into a fixed schedule of power-of-two blocks
    (``_long_stream_blocks``): once i samples are known, every level n = head, 2 head, 4 head, ... < K that divides i
    convolves the last n samples with the taps [n, 2n) -- a full linear convolution through ``fft_long_conv`` (small
    blocks hand off to the ``fft_conv`` kernels), spectra and plans made once at construction -- and adds the result
    to ``acc`` at the positions it reaches.  A step is then ONE launch (``fc_long_step``): it stores z_t, applies the head
    taps to the last ``head`` samples, adds ``acc`` and the bias and applies the gates.  O(L log^2 L) per sequence where
    re-running the causal call per token costs O(L^2 log L).  At positions divisible by a large power of two all levels
    fall due together: the cost is amortised, not flat.

    State (float32 whatever the tensors' dtype): ``hist`` (B, Cin, max_len) holds z, ``acc`` (B, Cout, max_len) the block
    results that have landed on future positions; ``state_bytes`` reports both.  16-bit streams compute what the float32
    stream on the widened tensors computes and round each output once.  The plan and spectrum of a push's bulk level are
    made at the first push that needs them (``bulk_spectrum_bytes``); a stream that never pushes a bulk holds none.

    ``prefill(x)``      x (B, Cin, L0), only at position 0, L0 <= max_len -> y (B, Cout, L0); ungated.
    ``step(x_t, pregate=None, postgate=None)``   x_t, pregate (B, Cin), postgate (B, Cout) -> y_t (B, Cout).
    ``push(x, pregate=None, postgate=None)``     x, pregate (B, Cin, T), postgate (B, Cout, T), at any position -> y
                        (B, Cout, T): the columns T steps would have returned, through the schedule of ``_long_push_plan``
                        (windows of ``fc_long_push``, the step's blocks, and one bulk convolution per aligned run of the
                        chunk; FFTCONV_LONG_PUSH_BULK=0: no bulks).  May be mixed freely with ``step``.
    ``speculate(x, pregate=None, postgate=None)``   shapes as ``push``, 1 <= T <= head -> y (B, Cout, T): the columns
                        ``push`` would return for T DRAFT tokens, in ONE launch (``fc_long_spec``) that leaves ``position``,
                        ``acc`` and ``hist[..., :position]`` alone.  The blocks that would fall due inside the draft (at the
                        one multiple M of ``head`` it can pass; ``_long_spec_plan``) are not run: the kernel adds what they
                        would have put on the columns t >= M as a direct sum over old samples of ``hist`` and the whole
                        filter (the flipped float32 copy the prefill uses; no further copy is kept).  z is stored into
                        ``hist[..., p:p + T]``: columns at or past the position are never read, so rejected ones are
                        dead data that the next call overwrites.  Columns t < M have the bits ``push`` gives them; columns
                        t >= M hold to the same error bound but sum the late pairs in another order than the blocks do.
    ``accept(count)``   commits the first ``count`` (0 ... T, an int; one count for the whole batch) tokens of the pending
                        draft: moves the position and runs the blocks due at M if p < M <= p + count.  No kernel of the
                        step, the push or the draft is launched.  Afterwards ``acc``, ``hist[..., :position]`` and every
                        later output have the bits they would have had after ``push`` of those ``count`` tokens alone:
                        nothing depends on what was speculated.  ``RuntimeError`` without a pending draft.
                        ``step``, ``push``, ``prefill``, ``reset`` and another ``speculate`` drop a pending draft silently,
                        as ``accept(0)`` does.
    ``reset()``         back to position 0.
    Stepping, pushing or speculating past ``max_len`` raises ``RuntimeError``; wrong shapes and devices ``ValueError``, wrong
    dtypes ``TypeError``, before any device call."""

    _draft = None      # (position, tokens) of the draft ``speculate`` left pending, until ``accept`` or any other call drops it

    def __init__(self, kernel: Tensor, bias: Optional[Tensor] = None, groups: int = 1, *, batch: int, max_len: int,
                 head: Optional[int] = None):
        cin, cout, taps, head = _long_stream_args(kernel, bias, groups, batch, max_len, head)
        self.batch, self.in_channels, self.out_channels, self.groups = batch, cin, cout, groups
        self.taps, self.head, self.max_len = taps, head, max_len
        self.dtype, self.device = kernel.dtype, kernel.device
        self._position = self._first = 0
        self._desc = _native.long_step_desc(batch, cin, cout, groups, taps, head, max_len, _DTYPE_CODES[kernel.dtype])
        with torch.no_grad(), torch.cuda.device(self.device):
            wide = kernel.detach().float()
            self._flipped = wide.flip(-1).contiguous()      # the prefill's operand: the whole filter in float32
            self._bias = None if bias is None else bias.detach().float().contiguous().clone()
            self._head_taps = torch.zeros((cout, cin // groups, head), dtype=torch.float32, device=self.device)
            self._head_taps[..., :min(head, taps)] = wide[..., :min(head, taps)]
            self.hist = torch.zeros((batch, cin, max_len), dtype=torch.float32, device=self.device)
            self.acc = torch.zeros((batch, cout, max_len), dtype=torch.float32, device=self.device)
            # one geometry, one plan and one spectrum per level that can fall due inside max_len
            self._levels, n = {}, head
            while n < taps and n < max_len:
                seg = wide[..., n:min(2 * n, taps)].flip(-1).contiguous()
                self._levels[n] = self._level(n, seg)
                n *= 2
        self._bulk_levels = {}      # level n of a push's bulk (``_run_bulk``): made at the first push that needs it

    def _level(self, n: int, seg: Tensor):
        """(flipped taps, padding, plan of the hand-off or None, spectrum) of the full convolution of n samples with ``seg``:
        the non-causal ``fft_long_conv(X, seg, None, padding=len - 1, groups=g)`` on X (B, Cin, n)."""
        pad = int(seg.shape[2]) - 1
        probe = torch.empty((self.batch, self.in_channels, n), dtype=torch.float32, device=self.device)
        pad_left, pad_right, need = _long_geometry(probe, seg, None, pad, self.groups, False)
        route = _long_route_of(n, pad + 1, pad_left, pad_right, need, False, 1, 1, 0, torch.float32, "ncl")
        if route == "handoff":
            plan = _plan_for(probe, seg, None, 1, pad, 1, self.groups, "constant")
            return seg, pad, plan, transform_kernel(plan, seg)
        plan = _long_forward_plan(probe, seg.shape, False, pad_left, pad_right, False, self.groups, 1, 1, 0, route)[0]
        return seg, pad, None, transform_kernel(plan, seg)

    def _full_conv(self, rows: Tensor, level) -> Tensor:
        seg, pad, plan, spectrum = level
        if plan is not None:
            return _fft_conv_impl(rows, seg, None, 1, pad, 1, self.groups, "constant", spectrum, plan)
        return _fft_long_conv_impl(rows, seg, None, pad, self.groups, False, spectrum)

    @property
    def position(self) -> int:
        """Samples of the row seen so far: the position the next ``step`` writes."""
        return self._position

    @property
    def state_bytes(self) -> int:
        """Bytes of ``hist`` and ``acc``."""
        return (self.hist.numel() + self.acc.numel()) * 4

    def reset(self):
        """Back to position 0: the history and the accumulator are cleared, plans and spectra stay."""
        self.hist.zero_()
        self.acc.zero_()
        self._position = self._first = 0
        self._draft = None

    @torch.no_grad()
    def prefill(self, x: Tensor) -> Tensor:
        if not isinstance(x, Tensor):
            raise TypeError(f"`x` must be a tensor, got {type(x).__name__}")
        if x.ndim != 3 or tuple(x.shape[:2]) != (self.batch, self.in_channels) or not 1 <= x.shape[2] <= self.max_len:
            raise ValueError(f"`x` must have shape ({self.batch}, {self.in_channels}, 1 ... max_len = {self.max_len}), got "
                             f"{tuple(x.shape)}")
        if x.dtype != self.dtype:
            raise TypeError(f"`x` has dtype {x.dtype} but the stream was made for {self.dtype}")
        if x.device != self.device:
            raise ValueError(f"`x` is on {x.device} but the stream is on {self.device}")
        if self._position:
            raise RuntimeError(f"prefill is allowed at position 0 only; the stream is at {self._position} (reset() first)")
        self._draft = None
        length = int(x.shape[2])
        rows = x.detach().float().contiguous()
        full = _fft_long_conv_impl(rows, self._flipped, None, self.taps - 1, self.groups, False, None)
        y = full[:, :, :length]
        if self._bias is not None:
            y = y + self._bias.view(1, -1, 1)
        reach = min(self.taps - 1, self.max_len - length)
        if reach > 0:
            self.acc[:, :, length:length + reach] += full[:, :, length:length + reach]
        self.hist[:, :, :length] = rows
        self._position = self._first = length
        return y.to(self.dtype).contiguous()

    def _on_device(self, run, *args):
        """``run(*args)`` with the stream's device current."""
        if torch.cuda.current_device() == _device_index(self.device):      # the common case: no device switch to pay for
            return run(*args)
        with torch.cuda.device(self.device):
            return run(*args)

    def _run_due(self, i: int, above: int = 0):
        """Run the blocks that fall due once ``i`` samples are known, the levels past ``above`` only (a push's bulk has
        covered those up to it).  Nothing is due at ``max_len``."""
        if i < self.max_len:
            for n, lo, _, _, _ in _long_stream_blocks(i, self.head, self.taps, self._first):
                if n > above:
                    self._run_block(i, n, lo)

    @torch.no_grad()
    def step(self, x_t: Tensor, pregate: Optional[Tensor] = None, postgate: Optional[Tensor] = None) -> Tensor:
        _long_step_args(x_t, pregate, postgate, self.batch, self.in_channels, self.out_channels, self.dtype, self.device)
        t = self._position
        if t >= self.max_len:
            raise RuntimeError(f"the stream is at position {t} = max_len: no further step (reset() starts a new row)")
        self._draft = None
        x_t, pregate, postgate = (None if v is None else v.detach().contiguous() for v in (x_t, pregate, postgate))
        y = self._on_device(self._launch_step, x_t, pregate, postgate, t)
        self._position = t + 1
        self._run_due(t + 1)
        return y

    @torch.no_grad()
    def push(self, x: Tensor, pregate: Optional[Tensor] = None, postgate: Optional[Tensor] = None) -> Tensor:
        """Append T tokens at the current position: the T columns that T calls of ``step`` would have returned, in order
        (``_long_push_plan`` has the schedule; a window is ONE launch of ``fc_long_push``)."""
        count = _long_push_args(x, pregate, postgate, self.batch, self.in_channels, self.out_channels, self.dtype, self.device)
        p = self._position
        if p + count > self.max_len:
            raise RuntimeError(f"a push of T = {count} tokens at position {p} passes max_len = {self.max_len} "
                               f"(reset() starts a new row)")
        self._draft = None
        x, pregate, postgate = (None if v is None else v.detach().contiguous() for v in (x, pregate, postgate))
        ops = _long_push_plan(p, count, self.head, self.taps, self._first, _long_push_bulk_enabled())
        y = self._on_device(self._run_push, ops, x, pregate, postgate, p, count)
        self._position = p + count
        return y

    @torch.no_grad()
    def speculate(self, x: Tensor, pregate: Optional[Tensor] = None, postgate: Optional[Tensor] = None) -> Tensor:
        """Verify T <= head draft tokens at the current position: the T columns ``push`` would return, in ONE library
        call (``fc_long_spec``) that does not touch ``acc``.  The position does not move and ``hist`` below it is not
        written; z = pregate * x is stored into ``hist[..., p:p + T]``, columns no kernel and no block reads until the
        position passes them.  The draft (p, T) stays pending until ``accept``; see the class docstring."""
        count = _long_push_args(x, pregate, postgate, self.batch, self.in_channels, self.out_channels, self.dtype, self.device)
        p = self._position
        if count > self.head:
            raise ValueError(f"a draft of T = {count} tokens exceeds head = {self.head}: speculate verifies at most `head` "
                             f"tokens at once (push appends any number)")
        if p + count > self.max_len:
            raise RuntimeError(f"a draft of T = {count} tokens at position p = {p} passes max_len = {self.max_len} "
                               f"(reset() starts a new row)")
        x, pregate, postgate = (None if v is None else v.detach().contiguous() for v in (x, pregate, postgate))
        y = self._on_device(self._launch_spec, x, pregate, postgate, p, count)
        self._draft = (p, count)
        return y

    def _launch_spec(self, x, pregate, postgate, p: int, count: int) -> Tensor:
        y = torch.empty((self.batch, self.out_channels, count), dtype=self.dtype, device=self.device)
        _native.long_spec(self._desc, x.data_ptr(), _ptr(pregate), _ptr(postgate), self._head_taps.data_ptr(),
                          self._flipped.data_ptr(), _ptr(self._bias), self.hist.data_ptr(), self.acc.data_ptr(), y.data_ptr(),
                          p, count, self._first, torch.cuda.current_stream(self.device).cuda_stream)
        return y

    @torch.no_grad()
    def accept(self, count: int) -> None:
        """Commit the first ``count`` tokens of the pending draft (0 ... T; one count for the whole batch): the position
        moves to p + count and, if a multiple M of ``head`` with p < M <= p + count lies below ``max_len``, the blocks due
        at M run from ``hist`` as a step runs them.  No step, push or draft kernel is launched.  ``accept(0)`` only
        clears the draft.  After it the state has the bits a ``push`` of those ``count`` tokens would have left."""
        if self._draft is None:
            raise RuntimeError("accept() without a pending draft: speculate() first (step, push, prefill, reset and another "
                               "speculate drop a draft)")
        p, T = self._draft
        if isinstance(count, bool) or not isinstance(count, int):
            raise TypeError(f"count must be an int, got {type(count).__name__}")
        if not 0 <= count <= T:
            raise ValueError(f"count must lie in [0, T = {T}], got {count}")
        self._draft = None
        self._position = p + count
        M = _long_spec_multiple(p, self.head)
        if M <= p + count:
            self._on_device(self._run_due, M)

    def _run_push(self, ops, x, pregate, postgate, p: int, count: int) -> Tensor:
        y = torch.empty((self.batch, self.out_channels, count), dtype=self.dtype, device=self.device)
        above = 0      # the level of the bulk that the next window follows: the blocks due behind it are the levels above
        for op in ops:
            if op[0] == "bulk":
                self._run_bulk(x, pregate, p, op[1], op[2])
                above = op[2]
            elif op[0] == "window":
                self._push_window(x, pregate, postgate, y, p, op[1], op[2])
                self._run_due(op[1] + op[2], above)      # the plan's "block" ops behind this window, as a step runs them
                above = 0
        return y

    def _push_window(self, x, pregate, postgate, y, p: int, t: int, m: int):
        """One ``fc_long_push`` launch over the columns [t, t + m) of a chunk that began at ``p``.  The call reads chunk
        tensors of row length m: a window that is not the whole chunk runs on contiguous copies of its columns."""
        whole = m == int(x.shape[2])
        cut = lambda v: v if v is None or whole else v[:, :, t - p:t - p + m].contiguous()      # noqa: E731
        xs, pre, post = cut(x), cut(pregate), cut(postgate)
        out = y if whole else torch.empty((self.batch, self.out_channels, m), dtype=self.dtype, device=self.device)
        _native.long_push(self._desc, xs.data_ptr(), _ptr(pre), _ptr(post), self._head_taps.data_ptr(), _ptr(self._bias),
                          self.hist.data_ptr(), self.acc.data_ptr(), out.data_ptr(), t, m, self._first,
                          torch.cuda.current_stream(self.device).cuda_stream)
        if not whole:
            y[:, :, t - p:t - p + m] = out

    def _run_bulk(self, x, pregate, p: int, i: int, n: int):
        """The chunk's samples [i, i + n) against the taps [head, min(2n, taps)): one full convolution added to ``acc`` from
        position i + head on, clipped at ``max_len``.  The level (geometry, plan, spectrum) is made at the first push that
        needs it and kept in ``_bulk_levels``."""
        level = self._bulk_levels.get(n)
        if level is None:
            hi = min(2 * n, self.taps)
            seg = self._flipped[..., self.taps - hi:self.taps - self.head].contiguous()      # the taps [head, hi), flipped
            level = self._bulk_levels[n] = self._level(n, seg)
        rows = x[:, :, i - p:i - p + n].float()
        if pregate is not None:
            rows = rows * pregate[:, :, i - p:i - p + n].float()
        out = self._full_conv(rows.contiguous(), level)
        at = i + self.head
        keep = min(int(out.shape[2]), self.max_len - at)
        self.acc[:, :, at:at + keep] += out[:, :, :keep]

    @property
    def bulk_spectrum_bytes(self) -> int:
        """Bytes of the spectra that pushes have made so far (``_bulk_levels``; none until a push runs a bulk)."""
        return sum(level[3].buf.numel() * level[3].buf.element_size() for level in self._bulk_levels.values())

    def _launch_step(self, x_t, pregate, postgate, t) -> Tensor:
        y = torch.empty((self.batch, self.out_channels), dtype=self.dtype, device=self.device)
        _native.long_step(self._desc, x_t.data_ptr(), _ptr(pregate), _ptr(postgate), self._head_taps.data_ptr(),
                          _ptr(self._bias), self.hist.data_ptr(), self.acc.data_ptr(), y.data_ptr(), t, self._first,
                          torch.cuda.current_stream(self.device).cuda_stream)
        return y

    def _run_block(self, i: int, n: int, lo: int):
        """Level n at i known samples: the full convolution of the samples [i - n, i) -- those below ``lo`` (the
        prefill's) as zeros, so that a level has one geometry -- with the level's taps, added to ``acc`` from position i
        on (the first lo - (i - n) results of a partial block are zero) and clipped at ``max_len``."""
        rows = self.hist[:, :, i - n:i].contiguous()
        if lo > i - n:
            rows[:, :, :lo - (i - n)] = 0.0
        out = self._full_conv(rows, self._levels[n])
        keep = min(int(out.shape[2]), self.max_len - i)
        self.acc[:, :, i:i + keep] += out[:, :, :keep]


# ---------------------------------------------------------------------------------- long transposed filters
LONG_PHASES_MAX_OUT = 1 << 29    # longest output row the phases plan addresses (include/fftconv_amd.h)
LONG_PHASES_MAX_STRIDE = 64       # (stride x transform points stays below 2**30 up to the 2**24-point limit)


def _long_poly_enabled() -> bool:
    """FFTCONV_LONG_POLY=0 (read per call): every long transposed convolution takes the zero-spread route."""
    return os.environ.get("FFTCONV_LONG_POLY", "1") != "0"


def _long_transpose_len(length: int, taps: int, stride: int, padding: int, output_padding: int, dilation: int) -> int:
    return (length - 1) * stride - 2 * padding + dilation * (taps - 1) + output_padding + 1


def _long_spread_args(length: int, taps: int, stride: int, padding: int, output_padding: int, dilation: int):
    """The zero-spread row of a transposed convolution as ``_long_run`` takes it -> (leading signal samples to drop, signal
    samples to read, pad_left, pad_right).  The row is the signal spread over a grid of ``stride`` with d*(K-1) - padding
    zeros in front; a padding wider than the filter cuts into the data, and then the leading (trailing) samples that no
    kept output meets are dropped, as the dX of ``FFTLongConvFunction`` drops them.  Zero samples to read: every output is
    bias alone."""
    lout = _long_transpose_len(length, taps, stride, padding, output_padding, dilation)
    ext = dilation * (taps - 1)
    lead, drop, n = ext - padding, 0, length
    if lead < 0:
        drop = min(n, -(lead // stride))
        lead, n = lead + drop * stride, n - drop
    if n:
        tail = lout + ext - lead - (stride * (n - 1) + 1)
        if tail < 0:
            n, tail = max(0, n - (-tail) // stride), 0
    if n == 0:
        return length, 0, 0, 0
    return drop, n, lead, max(tail, 0)


def _long_transpose_needs(length: int, taps: int, stride: int, padding: int, output_padding: int, dilation: int):
    """(points the zero-spread row needs, points the phases row needs): upper bounds of the cyclic lengths of the two
    plans (the library may still trim taps that meet padding only)."""
    lout = _long_transpose_len(length, taps, stride, padding, output_padding, dilation)
    kp = -(-taps // stride)
    t0 = min(padding // stride, kp - 1)
    t1 = (lout - 1 + padding) // stride
    return lout + dilation * (taps - 1), (t1 - t0 + 1) + kp - 1


def _long_transpose_route(signal_shape, kernel_shape, stride=1, padding=0, output_padding=0, dilation=1, groups=1,
                          dtype=torch.float32, layouts=("ncl", False)) -> str:
    """Which route a ``fft_long_conv_transpose`` call takes (pure: shapes, numbers and FFTCONV_LONG_POLY only):

    ``"handoff"``  a real row whose zero-spread form, Lout + dilation*(K-1) points, fits LONG_HANDOFF_POINTS: the
                   ``fft_conv_transpose`` kernels;
    ``"phases"``   stride >= 2 (at most 64), dilation 1, float32 / float16 / bfloat16, a signal that is not read as
                   channels-last and a contiguous result: ``stride`` ordinary convolutions of the unspread row, interleaved
                   by the store (a row of about L + 2*ceil(K/stride) points);
    ``"spread"``   everything else -- complex64, channels-last tensors, dilation > 1, stride 1, FFTCONV_LONG_POLY=0: the
                   long primitive on the row spread over a grid of ``stride`` (about stride*L + 2*dilation*K points).

    ``layouts``: (``_long_layout`` of the signal, ``channels_last``).  A row that fits neither long route inside 2**24
    points raises ``NotImplementedError`` with the count."""
    length, taps = int(signal_shape[2]), int(kernel_shape[2])
    x_layout, y_nlc = layouts
    spread, phases = _long_transpose_needs(length, taps, stride, padding, output_padding, dilation)
    lout = _long_transpose_len(length, taps, stride, padding, output_padding, dilation)
    if spread <= LONG_HANDOFF_POINTS and dtype != torch.complex64:
        return "handoff"
    if (_long_poly_enabled() and 2 <= stride <= LONG_PHASES_MAX_STRIDE and dilation == 1 and dtype in (torch.float32,) + _LOW_PRECISION
            and x_layout != "nlc" and not y_nlc and phases <= LONG_MAX_POINTS and lout < LONG_PHASES_MAX_OUT):
        return "phases"
    drop, n, lead, tail = _long_spread_args(length, taps, stride, padding, output_padding, dilation)
    need = lout + dilation * (taps - 1) if n else 1
    if need > LONG_MAX_POINTS:
        raise NotImplementedError(f"fft_long_conv_transpose: the row needs a transform of {need} points; the long-filter path "
                                  f"stops at 2**24 = {LONG_MAX_POINTS}")
    return "spread"


def _long_transpose_geometry(signal: Tensor, kernel: Tensor, bias, stride, padding, output_padding, dilation, groups):
    """Argument checks of ``fft_long_conv_transpose`` (ValueError, before any device call) -> (stride, padding,
    output_padding, dilation, output length)."""
    if signal.ndim != 3 or kernel.ndim != 3:
        raise ValueError(f"fft_long_conv_transpose expects a (batch, channels, length) signal and an (in, out/groups, taps) "
                         f"kernel, got shapes {tuple(signal.shape)} and {tuple(kernel.shape)}")
    if not isinstance(groups, int) or isinstance(groups, bool) or groups < 1:
        raise ValueError(f"groups must be a positive int, got {groups!r}")
    stride, dilation = _long_int("stride", stride), _long_int("dilation", dilation)

    def count(name, value):
        if isinstance(value, (tuple, list)) and len(value) == 1:
            value = value[0]
        if isinstance(value, bool) or not isinstance(value, int) or value < 0:
            raise ValueError(f"{name} must be a non-negative int, got {value!r}")
        return int(value)
    padding, output_padding = count("padding", padding), count("output_padding", output_padding)
    if output_padding >= max(stride, dilation):
        raise ValueError(f"output_padding ({output_padding}) must be smaller than either stride ({stride}) or dilation "
                         f"({dilation})")
    cin, length, taps = int(signal.shape[1]), int(signal.shape[2]), int(kernel.shape[2])
    cout = int(kernel.shape[1]) * groups
    if cin % groups or int(kernel.shape[0]) != cin:
        raise ValueError(f"channel mismatch: signal has {cin} channels, transposed kernel is {tuple(kernel.shape)} with "
                         f"groups={groups} (need kernel.shape[0] == in_channels and in_channels % groups == 0)")
    if bias is not None and tuple(bias.shape) != (cout,):
        raise ValueError(f"bias must have shape ({cout},), got {tuple(bias.shape)}")
    if length < 1 or taps < 1 or signal.shape[0] < 1 or kernel.shape[1] < 1:
        raise ValueError("batch, channels, length and taps must be positive")
    lout = _long_transpose_len(length, taps, stride, padding, output_padding, dilation)
    if lout < 1:
        raise ValueError(f"the output length (L-1)*stride - 2*padding + dilation*(K-1) + output_padding + 1 = {lout} must be "
                         f"positive")
    return stride, padding, output_padding, dilation, lout


def _long_phases_plan(signal: Tensor, cout: int, groups: int, taps: int, stride: int, padding: int, output_padding: int,
                      has_bias: bool):
    """Cached phases plan (``fc_long_phases_plan_create``) of a (B, Cin, L) signal; its cache key carries a tag of its own."""
    key = ("long_phases", int(signal.shape[0]), int(signal.shape[1]), int(cout), int(groups), int(signal.shape[2]), int(taps),
           int(stride), int(padding), int(output_padding), int(bool(has_bias)))
    return _cached_plan(_device_index(signal.device), key)


def _long_transposed_weight(kernel: Tensor, groups: int) -> Tensor:
    """The (Cin, Cout/g, K) weight of a transposed convolution as the (Cout, Cin/g, K) weight of the forward convolution on
    the spread row: in and out channels exchanged inside every group, one torch copy of the weight (the taps are flipped by
    the plan)."""
    cin, cog, taps = kernel.shape
    return kernel.detach().contiguous().view(groups, cin // groups, cog, taps).transpose(1, 2).reshape(groups * cog, cin // groups, taps).contiguous()


def _long_transpose_plan(signal: Tensor, kernel: Tensor, has_bias: bool, stride, padding, output_padding, dilation, groups,
                         route: str):
    """(plan, the part of the signal it reads, pad_left, pad_right) of a call on ``route`` ("phases" | "spread"); the
    plan is None where the spread row holds no sample any output meets.  The two paddings are the spread plan's."""
    length, cout, taps = int(signal.shape[2]), int(kernel.shape[1]) * groups, int(kernel.shape[2])
    if route == "phases":
        return _long_phases_plan(signal, cout, groups, taps, stride, padding, output_padding, has_bias), signal, 0, 0
    assert route == "spread", route
    drop, n, lead, tail = _long_spread_args(length, taps, stride, padding, output_padding, dilation)
    if n == 0:
        return None, signal, 0, 0
    sig = signal if (drop, n) == (0, length) else signal[..., drop:drop + n]
    lout = _long_transpose_len(length, taps, stride, padding, output_padding, dilation)
    return _long_plan(sig, cout, groups, taps, lead, tail, True, lout, has_bias, src_up=stride, tap_dil=dilation), sig, lead, tail


def _long_transpose_run(signal: Tensor, kernel: Tensor, bias: Optional[Tensor], stride: int, padding: int, output_padding: int,
                        dilation: int, groups: int, route: str, spectrum: Optional[KernelSpectrum] = None,
                        channels_last: bool = False) -> Tensor:
    """One long transposed convolution on ``route`` ("phases" | "spread"), no autograd.  ``spectrum``: the cached transform
    of the weight for this route's plan (phases: of the weight itself; spread: of ``_long_transposed_weight``)."""
    batch, cout, taps = int(signal.shape[0]), int(kernel.shape[1]) * groups, int(kernel.shape[2])
    lout = _long_transpose_len(int(signal.shape[2]), taps, stride, padding, output_padding, dilation)
    if route == "phases":
        signal = signal.detach().contiguous()
    plan, sig, lead, tail = _long_transpose_plan(signal, kernel, bias is not None, stride, padding, output_padding, dilation,
                                                 groups, route)
    if plan is None:       # padding wider than everything the data reaches: the bias alone
        sig = _resolved(sig.detach())
        out = sig.new_zeros((batch, cout, lout)) if bias is None else \
            _resolved(bias.detach()).to(sig.dtype).view(1, cout, 1).expand(batch, cout, lout).contiguous()
        return _as_channels_last(out) if channels_last else out
    if spectrum is None or spectrum.plan is not plan:
        spectrum = transform_kernel(plan, kernel if route == "phases" else _long_transposed_weight(_resolved(kernel), groups))
    # (the numbers are the spread plan's; a phases plan, whose route has a contiguous signal and result, carries its own)
    return _long_run(sig, None, bias, lead, tail, True, lout, groups, spectrum, src_up=stride, tap_dil=dilation,
                     channels_last=channels_last and route == "spread", weight_shape=(cout, taps), plan=plan)


def fft_long_conv_transpose(signal: Tensor, kernel: Tensor, bias: Tensor = None, stride: int = 1, padding: int = 0,
                            output_padding: int = 0, dilation: int = 1, groups: int = 1, *,
                            channels_last: bool = False) -> Tensor:
    """1-D transposed convolution with a filter as long as the row, equal to ``torch.nn.functional.conv_transpose1d(signal,
    kernel, bias, stride, padding, output_padding, groups, dilation)``: ``signal`` (B, Cin, L), ``kernel`` (Cin, Cout/groups,
    K), ``bias`` (Cout,) or None, on a ROCm device, all three float32, float16, bfloat16 or complex64; the argument order is
    that of ``fft_conv_transpose``.  ``stride`` and ``dilation`` are ints (or 1-tuples) >= 1, ``padding`` >= 0,
    0 <= ``output_padding`` < max(stride, dilation); the output length is (L-1)*stride - 2*padding + dilation*(K-1) +
    output_padding + 1 (``ValueError`` below 1).  Differentiable in signal, kernel and bias.

    Routes (``_long_transpose_route`` names the one a call takes):

    * a real row whose zero-spread form, Lout + dilation*(K-1) points, fits 4096 runs the ``fft_conv_transpose`` kernels
      (complex rows never hand off);
    * stride >= 2 with dilation 1 on float32 / float16 / bfloat16 tensors, a signal that is not read as channels-last and
      a contiguous result runs by PHASES: y[stride*t + p - padding] = sum_j kernel[p + stride*j] * x[t - j] is ``stride``
      ordinary convolutions of the row as it is, so the transform covers about L + 2*ceil(K/stride) points, the input side
      is transformed once for all phases, and the store interleaves them.  The weight is read where it lies: no flipped,
      transposed or phase-split copy exists;
    * everything else -- complex64 tensors, a channels-last signal or result, dilation > 1, stride 1 and every call under
      ``FFTCONV_LONG_POLY=0`` (read per call) -- runs the long primitive on the row spread over a grid of ``stride`` (about
      stride*L + 2*dilation*K points), with one torch copy of the weight (in and out channels exchanged).

    A row that fits neither long route inside 2**24 points raises ``NotImplementedError``.  Leading outputs that see only
    padding and the ``output_padding`` tail come out as the bias, as torch gives them.

    float16 / bfloat16 tensors are read and written by the kernels: float32 arithmetic, one rounding at the store, the bits
    of widening the tensors, running the float32 function and ``.to(dtype)`` -- for the result and for each gradient;
    autograd saves the 16-bit tensors.  ``FFTCONV_HALF_IO=0`` takes that cast path.  complex64: the product is plain
    bilinear (as torch's complex ``conv_transpose1d``), gradients follow PyTorch's convention, lazy conjugates are resolved
    on entry.  ``channels_last`` and a signal that lies as a contiguous (B, L, C) tensor mean what they mean in
    ``fft_long_conv``."""
    return _fft_long_conv_transpose_impl(signal, kernel, bias, stride, padding, output_padding, dilation, groups, None,
                                         channels_last)


def _fft_long_conv_transpose_impl(signal, kernel, bias, stride, padding, output_padding, dilation, groups, spectrum,
                                  channels_last=False):
    """Shared by the functional and ``FFTLongConvTranspose1d`` (``spectrum``: the module's cached one for this call's plan)."""
    stride, padding, output_padding, dilation, lout = _long_transpose_geometry(signal, kernel, bias, stride, padding,
                                                                               output_padding, dilation, groups)
    route = _long_transpose_route(signal.shape, kernel.shape, stride, padding, output_padding, dilation, groups, signal.dtype,
                                  (_long_call_layout(signal, channels_last), channels_last))
    signal, kernel, bias, cast = _long_operands(signal, kernel, bias)
    if cast:      # FFTCONV_HALF_IO=0
        out = _fft_long_conv_transpose_impl(signal.float(), kernel.float(), None if bias is None else bias.float(), stride,
                                            padding, output_padding, dilation, groups, None, channels_last)
        return out.to(signal.dtype)
    if route == "handoff":
        out = _fft_conv_transpose_impl(signal, kernel, bias, stride, padding, output_padding, dilation, groups, None)
        return _as_channels_last(out) if channels_last else out
    if _needs_grad(signal, kernel, bias):
        from .autograd import FFTLongConvTransposeFunction
        return FFTLongConvTransposeFunction.apply(signal, kernel, bias, stride, padding, output_padding, dilation, groups,
                                                  spectrum, channels_last, route)
    return _long_transpose_run(signal, kernel, bias, stride, padding, output_padding, dilation, groups, route, spectrum,
                               channels_last)
