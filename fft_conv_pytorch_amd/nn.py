"""Drop-in ``nn.Conv{N}d`` subclasses whose forward runs the HIP FFT convolution.

Mirrors /root/reference/fft_conv_pytorch/nn.py:7-51: constructor, parameters
and ``state_dict`` come unchanged from ``torch.nn.Conv{N}d`` through the MRO;
only ``forward`` differs.  On top of the reference, inference (``eval()`` or a
frozen weight) reuses the transformed kernel per (weight version, input geometry);
see ``_SpectrumCache`` for exactly when.  The 2-D and 3-D modules also run in complex64
(``dtype=torch.complex64`` or ``.to(torch.complex64)``): one complex plan, the same cache.
"""
import os

import torch
from torch import Tensor, nn

from . import functional as F_
from .utils import to_ntuple  # noqa: F401  (the reference's nn.py imports it too)


def _is_parametrized(module: nn.Module) -> bool:
    from torch.nn.utils import parametrize
    return parametrize.is_parametrized(module, "weight")


class _SpectrumCache:
    """Kernel-spectrum cache shared by the forward and the transposed modules.

    The transformed kernel is reused only while that is provably the same weight: the cache is consulted
    when the layer is in ``eval()`` mode, or the weight does not require grad, and the weight is a plain
    (un-parametrized) tensor; it is keyed on the plan, the weight's storage pointer and its version counter.
    A training step therefore always re-transforms (as the reference does on every call,
    /root/reference/fft_conv_pytorch/functional.py:71).  Writes that bypass the version counter
    (``layer.weight.data.copy_(...)``, ``dist.broadcast(layer.weight.data)``) are invisible to any key:
    call ``invalidate_kernel_spectrum()`` after them, or set ``cache_kernel_spectrum = False``."""

    cache_kernel_spectrum = True

    def invalidate_kernel_spectrum(self):
        self.__dict__.pop("_spectrum_cache", None)
        self.__dict__.pop("_bias_cache", None)

    def _cached_spectrum(self, plan, prepare=None):
        """``prepare``: what the plan transforms where that is not the weight itself (a rearranged copy), built only when
        the transform runs."""
        weight = self.weight
        usable = (self.cache_kernel_spectrum and not _is_parametrized(self)
                  and not (self.training and weight.requires_grad and torch.is_grad_enabled()))
        if not usable:
            self.__dict__.pop("_spectrum_cache", None)
            return None
        tag = (id(plan), weight.data_ptr(), weight._version)
        cached = self.__dict__.get("_spectrum_cache")
        if cached is None or cached[0] != tag:
            cached = (tag, F_.transform_kernel(plan, weight if prepare is None else prepare(weight)))
            self.__dict__["_spectrum_cache"] = cached
        return cached[1]

    def _cached_bias(self, plan):
        """The float32 bias (Cout values) a float16 / bfloat16 plan reads, widened once per bias version."""
        bias = self.bias
        if bias is None or bias.dtype == plan.weight_dtype:
            return bias
        tag = (bias.data_ptr(), bias._version)
        cached = self.__dict__.get("_bias_cache")
        if cached is None or cached[0] != tag:
            cached = (tag, bias.detach().to(plan.weight_dtype))
            self.__dict__["_bias_cache"] = cached
        return cached[1]

    # The cached spectrum and the remembered plan hold native handles (ctypes pointers, a loaded library): they are
    # per-process acceleration state, not part of the module.  copy.deepcopy (EMA / AveragedModel, quantization flows),
    # pickle and torch.save(module) therefore see the module WITHOUT them -- exactly what a reference FFTConv module,
    # a plain nn.Conv subclass, carries -- and the copy rebuilds its own on first use.
    _TRANSIENT = ("_spectrum_cache", "_last_plan", "_bias_cache")

    def __getstate__(self):
        state = self.__dict__.copy()
        for key in self._TRANSIENT:
            state.pop(key, None)
        return state

    def __deepcopy__(self, memo):
        import copy
        cls = self.__class__
        clone = cls.__new__(cls)
        memo[id(self)] = clone
        for key, value in self.__dict__.items():
            if key not in self._TRANSIENT:
                clone.__dict__[key] = copy.deepcopy(value, memo)
        return clone

    def _apply(self, fn, *args, **kwargs):       # .to() / .cuda() / .float(): new storage, new spectrum
        self.invalidate_kernel_spectrum()
        self.__dict__.pop("_last_plan", None)
        return super()._apply(fn, *args, **kwargs)


class _FFTConvForward(_SpectrumCache, nn.Module):
    """Shared ``forward`` for FFTConv1d/2d/3d (reference: nn.py:7-22)."""

    channels_last = False      # (the 2-D and 3-D modules take it at construction: _ChannelsLastOption)

    def forward(self, signal: Tensor):
        assert signal.ndim == self.weight.ndim
        padding_mode = "constant" if self.padding_mode == "zeros" else self.padding_mode
        cl = self.channels_last
        if isinstance(self.padding, str) or (signal.dtype not in (torch.float32, torch.float64, torch.complex64)
                                             and not F_._half_native(signal, self.weight, self.bias)):
            # padding='same' / 'valid' (torch stores the string) and half-precision calls the kernels do not read and write
            # in their own dtype (FFTCONV_HALF_IO=0, mixed dtypes): the functional resolves them
            return F_._fft_conv_impl(signal, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                     self.groups, padding_mode, None, channels_last=cl)
        try:
            plan = self._plan(signal, padding_mode)
        except NotImplementedError:
            if signal.dtype not in F_._LOW_PRECISION:
                raise
            # a float16 / bfloat16 shape whose route the library refuses: the functional's cast path
            return F_._fft_conv_impl(signal, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                     self.groups, padding_mode, None, channels_last=cl)
        spectrum = self._cached_spectrum(plan)
        if (spectrum is not None and signal.dtype in F_._LOW_PRECISION      # (no widening kernel per call)
                and not F_._needs_grad(signal, self.weight, self.bias)):
            return F_._forward_lay(signal, spectrum, self._cached_bias(plan), cl)
        return F_._fft_conv_impl(signal, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                 self.groups, padding_mode, spectrum, plan, channels_last=cl)

    def _plan(self, signal: Tensor, padding_mode: str):
        """Plan for this call; the argument validation and descriptor lookup are skipped while the call looks
        exactly like the previous one (same input geometry, devices, dtypes and hyper-parameters)."""
        weight, bias = self.weight, self.bias
        sig = (signal.shape, signal.device, signal.dtype, weight.device, weight.dtype,
               None if bias is None else (bias.device, bias.dtype), self.stride, self.padding, self.dilation,
               self.groups, padding_mode, os.environ.get("FFTCONV_TILE"))
        last = self.__dict__.get("_last_plan")
        if last is not None and last[0] == sig:
            return last[1]
        plan = F_._plan_for(signal, weight, bias, self.stride, self.padding, self.dilation, self.groups, padding_mode)
        self.__dict__["_last_plan"] = (sig, plan)
        return plan


class _FFTConvTransposeForward(_SpectrumCache, nn.Module):
    """Shared ``forward`` for FFTConvTranspose1d/2d/3d (reference: nn.py:25-39)."""

    channels_last = False

    def forward(self, signal: Tensor):
        assert signal.ndim == self.weight.ndim
        cl = self.channels_last
        cast = lambda: F_._fft_conv_transpose_impl(signal, self.weight, self.bias, self.stride, self.padding,  # noqa: E731
                                                   self.output_padding, self.dilation, self.groups, None, None,
                                                   channels_last=cl)
        if signal.dtype in F_._LOW_PRECISION and not F_._half_native(signal, self.weight, self.bias):
            return cast()      # half-precision call the kernels do not read and write natively: the functional casts
        try:
            plan = F_._plan_for(signal, self.weight, self.bias, self.stride, self.padding, self.dilation,
                                self.groups, "constant", transposed=True, output_padding=self.output_padding)
        except NotImplementedError:
            if signal.dtype not in F_._LOW_PRECISION:
                raise
            return cast()      # a float16 / bfloat16 shape whose route the library refuses
        spectrum = self._cached_spectrum(plan)
        if spectrum is not None and signal.dtype in F_._LOW_PRECISION and not F_._needs_grad(signal, self.weight, self.bias):
            return F_._forward_lay(signal, spectrum, self._cached_bias(plan), cl)
        return F_._fft_conv_transpose_impl(signal, self.weight, self.bias, self.stride, self.padding,
                                           self.output_padding, self.dilation, self.groups, spectrum, plan,
                                           channels_last=cl)


class _ChannelsLastOption:
    """``channels_last=True`` (keyword-only at construction; an attribute, shown by ``extra_repr``, not part of the
    state_dict, kept by deepcopy and pickle) of the 2-D and 3-D modules: the result comes back with the strides of a
    contiguous (B, *out, Cout) tensor, as ``fft_conv(..., channels_last=True)`` returns it -- from the cached spectrum too --
    and a signal that lies channels-last is then read where it lies.  A module without it copies such a signal, as ever,
    unless FFTCONV_ND_CL=1 (``functional._nd_cl_native``)."""

    channels_last = False      # (the default of a module pickled before the attribute existed)

    def __init__(self, *args, channels_last=False, **kwargs):
        if not isinstance(channels_last, bool):
            raise ValueError(f"channels_last must be a bool, got {channels_last!r}")
        super().__init__(*args, **kwargs)
        self.channels_last = channels_last

    def extra_repr(self):
        return super().extra_repr() + (", channels_last=True" if self.channels_last else "")


class FFTConv1d(_FFTConvForward, nn.Conv1d):
    ...


class FFTConv2d(_ChannelsLastOption, _FFTConvForward, nn.Conv2d):
    ...


class FFTConv3d(_ChannelsLastOption, _FFTConvForward, nn.Conv3d):
    ...


class FFTConvTranspose1d(_FFTConvTransposeForward, nn.ConvTranspose1d):
    ...


class FFTConvTranspose2d(_ChannelsLastOption, _FFTConvTransposeForward, nn.ConvTranspose2d):
    ...


class FFTConvTranspose3d(_ChannelsLastOption, _FFTConvTransposeForward, nn.ConvTranspose3d):
    ...


class FFTLongConv1d(_SpectrumCache, nn.Conv1d):
    """``nn.Conv1d`` (same parameters and attributes, so state_dict, deepcopy and pickle interchange with ``nn.Conv1d`` and
    ``FFTConv1d``) whose forward is
    ``fft_long_conv``: one transform over the whole padded row, for filters as long as the row.  ``causal=True``
    computes y[j] = sum_k weight[k] * x[stride*j - dilation*k] (output length ceil(L / stride); ``padding`` must be 0 and
    ``padding_mode`` 'zeros').  ``stride``, ``dilation`` and ``padding_mode`` are trailing keyword arguments, stored as
    ``nn.Conv1d`` stores them.  The kernel spectrum is cached
    under the rules of ``_SpectrumCache``, for a float32 module and for one in float16 / bfloat16 (``module.bfloat16()``:
    the kernels read the 16-bit weight and signal and write a 16-bit output; the cached spectrum stays float32) or in
    complex64 (``dtype=torch.complex64`` / ``.to(torch.complex64)``; state_dict interchanges with a complex ``nn.Conv1d``).

    ``channels_last=True`` (keyword-only; an attribute, not part of the state_dict) returns the (B, Cout, nout) result with
    strides (nout*Cout, 1, Cout), as ``fft_long_conv`` does: ``y.transpose(1, 2)`` is then contiguous, ready for the
    ``nn.Linear`` of a sequence model.  A signal that lies that way is read where it lies whatever this says.

    ``blocks`` (keyword-only; an attribute, not part of the state_dict): the ``blocks`` keyword of ``fft_long_conv`` --
    False, True, or the points of one block -- for the ungated forward; the spectrum cached is then that of the blocks
    plan, N bins per filter row however long the signal is.

    ``forward(signal, pregate=None, postgate=None)``: with a gate the forward is ``fft_long_conv_gated`` on the cached
    spectrum, postgate * conv(pregate * signal); without gates it is the call it always was."""

    channels_last = False      # (the default of a module pickled before the attribute existed)
    blocks = False             # (likewise)

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, groups=1, bias=True, causal=False, device=None,
                 dtype=None, *, channels_last=False, blocks=False, stride=1, dilation=1, padding_mode="zeros"):
        if causal and not (isinstance(padding, int) and padding == 0):
            raise ValueError("causal=True pads the row itself: padding must be 0")
        if causal and padding_mode != "zeros":
            raise ValueError("causal=True pads the row itself with zeros: padding_mode must be 'zeros'")
        super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding, dilation=dilation,
                         groups=groups, bias=bias, padding_mode=padding_mode, device=device, dtype=dtype)
        self.causal = bool(causal)
        if not isinstance(channels_last, bool):
            raise ValueError(f"channels_last must be a bool, got {channels_last!r}")
        self.channels_last = channels_last
        self.blocks = F_._long_blocks_arg(blocks)

    def extra_repr(self):
        return (super().extra_repr() + (", causal=True" if self.causal else "")
                + (", channels_last=True" if self.channels_last else "")
                + (f", blocks={self.blocks}" if self.blocks is not False else ""))

    def forward(self, signal: Tensor, pregate: Tensor = None, postgate: Tensor = None):
        padding = self.padding if isinstance(self.padding, str) else int(self.padding[0])
        stride, dilation = int(self.stride[0]), int(self.dilation[0])
        padding_mode = "constant" if self.padding_mode == "zeros" else self.padding_mode
        weight, bias = self.weight, self.bias
        pad_left, pad_right, need = F_._long_geometry(signal, weight, bias, padding, self.groups, self.causal, stride,
                                                      dilation, padding_mode)
        spectrum = None
        cx = signal.dtype == torch.complex64 and (bias is None or bias.dtype == signal.dtype)
        # (a complex row never hands off to fft_conv; a lazily conjugated signal gets a plan of the same key)
        if (signal.is_cuda and weight.is_cuda and signal.device == weight.device and signal.dtype == weight.dtype
                and (signal.dtype == torch.float32 or cx or F_._half_native(signal, weight, bias))):
            mode = F_._native.PAD_MODES[padding_mode]
            gated = pregate is not None or postgate is not None      # (the gated function does not take the keyword)
            layout = F_._long_layout(signal) if F_._long_nlc_enabled() else "ncl"
            points = None
            try:
                if self.blocks is False or gated:
                    route = F_._long_route_of(int(signal.shape[2]), int(weight.shape[2]), pad_left, pad_right, need, self.causal,
                                              stride, dilation, mode, signal.dtype, layout)
                else:
                    route, points = F_._long_blocks_route_of(
                        self.blocks, int(signal.shape[0]), int(signal.shape[1]), int(weight.shape[0]), self.groups,
                        int(signal.shape[2]), int(weight.shape[2]), pad_left, pad_right, need, self.causal, stride, dilation,
                        mode, signal.dtype, layout, self.channels_last)
            except NotImplementedError:
                route = None      # (the functional raises it again, after its own checks)
            if route not in (None, "handoff"):      # the plan the functional will run: every route transforms the weight itself
                plan = F_._long_forward_plan(signal, weight.shape, bias is not None, pad_left, pad_right, self.causal,
                                             self.groups, stride, dilation, mode, route, block_points=points)[0]
                spectrum = self._cached_spectrum(plan)
        if pregate is not None or postgate is not None:      # (the spectrum is that of the ungated call: the gates change no plan)
            return F_._fft_long_conv_gated_impl(signal, weight, bias, padding, self.groups, self.causal, spectrum, pregate,
                                                postgate, stride, dilation, padding_mode, self.channels_last)
        return F_._fft_long_conv_impl(signal, weight, bias, padding, self.groups, self.causal, spectrum, stride, dilation,
                                      padding_mode, self.channels_last, self.blocks)

    def stream(self, batch: int, max_len: int, head=None):
        """A ``FFTLongConvStream`` on this module's weight and bias as they are now (a snapshot), for decoding one token at
        a time: its outputs are the columns of this module's forward on the whole row.  Besides ``step``, ``push`` and
        ``prefill`` the stream verifies up to ``head`` draft tokens without committing them (``speculate``) and then
        commits the accepted ones (``accept``).  Only for a module with
        ``causal=True``, stride 1, dilation 1, padding_mode 'zeros' and ``channels_last=False`` (else ``ValueError``)."""
        if not (self.causal and int(self.stride[0]) == 1 and int(self.dilation[0]) == 1 and self.padding_mode == "zeros"
                and not self.channels_last):
            raise ValueError("stream() decodes a causal row one sample at a time: the module needs causal=True, stride 1, "
                             "dilation 1, padding_mode 'zeros' and channels_last=False")
        return F_.FFTLongConvStream(self.weight, self.bias, self.groups, batch=batch, max_len=max_len, head=head)


class FFTLongConvTranspose1d(_SpectrumCache, nn.ConvTranspose1d):
    """``nn.ConvTranspose1d`` (same parameters and attributes, so state_dict, deepcopy and pickle interchange with
    ``nn.ConvTranspose1d`` and ``FFTConvTranspose1d``) whose forward is ``fft_long_conv_transpose``: one transform over the
    whole row, for filters as long as the row -- by phases where the stride is at least 2 and the dilation 1, on the
    zero-spread row otherwise (the functional's docstring has the routes).  The kernel spectrum of the route's plan is
    cached under the rules of ``_SpectrumCache``, for float32, float16 / bfloat16 and complex64 modules.
    ``forward(signal, output_size=None)`` resolves ``output_size`` to an output padding as ``nn.ConvTranspose1d`` does.

    ``channels_last=True`` (keyword-only; an attribute, not part of the state_dict) returns the result with strides
    (Lout*Cout, 1, Cout), as ``fft_long_conv_transpose`` does."""

    channels_last = False

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, output_padding=0, groups=1, bias=True,
                 dilation=1, padding_mode="zeros", device=None, dtype=None, *, channels_last=False):
        super().__init__(in_channels, out_channels, kernel_size, stride=stride, padding=padding,
                         output_padding=output_padding, groups=groups, bias=bias, dilation=dilation,
                         padding_mode=padding_mode, device=device, dtype=dtype)
        if not isinstance(channels_last, bool):
            raise ValueError(f"channels_last must be a bool, got {channels_last!r}")
        self.channels_last = channels_last

    def extra_repr(self):
        return super().extra_repr() + (", channels_last=True" if self.channels_last else "")

    def forward(self, signal: Tensor, output_size=None):
        stride, padding, dilation = int(self.stride[0]), int(self.padding[0]), int(self.dilation[0])
        if output_size is None:
            output_padding = int(self.output_padding[0])
        else:
            output_padding = int(self._output_padding(signal, output_size, list(self.stride), list(self.padding),
                                                      list(self.kernel_size), 1, list(self.dilation))[0])
        weight, bias = self.weight, self.bias
        stride, padding, output_padding, dilation, _ = F_._long_transpose_geometry(signal, weight, bias, stride, padding,
                                                                                   output_padding, dilation, self.groups)
        spectrum = None
        cx = signal.dtype == torch.complex64 and (bias is None or bias.dtype == signal.dtype)
        if (signal.is_cuda and weight.is_cuda and signal.device == weight.device and signal.dtype == weight.dtype
                and (signal.dtype == torch.float32 or cx or F_._half_native(signal, weight, bias))):
            layouts = (F_._long_layout(signal) if F_._long_nlc_enabled() else "ncl", self.channels_last)
            route = F_._long_transpose_route(signal.shape, weight.shape, stride, padding, output_padding, dilation,
                                             self.groups, signal.dtype, layouts)
            if route != "handoff":
                plan = F_._long_transpose_plan(signal, weight, bias is not None, stride, padding, output_padding, dilation,
                                               self.groups, route)[0]
                if plan is not None:
                    prepare = None if route == "phases" else (lambda w: F_._long_transposed_weight(F_._resolved(w), self.groups))
                    spectrum = self._cached_spectrum(plan, prepare)
        return F_._fft_long_conv_transpose_impl(signal, weight, bias, stride, padding, output_padding, dilation, self.groups,
                                                spectrum, self.channels_last)
