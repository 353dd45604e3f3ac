"""ctypes binding of libfftconv_amd.so (C ABI in include/fftconv_amd.h).

There is deliberately no fallback: if the library is missing or a call fails,
an exception is raised.  The product path never computes on the CPU.
"""
from __future__ import annotations

import collections
import ctypes
import os
import threading
from typing import Optional, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libfftconv_amd.so"
LIB_PATH = os.environ.get("FFTCONV_LIB") or os.path.join(_HERE, LIB_NAME)   # env: A/B builds while tuning

FC_OK, FC_ERR_INVALID, FC_ERR_UNSUPPORTED, FC_ERR_HIP = 0, 1, 2, 3
PAD_MODES = {"constant": 0, "zeros": 0, "reflect": 1, "replicate": 2, "circular": 3}
ABI_VERSION = 7

# words of fc_debug_route after the plan kind, per kind (include/fftconv_amd.h)
ROUTE_KINDS = ("f32_1d", "f32_nd", "f64_direct", "f64_fft_1d", "f64_fft_nd", "f64_fft_long", "c64_nd")
ROUTE_WORDS = {
    "f32_1d": ("T", "ntiles", "pers_nb", "ph", "ph2", "slot_tiles", "nseg", "diag", "bd_gs", "wide", "dense",
               "chunk_launches", "accumulate", "n_ochunks", "pers_items"),
    "f32_nd": ("T", "ntiles", "Tx", "nxt", "Tm", "nyt", "planes", "cob", "accumulate",
               "nseg0", "nseg1", "nseg2", "seg_taps0", "seg_taps1", "seg_taps2"),
    "f64_direct": (),
    "f64_fft_1d": ("T", "ntiles", "cob"),
    "f64_fft_nd": ("t0", "t1", "t2", "nt0", "nt1", "nt2", "nb", "cob"),
    "f64_fft_long": ("N1", "N2", "ntiles", "cob"),
}
ROUTE_WORDS["c64_nd"] = ROUTE_WORDS["f32_nd"]      # a complex64 2-D / 3-D plan: the same words (planes is always 0)


class FcDesc(ctypes.Structure):
    """Mirror of ``struct fc_desc``."""
    _fields_ = [
        ("ndim", ctypes.c_int32), ("dtype", ctypes.c_int32),
        ("batch", ctypes.c_int64), ("in_channels", ctypes.c_int64), ("out_channels", ctypes.c_int64),
        ("groups", ctypes.c_int64),
        ("spatial", ctypes.c_int64 * 3), ("kernel", ctypes.c_int64 * 3), ("stride", ctypes.c_int64 * 3),
        ("padding", ctypes.c_int64 * 3), ("dilation", ctypes.c_int64 * 3),
        ("padding_mode", ctypes.c_int32), ("has_bias", ctypes.c_int32), ("tile_hint", ctypes.c_int32),
        ("transposed", ctypes.c_int32),
        ("output_padding", ctypes.c_int64 * 3),
    ]


class FcLongDesc(ctypes.Structure):
    """Mirror of ``struct fc_long_desc`` (the long-filter plans)."""
    _fields_ = [
        ("batch", ctypes.c_int64), ("in_channels", ctypes.c_int64), ("out_channels", ctypes.c_int64),
        ("groups", ctypes.c_int64), ("length", ctypes.c_int64), ("kernel", ctypes.c_int64),
        ("pad_left", ctypes.c_int64), ("pad_right", ctypes.c_int64), ("out_keep", ctypes.c_int64),
        ("flip", ctypes.c_int32), ("has_bias", ctypes.c_int32),
    ]


class FcLongExt(ctypes.Structure):
    """Mirror of ``struct fc_long_ext`` (padding mode, source spread, tap dilation and output step of a long plan)."""
    _fields_ = [("pad_mode", ctypes.c_int32), ("src_up", ctypes.c_int32), ("tap_dil", ctypes.c_int32),
                ("out_step", ctypes.c_int32)]


class FcLongPhasesDesc(ctypes.Structure):
    """Mirror of ``struct fc_long_phases_desc`` (a transposed convolution run as ``stride`` ordinary ones)."""
    _fields_ = [
        ("batch", ctypes.c_int64), ("in_channels", ctypes.c_int64), ("out_channels", ctypes.c_int64),
        ("groups", ctypes.c_int64), ("length", ctypes.c_int64), ("kernel", ctypes.c_int64),
        ("stride", ctypes.c_int64), ("padding", ctypes.c_int64), ("output_padding", ctypes.c_int64),
        ("has_bias", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


class FcLongDecimDesc(ctypes.Structure):
    """Mirror of ``struct fc_long_decim_desc`` (a strided convolution run on the ``stride`` decimated rows of the signal)."""
    _fields_ = [
        ("batch", ctypes.c_int64), ("in_channels", ctypes.c_int64), ("out_channels", ctypes.c_int64),
        ("groups", ctypes.c_int64), ("length", ctypes.c_int64), ("kernel", ctypes.c_int64),
        ("stride", ctypes.c_int64), ("pad_left", ctypes.c_int64), ("pad_right", ctypes.c_int64),
        ("out_keep", ctypes.c_int64),
        ("flip", ctypes.c_int32), ("has_bias", ctypes.c_int32),
    ]


class FcLongWgradDesc(ctypes.Structure):
    """Mirror of ``struct fc_long_wgrad_desc`` (the weight gradient of the layer a long plan runs)."""
    _fields_ = [
        ("batch", ctypes.c_int64), ("in_channels", ctypes.c_int64), ("out_channels", ctypes.c_int64),
        ("groups", ctypes.c_int64), ("length", ctypes.c_int64), ("kernel", ctypes.c_int64),
        ("pad_left", ctypes.c_int64), ("pad_right", ctypes.c_int64), ("out_len", ctypes.c_int64),
        ("flip", ctypes.c_int32), ("pad_mode", ctypes.c_int32), ("stride", ctypes.c_int32), ("dilation", ctypes.c_int32),
    ]


class FcLongBlocksDesc(ctypes.Structure):
    """Mirror of ``struct fc_long_blocks_desc`` (the plain real row in overlap-save blocks of ``block_points`` points)."""
    _fields_ = [("row", FcLongDesc), ("block_points", ctypes.c_int64)]


class FcLongStepDesc(ctypes.Structure):
    """Mirror of ``struct fc_long_step_desc`` (one decoding step of a causal long filter)."""
    _fields_ = [
        ("batch", ctypes.c_int64), ("in_channels", ctypes.c_int64), ("out_channels", ctypes.c_int64),
        ("groups", ctypes.c_int64), ("kernel", ctypes.c_int64), ("head", ctypes.c_int64), ("max_len", ctypes.c_int64),
        ("dtype", ctypes.c_int32), ("reserved", ctypes.c_int32),
    ]


LONG_EXT_DEFAULT = (0, 1, 1, 1)
FC_C64 = 4                                            # fc_dtype code of complex64 tensors (complex long plans; 2-D / 3-D fc_desc)
# enum fc_long_kind: the rows of a long plan, and what a complex plan reads conjugated
LONG_REAL, LONG_COMPLEX, LONG_CONJ_SIGNAL, LONG_CONJ_TAPS = 0, 1, 2, 4
# enum fc_long_layout: how x and y of fc_long_forward_lay lie, (B, C, L) contiguous or (B, L, C) contiguous
LONG_NCL, LONG_NLC = 0, 1
LONG_NLC_MAX_BYTES = 1 << 31      # one batch item's (L, C) block of a channels-last tensor stays below this
# enum fc_nd_layout: how x and y of fc_forward_lay lie, (B, C, *spatial) contiguous or channels-last (B, *spatial, C)
ND_PLANAR, ND_CHANNELS_LAST = 0, 1
LONG_INFO_WORDS = ("N1", "N2", "out_len", "spectrum_bytes", "workspace_bytes", "slabs", "out_block", "slab_pairs")
# the four words a blocks geometry call fills in besides: kept samples per block, blocks per row, units B * T, unit pairs
LONG_BLOCKS_WORDS = ("V", "T", "U", "pairs")
LONG_BLOCK_MIN, LONG_BLOCK_MAX = 1 << 12, 1 << 24      # block_points: a power of two in this range, 0 = the planner's choice
# ... of a weight-gradient plan: no spectrum; the taps of a row and how many of their lags are transformed
LONG_WGRAD_INFO_WORDS = ("N1", "N2", "taps", "lags", "workspace_bytes", "slabs", "out_block", "slab_pairs")


def _signatures() -> dict:
    vp, sz, i32, ll = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_longlong
    ptr = ctypes.POINTER
    desc, out, i64x8 = ptr(FcDesc), ptr(vp), ptr(ctypes.c_int64 * 8)
    ldesc, lext, wdesc = ptr(FcLongDesc), ptr(FcLongExt), ptr(FcLongWgradDesc)
    bdesc, i64, i64x4 = ptr(FcLongBlocksDesc), ctypes.c_int64, ptr(ctypes.c_int64 * 4)
    return {
        "fc_version": (i32, ()),
        "fc_last_error": (ctypes.c_char_p, ()),
        "fc_plan_create": (i32, (desc, out)),
        "fc_plan_destroy": (None, (vp,)),
        "fc_output_shape": (i32, (vp, ptr(ctypes.c_int64 * 3))),
        "fc_kernel_spectrum_bytes": (sz, (vp,)),
        "fc_workspace_bytes": (sz, (vp,)),
        "fc_plan_tile": (i32, (vp,)),
        "fc_plan_layout": (i32, (vp, ptr(ctypes.c_int32 * 8))),
        "fc_transform_kernel": (i32, (vp, vp, vp, vp, vp)),
        "fc_forward": (i32, (vp, vp, vp, vp, vp, vp, vp)),
        "fc_forward_stamped": (i32, (vp, vp, vp, vp, vp, vp, vp, vp)),
        "fc_wgrad1d_slices": (i32, (desc,)),
        "fc_wgrad1d": (i32, (desc, vp, vp, vp, i32, vp)),
        "fc_wgrad1d_db": (i32, (desc, vp, vp, vp, vp, ll, i32, vp)),
        "fc_wgrad1d_db_supported": (i32, (desc,)),
        "fc_debug_grid": (ll, (vp,)),
        "fc_wgrad_nd_plan_create": (i32, (desc, out)),
        "fc_wgrad_nd": (i32, (vp, vp, vp, vp, vp, vp, vp)),
        "fc_debug_route": (i32, (vp, ptr(ctypes.c_int32 * 16))),
        "fc_long_geometry": (i32, (ldesc, i64x8)),
        "fc_long_plan_create": (i32, (ldesc, out)),
        "fc_long_plan_destroy": (None, (vp,)),
        "fc_long_plan_info": (i32, (vp, i64x8)),
        "fc_long_transform_kernel": (i32, (vp, vp, vp, vp, vp)),
        "fc_long_forward": (i32, (vp, vp, vp, vp, vp, vp, vp)),
        "fc_long_transform_kernel_io": (i32, (vp, vp, i32, vp, vp, vp)),
        "fc_long_forward_io": (i32, (vp, vp, i32, vp, vp, vp, i32, vp, vp)),
        "fc_long_geometry_ext": (i32, (ldesc, lext, i64x8)),
        "fc_long_plan_create_ext": (i32, (ldesc, lext, out)),
        "fc_long_geometry_kind": (i32, (ldesc, lext, i32, i64x8)),
        "fc_long_plan_create_kind": (i32, (ldesc, lext, i32, out)),
        "fc_long_plan_kind": (i32, (vp,)),
        "fc_long_forward_lay": (i32, (vp, vp, i32, i32, vp, vp, vp, i32, i32, vp, vp)),
        "fc_long_phases_geometry": (i32, (ptr(FcLongPhasesDesc), i64x8)),
        "fc_long_phases_plan_create": (i32, (ptr(FcLongPhasesDesc), out)),
        "fc_long_decim_geometry": (i32, (ptr(FcLongDecimDesc), i64x8)),
        "fc_long_decim_plan_create": (i32, (ptr(FcLongDecimDesc), out)),
        "fc_long_wgrad_geometry": (i32, (wdesc, i64x8)),
        "fc_long_wgrad_check_io": (i32, (wdesc, i32, i32, i32, i32, i32)),
        "fc_long_wgrad_plan_create": (i32, (wdesc, out)),
        "fc_long_wgrad_plan_destroy": (None, (vp,)),
        "fc_long_wgrad_plan_info": (i32, (vp, i64x8)),
        "fc_long_wgrad": (i32, (vp, vp, i32, i32, vp, i32, i32, vp, i32, vp, vp)),
        "fc_long_wgrad_gated": (i32, (vp, vp, vp, i32, i32, vp, vp, i32, i32, vp, i32, vp, vp)),
        "fc_long_blocks_geometry": (i32, (bdesc, i64x8, i64x4)),
        "fc_long_blocks_plan_create": (i32, (bdesc, out)),
        "fc_long_wgrad_blocks_geometry": (i32, (wdesc, i64, i64x8, i64x4)),
        "fc_long_wgrad_blocks_plan_create": (i32, (wdesc, i64, out)),
        "fc_plan_takes_layout": (i32, (vp, i32, i32)),
        "fc_forward_lay": (i32, (vp, vp, i32, vp, vp, vp, i32, vp, vp)),
        # (the decoding step; the table's last entry stays the gated forward, which tests pin)
        "fc_long_step": (i32, (ptr(FcLongStepDesc), vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp)),
        "fc_long_push": (i32, (ptr(FcLongStepDesc), vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, vp)),
        "fc_long_spec": (i32, (ptr(FcLongStepDesc), vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, vp)),
        "fc_long_forward_gated": (i32, (vp, vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, vp)),
    }


# every export of include/fftconv_amd.h -> (restype, argtypes); the tests compare both with the header's declarations
SIGNATURES = _signatures()
EXPORTS = tuple(SIGNATURES)


class NativeLibraryMissing(ImportError):
    pass


_lib = None
_lib_lock = threading.Lock()


def load_library() -> ctypes.CDLL:
    """Load libfftconv_amd.so (built in-tree by ``__graft_entry__.build()`` / ``make``)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lib_lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise NativeLibraryMissing(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                f"(or `make -C fft_conv_pytorch_amd/csrc`). There is no CPU fallback.")
        lib = ctypes.CDLL(LIB_PATH)
        for name, (restype, argtypes) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
        if lib.fc_version() != ABI_VERSION:
            raise ImportError(f"{LIB_NAME}: ABI version {lib.fc_version()} != {ABI_VERSION}")
        _lib = lib
    return _lib


def _raise(lib, status: int):
    msg = lib.fc_last_error().decode("utf-8", "replace")
    if status == FC_ERR_INVALID:
        raise ValueError(msg)
    if status == FC_ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(f"libfftconv_amd: {msg}")


def _check(lib, status: int):
    if status != FC_OK:
        _raise(lib, status)


def _refs(args):
    """The arguments of a library call: structs by reference, everything else as it is."""
    return [ctypes.byref(a) if isinstance(a, ctypes.Structure) else a for a in args]


class _Handle:
    """Owns one native handle: ``_open`` creates it, ``_check`` raises what a failed call reports, and the call named
    ``_destroy`` frees it with the Python object."""

    _destroy = "fc_plan_destroy"

    def _open(self, create: str, *args):
        self._lib = load_library()
        handle = ctypes.c_void_p()
        self._check(getattr(self._lib, create)(*_refs(args), ctypes.byref(handle)))
        self._h = handle
        return self._lib, handle

    def _check(self, status: int):
        _check(self._lib, status)

    def __del__(self):
        try:
            if getattr(self, "_h", None):
                getattr(self._lib, self._destroy)(self._h)
                self._h = None
        except Exception:
            pass


def conv_desc(ndim, batch, cin, cout, groups, spatial, kernel, stride, padding, dilation, mode, dtype=0, *,
              has_bias=False, tile_hint=0, transposed=False, output_padding=(0, 0, 0)) -> FcDesc:
    """``struct fc_desc`` of a convolution (the calls that take a descriptor, and ``Plan``; the keywords default to a
    forward convolution without bias).  ``dtype``: the
    fc_dtype code of x and dY for the weight-gradient calls (0 float32, 2 float16, 3 bfloat16; dW stays float32)."""
    d = FcDesc()
    d.ndim, d.dtype = ndim, dtype
    d.batch, d.in_channels, d.out_channels, d.groups = batch, cin, cout, groups
    for i in range(3):
        d.spatial[i] = spatial[i] if i < ndim else 1
        d.kernel[i] = kernel[i] if i < ndim else 1
        d.stride[i] = stride[i] if i < ndim else 1
        d.padding[i] = padding[i] if i < ndim else 0
        d.dilation[i] = dilation[i] if i < ndim else 1
        d.output_padding[i] = output_padding[i] if i < ndim else 0
    d.padding_mode, d.has_bias, d.tile_hint, d.transposed = mode, int(has_bias), tile_hint, int(transposed)
    return d


def wgrad1d_slices(desc: FcDesc) -> int:
    """Partial-result count of ``fc_wgrad1d`` for this shape on the current device; 0 = not covered."""
    return int(load_library().fc_wgrad1d_slices(ctypes.byref(desc)))


def wgrad1d(desc: FcDesc, x_ptr: int, dy_ptr: int, partial_ptr: int, slices: int, stream: int):
    lib = load_library()
    _check(lib, lib.fc_wgrad1d(ctypes.byref(desc), x_ptr, dy_ptr, partial_ptr, slices, stream))


def wgrad1d_db_supported(desc: FcDesc) -> bool:
    return bool(load_library().fc_wgrad1d_db_supported(ctypes.byref(desc)))


def wgrad1d_db(desc: FcDesc, x_ptr: int, dy_ptr: int, partial_ptr: int, db_ptr: Optional[int], slice_stride: int,
               slices: int, stream: int):
    """fc_wgrad1d with the bias gradient folded in: rows [dW | db] of ``slice_stride`` floats per slice."""
    lib = load_library()
    _check(lib, lib.fc_wgrad1d_db(ctypes.byref(desc), x_ptr, dy_ptr, partial_ptr, db_ptr, slice_stride, slices, stream))


class WgradPlan(_Handle):
    """Owns the plan of ``fc_wgrad_nd`` for one convolution descriptor (2-D / 3-D; x and dY float32, float16 or bfloat16
    as the descriptor's dtype says): created on the CURRENT HIP device.  ``run`` reads x (B, Cin, *S) and dY (B, Cout, *Lout)
    and writes a float32 dW (Cout, Cin/g, *k) -- no copies around it."""

    def __init__(self, desc: FcDesc):
        lib, handle = self._open("fc_wgrad_nd_plan_create", desc)
        self.spectrum_bytes = int(lib.fc_kernel_spectrum_bytes(handle))
        self.workspace_bytes = int(lib.fc_workspace_bytes(handle))
        self.tile = int(lib.fc_plan_tile(handle))

    def run(self, x_ptr: int, dy_ptr: int, dw_ptr: int, spectrum_ptr: int, workspace_ptr: Optional[int], stream: int):
        self._check(self._lib.fc_wgrad_nd(self._h, x_ptr, dy_ptr, dw_ptr, spectrum_ptr, workspace_ptr, stream))


def read_route(lib, handle) -> dict:
    """``fc_debug_route`` as a dict: ``kind`` (a ROUTE_KINDS name) and that kind's ROUTE_WORDS (tests)."""
    words = (ctypes.c_int32 * 16)()
    _check(lib, lib.fc_debug_route(handle, ctypes.byref(words)))
    kind = ROUTE_KINDS[words[0]]
    route = {"kind": kind}
    route.update({name: int(words[1 + i]) for i, name in enumerate(ROUTE_WORDS[kind])})
    return route


class Plan(_Handle):
    """Owns one ``fc_plan`` (immutable after creation; shareable between threads and streams).

    The library builds a plan for the HIP device that is current at creation (twiddle tables, work list,
    CU count): create it under ``torch.cuda.device(index)`` and pass that index as ``device_index``."""

    def __init__(self, key: Tuple, device_index: int = 0):
        (ndim, batch, cin, cout, groups, spatial, kernel, stride, padding, dilation, mode, has_bias, tile_hint,
         transposed, output_padding, dtype_code) = key
        lib, handle = self._open("fc_plan_create", conv_desc(
            ndim, batch, cin, cout, groups, spatial, kernel, stride, padding, dilation, mode, dtype_code,
            has_bias=has_bias, tile_hint=tile_hint, transposed=transposed, output_padding=output_padding))
        self.key = key
        self.device_index = int(device_index)
        import torch
        # dtype: of the signal and the output; weight_dtype: of the weight and bias the library reads (a float16 /
        # bfloat16 plan reads and writes 16-bit x / y and takes a float32 weight and bias; a complex64 plan reads and
        # writes complex64 throughout, its spectrum and workspace stay float32 pairs)
        self.dtype = {1: torch.float64, 2: torch.float16, 3: torch.bfloat16, FC_C64: torch.complex64}.get(dtype_code, torch.float32)
        self.weight_dtype = {1: torch.float64, FC_C64: torch.complex64}.get(dtype_code, torch.float32)
        out = (ctypes.c_int64 * 3)()
        lib.fc_output_shape(handle, ctypes.byref(out))
        self.out_spatial = tuple(int(out[i]) for i in range(ndim))
        self.spectrum_bytes = int(lib.fc_kernel_spectrum_bytes(handle))
        self.workspace_bytes = int(lib.fc_workspace_bytes(handle))
        self.tile = int(lib.fc_plan_tile(handle))
        lay = (ctypes.c_int32 * 8)()
        lib.fc_plan_layout(handle, ctypes.byref(lay))
        # what the byte layout of the kernel spectrum depends on besides the descriptor: two plans with
        # equal signatures accept each other's spectra (used by the multi-GPU broadcast)
        self.layout = tuple(int(v) for v in lay)
        self.route = read_route(lib, handle)
        self._stamps = None
        self._takes: dict = {}      # (x_layout, y_layout) -> answer of fc_plan_takes_layout (the plan is immutable)

    def signature(self) -> Tuple:
        """(spectrum bytes, layout words) -- equal on two plans iff a kernel spectrum is interchangeable."""
        return (self.spectrum_bytes,) + self.layout

    def transform_kernel(self, weight_ptr: int, w_hat_ptr: int, workspace_ptr: Optional[int], stream: int):
        self._check(self._lib.fc_transform_kernel(self._h, weight_ptr, w_hat_ptr, workspace_ptr, stream))

    def forward(self, x_ptr: int, w_hat_ptr: int, bias_ptr: Optional[int], y_ptr: int,
                workspace_ptr: Optional[int], stream: int):
        if self._stamps is not None:      # profiling run (scripts/phase_profile.py)
            st = self._lib.fc_forward_stamped(self._h, x_ptr, w_hat_ptr, bias_ptr, y_ptr, workspace_ptr, stream,
                                              self._stamps)
        else:
            st = self._lib.fc_forward(self._h, x_ptr, w_hat_ptr, bias_ptr, y_ptr, workspace_ptr, stream)
        self._check(st)

    def takes_layout(self, x_layout: int, y_layout: int) -> Optional[str]:
        """``fc_plan_takes_layout`` (no device call): None when this plan's launches take x / y in these ``fc_nd_layout``
        layouts, else the library's sentence on why not.  An unknown code raises ``ValueError``."""
        key = (int(x_layout), int(y_layout))
        if key not in self._takes:
            st = self._lib.fc_plan_takes_layout(self._h, *key)
            if st not in (FC_OK, FC_ERR_UNSUPPORTED):
                self._check(st)
            self._takes[key] = None if st == FC_OK else self._lib.fc_last_error().decode("utf-8", "replace")
        return self._takes[key]

    def forward_lay(self, x_ptr: int, w_hat_ptr: int, bias_ptr: Optional[int], y_ptr: int, workspace_ptr: Optional[int],
                    stream: int, x_layout: int = ND_PLANAR, y_layout: int = ND_PLANAR):
        """``forward`` with the layouts of x and y named (``fc_nd_layout``: ND_PLANAR, or ND_CHANNELS_LAST for a tensor that
        lies as a contiguous (B, *spatial, C)).  A plan that does not take a layout: ``NotImplementedError``.  There is no
        stamped launch with layouts (``fc_forward_stamped`` takes none): while a profiling buffer is set
        (``debug_set_stamps``) this raises ``NotImplementedError`` instead of recording nothing."""
        if self._stamps is not None:
            raise NotImplementedError("a stamped (profiling) forward reads and writes contiguous tensors only: unset "
                                      "channels_last / FFTCONV_ND_CL for the profiled call")
        self._check(self._lib.fc_forward_lay(self._h, x_ptr, x_layout, w_hat_ptr, bias_ptr, y_ptr, y_layout, workspace_ptr,
                                             stream))

    def debug_set_stamps(self, ptr: Optional[int]):
        """Profiling hook of this Python handle (the native plan stays immutable): while set, ``forward``
        goes through ``fc_forward_stamped`` with this device buffer."""
        self._stamps = ptr

    def debug_grid(self) -> int:
        return int(self._lib.fc_debug_grid(self._h))


def _struct_of(cls, key: Tuple, words: int, what: str):
    """A descriptor struct filled from a key of ``words`` words in ``_fields_`` order (a field past them stays zero)."""
    if len(key) != words:
        raise ValueError(f"a {what} key has {words} words, got {len(key)}")
    return cls(*(int(v) for v in key))


def _info_words(call: str, names: Tuple, *args) -> dict:
    """The eight info words a geometry or plan-info call fills in, by name."""
    lib = load_library()
    info = (ctypes.c_int64 * 8)()
    _check(lib, getattr(lib, call)(*_refs(args), ctypes.byref(info)))
    return {name: int(info[i]) for i, name in enumerate(names)}


def long_desc(key: Tuple) -> FcLongDesc:
    """``struct fc_long_desc`` of a long-plan key: (batch, cin, cout, groups, L, K, pad_left, pad_right, out_keep, flip,
    has_bias), or those eleven words of an extended key."""
    if len(key) not in (11, 15, 16):
        raise ValueError(f"a long-plan key has 11 words, 15 with (pad_mode, src_up, tap_dil, out_step), or 16 with those and "
                         f"the kind of a complex plan; got {len(key)}")
    return _struct_of(FcLongDesc, key[:11], 11, "long-plan")


def long_ext(key: Tuple) -> FcLongExt:
    """``struct fc_long_ext`` of a long-plan key: words 11 to 14 (pad_mode, src_up, tap_dil, out_step) when it has 15 or
    16, the defaults (constant, 1, 1, 1) when it has 11."""
    return _struct_of(FcLongExt, key[11:15] if len(key) >= 15 else LONG_EXT_DEFAULT, 4, "long-plan extension")


def long_kind(key: Tuple) -> int:
    """``fc_long_kind`` bits of a long-plan key: its sixteenth word (a complex plan always has sixteen), else real."""
    return int(key[15]) if len(key) == 16 else LONG_REAL


def _long_args(key: Tuple):
    return long_desc(key), long_ext(key), long_kind(key)


def long_geometry(key: Tuple) -> dict:
    """``fc_long_geometry``: the info words of the plan this key would get, from the descriptor alone (no device)."""
    return _info_words("fc_long_geometry_kind", LONG_INFO_WORDS, *_long_args(key))


class LongPlan(_Handle):
    """Owns one ``fc_long_plan`` (long-filter path; immutable after creation): created on the CURRENT HIP device, which the
    caller sets to ``device_index``.  Quacks like ``Plan`` where ``KernelSpectrum`` and ``new_workspace`` look.

    The plan does not depend on the element types of real tensors: ``transform_kernel`` and ``forward`` name them per call
    as fc_dtype codes (0 float32, 2 float16, 3 bfloat16; default float32).  Spectrum, workspace and bias are float32.
    A complex plan (a key of 16 words, ``complex`` True) takes code 4, complex64, for every tensor and a complex64 bias."""

    _destroy = "fc_long_plan_destroy"
    _create, _describe = "fc_long_plan_create_kind", staticmethod(_long_args)      # which create call, its descriptor(s)

    def __init__(self, key: Tuple, device_index: int = 0):
        lib, handle = self._open(self._create, *self._describe(key))
        self.key = key
        self.device_index = int(device_index)
        self.info = _info_words("fc_long_plan_info", LONG_INFO_WORDS, handle)
        self.out_len = self.info["out_len"]
        self.spectrum_bytes = self.info["spectrum_bytes"]
        self.workspace_bytes = self.info["workspace_bytes"]
        self.kind = int(lib.fc_long_plan_kind(handle))
        self.complex = bool(self.kind & LONG_COMPLEX)
        import torch
        self.dtype = self.weight_dtype = torch.complex64 if self.complex else torch.float32

    def transform_kernel(self, weight_ptr: int, spectrum_ptr: int, workspace_ptr: int, stream: int,
                         weight_dtype: int = 0):
        self._check(self._lib.fc_long_transform_kernel_io(self._h, weight_ptr, weight_dtype, spectrum_ptr, workspace_ptr,
                                                          stream))

    def forward(self, x_ptr: int, spectrum_ptr: int, bias_ptr: Optional[int], y_ptr: int, workspace_ptr: int, stream: int,
                x_dtype: int = 0, y_dtype: int = 0):
        self._check(self._lib.fc_long_forward_io(self._h, x_ptr, x_dtype, spectrum_ptr, bias_ptr, y_ptr, y_dtype,
                                                 workspace_ptr, stream))

    def forward_lay(self, x_ptr: int, spectrum_ptr: int, bias_ptr: Optional[int], y_ptr: int, workspace_ptr: int,
                    stream: int, x_dtype: int = 0, y_dtype: int = 0, x_layout: int = LONG_NCL, y_layout: int = LONG_NCL):
        """``forward`` with the layouts of x and y named (``fc_long_layout``: LONG_NCL, or LONG_NLC for a tensor that lies
        as a contiguous (B, L, C)).  A channels-last block of 2**31 bytes or more: ``NotImplementedError``."""
        self._check(self._lib.fc_long_forward_lay(self._h, x_ptr, x_dtype, x_layout, spectrum_ptr, bias_ptr, y_ptr, y_dtype,
                                                  y_layout, workspace_ptr, stream))

    def forward_gated(self, x_ptr: int, spectrum_ptr: int, bias_ptr: Optional[int], y_ptr: int, workspace_ptr: int,
                      stream: int, x_dtype: int = 0, y_dtype: int = 0, *, pregate_ptr: Optional[int] = None,
                      gate_ptr: Optional[int] = None, y2_ptr: Optional[int] = None, gate2_ptr: Optional[int] = None,
                      y2_dtype: Optional[int] = None):
        """``forward`` with gates fused into the column passes (``fc_long_forward_gated``): the rows are pregate * x,
        y = gate * c and, where ``y2_ptr`` is given, y2 = gate2 * c for c = conv + bias; an absent gate is all ones.
        (B, C, L) contiguous tensors; ``y2_dtype`` is y's (default) or float32 with no gate2.  A plan the gated builds do
        not take (complex, a non-default ``fc_long_ext``, phases, decimation): ``NotImplementedError``, nothing launched."""
        self._check(self._lib.fc_long_forward_gated(self._h, x_ptr, x_dtype, pregate_ptr, spectrum_ptr, bias_ptr, y_ptr,
                                                    gate_ptr, y2_ptr, gate2_ptr, y_dtype,
                                                    y_dtype if y2_dtype is None else y2_dtype, workspace_ptr, stream))


def phases_desc(key: Tuple) -> FcLongPhasesDesc:
    """``struct fc_long_phases_desc`` of a phases-plan key: (batch, cin, cout, groups, L, K, stride, padding,
    output_padding, has_bias)."""
    return _struct_of(FcLongPhasesDesc, key, 10, "phases-plan")


def phases_geometry(key: Tuple) -> dict:
    """``fc_long_phases_geometry``: the info words of the phases plan this key would get (no device); ``out_len`` is the
    output length of the transposed convolution."""
    return _info_words("fc_long_phases_geometry", LONG_INFO_WORDS, phases_desc(key))


class LongPhasesPlan(LongPlan):
    """A long plan that runs a transposed convolution of dilation 1 as ``stride`` ordinary convolutions of the unspread row
    (``fc_long_phases_plan_create``).  ``transform_kernel`` takes the (Cin, Cout/groups, K) weight where it lies,
    ``forward`` x (B, Cin, L) and y (B, Cout, out_len), contiguous; ``forward_lay`` with LONG_NLC raises
    ``NotImplementedError``."""

    _create, _describe = "fc_long_phases_plan_create", staticmethod(lambda key: (phases_desc(key),))


def decim_desc(key: Tuple) -> FcLongDecimDesc:
    """``struct fc_long_decim_desc`` of a decimation-plan key: (batch, cin, cout, groups, L, K, stride, pad_left, pad_right,
    out_keep, flip, has_bias)."""
    return _struct_of(FcLongDecimDesc, key, 12, "decimation-plan")


def decim_geometry(key: Tuple) -> dict:
    """``fc_long_decim_geometry``: the info words of the decimation plan this key would get (no device)."""
    return _info_words("fc_long_decim_geometry", LONG_INFO_WORDS, decim_desc(key))


class LongDecimPlan(LongPlan):
    """A long plan that runs a strided convolution of dilation 1 on the ``stride`` decimated rows of the signal
    (``fc_long_decim_plan_create``): ``transform_kernel`` takes the (Cout, Cin/groups, K) weight where it lies, ``forward``
    a contiguous x (B, Cin, L); ``forward_lay`` takes LONG_NLC for y only (for x: ``NotImplementedError``)."""

    _create, _describe = "fc_long_decim_plan_create", staticmethod(lambda key: (decim_desc(key),))


def blocks_desc(key: Tuple) -> FcLongBlocksDesc:
    """``struct fc_long_blocks_desc`` of a blocks-plan key: the eleven words of a plain long-plan key, then block_points
    (0: the planner's choice)."""
    if len(key) != 12:
        raise ValueError(f"a blocks-plan key has 12 words, got {len(key)}")
    return FcLongBlocksDesc(long_desc(tuple(key[:11])), int(key[11]))


def _blocks_words(call: str, names: Tuple, *args) -> dict:
    """The eight info words and the four block words (LONG_BLOCKS_WORDS) of a blocks geometry call, by name."""
    lib = load_library()
    info, blocks = (ctypes.c_int64 * 8)(), (ctypes.c_int64 * 4)()
    _check(lib, getattr(lib, call)(*_refs(args), ctypes.byref(info), ctypes.byref(blocks)))
    words = {name: int(info[i]) for i, name in enumerate(names)}
    words.update({name: int(blocks[i]) for i, name in enumerate(LONG_BLOCKS_WORDS)})
    return words


def blocks_geometry(key: Tuple) -> dict:
    """``fc_long_blocks_geometry``: the info words of the blocks plan this key would get and V, T, U, pairs (no device)."""
    return _blocks_words("fc_long_blocks_geometry", LONG_INFO_WORDS, blocks_desc(key))


class LongBlocksPlan(LongPlan):
    """A long plan that runs the plain real primitive (zero padding, stride 1, dilation 1) on a row longer than its
    transform, in overlap-save blocks of ``N1 * N2`` points against one filter spectrum (``fc_long_blocks_plan_create``).
    ``transform_kernel`` takes the (Cout, Cin/groups, K) weight, ``forward`` x (B, Cin, L) and y (B, Cout, out_len),
    contiguous; ``forward_lay`` with LONG_NLC and ``forward_gated`` raise ``NotImplementedError``.  ``blocks``: V, T, U, pairs."""

    _create, _describe = "fc_long_blocks_plan_create", staticmethod(lambda key: (blocks_desc(key),))

    def __init__(self, key: Tuple, device_index: int = 0):
        super().__init__(key, device_index)
        words = blocks_geometry(key)
        self.blocks = {name: words[name] for name in LONG_BLOCKS_WORDS}


def wgrad_desc(key: Tuple) -> FcLongWgradDesc:
    """``struct fc_long_wgrad_desc`` of a weight-gradient key: (batch, cin, cout, groups, L, K, pad_left, pad_right, out_len,
    flip, pad_mode, stride, dilation)."""
    return _struct_of(FcLongWgradDesc, key, 13, "weight-gradient")


def wgrad_geometry(key: Tuple) -> dict:
    """``fc_long_wgrad_geometry``: the info words of the weight-gradient plan this key would get (no device)."""
    return _info_words("fc_long_wgrad_geometry", LONG_WGRAD_INFO_WORDS, wgrad_desc(key))


def wgrad_check_io(key: Tuple, x_dtype: int = 0, x_layout: int = LONG_NCL, dy_dtype: int = 0, dy_layout: int = LONG_NCL,
                   dw_dtype: int = 0):
    """``fc_long_wgrad_check_io``: raises what ``LongWgradPlan.run`` would raise for these element types and layouts, from
    the descriptor alone (no device)."""
    lib = load_library()
    _check(lib, lib.fc_long_wgrad_check_io(ctypes.byref(wgrad_desc(key)), x_dtype, x_layout, dy_dtype, dy_layout, dw_dtype))


class LongWgradPlan(_Handle):
    """Owns one ``fc_long_wgrad_plan`` (immutable after creation; created on the CURRENT HIP device, which the caller sets to
    ``device_index``): dW of the layer a long plan runs, from x and dY where they lie.  Element types (fc_dtype codes 0, 2,
    3) and layouts (LONG_NCL / LONG_NLC) of x and dY and the element type of dW are named per ``run``; the workspace is
    float32.  ``new_workspace`` sizes it by ``workspace_bytes``."""

    _destroy = "fc_long_wgrad_plan_destroy"

    def __init__(self, key: Tuple, device_index: int = 0):
        _, handle = self._open("fc_long_wgrad_plan_create", wgrad_desc(key))
        self.key = key
        self.device_index = int(device_index)
        self.info = _info_words("fc_long_wgrad_plan_info", LONG_WGRAD_INFO_WORDS, handle)
        self.workspace_bytes = self.info["workspace_bytes"]

    def run(self, x_ptr: int, dy_ptr: int, dw_ptr: int, workspace_ptr: int, stream: int, x_dtype: int = 0,
            dy_dtype: int = 0, dw_dtype: int = 0, x_layout: int = LONG_NCL, dy_layout: int = LONG_NCL):
        self._check(self._lib.fc_long_wgrad(self._h, x_ptr, x_dtype, x_layout, dy_ptr, dy_dtype, dy_layout, dw_ptr, dw_dtype,
                                            workspace_ptr, stream))

    def run_gated(self, x_ptr: int, pregate_ptr: Optional[int], dy_ptr: int, postgate_ptr: Optional[int], dw_ptr: int,
                  workspace_ptr: int, stream: int, x_dtype: int = 0, dy_dtype: int = 0, dw_dtype: int = 0,
                  x_layout: int = LONG_NCL, dy_layout: int = LONG_NCL):
        """``run`` on the rows pregate * x and postgate * dY, the gates multiplied in as the two column passes load their
        samples (``fc_long_wgrad_gated``): no product tensor exists.  A gate lies as its tensor does, contiguous (B, C, L)
        in that tensor's dtype; None: all ones, and with both None the call is ``run``.  A pregate on a plan with a padding
        mode or with a channels-last x, a postgate on a strided plan or with a channels-last dY:
        ``NotImplementedError``, nothing launched."""
        self._check(self._lib.fc_long_wgrad_gated(self._h, x_ptr, pregate_ptr, x_dtype, x_layout, dy_ptr, postgate_ptr,
                                                  dy_dtype, dy_layout, dw_ptr, dw_dtype, workspace_ptr, stream))


def wgrad_blocks_geometry(key: Tuple) -> dict:
    """``fc_long_wgrad_blocks_geometry`` of a key of 14 words, a weight-gradient key and block_points: the info words of the
    weight-gradient plan by blocks and V, T, U, pairs (no device)."""
    return _blocks_words("fc_long_wgrad_blocks_geometry", LONG_WGRAD_INFO_WORDS, wgrad_desc(tuple(key[:13])),
                         ctypes.c_int64(int(key[13])))


class LongWgradBlocksPlan(LongWgradPlan):
    """The weight-gradient plan of a layer whose forward runs by blocks (``fc_long_wgrad_blocks_plan_create``; a key of 14
    words: a weight-gradient key with stride 1, dilation 1 and pad_mode constant, then block_points).  ``run`` takes
    contiguous (B, C, L) tensors; ``run_gated`` with a gate and channels-last operands raise ``NotImplementedError``."""

    def __init__(self, key: Tuple, device_index: int = 0):
        if len(key) != 14:
            raise ValueError(f"a weight-gradient key by blocks has 14 words, got {len(key)}")
        _, handle = self._open("fc_long_wgrad_blocks_plan_create", wgrad_desc(tuple(key[:13])), ctypes.c_int64(int(key[13])))
        self.key = key
        self.device_index = int(device_index)
        self.info = _info_words("fc_long_wgrad_plan_info", LONG_WGRAD_INFO_WORDS, handle)
        self.workspace_bytes = self.info["workspace_bytes"]


LONG_STEP_HEAD_MIN, LONG_STEP_HEAD_MAX = 8, 1024      # head of fc_long_step: a power of two in this range


def long_step_desc(batch: int, cin: int, cout: int, groups: int, taps: int, head: int, max_len: int, dtype: int = 0) -> FcLongStepDesc:
    """``struct fc_long_step_desc`` of a stream: made once, passed to every ``long_step``."""
    return FcLongStepDesc(int(batch), int(cin), int(cout), int(groups), int(taps), int(head), int(max_len), int(dtype), 0)


def long_step(desc: FcLongStepDesc, x_ptr: int, pregate_ptr: Optional[int], postgate_ptr: Optional[int], taps_ptr: int,
              bias_ptr: Optional[int], hist_ptr: int, acc_ptr: int, y_ptr: int, t: int, first: int, stream: int):
    """``fc_long_step``: the one launch of a decoding step (the head taps, the gates, the store of column ``t`` of hist)."""
    lib = load_library()
    _check(lib, lib.fc_long_step(ctypes.byref(desc), x_ptr, pregate_ptr, postgate_ptr, taps_ptr, bias_ptr, hist_ptr, acc_ptr,
                                 y_ptr, t, first, stream))


def long_push(desc: FcLongStepDesc, x_ptr: int, pregate_ptr: Optional[int], postgate_ptr: Optional[int], taps_ptr: int,
              bias_ptr: Optional[int], hist_ptr: int, acc_ptr: int, y_ptr: int, t0: int, count: int, first: int, stream: int):
    """``fc_long_push``: ``count`` steps from position ``t0`` in one launch (chunk tensors of row length ``count``)."""
    lib = load_library()
    _check(lib, lib.fc_long_push(ctypes.byref(desc), x_ptr, pregate_ptr, postgate_ptr, taps_ptr, bias_ptr, hist_ptr, acc_ptr,
                                 y_ptr, t0, count, first, stream))


def long_spec(desc: FcLongStepDesc, x_ptr: int, pregate_ptr: Optional[int], postgate_ptr: Optional[int], taps_ptr: int,
              flipped_ptr: int, bias_ptr: Optional[int], hist_ptr: int, acc_ptr: int, y_ptr: int, t0: int, count: int,
              first: int, stream: int):
    """``fc_long_spec``: ``count`` <= head draft columns from position ``t0`` in one launch that only reads ``acc``."""
    lib = load_library()
    _check(lib, lib.fc_long_spec(ctypes.byref(desc), x_ptr, pregate_ptr, postgate_ptr, taps_ptr, flipped_ptr, bias_ptr,
                                 hist_ptr, acc_ptr, y_ptr, t0, count, first, stream))


# the tag of a long-filter key -> the class that owns its plan (forward plans and the weight-gradient plan: one cache)
_PLAN_TAGS = {"long": LongPlan, "long_phases": LongPhasesPlan, "long_decim": LongDecimPlan, "long_wgrad": LongWgradPlan}
# ... of the plans by blocks (a table of their own: the one above is what it was)
_BLOCKS_PLAN_TAGS = {"long_blocks": LongBlocksPlan, "long_wgrad_blocks": LongWgradBlocksPlan}


# Plan cache keyed on (device, descriptor): least-recently-used, bounded -- variable-length inputs would
# otherwise keep one plan (and its device work list) alive per shape ever seen.  An evicted plan is
# destroyed when the last KernelSpectrum / module that still refers to it lets go.
PLAN_CACHE_SIZE = int(os.environ.get("FFTCONV_PLAN_CACHE", "128"))
_plans: "collections.OrderedDict[Tuple, Plan]" = collections.OrderedDict()
_plans_lock = threading.Lock()


def lookup_plan(device_index: int, key: Tuple) -> Optional[Plan]:
    full = (device_index,) + key
    with _plans_lock:
        plan = _plans.get(full)
        if plan is not None:
            _plans.move_to_end(full)
        return plan


def get_plan(device_index: int, key: Tuple) -> Plan:
    """Cached plan for (device, descriptor); creates it on the CURRENT HIP device, which the caller
    must have set to ``device_index`` (``functional._cached_plan`` does)."""
    full = (device_index,) + key
    with _plans_lock:
        plan = _plans.get(full)
        if plan is None:
            # (a long-filter key is tagged: it shares the cache and its bound with the convolution plans)
            cls = (_PLAN_TAGS.get(key[0]) or _BLOCKS_PLAN_TAGS.get(key[0])) if key and isinstance(key[0], str) else None
            plan = cls(key[1:], device_index) if cls is not None else Plan(key, device_index)
            _plans[full] = plan
            while len(_plans) > max(1, PLAN_CACHE_SIZE):
                _plans.popitem(last=False)
        else:
            _plans.move_to_end(full)
    return plan


def clear_plan_cache():
    with _plans_lock:
        _plans.clear()
