"""The cross-feature sweep of the long-filter family (``fft_long_conv``, ``fft_long_conv_transpose`` and their modules):
a seeded table of cases that crosses the axes the family grew by, the exact truth and the float32 baseline of every case,
and the run with its checks.  tests/test_host_long_sweep.py holds the table to its conditions on the CPU,
tests/test_gpu_long_sweep.py and scripts/long_sweep_extended.py run it.  Nothing here touches a GPU or the library at import.

The table.  ``tables(seed)`` -> (forward cases, transposed cases), frozen ``Case`` records.  An AXIS is a named list of
values (``FWD_AXES`` / ``TR_AXES``); a case is one value per axis (``Case.pick``) made concrete: L, K and the padding are
drawn so that the row the call needs lands in the case's ``row`` class -- "short" (at most 4096 points: a real row hands
off to ``fft_conv``, a complex one stays on the long path at 64 x 64), "mid" (4097 ... 8192) or "big" (8193 ... 16384).
A combination the API refuses by contract is discarded by asking ``_long_geometry`` / ``_long_transpose_geometry`` on meta
tensors; no exception of a call under test is ever caught.  ``allowed_pairs`` computes, by the same rule, which two values
of two axes can occur together.  Cases are chosen greedily (the candidate that covers the most pairs not yet covered, with a
bonus for a route, slab count, forced N1 x N2 or trimmed geometry whose quota is still open), so that every allowed pair
occurs in each table by itself; the choice goes on past ``COUNTS`` until it does (seven forced-N values against five
paddings alone need 35 cases).  The ``trim`` class of a forward case (which taps long_geometry drops: "khi", "klo", or
all of them, "bias") steers the draw and has quotas but is no axis of the coverage.  Case i takes gradients when i is
even, goes through the module when i % 8 is 0 or 5, and draws the "offset" input class when i % 3 is 0.

Truth and baseline.  Inputs are ``accuracy_util.integers`` (float16: divided by 4 towards zero, offset 16, so that the
exact result stays below 65504).  ``conv`` is the model project's FFT formulation of a case with the long arguments
(separate left / right padding, causal) in the tensors' own precision: in float64 on integers, rounded by
``accuracy_util.whole``, it is the exact truth; in float32 / complex64 it is the baseline.  Its padding is written
as slices (``pad``) so that the baseline's gradients are the same in every run.  ``check_values`` is
``accuracy_util.check`` at its default margins on y, dX, dW and db.  A float16 / bfloat16 case is held to that bound
through its float32 twin (the call on the widened tensors, whose bits it must have after ``.to(dtype)``): the rounding of
a 16-bit result alone is 2**-9, far above any bound against a float32 baseline."""
import dataclasses
import functools
import random

import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import FFTLongConv1d, FFTLongConvTranspose1d, _native, autograd
from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests import guard_util as gu

SEED = 1
KNOBS = {"decim": "FFTCONV_LONG_DECIM", "wgrad": "FFTCONV_LONG_WGRAD", "poly": "FFTCONV_LONG_POLY", "nlc": "FFTCONV_LONG_NLC",
         "half": "FFTCONV_HALF_IO", "longn": "FFTCONV_LONG_N", "ws": "FFTCONV_LONG_WS_MB"}
ALL_KNOBS = tuple(KNOBS.values()) + ("FFTCONV_TILE",)
FORCED_N = ("64x64", "64x128", "128x64", "64x256", "128x128", "256x64")      # every tile pair with N <= 16384
DTYPES = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16, "c64": torch.complex64}
HALF = (torch.float16, torch.bfloat16)
ROW = {"short": (1100, 4096), "mid": (4097, 8192), "big": (8193, 16384)}
MODES = ("constant", "reflect", "replicate", "circular")
DEFAULT_BUDGET_MB = 8192          # kDefaultBudgetMB of csrc/host_long.cpp
F16_DIV, F16_OFFSET = 4, 16
F16_MAX = 65504.0

_SHARED = {
    "B": (1, 2, 3, 5), "groups": (1, 2, "dw"), "cig": (1, 2, 3), "cog": (1, 2, 3, 5), "row": ("short", "mid", "big"),
    "stride": (1, 2, 3, 7), "dilation": (1, 2, 3), "bias": (False, True), "channels_last": (False, True),
    "dtype": ("f32", "f16", "bf16", "c64"), "layout": ("ncl", "nlc0", "nlc_off", "copy"), "dy": ("none", "ncl", "nlc"),
    "grads": (False, True), "module": (False, True), "cls": ("centred", "offset"),
    "decim": (None, "0", "1"), "poly": (None, "0"), "nlc": (None, "0"), "half": (None, "0"),
    "longn": (None,) + FORCED_N, "ws": (None, "1"),
}
FWD_AXES = dict(_SHARED, kclass=("few", "mid", "row"), trim=("none", "khi", "klo", "bias"),
                padding=("0", "odd", "same", "valid", "max"), mode=MODES, causal=(False, True), wgrad=(None, "1"))
TR_AXES = dict(_SHARED, kclass=("few", "mid"), padding=("0", "below", "above"), opad=("0", "1", "top"))
AXES = {"fwd": FWD_AXES, "tr": TR_AXES}
CANDIDATES = 200
COUNTS = {"fwd": 48, "tr": 24}          # about: the greedy choice goes on until every allowed pair is covered


@dataclasses.dataclass(frozen=True)
class Case:
    kind: str                 # "fwd" (fft_long_conv) | "tr" (fft_long_conv_transpose)
    idx: int
    seed: int
    pick: tuple               # ((axis, value), ...): what the pair coverage counts
    B: int
    groups: int
    cig: int                  # fwd: Cin/g; tr: Cin/g as well (the weight is (Cin, Cout/g, K))
    cog: int
    L: int
    K: int
    padding: object           # int | 'same' | 'valid'
    mode: str
    stride: int
    dilation: int
    causal: bool
    opad: int
    bias: bool
    channels_last: bool
    dtype: str
    layout: str
    dy: str
    grads: bool
    module: bool
    cls: str
    env: tuple                # ((variable, value), ...) of the switches that are set
    pl: int                   # fwd: pad_left / pad_right of _long_geometry; tr: the padding twice
    pr: int
    rowlen: int               # points the call needs as the Python layer counts them (the hand-off threshold)
    nout: int
    route: str                # the forward route the generator expects
    n1n2: tuple               # N1, N2 of the forward plan (None: hand-off or no plan)
    slabs: int                # ... and its slab count (0: no plan)
    slab_pairs: int
    klo: int                  # fwd: the taps long_geometry keeps
    khi: int
    drop: int                 # tr: leading samples _long_spread_args drops
    needs: tuple              # points of the plain plans of forward, dX and dW (what a forced N1 x N2 must hold)

    @property
    def cin(self):
        return self.groups * self.cig

    @property
    def cout(self):
        return self.groups * self.cog

    @property
    def id(self):
        sw = "".join(f"-{k}{v}" for k, v in ((k, dict(self.pick)[k]) for k in KNOBS if k in dict(self.pick)) if v is not None)
        tag = "F" if self.kind == "fwd" else "T"
        pad = self.padding if isinstance(self.padding, str) else f"p{self.padding}"
        tail = ("c" if self.causal else "") + ("b" if self.bias else "") + ("l" if self.channels_last else "") + \
               ("g" if self.grads else "") + ("m" if self.module else "") + (f"o{self.opad}" if self.kind == "tr" else "")
        return (f"{tag}{self.idx:02d}-{self.dtype}-B{self.B}g{self.groups}i{self.cig}o{self.cog}-L{self.L}K{self.K}-{pad}"
                f"{self.mode[:4]}-s{self.stride}d{self.dilation}-{self.layout}{'' if self.dy == 'none' else '/' + self.dy}-{tail}{sw}")

    @property
    def tdtype(self):
        return DTYPES[self.dtype]

    @property
    def complex(self):
        return self.dtype == "c64"

    @property
    def wshape(self):
        return (self.cout, self.cig, self.K) if self.kind == "fwd" else (self.cin, self.cog, self.K)

    @property
    def forced(self):
        n = dict(self.env).get(KNOBS["longn"])
        return tuple(int(v) for v in n.split("x")) if n else None


# ------------------------------------------------------------------------------------------------ geometry, restated
def geom(L, K, pl, pr, keep, mode, up, dil, step):
    """long_geometry of csrc/host_long.cpp for a valid descriptor -> (nout, klo, khi, points the transform needs)."""
    span = up * (L - 1) + 1
    full = (span + pl + pr - dil * (K - 1) - 1) // step + 1
    nout = keep or full
    klo, khi = 0, K - 1
    if mode == 0:
        lo = pl - step * (nout - 1)
        klo = -(-lo // dil) if lo > 0 else 0
        khi = min(K - 1, (pl + span - 1) // dil)
    keff = 1 if khi < klo else khi - klo + 1
    return nout, klo, khi, step * (nout - 1) + dil * (keff - 1) + 1


def plan_size(need, batch, cin, cout, cx, forced, ws):
    """N1, N2, slabs and slab_pairs of a long plan of ``need`` points (FFTCONV_LONG_N ``forced``, FFTCONV_LONG_WS_MB ``ws``)."""
    if forced:
        n1, n2 = forced
    else:
        lg = max(12, (need - 1).bit_length())
        n1, n2 = 1 << (lg // 2), 1 << (lg - lg // 2)
    npairs = batch if cx else (batch + 1) // 2
    budget = (int(ws) if ws else DEFAULT_BUDGET_MB) << 20
    slab_pairs = max(1, min(npairs, budget // ((cin + cout) * n1 * n2 * 8)))
    return (n1, n2), -(-npairs // slab_pairs), slab_pairs


def dx_rows(c):
    """(samples of dY the dX run of FFTLongConvFunction.backward reads, lead, tail, keep); 0 samples: dX is zeros."""
    ext, s = c.dilation * (c.K - 1), c.stride
    keep, lead = (c.L, ext - c.pl) if c.mode == "constant" else (c.L + c.pl + c.pr, ext)
    n = c.nout
    if lead < 0:
        drop = -(lead // s)
        n, lead = max(0, n - drop), lead + drop * s
    tail = keep + ext - lead - (s * (n - 1) + 1)
    if tail < 0 and n:
        n, tail = max(0, n - (-tail) // s), 0
    return n, lead, max(tail, 0), keep


def _meta(*shape):
    return torch.empty(shape, device="meta")


def _layout_strides(layout, B, C, L):
    """(storage elements, storage offset, strides) of a (B, C, L) signal in ``layout``."""
    if layout == "ncl":
        return B * C * L, 0, (C * L, L, 1)
    if layout in ("nlc0", "nlc_off"):
        off = 3 if layout == "nlc_off" else 0
        return B * C * L + off, off, (L * C, 1, C)
    return B * C * (L + 5), 2, (C * (L + 5), L + 5, 1)        # "copy": the time slice [2, 2 + L) of rows of L + 5


def place(t, layout, device):
    """``t`` (contiguous (B, C, L)) on ``device`` in ``layout``."""
    n, off, strides = _layout_strides(layout, *t.shape)
    out = torch.zeros(n, dtype=t.dtype, device=device).as_strided(tuple(t.shape), strides, off)
    out.copy_(t)
    return out


def _seen_layout(layout, B, C, L):
    n, off, strides = _layout_strides(layout, B, C, L)
    return F_._long_layout(torch.empty(n, device="meta").as_strided((B, C, L), strides, off))


# ------------------------------------------------------------------------------------------------ generator
def _repair(kind, p, fixed):
    """Pull the axes that are not ``fixed`` towards what the others imply (the rejection rule decides afterwards)."""
    def put(a, v):
        if a not in fixed:
            p[a] = v
    if kind == "fwd":
        if p["trim"] == "bias":
            for a, v in (("mode", "constant"), ("padding", "max"), ("causal", False), ("kclass", "mid")):
                put(a, v)
            if p["dilation"] == 1:
                put("dilation", 2)
            if p["dilation"] == 2:
                put("layout", "ncl" if p["layout"] != "copy" else "copy")
        if p["trim"] == "klo":
            for a, v in (("mode", "constant"), ("padding", "max"), ("causal", False), ("kclass", "mid")):
                put(a, v)
        if p["kclass"] == "row":
            put("causal", True)
        if p["trim"] == "khi" and p["padding"] != "max":
            put("kclass", "row")
            put("causal", True)
        if p["causal"]:
            put("padding", "0")
            put("mode", "constant")
            if p["trim"] in ("klo", "bias"):
                put("trim", "none")
        elif p["kclass"] == "row":
            put("kclass", "mid")
        if p["padding"] == "same":
            put("stride", 1)
    if p["groups"] == "dw":
        put("cig", 1)
    if p["longn"] == "64x64":
        put("row", "short")
    elif p["longn"] in ("64x128", "128x64") and p["row"] == "big":
        put("row", "mid")
    if not p["grads"]:
        put("dy", "none")
    elif p["dy"] == "none":
        put("dy", "ncl")
    if p["dy"] != "none":
        put("grads", True)
    cin = (3 if p["groups"] == "dw" else p["groups"]) * p["cig"]
    if cin == 1 and p["layout"] in ("nlc0", "nlc_off"):
        put("groups", 2)
    if p["dy"] == "nlc" and p["groups"] == 1 and p["cog"] == 1:
        put("cog", 2)


def _draw_fwd(p, rng):
    """L, K and the padding of a forward pick, aimed at its row class -> (L, K, padding) or None."""
    d, target = p["dilation"], rng.randint(*ROW[p["row"]])
    if p["trim"] in ("bias", "klo") and (p["padding"], p["mode"], p["causal"]) != ("max", "constant", False):
        return None
    if p["causal"] and p["padding"] != "0":
        return None          # (the call would be refused: causal pads the row itself)
    if p["trim"] == "bias":
        # L = d - 1 samples at positions = 1 ... d - 1 (mod d), one output: no tap of the dilated filter meets them
        K = ((target - 1) // d + 1) & ~1
        return (d - 1, K, d * (K - 2) // 2 + 1) if d > 1 and K >= 4 else None
    if p["trim"] == "klo":
        L = target // 3
        return L, rng.randint(2 * L + L // 4, 3 * L - L // 4) // d + 1, L
    if p["causal"]:
        if p["kclass"] == "row":
            L = target // 2 + 1
            return L, rng.randint(L, L + L // 3), 0
        K = rng.randint(3, 17) if p["kclass"] == "few" else rng.randint(target // 8, target // 2) // d + 1
        return target - d * (K - 1), K, 0
    K = rng.randint(3, 17) if p["kclass"] == "few" else rng.randint(target // 8, target // 2) // d + 1
    pk, ext = p["padding"], d * (K - 1)
    if pk in ("0", "valid"):
        return target, K, 0 if pk == "0" else "valid"
    if pk == "odd":
        pd = rng.choice((1, 3, 5, 17, 37))
        return target - 2 * pd, K, pd
    if pk == "same":
        return target - ext, K, "same"
    L = (target + 2) // 3 if p["mode"] == "reflect" else target // 3
    if p["trim"] == "khi":      # a filter longer than the data and one padding
        K = rng.randint(2 * L + L // 8, 3 * L - L // 8) // d + 1
    return L, K, L - 1 if p["mode"] == "reflect" else L


def _realise_fwd(p, rng, idx, seed):
    drawn = _draw_fwd(p, rng)
    if drawn is None:
        return None
    L, K, padding = drawn
    if (p["groups"] == "dw" and p["cig"] != 1) or (p["dy"] == "none") != (not p["grads"]):
        return None          # (depthwise: groups = Cin; dY lies somewhere exactly when gradients are taken)
    g = 3 if p["groups"] == "dw" else p["groups"]
    cin, cout, s, d = g * p["cig"], g * p["cog"], p["stride"], p["dilation"]
    if L < 1 or K < 1:
        return None
    try:      # the API's own rejection rule, on meta tensors
        pl, pr, rowlen = F_._long_geometry(_meta(p["B"], cin, L), _meta(cout, p["cig"], K), None, padding, g, p["causal"], s, d,
                                           p["mode"])
    except ValueError:
        return None
    mode = _native.PAD_MODES[p["mode"]]
    keep = F_._long_keep(L, p["causal"], s)
    nout, klo, khi, need = geom(L, K, pl, pr, keep, mode, 1, d, s)
    p = dict(p, row=next((k for k, (lo, hi) in ROW.items() if lo <= rowlen <= hi), None),
             trim="bias" if khi < klo else "klo" if klo > 0 else "khi" if khi < K - 1 else "none",
             kclass="row" if p["causal"] and K >= L else "few" if K <= 17 else "mid")
    if p["row"] is None:
        return None
    dt = DTYPES[p["dtype"]]
    cx = dt == torch.complex64
    nlc_on = p["nlc"] is None
    seen = _seen_layout(p["layout"], p["B"], cin, L)
    if seen != {"ncl": "ncl", "nlc0": "nlc", "nlc_off": "nlc", "copy": "copy"}[p["layout"]]:
        return None          # (one channel or one sample: the strides say nothing)
    if p["dy"] == "nlc" and (cout == 1 or nout == 1):
        return None
    xl = seen if nlc_on else "ncl"
    if rowlen <= F_.LONG_HANDOFF_POINTS and not cx:
        route = "handoff"
    elif p["decim"] == "1" and F_._long_decim_eligible(L, K, s, pl, pr, keep, d, mode, dt, xl):
        route = "phases"
    else:
        route = "plain"
    case = Case("fwd", idx, seed, (), p["B"], g, p["cig"], p["cog"], L, K, padding, p["mode"], s, d, p["causal"], 0, p["bias"],
                p["channels_last"], p["dtype"], p["layout"], p["dy"], p["grads"], p["module"], p["cls"],
                tuple((KNOBS[k], p[k]) for k in KNOBS if p.get(k) is not None), pl, pr, rowlen, nout, route, None, 0, 0,
                klo, khi, 0, ())
    needs = [need]
    if p["grads"]:
        n, lead, tail, dkeep = dx_rows(case)
        if n:
            needs.append(geom(n, K, lead, tail, dkeep, 0, s, d, 1)[3])
        needs.append(geom(L, nout, pl, pr, K, mode, 1, s, d)[3])
    forced = case.forced
    if route != "handoff" and forced and forced[0] * forced[1] < max(needs):
        return None
    n1n2, slabs, slab_pairs = None, 0, 0
    if route == "plain":
        n1n2, slabs, slab_pairs = plan_size(need, p["B"], cin, cout, cx, forced, p["ws"])
    elif route == "phases":
        n1n2, slabs, slab_pairs = plan_size(nout + -(-K // s) - 1, p["B"], cin * s, cout, False, forced, p["ws"])
    return dataclasses.replace(case, pick=tuple(p.items()), n1n2=n1n2, slabs=slabs, slab_pairs=slab_pairs, needs=tuple(needs))


def _realise_tr(p, rng, idx, seed):
    if (p["groups"] == "dw" and p["cig"] != 1) or (p["dy"] == "none") != (not p["grads"]):
        return None          # (depthwise: groups = Cin; dY lies somewhere exactly when gradients are taken)
    g = 3 if p["groups"] == "dw" else p["groups"]
    cin, cout, s, d = g * p["cig"], g * p["cog"], p["stride"], p["dilation"]
    target = rng.randint(*ROW[p["row"]])
    K = rng.randint(3, 17) if p["kclass"] == "few" else rng.randint(target // 8, target // 3) // d + 1
    ext = d * (K - 1)
    top = max(s, d) - 1
    op = {"0": 0, "1": 1, "top": top}[p["opad"]]
    if p["opad"] == "1" and top < 1 or p["opad"] == "top" and top < 2:
        return None          # (the value is another one's at this stride and dilation)
    if p["padding"] == "0":
        pad = 0
    elif p["padding"] == "below":
        pad = min(ext - 1, rng.choice((1, 3, 5, 17, 37)))
        if pad < 1:
            return None
    else:
        pad = ext + s * rng.randint(1, 5) + rng.randint(0, s)
    L = (target + 2 * pad - 2 * ext - op - 1) // s + 1
    if L < 2:
        return None
    try:
        _, _, _, _, lout = F_._long_transpose_geometry(_meta(p["B"], cin, L), _meta(cin, p["cog"], K), None, s, pad, op, d, g)
    except ValueError:
        return None
    rowlen = lout + ext
    p = dict(p, row=next((k for k, (lo, hi) in ROW.items() if lo <= rowlen <= hi), None))
    if p["row"] is None:
        return None
    dt = DTYPES[p["dtype"]]
    cx = dt == torch.complex64
    seen = _seen_layout(p["layout"], p["B"], cin, L)
    if seen != {"ncl": "ncl", "nlc0": "nlc", "nlc_off": "nlc", "copy": "copy"}[p["layout"]]:
        return None
    if p["dy"] == "nlc" and cout == 1:
        return None
    xl = seen if p["nlc"] is None else "ncl"
    drop, n, lead, tail = F_._long_spread_args(L, K, s, pad, op, d)
    if n == 0:
        return None
    kp = -(-K // s)
    if rowlen <= F_.LONG_HANDOFF_POINTS and not cx:
        route = "handoff"
    elif p["poly"] is None and 2 <= s <= F_.LONG_PHASES_MAX_STRIDE and d == 1 and not cx and xl != "nlc" and not p["channels_last"]:
        route = "phases"
    else:
        route = "spread"
    case = Case("tr", idx, seed, (), p["B"], g, p["cig"], p["cog"], L, K, pad, "constant", s, d, False, op, p["bias"],
                p["channels_last"], p["dtype"], p["layout"], p["dy"], p["grads"], p["module"], p["cls"],
                tuple((KNOBS[k], p[k]) for k in KNOBS if p.get(k) is not None), pad, pad, rowlen, lout, route, None, 0, 0,
                0, K - 1, drop, ())
    spread_need = geom(n, K, lead, tail, lout, 0, s, d, 1)[3]
    needs = [spread_need]
    if p["grads"]:
        needs += [geom(lout, K, pad, pad, L, 0, 1, d, s)[3], geom(lout, L, pad, max(0, pad - op), K, 0, 1, s, d)[3]]
    forced = case.forced
    if route != "handoff" and forced and forced[0] * forced[1] < max(needs):
        return None
    n1n2, slabs, slab_pairs = None, 0, 0
    if route == "spread":
        n1n2, slabs, slab_pairs = plan_size(spread_need, p["B"], cin, cout, cx, forced, p["ws"])
    elif route == "phases":
        t0, t1 = min(pad // s, kp - 1), (lout - 1 + pad) // s
        nt = t1 - t0 + 1
        fpl = kp - 1 - t0
        need = geom(L, kp, fpl, max(0, nt + kp - 1 - fpl - L), nt, 0, 1, 1, 1)[3]
        n1n2, slabs, slab_pairs = plan_size(need, p["B"], cin, cout * s, False, forced, p["ws"])
    return dataclasses.replace(case, pick=tuple(p.items()), n1n2=n1n2, slabs=slabs, slab_pairs=slab_pairs, needs=tuple(needs))


_REALISE = {"fwd": _realise_fwd, "tr": _realise_tr}


def _candidate(kind, rng, fixed, idx=0, seed=0, tries=6):
    """A case with the axis values ``fixed`` and the rest drawn, or None after ``tries`` rejected draws."""
    axes = AXES[kind]
    for _ in range(tries):
        p = {a: rng.choice(v) for a, v in axes.items()}
        if "trim" in p and rng.random() < 0.7:
            p["trim"] = "none"          # (the trimmed geometries are edge cases: a quota each, not a quarter of the table)
        p.update(fixed)
        _repair(kind, p, fixed)
        case = _REALISE[kind](p, rng, idx, seed)
        if case is not None and all(dict(case.pick)[a] == v for a, v in fixed.items()):
            return case
    return None


STEERING = ("trim",)          # drawn and recorded, with quotas of its own, but no axis of the pair coverage


def pairs_of(case):
    pick = tuple(av for av in case.pick if av[0] not in STEERING)
    return {(a, va, b, vb) for i, (a, va) in enumerate(pick) for b, vb in pick[i + 1:]}


@functools.lru_cache(maxsize=None)
def allowed_pairs(kind):
    """Every (axis, value, axis, value) that some case the API accepts can hold, by trial against the rejection rule."""
    axes = AXES[kind]
    names = [a for a in axes if a not in STEERING]
    out = set()
    rng = random.Random(12345)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            for va in axes[a]:
                for vb in axes[b]:
                    if (a, va, b, vb) in out:
                        continue
                    case = _candidate(kind, rng, {a: va, b: vb}, tries=40)
                    if case is not None:
                        out |= pairs_of(case)
    return frozenset(out)


def by_index(i):
    """The axes a case's place in the table decides."""
    return {"grads": i % 2 == 0, "module": i % 8 in (0, 5), "cls": "offset" if i % 3 == 0 else "centred"}


def features(c):
    """The quota features a case has by its record alone (tests/test_host_long_sweep.py counts the routes the library
    predicts; these steer the greedy choice)."""
    f = [f"{c.kind}:{c.route}"]
    if c.slabs >= 2:
        f.append("slabs")
    if c.forced and c.route != "handoff":
        f.append("N" + "x".join(map(str, c.forced)))
    if c.kind == "fwd":
        if c.khi < c.klo:
            f.append("bias_only")
        elif c.klo > 0:
            f.append("klo")
        if c.grads and c.route != "handoff":
            real = not c.complex
            by_phases = c.route == "phases" and not c.causal
            f.append("dw_phases" if by_phases else
                     "dw_plan" if real and dict(c.env).get(KNOBS["wgrad"]) == "1" else "dw_exchanged")
    else:
        if c.drop and c.route == "spread":
            f.append("dropped")
        if c.grads and c.route != "handoff" and dict(c.env).get(KNOBS["decim"]) == "1" and c.stride >= 2 \
                and c.dilation == 1 and not c.complex:
            f.append("tr_decim")
    return f


QUOTAS = {"fwd:handoff": 3, "fwd:plain": 12, "fwd:phases": 8, "dw_plan": 6, "dw_exchanged": 6, "dw_phases": 3, "tr:handoff": 2,
          "tr:phases": 6, "tr:spread": 6, "tr_decim": 3, "slabs": 8, "klo": 3, "bias_only": 1, "dropped": 2,
          **{"N" + n: 2 for n in FORCED_N}}


@functools.lru_cache(maxsize=None)
def tables(seed=SEED):
    """(forward cases, transposed cases) of ``seed``: greedy over seeded candidates until every allowed pair is covered
    and the table has its count, each table by itself."""
    rng = random.Random(seed)
    have, out = {}, {}
    for kind in ("fwd", "tr"):
        covered = set()
        allowed = allowed_pairs(kind)
        order = sorted(allowed, key=repr)
        cases = []
        while len(cases) < COUNTS[kind] or not covered >= allowed:
            i = len(cases)
            assert i < 3 * COUNTS[kind], f"{kind}: the greedy choice does not converge"
            fixed = by_index(i)
            still = [q for q in order if q not in covered]
            open_ = [q for q in still if all(fixed.get(a, v) == v for a, v in (q[:2], q[2:]))]
            best, best_score = None, -1
            for n in range(CANDIDATES):
                want = dict(fixed)
                for _ in range(n % 4 if open_ else 0):      # aim at up to three pairs still open
                    q = open_[rng.randrange(len(open_))]
                    if all(want.get(a, v) == v for a, v in (q[:2], q[2:])):
                        want.update({q[0]: q[1], q[2]: q[3]})
                c = _candidate(kind, rng, want, i, seed)
                if c is None:
                    continue
                if len(still) < 300:      # (the same count, from the short side)
                    pick = dict(c.pick)
                    new = sum(1 for q in still if pick[q[0]] == q[1] and pick[q[2]] == q[3])
                else:
                    new = len((pairs_of(c) & allowed) - covered)
                score = new + 12 * sum(have.get(f, 0) < QUOTAS.get(f, 0) for f in features(c))
                if c.route == "handoff" and have.get(f"{kind}:handoff", 0) >= QUOTAS[f"{kind}:handoff"] + 2:
                    score = max(1 if new else 0, score - 10)      # (a hand-off runs no long kernel: no more than the pairs need)
                if score > best_score:
                    best, best_score = c, score
            assert best is not None, (kind, i)
            cases.append(best)
            covered |= pairs_of(best)
            for f in features(best):
                have[f] = have.get(f, 0) + 1
        out[kind] = tuple(cases)
    return out["fwd"], out["tr"]


# ------------------------------------------------------------------------------------------------ switches
def set_switches(case, setenv):
    """The case's switches through ``setenv(name, value or None)``, every other knob deleted; the plan caches cleared
    (FFTCONV_LONG_N and FFTCONV_LONG_WS_MB are read when a plan is created)."""
    env = dict(case.env)
    for k in ALL_KNOBS:
        setenv(k, env.get(k))
    clear()


def clear():
    _native.clear_plan_cache()
    F_._REFUSED_HALF.clear()
    autograd._BWD_PLANS.clear()


def os_setenv(name, value):
    import os
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = value


# ------------------------------------------------------------------------------------------------ prediction
def predict(c):
    """Routes and the plans that run, in order, under the switches now in the environment: {"route", "dw" ("plan" |
    "exchanged" | None), "dw_phases", "dx_decim", "dw_decim", "tokens"}.  A token names one launch: "native" (fft_conv's
    kernels), "long/<out_keep>" (a plain long plan), "decim", "phases", "wgrad"."""
    xl = {"ncl": "ncl", "nlc0": "nlc", "nlc_off": "nlc", "copy": "copy"}[c.layout] if F_._long_nlc_enabled() else "ncl"
    out = dict(route=None, dw=None, dw_phases=False, dx_decim=False, dw_decim=False)
    kp = -(-c.K // c.stride)
    if c.kind == "fwd":
        args = ((c.B, c.cin, c.L), c.wshape, c.stride, c.padding, c.dilation, c.groups, c.causal, c.mode, c.tdtype, xl)
        route = F_._long_route(*args)
        toks = [{"handoff": "native", "plain": f"long/{F_._long_keep(c.L, c.causal, c.stride)}", "phases": "decim"}[route]]
        if c.grads and route != "handoff":
            out["dw"] = F_._long_wgrad_route(*args)
            if route == "phases" and not c.causal:
                out["dw_phases"] = True
                toks += ["phases", f"long/{kp}"]
            else:
                n, _, _, keep = dx_rows(c)
                toks += ([f"long/{keep}"] if n else []) + ["wgrad" if out["dw"] == "plan" else f"long/{c.K}"]
    else:
        route = F_._long_transpose_route((c.B, c.cin, c.L), c.wshape, c.stride, c.padding, c.opad, c.dilation, c.groups,
                                         c.tdtype, (xl, c.channels_last))
        toks = [{"handoff": "native", "phases": "phases", "spread": f"long/{c.nout}"}[route]]
        if c.grads and route != "handoff":
            mode = F_._long_decim_mode()
            decim = bool(mode) and F_._long_decim_eligible(c.nout, c.K, c.stride, c.pl, c.pl, c.L, c.dilation, 0, c.tdtype)
            out["dx_decim"] = out["dw_decim"] = decim      # (unset: the plain constructions fit at these sizes)
            toks += ["decim" if decim else f"long/{c.L}", f"long/{kp}" if decim else f"long/{c.K}"]
    out.update(route=route, tokens=toks)
    return out


class Spy:
    """Records the launches of the long family while it is active: ``events`` = [(token, plan key, info words)]."""

    def __init__(self):
        self.events = []

    def __enter__(self):
        ev = self.events
        self._saved = [(_native.LongPlan, "forward", _native.LongPlan.forward), (_native.LongPlan, "forward_lay", _native.LongPlan.forward_lay),
                       (_native.LongWgradPlan, "run", _native.LongWgradPlan.run), (F_, "_forward_native", F_._forward_native)]
        names = {"LongPlan": "long", "LongDecimPlan": "decim", "LongPhasesPlan": "phases"}

        def wrap(real, token_of):
            def spied(first, *a, **k):
                ev.append((token_of(first), getattr(first, "key", None), dict(getattr(first, "info", {}))))
                return real(first, *a, **k)
            return spied

        def long_token(plan):
            name = names[type(plan).__name__]
            return f"long/{plan.key[8]}" if name == "long" else name
        setattr(_native.LongPlan, "forward", wrap(self._saved[0][2], long_token))
        setattr(_native.LongPlan, "forward_lay", wrap(self._saved[1][2], long_token))
        setattr(_native.LongWgradPlan, "run", wrap(self._saved[2][2], lambda plan: "wgrad"))
        real_native = self._saved[3][2]

        def native(signal, spectrum, bias):
            ev.append(("native", None, {}))
            return real_native(signal, spectrum, bias)
        F_._forward_native = native
        return self

    def __exit__(self, *exc):
        for owner, name, real in self._saved:
            setattr(owner, name, real)
        return False

    def tokens(self):
        return [e[0] for e in self.events]


# ------------------------------------------------------------------------------------------------ tensors
def inputs(c):
    """(x, w, b, dY) of a case on the CPU, contiguous, in its dtype: integers (``accuracy_util.integers``)."""
    gen = torch.Generator().manual_seed(7919 * c.seed + 31 * c.idx + (5003 if c.kind == "tr" else 0))
    dt = c.tdtype
    draw = dt if dt.is_complex else torch.float32

    def ints(shape, offset=0):
        t = au.integers(shape, gen, draw)
        if dt == torch.float16:
            t = torch.div(t, F16_DIV, rounding_mode="trunc")
            offset = F16_OFFSET if offset else 0
        return (t + offset).to(dt)
    x = ints((c.B, c.cin, c.L), au.OFFSET if c.cls == "offset" else 0)
    w = ints(c.wshape)
    b = ints((c.cout,)) if c.bias else None
    gy = ints((c.B, c.cout, c.nout)) if c.grads else None
    return x, w, b, gy


def pad(x, pl, pr, mode):
    """``F.pad(x, (pl, pr), mode)`` of a (B, C, L) tensor written as slices and one cat, so that its backward is a fixed
    sequence of adds: torch's own padding kernels accumulate their backward with atomic adds, and the edge sample of a
    replicate padding (the sum of up to L border samples) then differs from run to run -- in the baseline, against which
    the kernels are measured."""
    if not (pl or pr):
        return x
    if mode == "constant":
        return F.pad(x, (pl, pr))
    L = x.shape[2]
    if mode == "replicate":
        parts = [x[..., :1].expand(-1, -1, pl), x, x[..., -1:].expand(-1, -1, pr)]
    elif mode == "reflect":
        parts = [x[..., 1:pl + 1].flip(-1), x, x[..., L - 1 - pr:L - 1].flip(-1)]
    else:
        parts = [x[..., L - pl:], x, x[..., :pr]]
    return torch.cat(parts, dim=2)


def conv(c, x, w, b):
    """The FFT formulation of the case (module docstring) on (B, C, L) tensors of any precision; differentiable."""
    if c.kind == "tr":
        return au.baseline_conv_transpose(x, w, b, c.stride, c.padding, c.opad, c.dilation, c.groups)
    pl, pr = (c.dilation * (c.K - 1), 0) if c.causal else (c.pl, c.pr)

    def real(x_, w_, b_):
        xp = pad(x_, pl, pr, c.mode)
        return au._baseline_real(xp, w_, b_, (c.stride,), (0,), (c.dilation,), c.groups, "constant")
    return au._via_real(real, x, w.flip(-1) if c.causal else w, b)


def results(c, x, w, b, gy, exact=False):
    """{"y", "dX", "dW", "db"} of ``conv`` on these tensors by autograd (gradients None without ``gy``); ``exact``: the
    tensors are float64 integers and every value is rounded to the whole number it is (``accuracy_util.whole``)."""
    leaves = [t if t is None else t.detach().clone().requires_grad_(gy is not None) for t in (x, w, b)]
    y = conv(c, *leaves)
    out = dict(y=y.detach(), dX=None, dW=None, db=None)
    if gy is not None:
        y.backward(gy)
        out.update(dX=leaves[0].grad, dW=leaves[1].grad, db=None if b is None else leaves[2].grad)
    if exact:
        out = {k: v if v is None else au.whole(v, f"{c.id} {k}") for k, v in out.items()}
    return out


def wide(t):
    return None if t is None else au._wide(t)


def truth(c, x, w, b, gy):
    """The exact results in float64 / complex128 on the CPU."""
    return results(c, *(wide(None if t is None else t.cpu()) for t in (x, w, b, gy)), exact=True)


def compute_dtype(c):
    return torch.complex64 if c.complex else torch.float32


def baseline(c, x, w, b, gy):
    """The baseline in float32 / complex64 on the tensors' device (16-bit tensors widened)."""
    dt = compute_dtype(c)
    return results(c, *(None if t is None else t.detach().to(dt).contiguous() for t in (x, w, b, gy)))


def sample_positions(c):
    """Output positions worth an explicit dot product: the row ends, both sides of pad_left, the last strided sample."""
    at = -(-c.pl // c.stride) if c.kind == "fwd" else max(0, c.dilation * (c.K - 1) - c.padding)
    js = {0, c.nout - 1, c.nout - 2, at - 1, at, at + 1, c.nout // 2}
    return sorted(j for j in js if 0 <= j < c.nout)


def dots(c, x, w, b, js):
    """Explicit float64 dot products y[b, o, j] for b in (0, B - 1), every o, j in ``js`` -> (2, Cout, len(js))."""
    x, w = wide(x), wide(w)
    if c.kind == "tr":
        x, w = au.transposed_as_forward(x, w, (c.stride,), (c.padding,), (c.opad,), (c.dilation,), c.groups)
        s, cig = 1, c.cin // c.groups
    else:
        pl, pr = (c.dilation * (c.K - 1), 0) if c.causal else (c.pl, c.pr)
        pad = lambda t: F.pad(t, (pl, pr), mode=c.mode) if pl or pr else t      # noqa: E731
        x = torch.complex(pad(x.real), pad(x.imag)) if x.is_complex() else pad(x)
        w = w.flip(-1) if c.causal else w
        s, cig = c.stride, c.cig
    d, K, cog = c.dilation, c.K, c.cog
    out = torch.zeros(2, c.cout, len(js), dtype=x.dtype)
    for n, bi in enumerate((0, c.B - 1)):
        for o in range(c.cout):
            rows = x[bi, (o // cog) * cig:(o // cog + 1) * cig]
            for m, j in enumerate(js):
                out[n, o, m] = (w[o] * rows[:, s * j:s * j + d * (K - 1) + 1:d]).sum()
            if b is not None:
                out[n, o] += wide(b)[o]
    return out


def check_values(c, got, want, base, tag=""):
    """``accuracy_util.check`` at its default margins on every result ``got`` holds -> {name: measures}."""
    out = {}
    for name in ("y", "dX", "dW", "db"):
        if got.get(name) is not None:
            out[name] = au.check(f"{c.id}{tag} {name}", got[name], want[name], base[name], compute_dtype(c))
    return out


# ------------------------------------------------------------------------------------------------ the run
def call(c, x, w, b, channels_last=None):
    cl = c.channels_last if channels_last is None else channels_last
    if c.kind == "fwd":
        return F_.fft_long_conv(x, w, b, padding=c.padding, groups=c.groups, causal=c.causal, stride=c.stride,
                                dilation=c.dilation, padding_mode=c.mode, channels_last=cl)
    return F_.fft_long_conv_transpose(x, w, b, c.stride, c.padding, c.opad, c.dilation, c.groups, channels_last=cl)


def make_module(c, w, b):
    if c.kind == "fwd":
        layer = FFTLongConv1d(c.cin, c.cout, c.K, padding=c.padding, groups=c.groups, bias=c.bias, causal=c.causal,
                              device=w.device, dtype=w.dtype, channels_last=c.channels_last, stride=c.stride,
                              dilation=c.dilation, padding_mode="zeros" if c.mode == "constant" else c.mode)
    else:
        layer = FFTLongConvTranspose1d(c.cin, c.cout, c.K, stride=c.stride, padding=c.padding, output_padding=c.opad,
                                       groups=c.groups, bias=c.bias, dilation=c.dilation, device=w.device, dtype=w.dtype,
                                       channels_last=c.channels_last)
    with torch.no_grad():
        layer.weight.copy_(w)
        if b is not None:
            layer.bias.copy_(b)
    return layer.eval()


def step(c, x, w, b, gy, channels_last=None, layer=None):
    """One call (through ``layer`` if given) and, with ``gy``, its backward -> {"y", "dX", "dW", "db", "dx_strides" (of
    the dX backward returned, before autograd lays it out), "n_fwd" (launches the spy saw by the end of the forward)}."""
    grads = gy is not None
    xs = x.detach().requires_grad_(grads)
    if layer is None:
        ws = w.detach().clone().requires_grad_(grads)
        bs = None if b is None else b.detach().clone().requires_grad_(grads)
    else:
        ws, bs = layer.weight, layer.bias
        for t in (ws, bs):
            if t is not None:
                t.grad = None
                t.requires_grad_(grads)
    seen = []
    if grads:
        xs.register_hook(lambda g: seen.append(tuple(g.stride())))
    with torch.set_grad_enabled(grads):
        y = layer(xs) if layer is not None else call(c, xs, ws, bs, channels_last)
    out = dict(y=y.detach(), dX=None, dW=None, db=None, dx_strides=None)
    if grads:
        y.backward(gy)
        out.update(dX=xs.grad, dW=ws.grad, db=None if bs is None else bs.grad, dx_strides=seen[0] if seen else None)
    torch.cuda.synchronize()
    return out


def _strides_are(shape, strides, want):
    """Strides compared where they mean something: over the dimensions of more than one element."""
    return all(a == b for n, a, b in zip(shape, strides, want) if n > 1)


def _bits(c, a, b, what, names=("y", "dX", "dW", "db")):
    for name in names:
        if a.get(name) is not None:
            gu.same_bits(a[name], b[name], f"{c.id} {name}: {what}")


def run_case(c, device, setenv, log=print):
    """Run one case under its switches and hold it to (a) routes, (b) values, (c) shape / dtype / strides, (d) the bit
    relations the docstrings promise and (e) untouched inputs.  -> a record for scripts/long_sweep_extended.py."""
    log(f"case {c.id}")
    set_switches(c, setenv)
    dt, half = c.tdtype, c.tdtype in HALF
    pred = predict(c)
    x0, w0, b0, gy0 = inputs(c)
    want = truth(c, x0, w0, b0, gy0)
    dev = lambda t, layout="ncl": None if t is None else place(t, layout, device) if t.ndim == 3 and layout != "ncl" else t.to(device)  # noqa: E731
    x, w, b = dev(x0, c.layout), dev(w0), dev(b0)
    gy = dev(gy0, "nlc0" if c.dy == "nlc" else "ncl")
    assert F_._long_layout(x) == {"ncl": "ncl", "nlc0": "nlc", "nlc_off": "nlc", "copy": "copy"}[c.layout], c.id
    kept = [None if t is None else t.clone() for t in (x, w, b, gy)]
    layer = make_module(c, w, b) if c.module else None

    # ---- the call
    with Spy() as spy:
        got = step(c, x, w, b, gy, layer=layer)
    events = list(spy.events)
    # (a) routes
    toks = [e[0] for e in events]
    if pred["route"] == "handoff":
        assert toks and toks[0] == "native" and not any(t != "native" for t in toks), f"{c.id}: expected a hand-off, ran {toks}"
    else:
        assert toks == pred["tokens"], f"{c.id}: ran {toks}, predicted {pred['tokens']}"
        assert pred["route"] == c.route, f"{c.id}: route {pred['route']}, the table expected {c.route}"
        n12 = [(e[2]["N1"], e[2]["N2"]) for e in events if e[2]]
        if c.forced:
            assert all(n == c.forced for n in n12), f"{c.id}: N1 x N2 {n12}, forced {c.forced}"
        if c.n1n2 is not None:
            info = events[0][2]
            assert (info["N1"], info["N2"]) == c.n1n2, f"{c.id}: N1 x N2 {info['N1']}x{info['N2']}, expected {c.n1n2}"
            assert info["slabs"] == c.slabs, f"{c.id}: {info['slabs']} slabs, expected {c.slabs}"
    # (e) untouched inputs
    now = (x, w, b, gy) if layer is None else (x, layer.weight.detach(), None if b is None else layer.bias.detach(), gy)
    for name, t, k in zip(("x", "w", "b", "dY"), now, kept):
        if t is not None:
            gu.same_bits(t, k, f"{c.id}: input {name} after the call")
    # (c) shape, dtype, strides
    y = got["y"]
    assert tuple(y.shape) == (c.B, c.cout, c.nout) and y.dtype == dt, f"{c.id}: y {tuple(y.shape)} {y.dtype}"
    cl_strides = (c.nout * c.cout, 1, c.cout)
    if c.channels_last:
        assert _strides_are(y.shape, y.stride(), cl_strides), f"{c.id}: y strides {tuple(y.stride())}, channels-last is {cl_strides}"
    else:
        assert y.is_contiguous() and (c.cout == 1 or c.nout == 1 or tuple(y.stride()) != cl_strides), \
            f"{c.id}: y strides {tuple(y.stride())} of a contiguous result"
    if c.grads:
        for name, t, shape in (("dX", got["dX"], x.shape), ("dW", got["dW"], w.shape), ("db", got["db"], (c.cout,))):
            if t is not None or name != "db":
                assert t is not None and tuple(t.shape) == tuple(shape) and t.dtype == dt, f"{c.id}: {name} {None if t is None else (tuple(t.shape), t.dtype)}"
        if pred["route"] != "handoff" and c.layout in ("ncl", "nlc0", "nlc_off"):
            assert got["dx_strides"] is not None and _strides_are(x.shape, got["dx_strides"], x.stride()), \
                f"{c.id}: backward returned dX with strides {got['dx_strides']}, the signal has {tuple(x.stride())}"

    # (b) values, and (d) the 16-bit relation: the float32 twin is held to the bound, the case has its rounded bits
    record = dict(id=c.id, predicted=pred["tokens"], observed=toks, n1n2=None if not events or not events[0][2] else
                  f"{events[0][2]['N1']}x{events[0][2]['N2']}", slabs=events[0][2].get("slabs") if events else None)
    base = baseline(c, x, w, b, gy)
    if half:
        clear()
        wide_args = [None if t is None else t.float() for t in (x, w, b, gy)]
        twin = step(c, *wide_args)
        measures = check_values(c, twin, want, base, " (float32 twin)")
        _bits(c, got, {k: None if twin.get(k) is None or k in ("dx_strides",) else twin[k].to(dt) for k in ("y", "dX", "dW", "db")},
              f"the {c.dtype} call against the float32 call rounded")
        clear()
    else:
        measures = check_values(c, got, want, base)
    for name, m in measures.items():
        record[name] = dict(e_rms=m["e_rms"], e_max=m["e_max"], rms_ratio=m["rms_ratio"], max_ratio=m["max_ratio"])

    # (d) layouts: the bits of the contiguous call, where it takes the same plans
    plain = dataclasses.replace(c, layout="ncl", channels_last=False, dy="ncl" if c.grads else "none")
    if plain != c and pred["route"] != "handoff":
        if predict(plain)["tokens"] == pred["tokens"]:
            ref = step(plain, x.contiguous(), w, b, None if gy is None else gy.contiguous(), channels_last=False)
            _bits(c, got, ref, "a strided call against the contiguous call")
        if dict(c.env).get(KNOBS["nlc"]) == "0":      # ... and FFTCONV_LONG_NLC=0 changes neither values nor strides
            setenv(KNOBS["nlc"], None)
            same = predict(c)["tokens"] == pred["tokens"]
            ref = step(c, x, w, b, gy)
            setenv(KNOBS["nlc"], "0")
            assert _strides_are(y.shape, ref["y"].stride(), y.stride()), f"{c.id}: FFTCONV_LONG_NLC=0 changes the strides of y"
            if same:
                _bits(c, got, ref, "FFTCONV_LONG_NLC=0 against the switch unset")
    # (d) slabs: a forward in several slabs has the bits of the forward in one
    if c.slabs >= 2 and pred["route"] != "handoff":
        setenv(KNOBS["ws"], None)
        clear()
        with Spy() as one:
            ref = step(c, x, w, b, None)
        setenv(KNOBS["ws"], "1")
        clear()
        assert one.events[0][2]["slabs"] == 1, f"{c.id}: the default budget still splits the batch"
        _bits(c, got, ref, f"{c.slabs} slabs against one", ("y",))
    # (d) module: the functional's bits on the first call, the second (cached spectrum) and after a weight update
    if layer is not None:
        ref = step(c, x, w, b, gy)
        _bits(c, got, ref, "the module's first call against the functional")
        with torch.no_grad():
            _bits(c, dict(y=layer(x)), ref, "the module's second call against the functional", ("y",))
            layer.weight.neg_()
            _bits(c, dict(y=layer(x)), dict(y=call(c, x, -w, b)), "the module after an in-place weight update", ("y",))
    # (d) complex: a purely real signal and weight agree with the float32 call in the real part, to the bound of (b)
    if c.complex:
        real = dataclasses.replace(c, dtype="f32")
        xr, wr, br = x0.real.contiguous(), w0.real.contiguous(), None if b0 is None else b0.real.contiguous()
        zero = lambda t: None if t is None else torch.complex(t, torch.zeros_like(t))      # noqa: E731
        with torch.no_grad():
            yc = call(c, dev(zero(xr), c.layout), dev(zero(wr)), dev(zero(br)))
        torch.cuda.synchronize()
        au.check(f"{c.id} real part of the purely real complex call", yc.real.contiguous(), truth(real, xr, wr, br, None)["y"],
                 baseline(real, dev(xr), dev(wr), dev(br), None)["y"], torch.float32)
    torch.cuda.synchronize()
    return record
