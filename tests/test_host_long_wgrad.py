"""The weight-gradient plan of ``fft_long_conv`` without a GPU: exports and the C ABI, the geometry of the plan from its
descriptor alone (the forward plan's N1 x N2, the workspace formula, slabs, refusals), the route query, and a float64
numpy restatement of the three passes against torch's float64 autograd, on the table tests/test_gpu_long_wgrad.py runs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import _native
from fft_conv_pytorch_amd import functional as F_

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, C64 = torch.float32, torch.complex64
KNOBS = ("FFTCONV_LONG_WGRAD", "FFTCONV_LONG_DECIM", "FFTCONV_LONG_POLY", "FFTCONV_LONG_NLC", "FFTCONV_LONG_N",
         "FFTCONV_LONG_WS_MB", "FFTCONV_HALF_IO")


class Layer:
    """One ``fft_long_conv`` call: (B, cin) -> cout over L samples with K taps."""

    def __init__(self, B, cin, cout, L, K, g=1, s=1, d=1, p=0, causal=False, mode="constant", note=""):
        self.B, self.cin, self.cout, self.L, self.K, self.g, self.s, self.d = B, cin, cout, L, K, g, s, d
        self.p, self.causal, self.mode, self.note = p, causal, mode, note

    @property
    def wshape(self):
        return (self.cout, self.cin // self.g, self.K)

    def words(self):
        """(pad_left, pad_right, nout) of the forward."""
        meta = dict(device="meta")
        x, w = torch.empty((self.B, self.cin, self.L), **meta), torch.empty(self.wshape, **meta)
        pl, pr, _ = F_._long_geometry(x, w, None, self.p, self.g, self.causal, self.s, self.d, self.mode)
        nout = F_._long_keep(self.L, self.causal, self.s) or (self.L + pl + pr - self.d * (self.K - 1) - 1) // self.s + 1
        return pl, pr, nout

    def key(self):
        pl, pr, nout = self.words()
        return F_._long_wgrad_key(self.B, self.cin, self.cout, self.g, self.L, self.K, pl, pr, nout, self.causal,
                                  _native.PAD_MODES[self.mode], self.s, self.d)

    def forward_key(self):
        """The 15 words of the forward plan of the layer (``_native.long_desc`` / ``long_ext``), no bias."""
        pl, pr, _ = self.words()
        return (self.B, self.cin, self.cout, self.g, self.L, self.K, pl, pr, F_._long_keep(self.L, self.causal, self.s),
                int(self.causal), 0, _native.PAD_MODES[self.mode], 1, self.d, self.s)

    def route(self, dtype=F32, x_layout="ncl"):
        return F_._long_wgrad_route((self.B, self.cin, self.L), self.wshape, self.s, self.p, self.d, self.g, self.causal,
                                    self.mode, dtype, x_layout)


# the table of the GPU tests: every row only just past the 4096-point hand-off
#   1   depthwise causal K = L, odd batch (the last pair is half empty)
#   2   grouped dense, non-causal, equal paddings
#   3   stride 3 and dilation 2 through reflect padding
#   3s  'same' in reflect mode with unequal paddings (58 / 59; 'same' goes with stride 1, and an even extent needs an odd
#       dilation)
#   3c, 3r  the circular and the replicate row of 3
#   4   causal K > L: the lags no tap reaches
#   6a, 6b  B 1 and B 5 (6b in three slabs under FFTCONV_LONG_WS_MB)
TABLE = {
    "1": Layer(3, 4, 4, 4100, 4100, g=4, causal=True, note="depthwise causal K = L"),
    "2": Layer(4, 6, 4, 5000, 301, g=2, p=150, note="grouped dense"),
    "3": Layer(2, 2, 3, 4500, 40, s=3, d=2, p=39, mode="reflect", note="stride 3, dilation 2, reflect"),
    "3s": Layer(2, 2, 3, 4500, 40, d=3, p="same", mode="reflect", note="'same', unequal reflect paddings"),
    "3c": Layer(2, 2, 3, 4500, 40, s=3, d=2, p=39, mode="circular", note="circular"),
    "3r": Layer(2, 2, 3, 4500, 40, s=3, d=2, p=39, mode="replicate", note="replicate"),
    "4": Layer(2, 2, 2, 4500, 6000, causal=True, note="causal K > L"),
    "6a": Layer(1, 2, 2, 4300, 200, p=7, note="B 1"),
    "6b": Layer(5, 16, 16, 4300, 200, g=16, p=7, note="B 5"),
}


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------ exports and ABI
NEW = ("fc_long_wgrad_geometry", "fc_long_wgrad_check_io", "fc_long_wgrad_plan_create", "fc_long_wgrad_plan_destroy",
       "fc_long_wgrad_plan_info", "fc_long_wgrad")


def test_new_entry_points_only_and_abi_7():
    header = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", header))
    assert set(NEW) <= declared and declared == set(_native.EXPORTS)
    lib = _native.load_library()
    for name in NEW:
        assert hasattr(lib, name), name
    m = re.search(r"#define\s+FC_ABI_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == 7 == _native.ABI_VERSION == lib.fc_version()
    # the descriptor: nine int64 and four int32 words, in the header's order
    body = re.search(r"typedef struct fc_long_wgrad_desc \{(.*?)\} fc_long_wgrad_desc;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, names in re.findall(r"(int64_t|int32_t)\s+([^;]+);", body):
        fields += [(n.strip(), ctypes.c_int64 if ctype == "int64_t" else ctypes.c_int32) for n in names.split(",")]
    assert fields == list(_native.FcLongWgradDesc._fields_)
    assert ctypes.sizeof(_native.FcLongWgradDesc) == 9 * 8 + 4 * 4
    # nothing that existed changes
    assert ctypes.sizeof(_native.FcLongDesc) == 80 and ctypes.sizeof(_native.FcLongExt) == 16
    assert ctypes.sizeof(_native.FcLongPhasesDesc) == 80 and ctypes.sizeof(_native.FcLongDecimDesc) == 88
    assert _native._PLAN_TAGS == {"long": _native.LongPlan, "long_phases": _native.LongPhasesPlan, "long_decim": _native.LongDecimPlan,
                                  "long_wgrad": _native.LongWgradPlan}


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("name", sorted(TABLE))
def test_geometry_is_the_forward_plans_and_touches_no_device(name, monkeypatch):
    import torch.cuda
    monkeypatch.setattr(torch.cuda, "is_available", lambda: (_ for _ in ()).throw(AssertionError("device touched")))
    lay = TABLE[name]
    info = _native.wgrad_geometry(lay.key())
    fwd = _native.long_geometry(lay.forward_key())
    assert (info["N1"], info["N2"]) == (fwd["N1"], fwd["N2"]), (info, fwd)
    assert info["N1"] * info["N2"] > F_.LONG_HANDOFF_POINTS
    assert info["taps"] == lay.K and 1 <= info["lags"] <= lay.K
    if name == "4":      # taps at a lag of L or more meet no data
        assert info["lags"] == lay.L
    # the workspace: W1 of x and of dY for the pairs of a slab, W2 for all of dW; no spectrum
    n = info["N1"] * info["N2"]
    assert info["workspace_bytes"] == (info["slab_pairs"] * (lay.cin + lay.cout) + lay.cout * lay.cin // lay.g) * n * 8
    assert info["slab_pairs"] == (lay.B + 1) // 2 and info["slabs"] == 1


def test_a_forced_factorisation_is_taken_as_by_the_forward_plan(monkeypatch):
    lay = TABLE["2"]
    for n1, n2 in ((64, 128), (128, 64), (64, 4096), (4096, 64), (512, 512)):
        monkeypatch.setenv("FFTCONV_LONG_N", f"{n1}x{n2}")
        info = _native.wgrad_geometry(lay.key())
        assert (info["N1"], info["N2"]) == (n1, n2)
    monkeypatch.setenv("FFTCONV_LONG_N", "64x64")
    with pytest.raises(ValueError, match="holds 4096 points but the row needs"):
        _native.wgrad_geometry(lay.key())


def test_the_budget_changes_the_slabs_and_never_the_points(monkeypatch):
    lay = TABLE["6b"]
    free = _native.wgrad_geometry(lay.key())
    n = free["N1"] * free["N2"]
    rows = lay.cout * lay.cin // lay.g
    assert (free["slabs"], free["slab_pairs"]) == (1, 3)
    # room for W2 and one pair, not two: three slabs
    mb = -(-((rows + (lay.cin + lay.cout)) * n * 8) // (1 << 20))
    assert (rows + 2 * (lay.cin + lay.cout)) * n * 8 > mb << 20
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", str(mb))
    tight = _native.wgrad_geometry(lay.key())
    assert (tight["N1"], tight["N2"]) == (free["N1"], free["N2"])
    assert (tight["slabs"], tight["slab_pairs"]) == (3, 1)
    assert tight["workspace_bytes"] == ((lay.cin + lay.cout) + rows) * n * 8
    # the rows of W2 alone above the budget: refused, with text
    wide = Layer(2, 64, 64, 4300, 200)
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "16")
    with pytest.raises(NotImplementedError, match=r"64 x 64 rows of 8192 points \(256 MiB\).*budget of 16 MiB"):
        _native.wgrad_geometry(wide.key())
    assert wide.route() == "exchanged"
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    assert wide.route() == "exchanged"
    monkeypatch.delenv("FFTCONV_LONG_WS_MB")
    assert wide.route() == "plan"


def test_refusals_carry_text():
    big = 1 << 24
    with pytest.raises(NotImplementedError, match="needs a transform of 33554431 points; the long-filter path stops at 2\\^24"):
        _native.wgrad_geometry((1, 1, 1, 1, big, big, big - 1, 0, big, 1, 0, 1, 1))
    good = TABLE["2"].key()
    with pytest.raises(ValueError, match=r"stride \(0\) and dilation \(1\) must be >= 1"):
        _native.wgrad_geometry(good[:11] + (0, 1))
    with pytest.raises(ValueError, match=r"stride \(1\) and dilation \(-2\) must be >= 1"):
        _native.wgrad_geometry(good[:11] + (1, -2))
    with pytest.raises(ValueError, match=r"out_len \(0\) must be positive"):
        _native.wgrad_geometry(good[:8] + (0,) + good[9:])
    with pytest.raises(ValueError, match="out_keep .* exceeds the output length"):
        _native.wgrad_geometry(good[:8] + (good[8] + 1,) + good[9:])
    # a channels-last block of 2**31 bytes: x (L * Cin * 4) and dY (nout * Cout * 2), each refused on its own
    lay = Layer(1, 131072, 131072, 4200, 9, g=131072, p=4)
    assert lay.L * lay.cin * 4 >= 1 << 31 > lay.L * lay.cin * 2
    key = lay.key()
    _native.wgrad_check_io(key)
    _native.wgrad_check_io(key, 0, _native.LONG_NCL, 0, _native.LONG_NCL, 0)
    with pytest.raises(NotImplementedError, match="x in the channels-last layout: one batch item is 4200 samples x 131072 channels x 4"):
        _native.wgrad_check_io(key, 0, _native.LONG_NLC, 0, _native.LONG_NCL, 0)
    with pytest.raises(NotImplementedError, match="dy in the channels-last layout"):
        _native.wgrad_check_io(key, 2, _native.LONG_NLC, 0, _native.LONG_NLC, 0)
    _native.wgrad_check_io(key, 2, _native.LONG_NLC, 3, _native.LONG_NLC, 0)
    with pytest.raises(NotImplementedError, match="float64"):
        _native.wgrad_check_io(key, 1, 0, 0, 0, 0)
    with pytest.raises(ValueError, match="dw has dtype code 4"):
        _native.wgrad_check_io(key, 0, 0, 0, 0, 4)
    with pytest.raises(ValueError, match="dy has layout code 2"):
        _native.wgrad_check_io(key, 0, 0, 0, 2, 0)


# ------------------------------------------------------------------------------------------------ route
def test_the_route_query(monkeypatch):
    assert not F_._long_wgrad_mode()
    for name, lay in TABLE.items():
        assert lay.route() == "exchanged", name              # the switch unset
    for value in ("0", "", "yes"):
        monkeypatch.setenv("FFTCONV_LONG_WGRAD", value)
        assert not F_._long_wgrad_mode() and TABLE["1"].route() == "exchanged"
    monkeypatch.setenv("FFTCONV_LONG_WGRAD", "1")
    assert F_._long_wgrad_mode()
    for name, lay in TABLE.items():
        for dtype in (F32, torch.float16, torch.bfloat16):
            assert lay.route(dtype) == "plan", (name, dtype)
        assert lay.route(F32, "nlc") == "plan", name
        assert lay.route(C64) == "exchanged", name
    # a forward that ran by phases has its gradients by phases; a causal one keeps the plain branch
    strided = Layer(2, 2, 2, 9000, 600, s=2, p=3)
    causal = Layer(2, 2, 2, 9000, 9000, s=4, causal=True)
    assert strided.route() == "plan" and causal.route() == "plan"
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    assert F_._long_route((2, 2, 9000), strided.wshape, 2, 3) == "phases"
    assert strided.route() == "exchanged" and causal.route() == "plan"
    # a row that hands off to fft_conv never gets here
    assert Layer(2, 2, 2, 1000, 100).route() == "exchanged"


# ------------------------------------------------------------------------------------------------ the three passes
def _pad_row(x, pl, pr, mode):
    """(B, C, L) float64 -> the padded row the forward reads."""
    t = torch.from_numpy(x)
    if mode == "constant":
        return F.pad(t, (pl, pr)).numpy()
    return F.pad(t, (pl, pr), mode=mode).numpy()


def three_passes(x, dy, lay, n1, n2):
    """dW of the layer as the library computes it, in float64 numpy: batch pairs packed into complex rows (an odd batch
    leaves the last imaginary part zero), both operands through the column pass (N1-point transforms along n1, the twiddle
    w_N^(n2*k1)), the row pass (N2-point transforms, X * conj(D) summed over the pairs, back, 1 / N, the conjugate
    twiddle), the inverse column pass, the real part of every dilation-th lag stored at the place of its tap; with zero
    padding the lags of taps that can meet no data are not computed but written as zero."""
    B, K, g, s, d = lay.B, lay.K, lay.g, lay.s, lay.d
    pl, pr, nout = lay.words()
    N = n1 * n2
    # the taps the forward plan reads (host_long.cpp long_geometry), u = w in tensor order or flipped
    klo, khi = 0, K - 1
    if lay.mode == "constant":
        lo = pl - s * (nout - 1)
        klo = -(-lo // d) if lo > 0 else 0
        khi = min(K - 1, (pl + lay.L - 1) // d)
    assert khi >= klo
    keff, padl = khi - klo + 1, pl - d * klo
    assert N >= s * (nout - 1) + d * (keff - 1) + 1
    xrow = _pad_row(x, pl, pr, lay.mode)
    front = pl - padl
    xrow = xrow[..., front:] if front >= 0 else np.pad(xrow, ((0, 0), (0, 0), (-front, 0)))
    rows = np.zeros((B, lay.cin, N))
    m = min(N, xrow.shape[2])
    rows[..., :m] = xrow[..., :m]
    spread = np.zeros((B, lay.cout, N))
    spread[..., 0:s * (nout - 1) + 1:s] = dy

    def pack(t):
        pairs = -(-B // 2)
        z = np.zeros((pairs,) + t.shape[1:], dtype=complex)
        z += t[0::2]
        z[:B // 2] += 1j * t[1::2]
        return z

    tw = np.exp(-2j * np.pi * np.outer(np.arange(n1), np.arange(n2)) / N)      # [k1][n2]

    def cols_fwd(z):
        return np.fft.fft(z.reshape(z.shape[:-1] + (n1, n2)), axis=-2) * tw

    w1x, w1d = cols_fwd(pack(rows)), cols_fwd(pack(spread))
    cig, cog = lay.cin // g, lay.cout // g
    w2 = np.zeros((lay.cout, cig, n1, n2), dtype=complex)
    for o in range(lay.cout):
        for i in range(cig):
            acc = np.zeros((n1, n2), dtype=complex)
            for p in range(w1x.shape[0]):
                acc += np.fft.fft(w1x[p, (o // cog) * cig + i], axis=-1) * np.conj(np.fft.fft(w1d[p, o], axis=-1))
            w2[o, i] = np.fft.ifft(acc, axis=-1) * n2 / N * np.conj(tw)
    c = (np.fft.ifft(w2, axis=-2) * n1).reshape(lay.cout, cig, N)
    dw = np.zeros((lay.cout, cig, K))
    for q in range(keff):
        k = klo + q
        dw[..., K - 1 - k if lay.causal else k] = c[..., d * q].real
    return dw, (klo, khi)


@pytest.mark.parametrize("name", sorted(TABLE))
def test_three_passes_against_float64_autograd(name):
    lay = TABLE[name]
    if name in ("1", "2", "4"):      # the same layer on a row a CPU test affords (all the passes, a 64 x 64 transform at most)
        small = {"1": Layer(3, 4, 4, 50, 50, g=4, causal=True), "2": Layer(4, 6, 4, 70, 31, g=2, p=15),
                 "4": Layer(2, 2, 2, 45, 60, causal=True)}[name]
        lay, n1, n2 = small, 16, 8
    else:
        lay = Layer(lay.B, lay.cin, lay.cout, lay.L // 50, lay.K // 5 if lay.K > 100 else 12, g=lay.g, s=lay.s, d=lay.d,
                    p=11 * lay.d if lay.p == 39 else lay.p, causal=lay.causal, mode=lay.mode)
        n1, n2 = 8, 32
    pl, pr, nout = lay.words()
    rng = np.random.default_rng(len(name) + lay.L)
    x = rng.integers(-8, 9, (lay.B, lay.cin, lay.L)).astype(float)
    dy = rng.integers(-8, 9, (lay.B, lay.cout, nout)).astype(float)
    got, (klo, khi) = three_passes(x, dy, lay, n1, n2)
    # torch's float64 autograd of conv1d on the padded row (a causal layer: against the flipped taps)
    w = torch.zeros(lay.wshape, dtype=torch.float64, requires_grad=True)
    xrow = torch.from_numpy(_pad_row(x, pl, pr, lay.mode))
    y = F.conv1d(xrow, w.flip(-1) if lay.causal else w, None, lay.s, 0, lay.d, lay.g)[..., :nout]
    assert y.shape[2] == nout
    y.backward(torch.from_numpy(dy))
    want = w.grad.numpy()
    assert np.abs(got - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), np.abs(got - want).max()
    # the lags that were not transformed are exactly zero, in the truth too
    untouched = [k for k in range(lay.K) if not klo <= k <= khi]
    if name == "4":
        assert untouched and khi == lay.K - 1 and klo == lay.K - lay.L
    for k in untouched:
        e = lay.K - 1 - k if lay.causal else k
        assert not got[..., e].any() and not want[..., e].any()
