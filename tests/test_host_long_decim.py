"""``fft_long_conv`` by phases without a GPU: the identity the decimation plan rests on and the gradient constructions of
both long ops restated on the CPU, the route of every case tests/test_gpu_long_decim.py runs, the geometry of the
decimation plan from its descriptor alone, exports and the C ABI."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from fft_conv_pytorch_amd import _native, autograd
from fft_conv_pytorch_amd import functional as F_
from tests import accuracy_util as au
from tests.route_util import Case
from tests.test_host_long_transpose import _by_phases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, C64 = torch.float32, torch.complex64

# the table of the GPU tests: every row just past the hand-off in plain form
#   1  the basic case: odd batch, groups, phases of 501 and 500 taps
#   2  depthwise, three phases in blocks of four (one idle), a padding that is no multiple of the stride
#   3  K < stride: phase 2 has no tap
#   4  a padding far wider than the stride
#   5  depthwise rows, four phases of equal length
#   6  five phases in blocks of two, the last block partial
#   7  causal with K = L: flipped taps
#   8  the largest stride
#   9  dilation 2: plain in every mode
CASES = {
    1: Case(3, 4, 6, (9000,), (1001,), s=2, g=2, note="case1"),
    2: Case(2, 3, 3, (7000,), (700,), s=3, p=5, g=3, note="case2"),
    3: Case(1, 2, 2, (9000,), (2,), s=3, note="case3"),
    4: Case(2, 2, 2, (6000,), (4001,), s=2, p=2000, note="case4"),
    5: Case(4, 8, 8, (9000,), (512,), s=4, g=8, note="case5"),
    6: Case(2, 2, 4, (12000,), (50,), s=5, p=7, note="case6"),
    7: Case(3, 2, 2, (9000,), (9000,), s=4, note="case7-causal"),
    8: Case(1, 1, 1, (70000,), (130,), s=64, p=3, note="case8"),
    9: Case(2, 2, 4, (6000,), (600,), s=2, d=2, note="case9"),
}
CAUSAL = (7,)
PHASES_CASES = (1, 2, 3, 4, 5, 6, 7, 8)
POINTS = {1: (8999, 4500), 2: (7009, 2337), 3: (8999, 3000), 4: (9999, 5000), 5: (9000, 2250), 6: (12010, 2402),
          8: (69954, 1094)}        # (plain, decimated) points of the row before rounding up


def route_of(i, dtype=F32, x_layout="ncl"):
    c = CASES[i]
    return F_._long_route((c.B, c.cin, c.size[0]), c.wshape, c.s, c.p, c.d, c.g, i in CAUSAL, c.mode, dtype, x_layout)


def out_len(i):
    c = CASES[i]
    if i in CAUSAL:
        return -(-c.size[0] // c.s)
    return (c.size[0] + 2 * c.p - c.d * (c.k[0] - 1) - 1) // c.s + 1


def decim_key(i, has_bias=True):
    c = CASES[i]
    if i in CAUSAL:
        return (c.B, c.cin, c.cout, c.g, c.size[0], c.k[0], c.s, c.k[0] - 1, 0, out_len(i), 1, int(has_bias))
    return (c.B, c.cin, c.cout, c.g, c.size[0], c.k[0], c.s, c.p, c.p, 0, 0, int(has_bias))


def plain_key(i, has_bias=True):
    c = CASES[i]
    if i in CAUSAL:
        return (c.B, c.cin, c.cout, c.g, c.size[0], c.k[0], c.d * (c.k[0] - 1), 0, out_len(i), 1, int(has_bias), 0, 1, c.d, c.s)
    return (c.B, c.cin, c.cout, c.g, c.size[0], c.k[0], c.p, c.p, 0, 0, int(has_bias), 0, 1, c.d, c.s)


def as_forward_case(i):
    """The case as a plain strided cross-correlation ``accuracy_util`` knows: itself, or for a causal row the row with
    K - 1 zeros in front against the flipped taps -> (case, prepare(x, w) -> (x', w'))."""
    c = CASES[i]
    if i not in CAUSAL:
        return c, lambda x, w: (x, w)
    K = c.k[0]
    view = Case(c.B, c.cin, c.cout, (c.size[0] + K - 1,), c.k, s=c.s, g=c.g, note=c.note)
    return view, lambda x, w: (F.pad(x, (K - 1, 0)), w.flip(-1))


@pytest.fixture(autouse=True)
def _knobs(monkeypatch):
    for k in ("FFTCONV_LONG_DECIM", "FFTCONV_LONG_POLY", "FFTCONV_LONG_NLC", "FFTCONV_LONG_N", "FFTCONV_LONG_WS_MB", "FFTCONV_HALF_IO"):
        monkeypatch.delenv(k, raising=False)


# ------------------------------------------------------------------------------------------------ the identity
def _ints(rng, n):
    return rng.integers(-8, 9, n).astype(float)


def _strided(xrow, u, s, nout):
    return np.array([np.dot(u, xrow[s * j:s * j + len(u)]) for j in range(nout)])


def _by_decimation(xrow, u, s, nout):
    """y[j] = sum_p (u_p * x_p)[j], x_p[t] = xrow[s*t + p], u_p[m] = u[s*m + p]: a shorter phase ends early, a phase
    p >= K has no tap; rows of T = nout + Kp - 1 positions, zero past the row."""
    K = len(u)
    kp = -(-K // s)
    T = nout + kp - 1
    row = np.zeros(s * T)
    n = min(len(xrow), s * T)
    row[:n] = xrow[:n]
    y = np.zeros(nout)
    for p in range(s):
        up = u[p::s]
        if len(up) == 0:
            continue
        xp = row[p::s]
        y += np.array([np.dot(up, xp[j:j + len(up)]) for j in range(nout)])
    return y


SHAPES = [(50, 7, 2, 0), (50, 7, 3, 4), (41, 13, 4, 6), (30, 2, 3, 0), (64, 64, 5, 10), (33, 5, 8, 3)]


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("L,K,s,p", SHAPES)
def test_decimated_convolutions_sum_to_the_strided_convolution(L, K, s, p, flip):
    rng = np.random.default_rng(L + K + s)
    x, w = _ints(rng, L), _ints(rng, K)
    u = w[::-1] if flip else w
    xrow = np.concatenate([np.zeros(p), x, np.zeros(p)])
    nout = (L + 2 * p - K) // s + 1
    want = _strided(xrow, u, s, nout)
    assert np.array_equal(_by_decimation(xrow, u, s, nout), want)
    ref = F.conv1d(torch.tensor(x)[None, None], torch.tensor(u.copy())[None, None], None, s, p)
    assert np.array_equal(ref[0, 0].numpy(), want)


@pytest.mark.parametrize("L,K,s,p", SHAPES)
def test_gradients_of_the_strided_convolution_by_phases(L, K, s, p):
    """dX = the transposed convolution of dY by phases with output_padding (L + 2p - K) mod s; dW[s*m + q] = sum_j dY[j] *
    x_q[j + m], the phases of x as a batch-like index."""
    rng = np.random.default_rng(7 * L + K)
    x, w = _ints(rng, L), _ints(rng, K)
    nout = (L + 2 * p - K) // s + 1
    gy = _ints(rng, nout)
    xt, wt = torch.tensor(x).requires_grad_(), torch.tensor(w).requires_grad_()
    F.conv1d(xt[None, None], wt[None, None], None, s, p).backward(torch.tensor(gy)[None, None])
    dx = _by_phases(gy, w, s, p, (L + 2 * p - K) % s)
    assert dx.shape == (L,) and np.array_equal(dx, xt.grad.numpy())
    kp = -(-K // s)
    T = nout + kp - 1
    xrow = np.zeros(s * T + s)
    seg = np.concatenate([np.zeros(p), x])[:s * T]
    xrow[:len(seg)] = seg
    dw = np.zeros(kp * s)
    for q in range(s):
        xq = xrow[q::s]
        for m in range(kp):
            dw[s * m + q] = np.dot(gy, xq[m:m + nout])
    assert np.array_equal(dw[:K], wt.grad.numpy())


@pytest.mark.parametrize("L,K,s,p", SHAPES)
def test_gradients_of_the_transposed_convolution_by_phases(L, K, s, p):
    """dX = the strided convolution of dY (p zeros on both sides, L kept) by decimation; dW[s*m + q] = sum_t x[t] *
    dY_q[t + m], the phases of dY read with p zeros in front."""
    op = (L + K) % s if s > 1 else 0
    lout = (L - 1) * s - 2 * p + K + op
    assert lout >= 1
    rng = np.random.default_rng(3 * L + K)
    x, w, gy = _ints(rng, L), _ints(rng, K), _ints(rng, lout)
    xt, wt = torch.tensor(x).requires_grad_(), torch.tensor(w).requires_grad_()
    F.conv_transpose1d(xt[None, None], wt[None, None], None, s, p, op).backward(torch.tensor(gy)[None, None])
    grow = np.concatenate([np.zeros(p), gy, np.zeros(p)])
    assert np.array_equal(_by_decimation(grow, w, s, L), xt.grad.numpy())
    kp = -(-K // s)
    T = L + kp - 1
    row = np.zeros(s * T)
    seg = np.concatenate([np.zeros(p), gy])[:s * T]
    row[:len(seg)] = seg
    dw = np.zeros(kp * s)
    for q in range(s):
        gq = row[q::s]
        for m in range(kp):
            dw[s * m + q] = np.dot(x, gq[m:m + L])
    assert np.array_equal(dw[:K], wt.grad.numpy())


@pytest.mark.parametrize("L,K,s,p,g", [(50, 7, 2, 0, 1), (50, 7, 3, 4, 2), (41, 13, 4, 6, 2), (30, 2, 3, 0, 1), (33, 5, 8, 3, 2)])
def test_the_weight_gradient_operands_autograd_builds(L, K, s, p, g):
    """``autograd._phase_rows`` / ``_interleave_lags`` with torch's conv1d in the place of the long primitive, batch 3 and
    groups: the dW of both ops as ``backward`` assembles them, against float64 autograd."""
    B, cig, cog = 3, 2, 3
    gen = torch.Generator().manual_seed(L + K)
    x = au.integers((B, g * cig, L), gen, torch.float64).requires_grad_()
    kp = -(-K // s)

    def primitive(signal, kernel, keep):          # y[j] = sum u[k] * row[j + k], `keep` samples
        return F.conv1d(signal, kernel, None, groups=g)[..., :keep]
    # the strided forward
    w = au.integers((g * cog, cig, K), gen, torch.float64).requires_grad_()
    y = F.conv1d(x, w, None, s, p, 1, g)
    gy = au.integers(y.shape, gen, torch.float64)
    y.backward(gy)
    xt = autograd._phase_rows(x.detach(), p, s, y.shape[2] + kp - 1, g)
    du = primitive(xt, gy.permute(1, 0, 2).contiguous(), kp)
    assert torch.equal(autograd._interleave_lags(du, s, K), w.grad)
    # the transposed op
    x.grad = None
    wt = au.integers((g * cig, cog, K), gen, torch.float64).requires_grad_()
    op = 1 if s > 1 else 0
    yt = F.conv_transpose1d(x, wt, None, s, p, op, g)
    gyt = au.integers(yt.shape, gen, torch.float64)
    yt.backward(gyt)
    dyt = autograd._phase_rows(gyt, p, s, L + kp - 1, g)
    du = primitive(dyt, x.detach().permute(1, 0, 2).contiguous(), kp)
    assert torch.equal(autograd._interleave_lags(du, s, K), wt.grad)


# ------------------------------------------------------------------------------------------------ routes
def test_the_table_fits_the_exact_truth_and_sits_just_past_the_handoff():
    for i, c in CASES.items():
        view, _ = as_forward_case(i)
        for cls in au.CLASSES:
            au.assert_exact(view, cls)
        if i in POINTS:
            plain, dec = POINTS[i]
            lib = _native.long_geometry(plain_key(i))
            assert F_.LONG_HANDOFF_POINTS < plain <= lib["N1"] * lib["N2"], i
            L, K = c.size[0], c.k[0]
            assert c.s * (out_len(i) - 1) + K == plain and F_._long_decim_points(L, K, c.s, c.p, c.p) == dec, i


def test_routes_of_the_gpu_table_in_the_three_modes(monkeypatch):
    for i in CASES:
        assert route_of(i) == "plain", i                       # unset: every row fits in plain form
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "0")
    for i in CASES:
        assert route_of(i) == "plain", i
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    for i in CASES:
        want = "phases" if i in PHASES_CASES else "plain"
        assert route_of(i) == route_of(i, torch.float16) == route_of(i, torch.bfloat16) == want, i
        assert route_of(i, C64) == "plain" and route_of(i, F32, "nlc") == "plain", i
        assert route_of(i, F32, "copy") == want, i


def test_handoff_and_the_edges_of_the_phases_route(monkeypatch):
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "1")
    route = F_._long_route
    # the padded row decides the hand-off, as ever: 4096 against 4097; complex rows never hand off
    assert route((1, 1, 4000), (1, 1, 100), 2, 48) == "handoff" and route((1, 1, 4000), (1, 1, 100), 2, 48, dtype=C64) == "plain"
    assert route((1, 1, 4001), (1, 1, 100), 2, 48) == "phases"
    assert route((1, 1, 4096), (1, 1, 100), 2, causal=True) == "phases"      # L + K - 1 points
    assert route((1, 1, 3997), (1, 1, 100), 2, causal=True) == "handoff"
    big = ((2, 2, 9000), (2, 2, 1000))
    assert route(*big, 1) == "plain"                       # stride 1 has one phase: the row itself
    assert route(*big, 64) == "phases" and route(*big, 65) == "plain"
    assert route(*big, 2, dilation=2) == "plain"
    assert route(*big, 2, 10, padding_mode="reflect") == "plain" and route(*big, 2, 10, padding_mode="zeros") == "phases"
    assert route(*big, 2, dtype=C64) == "plain" and route(*big, 2, x_layout="nlc") == "plain"
    assert route(*big, 2, "valid") == "phases"
    with pytest.raises(ValueError, match="same"):
        route(*big, 2, "same")


def test_a_row_past_the_plain_limit_runs_by_phases_and_past_both_raises(monkeypatch):
    shape = ((1, 1, (1 << 24) + 4096), (1, 1, 1000))
    assert F_._long_route(*shape, 64) == "phases"            # with nothing set
    assert F_._long_decim_points(shape[0][2], 1000, 64, 0, 0) <= 1 << 19
    info = _native.decim_geometry((1, 1, 1, 1, shape[0][2], 1000, 64, 0, 0, 0, 0, 0))
    assert info["N1"] * info["N2"] == 1 << 19 and info["out_len"] == (shape[0][2] - 1000) // 64 + 1
    with pytest.raises(NotImplementedError, match=r"2\^24"):      # the plain plan of the same row
        _native.long_geometry((1, 1, 1, 1, shape[0][2], 1000, 0, 0, 0, 0, 0, 0, 1, 1, 64))
    monkeypatch.setenv("FFTCONV_LONG_DECIM", "0")
    with pytest.raises(NotImplementedError, match=str(shape[0][2])):
        F_._long_route(*shape, 64)
    monkeypatch.delenv("FFTCONV_LONG_DECIM")
    # not eligible: the error of today; past both limits: the count
    with pytest.raises(NotImplementedError, match=str(shape[0][2])):
        F_._long_route(*shape, 65)
    with pytest.raises(NotImplementedError, match=r"2\*\*24"):
        F_._long_route((1, 1, 40_000_000), (1, 1, 1000), 2)
    with pytest.raises(NotImplementedError, match=r"2\^24"):
        _native.decim_geometry((1, 1, 1, 1, 40_000_000, 1000, 2, 0, 0, 0, 0, 0))
    # a causal row past the limit runs forward by phases too
    assert F_._long_route((1, 1, 1 << 24), (1, 1, 5000), 4, causal=True) == "phases"


# ------------------------------------------------------------------------------------------------ geometry
def test_decim_geometry_of_case_1_against_the_plain_plan():
    c = CASES[1]
    dec, plain = _native.decim_geometry(decim_key(1)), _native.long_geometry(plain_key(1))
    assert (dec["N1"], dec["N2"]) == (64, 128) and (plain["N1"], plain["N2"]) == (128, 128)
    assert dec["out_len"] == plain["out_len"] == out_len(1) == 4000
    # s decimated rows per input channel on half the points: the same spectrum, a smaller workspace
    assert dec["spectrum_bytes"] == c.cout * c.s * (c.cin // c.g) * 8192 * 8 == plain["spectrum_bytes"]
    assert dec["workspace_bytes"] == dec["slab_pairs"] * (c.s * c.cin + c.cout) * 8192 * 8
    assert plain["workspace_bytes"] == plain["slab_pairs"] * (c.cin + c.cout) * 16384 * 8 and dec["slab_pairs"] == plain["slab_pairs"] == 2


@pytest.mark.parametrize("i", PHASES_CASES)
def test_decim_geometry_of_the_table(i, monkeypatch):
    c = CASES[i]
    info = _native.decim_geometry(decim_key(i))
    n = info["N1"] * info["N2"]
    L, K = c.size[0], c.k[0]
    need = out_len(i) + -(-K // c.s) - 1
    assert info["out_len"] == out_len(i) and n >= need and (n == 4096 or n < 2 * need), (n, need)
    assert info["spectrum_bytes"] == c.cout * c.s * (c.cin // c.g) * n * 8
    assert info["workspace_bytes"] == info["slab_pairs"] * (c.s * c.cin + c.cout) * n * 8
    monkeypatch.setenv("FFTCONV_LONG_N", "128x128")          # the factorisation knob of every long plan
    forced = _native.decim_geometry(decim_key(i))
    assert (forced["N1"], forced["N2"]) == (128, 128)


@pytest.mark.parametrize("key,text", [
    ((1, 4, 6, 2, 100, 10, 1, 0, 0, 0, 0, 0), "stride"), ((1, 4, 6, 2, 100, 10, 65, 0, 0, 0, 0, 0), "stride"),
    ((1, 4, 6, 2, 100, 10, 2, -1, 0, 0, 0, 0), "padding"), ((1, 4, 6, 2, 100, 10, 2, 0, 0, -1, 0, 0), "out_keep"),
    ((1, 4, 6, 2, 100, 10, 2, 0, 0, 0, 2, 0), "flip"), ((1, 4, 6, 4, 100, 10, 2, 0, 0, 0, 0, 0), "divisible"),
    ((1, 4, 6, 2, 100, 110, 2, 4, 4, 0, 0, 0), "longer than the padded row"), ((1, 4, 6, 2, 100, 10, 2, 0, 0, 47, 0, 0), "out_keep"),
    ((0, 4, 6, 2, 100, 10, 2, 0, 0, 0, 0, 0), "positive"), ((1, 4, 6, 2, 100, 0, 2, 0, 0, 0, 0, 0), "positive"),
])
def test_decim_geometry_refuses_bad_descriptors(key, text):
    with pytest.raises(ValueError, match=text):
        _native.decim_geometry(key)
    with pytest.raises(ValueError, match="12 words"):
        _native.decim_desc(key[:-1])


def test_decim_geometry_limits(monkeypatch):
    with pytest.raises(NotImplementedError, match=r"2\^29"):          # a row of x behind one buffer resource
        _native.decim_geometry((1, 1, 1, 1, 1 << 29, 1000, 64, 0, 0, 0, 0, 0))
    assert _native.decim_geometry((1, 1, 1, 1, (1 << 29) - 1, 1000, 64, 0, 0, 0, 0, 0))["N1"] * 64 <= 1 << 30
    with pytest.raises(NotImplementedError, match=r"2\^24"):
        _native.decim_geometry((1, 1, 1, 1, (1 << 29) - 1, 1000, 16, 0, 0, 0, 0, 0))
    # 4096 pairs x 4096 channels x 2 phases at 64 x 64 points: the passes every long plan runs stay inside 2^31 workgroups,
    # the phase blocks of the forward column pass, two of them per channel at NC = 2, do not
    key = (8192, 4096, 4096, 4096, 6000, 1001, 2, 0, 0, 0, 0, 0)
    assert _native.decim_geometry(key)["slab_pairs"] < 64
    monkeypatch.setenv("FFTCONV_LONG_WS_MB", "2000000")
    with pytest.raises(NotImplementedError, match=r"phases .* exceeds the 2\^31 workgroups"):
        _native.decim_geometry(key)
    assert _native.decim_geometry((2048,) + key[1:])["slab_pairs"] == 1024


# ------------------------------------------------------------------------------------------------ exports and ABI
def test_new_entry_points_only_and_abi_7():
    header = open(os.path.join(ROOT, "include", "fftconv_amd.h")).read()
    declared = set(re.findall(r"\b(fc_[a-z0-9_]+)\s*\(", header))
    new = {"fc_long_decim_geometry", "fc_long_decim_plan_create"}
    assert new <= declared and declared == set(_native.EXPORTS)
    assert re.search(r"int fc_long_decim_geometry\(const fc_long_decim_desc\* desc, int64_t info\[8\]\);", header)
    assert re.search(r"int fc_long_decim_plan_create\(const fc_long_decim_desc\* desc, fc_long_plan\*\* out_plan\);", header)
    lib = _native.load_library()
    for name in _native.EXPORTS:
        assert hasattr(lib, name), name
    m = re.search(r"#define\s+FC_ABI_VERSION\s+(\d+)", header)
    assert m and int(m.group(1)) == 7 == _native.ABI_VERSION == lib.fc_version()
    # nothing that existed changes
    assert ctypes.sizeof(_native.FcLongDesc) == 80 and ctypes.sizeof(_native.FcLongExt) == 16
    assert ctypes.sizeof(_native.FcLongPhasesDesc) == 80 and ctypes.sizeof(_native.FcLongDecimDesc) == 88
    assert _native._PLAN_TAGS == {"long": _native.LongPlan, "long_phases": _native.LongPhasesPlan, "long_decim": _native.LongDecimPlan,
                                  "long_wgrad": _native.LongWgradPlan}
    assert issubclass(_native.LongDecimPlan, _native.LongPlan)


def test_the_switch_is_read_per_call(monkeypatch):
    assert F_._long_decim_mode() is None
    for value, want in (("0", False), ("1", True), ("", None), ("yes", None)):
        monkeypatch.setenv("FFTCONV_LONG_DECIM", value)
        assert F_._long_decim_mode() is want
